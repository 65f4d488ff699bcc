"""lantern_gpu_exact_search on a compact pq index under lantern_gpu_set_exact_adc (include/lantern_gpu.h; DESIGN.md 4.5 "Compact pq
indexes: ADC pre-selection"): the pre-selection scans the code rows against per-query tables (k_adc_tables, k_scan_adc:
csrc/dense_adc.hip); everything behind it, and so the answer, is unchanged.  Needs an MI355X.

The indexes, the float64 reference over the decoded rows and the checks (float64 top-k at 1e-5 max(1, |x|); the expanded twin's slots and
distance bits; still compact) are tests/test_gpu_exact_compact.py's, built once for both files.
"""
import pytest

from tests.test_gpu_exact_compact import SHAPES, built, check

pytestmark = pytest.mark.gpu

# the shapes of the code-row path at which the scan can go wrong, by the tables a workgroup holds (T) and the chunks of a code row:
#   cps1_eight_codes_a_step  T = 4, 16 subvectors      cps6_one_code_chunk  4 subvectors padded to 16, a second query tile at 1025
#   cos_768_zero_norms       T = 1, 96 subvectors at the 128-byte stride, zero rows / query / centroid
#   second_row_chunk         65 536 + 129 rows         fused_past_seed_cols  256 centroids, T = 4 at two code chunks
# and one of this file's: T = 2 (48 subvectors, three code chunks), more rows than the seed columns, an odd query left in the last group
ADC_SHAPES = {name: SHAPES[name][:6] for name in
              ("cps1_eight_codes_a_step", "cps6_one_code_chunk", "cos_768_zero_norms", "second_row_chunk", "fused_past_seed_cols")}
ADC_SHAPES["t2_48_subvectors"] = ("l2sq", 4200, 192, 48, 16, (1, 129))


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


@pytest.fixture
def scanning(capi, monkeypatch):
    """name -> the shape's index with the scan on for every batch size; off again afterwards (the other file shares the indexes)"""
    monkeypatch.delenv("LANTERN_GPU_DENSE_FUSED", raising=False)
    on = []

    def get(name, shape, max_queries=4096):
        b = built(capi, name, *shape[:5])
        b["ix"].set_exact_adc(max_queries)
        on.append(b["ix"])
        return b

    yield get
    for ix in on:
        ix.set_exact_adc(0)


@pytest.mark.parametrize("fused", [None, "0"])
@pytest.mark.parametrize("name", ADC_SHAPES)
def test_scanned_answers_match_float64_and_the_expanded_twin(capi, scanning, monkeypatch, name, fused):
    if fused is not None:
        monkeypatch.setenv("LANTERN_GPU_DENSE_FUSED", fused)
    metric, n, d, S, C, nqs = ADC_SHAPES[name]
    b = scanning(name, ADC_SHAPES[name])
    assert b["ix"].exact_adc() == 4096 and b["ix"].exact_compact() == 2
    for nq in nqs:
        for k in (1, 10):
            before = capi.exact_adc_stats()
            check(b, nq, k)  # (asserts the index is still compact)
            steps = capi.plan_exact_knn({"l2sq": 3, "cos": 1}[metric] + 600, d // 4, n, nq, k, fused=-1 if fused is None else 0)["n_steps"]
            after = capi.exact_adc_stats()
            assert (after["tables"] - before["tables"], after["scans"] - before["scans"]) == (1, steps)


def test_cancelling_data_still_ends_in_the_twins_answers_through_the_fallback(capi, scanning):
    b = scanning("cancelling", SHAPES["cancelling"])
    before, scans = capi.exact_knn_stats()["fallback"], capi.exact_adc_stats()["scans"]
    check(b, 129, 10)
    assert capi.exact_knn_stats()["fallback"] > before and capi.exact_adc_stats()["scans"] > scans


def test_larger_batches_and_the_switch_at_zero_do_not_scan(capi, scanning):
    name = "cps1_eight_codes_a_step"
    b = scanning(name, SHAPES[name], max_queries=64)
    before = capi.exact_adc_stats()
    check(b, 65, 10)
    b["ix"].set_exact_adc(0)
    check(b, 1, 10)
    assert capi.exact_adc_stats() == before
    with pytest.raises(capi.LanternGpuError, match="exact_adc must be 0"):
        b["ix"].set_exact_adc(-1)
    b["ix"].set_exact_adc(64)
    check(b, 64, 10)
    assert capi.exact_adc_stats()["scans"] > before["scans"]
