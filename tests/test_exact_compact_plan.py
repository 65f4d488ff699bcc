"""lantern_gpu_plan_exact_compact: whether lantern_gpu_exact_search answers a compact pq index from its code rows, as a pure function
(include/lantern_gpu.h; DESIGN.md 4.5 "Compact pq indexes").  No device.  The entry point decides through this function.
"""
import pytest

from lantern_amd import capi

M_COS, M_L2SQ, M_HAMMING, M_F16, M_PQD = 1, 3, 8, 100, 600
CHUNKS, S16, INV = 192, 128, 8192  # 768-d rows in 96 subvectors of 8 dimensions: cps = 2, inv = 2^16 / 2


@pytest.mark.parametrize("metric", [M_L2SQ, M_COS])
@pytest.mark.parametrize("inv", [0, INV])
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("on", [False, True])
def test_the_decision_and_its_reason(on, compact, inv, metric):
    nb, nq, k = 1_000_000, 64, 10
    p = capi.plan_exact_compact(metric, CHUNKS, nb, nq, k, on, compact, inv, S16)
    want = "off" if not on else "expanded" if not compact else "no_decode" if inv == 0 else "taken"
    assert (p["why"], p["taken"]) == (want, want == "taken")
    rows = nb * CHUNKS * 16
    if want == "taken":
        knn = capi.plan_exact_knn(metric + M_PQD, CHUNKS, nb, nq, k)
        assert (p["kind"], p["mcode"], knn["kind"]) == (4, metric + M_PQD, 4)
        # the certificate is told the decoded row's f32 scalars, the K steps are the f32 rows': kind 0's plan in everything but the kind
        f32 = capi.plan_exact_knn(metric, CHUNKS, nb, nq, k)
        assert {**knn, "kind": 0} == f32 and knn["dims"] == CHUNKS * 4
        # no copy of the rows: the run's blocks are the f32 plan's own three, the fallback's one decoded chunk does not grow with nb
        assert (knn["fq_bytes"], knn["fb_bytes"]) == (0, 0)
        assert p["run_bytes"] == knn["aux_bytes"] + knn["dd_bytes"] + knn["cand_bytes"] < rows // 100
        assert p["fallback_bytes"] == 65536 * CHUNKS * 16 and p["expand_bytes"] == 0
    else:
        assert (p["run_bytes"], p["fallback_bytes"]) == (0, 0)
        assert p["expand_bytes"] == (rows if compact else 0)  # what the call decodes the index into


def test_other_metrics_and_bad_inputs():
    for mcode in (M_HAMMING, M_L2SQ + M_F16, M_L2SQ + M_PQD):
        assert capi.plan_exact_compact(mcode, CHUNKS, 1000, 1, 10, True, True, INV, S16)["why"] == "metric"
    small = capi.plan_exact_compact(M_L2SQ, 24, 300, 1, 10, True, True, 10923, 16)
    assert small["taken"] and small["fallback_bytes"] == 300 * 24 * 16
    for bad in [dict(chunks=0), dict(nb=-1), dict(code_row_bytes=0), dict(code_row_bytes=24), dict(k=241), dict(pqd_inv=-1)]:
        args = dict(mcode=M_L2SQ, chunks=CHUNKS, nb=1000, nq=1, k=10, on=True, compact=True, pqd_inv=INV, code_row_bytes=S16)
        with pytest.raises(capi.LanternGpuError, match="lantern_gpu: bad plan input"):
            capi.plan_exact_compact(**{**args, **bad})
