"""The forced log regimes of the visited bitmaps' undo log (walk.hpp VisUndo) in reused workgroups: tests/visited_undo_probe.py in a process
of its own per run -- LANTERN_GPU_VIS_UNDO is read once per process -- and its answers against the ORACLE on the same graphs, bit for bit
(not against another run's digest).  Needs an MI355X.

  LANTERN_GPU_VIS_UNDO = 16, V = 256 and V = 0, and = 0, V = 256: every walk of every launch overflows its log (D - U - V > 16) and clears
      its whole bitmap at its end, with the workgroup's next walk right behind it;
  LANTERN_GPU_VIS_UNDO = visited_regimes.MIXED_CAP, V = 0, per-query ef 8 | 64 in one launch: the whole-bitmap clear of one walk directly in
      front of a logged walk on the same bitmap (inside a launch the clearing walks come first: a per-query launch walks its list by
      expansion, descending), and a clearing walk behind a logged one where the launch is repeated.

The conditions are tests/visited_regimes.py's, proven without a device by tests/test_visited_regimes_ref.py."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import visited_regimes as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# One run of the probe takes 3.0 - 3.9 s of wall time on an MI355X box (three imports, 102 launches -- twelve of them 1088 queries on three
# workgroups --, a 1200-row build; the log's capacity changes it by less than the start of the process varies); a child gets three times
# that.  One that times out or is killed by a signal is a failure and ends the session: nothing is started on a device after a hang or a
# fault, and the child is not retried.
PROBE_SECONDS = 4
TIMEOUT = 3 * PROBE_SECONDS


@pytest.fixture(scope="module")
def inputs(oracle, tmp_path_factory):
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    d = tmp_path_factory.mktemp("visited_undo_in")
    for name in vr.PROBE_INDEXES:
        ix = vr.small_index(name)
        g = ix["g"]
        np.savez(d / (name + ".npz"), base=ix["base"], queries=ix["queries"], entry_slot=g["entry_slot"], max_level=g["max_level"],
                 **{a: g[a] for a in vr.GRAPH_ARRAYS})
    o = vr.probe_insert_oracle()
    np.savez(d / "insert.npz", base=o["base"], labels=o["labels"])
    return str(d)


@pytest.mark.parametrize("run", list(vr.PROBE_RUNS))
def test_forced_log_regimes_against_the_oracle(oracle, inputs, tmp_path, run):
    undo, V, regime = vr.PROBE_RUNS[run]
    cap = vr.MIXED_CAP if undo is None else undo
    for name in vr.PROBE_INDEXES:  # the regime, from the oracle's counts
        U = vr.descent(name)
        vr.assert_regime("overflow", vr.reference(name, 64)[3], U, V, cap)
        if regime == "mixed":
            vr.assert_mixed(vr.reference(name, vr.PROBE_MIXED)[3], U, V, cap)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LANTERN_GPU_")}
    env.update(LANTERN_GPU_VIS_UNDO=str(cap), LANTERN_GPU_VIS_SLOTS=str(V), LANTERN_GPU_INSERT_VIS_SLOTS=str(V), LANTERN_GPU_INSERT_SPEC="0")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "visited_undo_probe.py"), inputs, str(tmp_path)], capture_output=True, text=True,
                           timeout=TIMEOUT, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as ex:  # a hang: nothing more is started on the device in this session
        pytest.exit(f"{run}: the probe did not end within {TIMEOUT} s: {(ex.stderr or b'')[-1500:]!r}", returncode=1)
    print(f"{run}: the probe took {time.time() - t0:.1f} s")
    if p.returncode < 0:  # killed by a signal (an abort, a fault): likewise
        pytest.exit(f"{run}: the probe died with status {p.returncode}: {p.stderr[-3000:]}", returncode=1)
    assert p.returncode == 0, (run, p.stdout[-1500:], p.stderr[-3000:])
    out = np.load(tmp_path / "out.npz")
    meta = json.load(open(tmp_path / "meta.json"))
    checked = 0
    for name in vr.PROBE_INDEXES:
        for kind, families, params in (("uniform", vr.PROBE_FAMILIES, 64), ("each", vr.PROBE_EACH_FAMILIES, vr.PROBE_MIXED)):
            want = vr.reference(name, params)
            for family in families:
                for W in vr.PROBE_W:
                    for step in ("first", "again", "rolled"):
                        key = f"{name}.{kind}.{family}.W{W}.{step}"
                        got = tuple(out[f"{key}.{what}"] for what in ("slots", "dists", "counts", "D", "E", "labels"))
                        vr.check(got, vr.rolled(want) if step == "rolled" else want, f"{run} {key}")
                        assert meta["grid"][key] == W, (key, meta["grid"][key])
                        checked += 1
                logical, exact = meta["screen"][f"{name}.{kind}.{family}"]
                if family == "classic" and name in vr.SCREENED:  # the screened form of the walk ran (undo_apply<FRESH_ZERO>), and rejected rows
                    assert 0 < exact < logical, (run, name, kind, logical, exact)
    for name, ef in vr.PROBE_TILED:
        want = vr.tiled(vr.reference(name, ef), vr.TILED_NQ)
        vr.assert_regime("overflow", vr.reference(name, ef)[3], vr.descent(name), V, cap)
        for step in ("first", "again", "rolled"):
            key = f"{name}.tiled{ef}.classic.W{vr.INSERT_W}.{step}"
            got = tuple(out[f"{key}.{what}"] for what in ("slots", "dists", "counts", "D", "E", "labels"))
            vr.check(got, vr.rolled(want) if step == "rolled" else want, f"{run} {key}")
            assert meta["grid"][key] == vr.INSERT_W
            checked += 1
        logical, exact = meta["screen"][f"{name}.tiled{ef}.classic"]
        assert 0 < exact < logical, (run, name, ef, logical, exact)
    assert checked == len(meta["grid"]) == 3 * (3 + 2) * 2 * 3 + 3 * len(vr.PROBE_TILED)
    # the build: every batch by k_insert, unscreened, on three workgroups; the oracle's graph edge for edge
    o = vr.probe_insert_oracle()
    if regime == "overflow":  # PROXY (an insertion walk has no oracle D): the oracle's search at ef = ef_construction on the finished graph
        assert (o["finished"] - V).min() > cap
    screened, plain, tested, rejected = meta["insert"]["stats"]
    assert meta["insert"]["rows"] == vr.PROBE_INSERT[1] and screened == 0 and plain >= 10 and tested == 0
    g = {a: out["insert." + a] for a in vr.GRAPH_ARRAYS}
    g["entry_slot"], g["max_level"] = meta["insert"]["entry_slot"], meta["insert"]["max_level"]
    vr.same_graph(g, o["g"], f"{run}: the build on {vr.INSERT_W} workgroups against the oracle")
