"""`python tests/screen_cos_probe.py` in a process of its own (LANTERN_GPU_SCREEN is read when an index is created): the cosine twin of
tests/screen_probe.py.  f32 cosine indexes whose walks the int8 screen serves (rows of >= 128 chunks: d = 509, 512, 768, 2000) and one
it does not (d = 504), over data that stresses the cosine bound -- Gaussian, clustered, tie-heavy, duplicates, outlier components, rows
at 2^-45, 1 and 2^55 with all-zero rows among them, per-row scales e^+-20, a common mean -- searched in the classic walk at several ef and
k, by batch, by lone query and by streaming cursor, also after rows entered by insertion, file load, graph import and the two sharded
builds.  One JSON line of digests of the answers (ids, distance bits, counts), the search counters (D, E) and, under "screen", each
index's lantern_gpu_search_screen_stats.  tests/test_gpu_screen_cos.py runs it with the screen on and off and requires the same line
apart from "screen", and that the screen rejected rows wherever it is on."""
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lantern_amd import capi  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from tests.screen_probe import digest, searches  # noqa: E402

DIMS = (768, 509, 512, 2000, 504)


def datasets(rng, n, d):
    g = rng.standard_normal((n, d), dtype=np.float32)
    yield "gaussian", g, rng.standard_normal((96, d), dtype=np.float32)
    centres = rng.standard_normal((16, d), dtype=np.float32) * 4
    cl = centres[rng.integers(0, 16, n)] + rng.standard_normal((n, d), dtype=np.float32) * 0.5
    yield "clustered", cl.astype(np.float32), (centres[rng.integers(0, 16, 96)] + rng.standard_normal((96, d), dtype=np.float32) * 0.5).astype(np.float32)
    lat = rng.integers(-1, 2, size=(n, d)).astype(np.float32)
    yield "lattice", lat, rng.integers(-1, 2, size=(64, d)).astype(np.float32)
    dup = np.repeat(g[: n // 3 + 1], 3, axis=0)[:n].copy()  # every row three times: ties exactly at the radius
    yield "triplicates", dup, dup[rng.integers(0, n, 64)] + np.float32(0.01)
    out = g.copy()
    out[np.arange(n), rng.integers(0, d, n)] = np.float32(1e4)  # one outlier component per row: a coarse int8 scale, a small rho
    yield "outlier", out, g[rng.integers(0, n, 64)]
    mix = g.copy()  # (tests/value_range.py cos_mixed: norms below, inside and above the range in which the screen rejects)
    mix[0::3] *= np.float32(2.0 ** -45)
    mix[2::3] *= np.float32(2.0 ** 55)
    mix[rng.choice(n, 50, replace=False)] = 0
    mq = np.concatenate([mix[rng.integers(0, n, 32)], g[:31], np.zeros((1, d), np.float32)])
    yield "mixed_scale", mix, mq
    sc = np.exp(rng.uniform(-20, 20, n)).astype(np.float32)[:, None]
    yield "row_scales", (g * sc).astype(np.float32), rng.standard_normal((64, d), dtype=np.float32)
    yield "common_mean", g + np.float32(3), rng.standard_normal((64, d), dtype=np.float32) + np.float32(3)


def new_index(d):
    ix = capi.GpuIndex("cos", d, M=16, ef_construction=64, ef=64, seed=3)
    ix.set_add_batch(512, 16)
    return ix


def local_world_build(d, base, labels, rows):
    """two ranks as threads over the in-process hub: lantern_gpu_add_sharded (rows = False) or lantern_gpu_add_row_sharded"""
    comms = capi.Comm.local_world(2)
    out, errs = [None, None], []

    def run(r):
        try:
            comms[r].set_timeout(120)
            ix = new_index(d)
            lo, hi = capi.shard_range(len(base), 2, r)
            (ix.add_row_sharded if rows else ix.add_sharded)(comms[r], labels[lo:hi], base[lo:hi])
            out[r] = ix
        except Exception as e:  # noqa: BLE001 -- reported below
            errs.append((r, repr(e)))

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    return out, comms


def main():
    rng = np.random.default_rng(12)
    out = {"screen": {}}
    for d in DIMS:
        n = 3000 if d <= 768 else 1500
        screened = d >= 509  # rows of >= 128 chunks
        for name, base, queries in datasets(rng, n, d):
            labels = np.arange(n, dtype=np.uint64) + 1
            ix = new_index(d)
            ix.add_many(labels, base)
            ix.flush()
            tag = f"{name}_{d}"
            out[tag + "_graph"] = f"{ix.checksum():016x}"
            searches(ix, queries, out, tag, screened)
            if name == "gaussian" and d == 768:
                # rows that enter after the build -- one ldb_aminsert-sized insertion, a batch -- and through every other path that
                # stores rows (a file, an imported graph: the mirror's path, the two sharded builds): their screen rows and their
                # cosine metadata must be there.  A query equal to such a row finds it at the device's distance of the row to itself
                # (a few ulps either side of 0), or below, only if the screen did not reject it.
                ix.add(10**6, queries[2])
                ix.add_many(np.arange(10**6 + 1, 10**6 + 65, dtype=np.uint64), queries[3:67])
                ix.flush()
                ix.set_search_shape(4)
                lab, dist, cnt = ix.search_batch(queries[2:67], 10)
                ix.set_search_shape(0)
                self_d = np.array([oracle.distance(q, q, "cos", oracle.SUM_WAVE64) for q in queries[2:67]], dtype=np.float32)
                out[tag + "_inserted"] = digest(lab, dist, cnt)
                out[tag + "_inserted_found"] = float(np.mean(dist[:, 0] <= self_d))
                others = []
                ix2 = new_index(d)
                ix2.load_buffer(ix.save_buffer())
                others.append(("loaded", ix2))
                g = ix.export_graph(with_vectors=True)
                ix3 = new_index(d)
                ix3.import_graph(g["vectors"], g)
                others.append(("imported", ix3))
                for rows in (False, True):
                    replicas, _comms = local_world_build(d, base, labels, rows)
                    for r, rep in enumerate(replicas):
                        others.append((f"{'row_' if rows else ''}sharded_rank{r}", rep))
                for what, other in others:
                    searches(other, queries, out, f"{tag}_{what}", screened)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
