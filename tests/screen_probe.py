"""`python tests/screen_probe.py` in a process of its own (LANTERN_GPU_SCREEN is read when an index is created): f32 l2sq indexes whose
walks the int8 screen serves (rows of >= 128 chunks) and some it does not, over data that stresses the screen's bound -- Gaussian,
clustered, tie-heavy, duplicates, outlier components, rows mixing 1e30 and 1e-30, all-zero rows -- searched in the classic walk at
several ef and k, by batch, by lone query and by streaming cursor, also after rows entered by insertion, file load, graph import and
the two sharded builds.  One JSON line of digests of the answers (ids, distance bits, counts), the search counters (D, E) and, under
"screen", each index's lantern_gpu_search_screen_stats.  tests/test_gpu_screen.py runs it with the screen on and off and requires the
same line apart from "screen", and that the screen rejected rows wherever it is on."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lantern_amd import capi  # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


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
    out[np.arange(n), rng.integers(0, d, n)] = np.float32(1e4)  # one outlier component per row: a coarse int8 scale
    yield "outlier", out, g[rng.integers(0, n, 64)]
    mix = g.copy()
    mix[: n // 4, : d // 2] *= np.float32(1e30)
    mix[n // 4: n // 2] *= np.float32(1e-30)
    mix[n // 2: n // 2 + 50] = 0
    yield "mixed_scale", mix, np.concatenate([mix[rng.integers(0, n, 32)], g[:32]])


def searches(ix, queries, out, tag, screened):
    """every search form, in the CLASSIC walk (an explicit wave count: 4 and 8 waves per query) -- the walk the screen serves; without it
    batches of up to 2 x CUs queries and the lone query would take the latency-bound walk of walk_spec.hpp, which the screen leaves alone"""
    for waves in (4, 8):
        ix.set_search_shape(waves)
        for ef, k in ((1, 1), (10, 10), (64, 10), (64, 64), (128, 5), (400, 10)):  # (ef 400: the LDS-list walk, not screened)
            lab, dist, cnt = ix.search_batch(queries, k, ef)
            out[f"{tag}_w{waves}_ef{ef}_k{k}"] = digest(lab, dist, cnt)
        lab1, dist1 = ix.search(queries[0], 10)
        cur = ix.cursor()
        pages = [cur.search(queries[1], 5, 40, streaming=True) for _ in range(3)]
        out[f"{tag}_w{waves}_lone_and_cursor"] = digest(lab1, dist1, *[a for p in pages for a in p])
    ix.set_search_shape(0)
    c = ix.counters()
    out[tag + "_DE"] = [c["search_dist_evals"], c["search_expansions"]]
    logical, exact = ix.screen_stats()
    out["screen"][tag] = {"screened": screened, "logical": logical, "exact": exact}


def local_world_build(d, base, labels, rows):
    """two ranks as threads over the in-process hub: lantern_gpu_add_sharded (rows = False) or lantern_gpu_add_row_sharded"""
    import threading

    comms = capi.Comm.local_world(2)
    out, errs = [None, None], []

    def run(r):
        try:
            comms[r].set_timeout(120)
            ix = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=3)
            ix.set_add_batch(512, 16)
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
    rng = np.random.default_rng(11)
    out = {"screen": {}}
    for d in (768, 129, 1536, 2000, 520):
        n = 3000 if d <= 768 else 1500
        screened = d >= 509  # rows of >= 128 chunks
        for name, base, queries in datasets(rng, n, d):
            if d != 768 and name not in ("gaussian", "outlier"):
                continue
            labels = np.arange(n, dtype=np.uint64) + 1
            ix = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=3)
            ix.set_add_batch(512, 16)
            ix.add_many(labels, base)
            ix.flush()
            tag = f"{name}_{d}"
            out[tag + "_graph"] = f"{ix.checksum():016x}"
            searches(ix, queries, out, tag, screened)
            if name == "gaussian" and d == 768:
                # rows that enter after the build -- one ldb_aminsert-sized insertion, a batch -- and through every other path that
                # stores rows (a file, an imported graph: the mirror's path, the two sharded builds): their screen rows must be there.
                # A query equal to such a row finds it at distance 0 only if the screen did not reject it.
                ix.add(10**6, queries[2])
                ix.add_many(np.arange(10**6 + 1, 10**6 + 65, dtype=np.uint64), queries[3:67])
                ix.flush()
                ix.set_search_shape(4)
                lab, dist, cnt = ix.search_batch(queries[2:67], 10)
                ix.set_search_shape(0)
                out[tag + "_inserted"] = digest(lab, dist, cnt)
                out[tag + "_inserted_found"] = float(np.mean(dist[:, 0] == 0))
                others = []
                ix2 = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=3)
                ix2.load_buffer(ix.save_buffer())
                others.append(("loaded", ix2))
                g = ix.export_graph(with_vectors=True)
                ix3 = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=3)
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
