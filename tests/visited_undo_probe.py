"""`python tests/visited_undo_probe.py IN_DIR OUT_DIR` in a process of its own: LANTERN_GPU_VIS_UNDO (the capacity of the visited bitmaps' undo
logs) and LANTERN_GPU_INSERT_SPEC are read once per process, so the forced-overflow and forced-mixed regimes of the register-list, screened,
latency-bound and insertion walks need a fresh process each.  tests/test_gpu_visited_undo_probe.py writes the oracle's graphs to IN_DIR, starts
this with the run's environment and compares what it leaves in OUT_DIR with the oracle, bit for bit.

What it runs (tests/visited_regimes.py has the shapes): on the three imported indexes, on W = 1 and W = 3 workgroups -- the launch, the launch
again, the launch with its queries rolled by one -- of
  * the uniform search at ef = 64 in the classic shape (screened on the 768-d indexes), LANTERN_GPU_SPEC=1 and =2,
  * the per-query search with ef 8 | 64 by turns, classic and in the 3 + 8 wave shape,
  * on the 768-d indexes, 1088 queries on three workgroups at ef = 64 and 128: the screened walk with two rows in flight per group;
and one build in which every batch goes to k_insert on three workgroups.  OUT_DIR/out.npz holds every answer, OUT_DIR/meta.json the grids, the
screen counters and the build's counters."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lantern_amd import capi  # noqa: E402
from tests import visited_regimes as vr  # noqa: E402

KEYS = ("slots", "dists", "counts", "D", "E", "labels")


def set_env(env):
    for name in ("LANTERN_GPU_SPEC", "LANTERN_GPU_LDS_LIST"):
        os.environ.pop(name, None)
    os.environ.update(env)


def main(in_dir, out_dir):
    out, meta = {}, {"grid": {}, "screen": {}}
    for name in vr.PROBE_INDEXES:
        metric, n, d, M, efc, storage = vr.SHAPES[name]
        z = np.load(os.path.join(in_dir, name + ".npz"))
        g = {a: z[a] for a in vr.GRAPH_ARRAYS}
        g["entry_slot"], g["max_level"] = int(z["entry_slot"]), int(z["max_level"])
        gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=vr.EF_DEFAULT, seed=vr.INDEX_SEED, quantization=storage)
        gpu.import_graph(z["base"], g)
        queries = z["queries"]
        for kind, families, params, width in (("uniform", vr.PROBE_FAMILIES, 64, vr.K), ("each", vr.PROBE_EACH_FAMILIES, vr.PROBE_MIXED, vr.PROBE_K)):
            A, B = vr.Launcher(gpu, queries, width), vr.Launcher(gpu, np.roll(queries, 1, axis=0), width)
            for family, env in families.items():
                set_env(env)
                before = gpu.screen_stats()
                for W in vr.PROBE_W:
                    gpu.set_search_shape(0, W)
                    for step, launcher, p in (("first", A, params), ("again", A, params), ("rolled", B, vr.roll_params(params))):
                        key = f"{name}.{kind}.{family}.W{W}.{step}"
                        for what, a in zip(KEYS, launcher.run(p)):
                            out[f"{key}.{what}"] = a
                        meta["grid"][key] = gpu.last_search_grid()
                gpu.set_search_shape(0, 0)
                meta["screen"][f"{name}.{kind}.{family}"] = [a - b for a, b in zip(gpu.screen_stats(), before)]
        for tname, ef in vr.PROBE_TILED:  # the screened walk with two rows in flight per group: TILED_NQ queries on three workgroups
            if tname != name:
                continue
            tq = vr.tiled(queries, vr.TILED_NQ)
            A, B = vr.Launcher(gpu, tq), vr.Launcher(gpu, np.roll(tq, 1, axis=0))
            set_env(vr.env_of(spec=0))
            before = gpu.screen_stats()
            gpu.set_search_shape(0, vr.INSERT_W)
            for step, launcher in (("first", A), ("again", A), ("rolled", B)):
                key = f"{name}.tiled{ef}.classic.W{vr.INSERT_W}.{step}"
                for what, a in zip(KEYS, launcher.run(ef)):
                    out[f"{key}.{what}"] = a
                meta["grid"][key] = gpu.last_search_grid()
            gpu.set_search_shape(0, 0)
            meta["screen"][f"{name}.tiled{ef}.classic"] = [a - b for a, b in zip(gpu.screen_stats(), before)]
        set_env({})
        gpu.close()
    # the build: plan (512, 16), every batch by k_insert (LANTERN_GPU_INSERT_SPEC=0 in this process's environment) on three workgroups
    metric, n, d, M, efc, plan = vr.PROBE_INSERT
    z = np.load(os.path.join(in_dir, "insert.npz"))
    ix = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=vr.EF_DEFAULT, seed=vr.INDEX_SEED)
    ix.set_search_shape(0, vr.INSERT_W)
    ix.set_add_batch(*plan)
    ix.add_many(z["labels"], z["base"])
    ix.flush()
    g = ix.export_graph()
    for a in vr.GRAPH_ARRAYS:
        out["insert." + a] = g[a]
    meta["insert"] = {"entry_slot": int(g["entry_slot"]), "max_level": int(g["max_level"]), "stats": list(ix.insert_screen_stats()), "rows": len(ix)}
    np.savez(os.path.join(out_dir, "out.npz"), **out)
    with open(os.path.join(out_dir, "meta.json"), "w") as f:
        json.dump(meta, f)
    print(json.dumps({"answers": len(out), "launches": len(meta["grid"])}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
