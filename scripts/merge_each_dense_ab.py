#!/usr/bin/env python
"""Assemble profiles/filtered_each_dense_1Mx768_clustered.json from alternated runs of `scripts/bench_filtered.py --each-dense`.

    python scripts/merge_each_dense_ab.py --ab DIR [--like DIR] [--headline DIR] [--parent COMMIT] > profiles/filtered_each_dense_1Mx768_clustered.json

The A/B against the parent commit is two processes, because one process loads one library: the caller runs the script from a checkout
of the parent (a build without the setting times "setting_0" only) and from this tree, alternated, and keeps each process's JSON line:
  --ab DIR        parent_1.json, tree_1.json, parent_2.json, ... : `--each-dense --reps 1` per process, in the order run.  Per case the
                  repeats of the parent's call, of the tree's call with the setting at 0 and at 2 (and, on the one-filter case, of the
                  single-filter fused route), their medians, the dense run's diagnostic, whether every tree process found the slots of
                  all its modes equal.
  --like DIR      the same file names from a second call (`--reps 3`; the tree's with `--setting-0-only`) in which the tree's process never
                  touches the setting (it times "setting_0" only, as the parent's does): like for like, no dense call between the timed calls.
  --headline DIR  parent_1.json, tree_1.json, ... : the last line of `python bench.py --gpus 1 --steps 20 --warmup 3` per process.
"""
import argparse
import glob
import json
import os
import re

import numpy as np


def runs(directory, side):
    files = sorted(glob.glob(os.path.join(directory, side + "_*.json")), key=lambda f: int(re.search(r"_(\d+)\.json$", f).group(1)))
    return [json.loads(open(f).read().strip().splitlines()[-1]) for f in files]


def rounded(values):
    return [round(float(x), 3) for x in values]


def median(values):
    return round(float(np.median(values)), 3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ab", required=True)
    p.add_argument("--like")
    p.add_argument("--headline")
    p.add_argument("--parent", default="", help="the parent commit, for the note")
    a = p.parse_args()
    par, tre = runs(a.ab, "parent"), runs(a.ab, "tree")
    assert par and tre and not par[0]["has_setting"] and tre[0]["has_setting"]
    cases = []
    for i, leg in enumerate(tre[0]["each_dense"]):
        wall = {"parent_commit": [x for r in par for x in r["each_dense"][i]["wall_ms"]["setting_0"]]}
        for mode in leg["wall_ms"]:
            wall["tree_" + mode] = [x for r in tre for x in r["each_dense"][i]["wall_ms"][mode]]
        cases.append({"case": leg["case"], "filters": leg["filters"], "rows_per_filter": leg["rows_per_filter"], "queries": leg["queries"],
                      "dense_run": leg["dense_run"], "wall_ms": {k: rounded(v) for k, v in wall.items()}, "median_ms": {k: median(v) for k, v in wall.items()},
                      "slots_equal_setting_0": all(all(r["each_dense"][i]["answers_equal"].values()) for r in tre)})
    out = {"command": tre[0]["command"], "assembled_by": "python scripts/merge_each_dense_ab.py",
           "note": f"one MI355X, one call: a build of the parent commit {a.parent} and this tree as two processes, alternated {len(tre)} times (parent first); "
                   "each process warms every mode once, then times one call per mode behind one untimed call of the same mode; wall-clock ms per call with "
                   "a device synchronisation; the parent has no setting (its call is 'setting 0')",
           "workload": tre[0]["workload"], "min_group": tre[0]["min_group"], "cases": cases}
    if a.like:
        lp, lt = runs(a.like, "parent"), runs(a.like, "tree")
        assert lp and lt and not lt[0]["has_setting"]
        like = []
        for i, leg in enumerate(lt[0]["each_dense"]):
            row = {"case": leg["case"], "parent_commit": rounded(x for r in lp for x in r["each_dense"][i]["wall_ms"]["setting_0"]),
                   "tree_setting_never_touched": rounded(x for r in lt for x in r["each_dense"][i]["wall_ms"]["setting_0"])}
            row["median_ms"] = {k: median(row[k]) for k in ("parent_commit", "tree_setting_never_touched")}
            like.append(row)
        out["setting_0_like_for_like"] = {"command": lp[0]["command"] + " (the tree's process with --setting-0-only)",
                                          "note": f"a second call on the same box: parent build and this tree's library alternated {len(lt)} times as processes, the tree's "
                                                  "setting never touched (no dense call in the process)", "cases": like}
    if a.headline:
        sides = [(s, r) for pair in zip(runs(a.headline, "parent"), runs(a.headline, "tree")) for s, r in zip(("parent", "tree"), pair)]
        out["headline_before_after"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 3",
                                        "note": f"a build of the parent commit and this tree, alternated {len(sides) // 2} times on one box in one call",
                                        "runs": [{"side": s, "value": r["value"], "unit": r["unit"], "ms_per_step": r["ms_per_step"], "recall_at_10": r.get("recall_at_10")}
                                                 for s, r in sides]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
