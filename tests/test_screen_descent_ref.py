"""The screened descent (walk.hpp greedy_descent<.., SCREEN>) restated in numpy: search_for_one_ over the upper levels of a graph the
oracle built and exported, once as it is and once with "skip the rows whose restated screen bound is strictly above the best distance
when the step starts" (the bound: tests/test_screen_bound_int.py, operation by operation).  Both must end at the same node after the
same number of listed rows D, and at the oracle's: the oracle searches the same graph with its level-0 lists emptied, so that its
answer is the descent's end node and its D the descent's plus the one evaluation that opens level 0.  CPU only;
tests/test_gpu_screen_descent.py holds the device to the oracle.

Why skipping is sound: a rejected row's f32 distance is strictly above the radius (checked here row by row), the scan takes a row
only if it is strictly below the running best, and the running best is never above the best at step start."""
import numpy as np
import pytest

from oracle import binding as oracle
from tests import test_screen_bound as l2
from tests import test_screen_bound_cos as cs
from tests import test_screen_bound_int as si

F32 = np.float32
EMPTY = 0xFFFFFFFF
N, D_, NQ, EFC, SEED = 1200, 80, 24, 32, 7


def upper_slots(M, n=N):
    """the slots of the two highest levels the level draw gives n rows (the oracle's own draw: binding.levels_for)"""
    lv = oracle.levels_for(SEED, 0, n, M)
    order = np.argsort(-lv, kind="stable")
    assert lv[order[2]] >= 1
    return int(order[1]), int(order[2])


def data(kind, M):
    rng = np.random.default_rng(900 + len(kind))
    g = rng.standard_normal((N, D_), dtype=F32)
    q = rng.standard_normal((NQ, D_), dtype=F32)
    if kind == "clustered":
        centres = rng.standard_normal((12, D_), dtype=F32) * 4
        g = (centres[rng.integers(0, 12, N)] + F32(0.5) * g).astype(F32)
        q = (centres[rng.integers(0, 12, NQ)] + F32(0.5) * q).astype(F32)
    elif kind == "mean3":
        g, q = (g + F32(3)).astype(F32), (q + F32(3)).astype(F32)
    elif kind == "duplicates":  # every row four times; half of the queries ARE rows: distances equal to the best, and 0
        g = np.tile(g[: N // 4], (4, 1))
        q[: NQ // 2] = g[rng.integers(0, N, NQ // 2)]
    elif kind == "special":  # a non-finite row and a zero row in the upper levels
        a, b = upper_slots(M)
        g[a, 3] = F32(np.inf)
        g[b] = 0
    return np.ascontiguousarray(g), np.ascontiguousarray(q)


def graph_of(metric, base, M):
    ix = oracle.OracleIndex(metric, base.shape[1], M=M, ef_construction=EFC, ef=64, seed=SEED, sum_mode=oracle.SUM_WAVE64)
    with np.errstate(all="ignore"):
        ix.add_many(np.arange(len(base), dtype=np.uint64) + 1, base)
    return ix.export_graph()


def oracle_descent(metric, base, g, M, queries):
    """(end node, D of the descent) per query: the oracle's search of the graph without level-0 lists"""
    bare = dict(g, nbr0=np.full_like(g["nbr0"], EMPTY))
    ora = oracle.OracleIndex.from_graph(metric, base, bare, M, EFC, 64, SEED, oracle.SUM_WAVE64)
    _, _, slots, D, E = ora.search_batch(queries, 1, 1)
    assert np.all(E == 1)
    return slots[:, 0].astype(np.int64), D.astype(np.int64) - 1


class Screen:
    """the restated test of one query against the rows of `base`: rejects(slot, radius)"""

    def __init__(self, metric, base, x):
        self.metric, self.base, self.x = metric, base, x
        self.chunks = (base.shape[1] + 3) // 4
        self.ra = cs.rooted_norm(x) if metric == "cos" else None
        self.st = si.Staged(x, metric, ra=self.ra)

    def rejects(self, slot, radius):
        y = self.base[slot]
        with np.errstate(**si.NP_QUIET):
            if self.metric == "l2sq":
                c, s, r = l2.screen_of(y)
                thr = si.l2_threshold(self.st, c, s, r, self.chunks)
            else:
                c, t, rho = cs.screen_of(y, cs.rooted_norm(y))
                thr = si.cos_threshold(self.st, c, t, rho, self.ra, self.chunks)
        return si.rejects(thr, radius)


def descent(metric, base, g, x, screen=None, seen=None):
    """search_for_one_ over levels (max_level, 0]: (end node, D, rows read in f32).  screen: skip what it rejects at the step's radius"""
    def dist(slot):
        with np.errstate(all="ignore"):
            return F32(oracle.distance(x, base[slot], metric, oracle.SUM_WAVE64))

    cur = int(g["entry_slot"])
    best = dist(cur)
    D = reads = 1
    for level in range(int(g["max_level"]), 0, -1):
        while True:
            lst = g["upper_nbr"][int(g["upper_off"][cur]) + level - 1]
            radius, changed = best, False
            for nb in lst:
                if nb == EMPTY:
                    break
                nb = int(nb)
                D += 1
                if seen is not None:
                    seen.add(nb)
                if screen is not None and screen.rejects(nb, radius):
                    d = dist(nb)
                    assert d > radius, (nb, float(d), float(radius))  # strictly above the radius: it could not have been taken
                    continue
                reads += 1
                d = dist(nb)
                if d < best:
                    best, cur, changed = d, nb, True
            if not changed:
                break
    return cur, D, reads


CASES = [("gaussian", 4), ("gaussian", 16), ("clustered", 4), ("mean3", 4), ("duplicates", 4), ("special", 4)]


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("kind,M", CASES)
def test_the_screened_descent_ends_where_the_oracle_s_does(kind, M, metric):
    base, queries = data(kind, M)
    g = graph_of(metric, base, M)
    assert g["max_level"] >= (2 if M == 16 else 3)
    want_end, want_D = oracle_descent(metric, base, g, M, queries)
    plain_reads = screened_reads = 0
    seen = set()
    for x, e, d_ in zip(queries, want_end, want_D):
        end0, D0, r0 = descent(metric, base, g, x)
        end1, D1, r1 = descent(metric, base, g, x, Screen(metric, base, x), seen)
        assert (end0, D0) == (int(e), int(d_)), (kind, M, metric, "the restatement without the screen is not the oracle's descent")
        assert (end1, D1) == (int(e), int(d_)), (kind, M, metric, "the screened descent left the oracle's")
        assert r0 == D0 and r1 <= r0
        plain_reads += r0
        screened_reads += r1
    print(f"{kind} M={M} {metric}: listed rows {plain_reads}, read in f32 with the screen {screened_reads}")
    if kind == "special":
        a, b = upper_slots(M)
        assert a in seen or b in seen, "no descent listed a special row"
    else:
        assert screened_reads < plain_reads  # the screen rejects at all


def test_queries_that_cannot_be_quantised_skip_nothing():
    base, queries = data("gaussian", 4)
    g = graph_of("l2sq", base, 4)
    bad = [np.zeros(D_, F32), queries[0].copy(), queries[1] * F32(1e25)]
    bad[1][5] = F32(np.nan)
    for metric in ("l2sq", "cos"):
        for x in bad[:2] if metric == "cos" else bad:
            end0, D0, r0 = descent(metric, base, g, x)
            end1, D1, r1 = descent(metric, base, g, x, Screen(metric, base, x))
            assert (end1, D1, r1) == (end0, D0, r0) and r1 == D1
