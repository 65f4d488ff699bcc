"""CPU restatement of lantern_gpu_compact_deleted's renumbering (include/lantern_gpu.h "Deleting rows"), written from the
definition and not from the C++: live slot s moves to the number of live slots below it, lists go through that map in stored order,
upper_off is the exclusive prefix sum of the levels of the new slots."""
import numpy as np

EMPTY = 0xFFFFFFFF


def plan(labels, levels):
    """(slot_map [n], upper_off_new [live], live, upper_blocks)"""
    labels, levels = np.asarray(labels, dtype=np.uint64), np.asarray(levels, dtype=np.uint8)
    live = labels != 0
    slot_map = np.where(live, np.cumsum(live) - live, EMPTY).astype(np.uint32)
    lv = levels[live].astype(np.int64)
    return slot_map, (np.cumsum(lv) - lv).astype(np.uint32), int(live.sum()), int(lv.sum())


def compact(graph, rows=None):
    """The compacted form of an exported graph no live list of which names a tombstone (the state after an unlink).  Returns
    (graph, rows of the live slots or None, slot_map)."""
    labels, levels = graph["labels"], graph["levels"]
    slot_map, upper_off, live, blocks = plan(labels, levels)
    keep = np.flatnonzero(labels != 0)

    def through(lists):
        out, named = lists.copy(), lists != EMPTY
        out[named] = slot_map[lists[named]]
        assert not (out[named] == EMPTY).any(), "a live list names a tombstone"
        return out

    M = graph["nbr0"].shape[1] // 2
    upper = np.full((blocks, M), EMPTY, dtype=np.uint32)
    for j, s in enumerate(keep):
        L, at = int(levels[s]), int(graph["upper_off"][s])
        if L:
            upper[upper_off[j]:upper_off[j] + L] = through(graph["upper_nbr"][at:at + L])
    out = {
        "levels": levels[keep].copy(), "labels": labels[keep].copy(), "nbr0": through(graph["nbr0"][keep]), "upper_off": upper_off, "upper_nbr": upper,
        "entry_slot": int(slot_map[graph["entry_slot"]]) if live else EMPTY, "max_level": int(graph["max_level"]) if live else -1,
    }
    return out, (None if rows is None else np.ascontiguousarray(np.asarray(rows)[keep])), slot_map
