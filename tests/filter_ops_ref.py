"""The numpy reference of a filter's bitmap and slot list (lantern_gpu.h "A FILTER'S LIFE CYCLE"): label membership, the three
word-wise operations, flatnonzero.  An allow-set is a bool array over the slots; the device's words are compared with `pack`."""
import numpy as np

OPS = ("and", "or", "andnot")
PATTERNS = ("nothing", "everything", "first", "last", "third", "half")


def words_for(n):
    """32-bit words of a device bitmap over n slots: whole multiples of 4"""
    return ((max(n, 1) + 31) // 32 + 3) // 4 * 4


def pack(allowed):
    """the device bitmap of an allow-set: bit s of word s // 32, zero from n on, words_for(n) words"""
    allowed = np.asarray(allowed, dtype=bool)
    bits = np.zeros(words_for(allowed.size) * 32, dtype=np.uint8)
    bits[: allowed.size] = allowed
    return np.packbits(bits, bitorder="little").view(np.uint32)


def slots(allowed):
    """the allowed slots, ascending"""
    return np.flatnonzero(np.asarray(allowed, dtype=bool)).astype(np.uint32)


def from_labels(slot_labels, labels, skip_deleted=False):
    """allowed iff the slot's label is among `labels` (and, skip_deleted, is not 0)"""
    slot_labels = np.asarray(slot_labels, dtype=np.uint64)
    a = np.isin(slot_labels, np.asarray(labels, dtype=np.uint64))
    return a & (slot_labels != 0) if skip_deleted else a


def combine(a, b, op):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    return {"and": a & b, "or": a | b, "andnot": a & ~b}[op]


def extend(old, slot_labels, labels=(), all_new=False, skip_deleted=False):
    """`old` (over the first old.size slots) brought to slot_labels.size slots: the old bits as they are; a new slot by its label"""
    slot_labels = np.asarray(slot_labels, dtype=np.uint64)
    new = np.ones(slot_labels.size, dtype=bool) if all_new else from_labels(slot_labels, labels)
    if skip_deleted:
        new &= slot_labels != 0
    new[: old.size] = old
    return new


def pattern(name, n, seed=0):
    a = np.zeros(n, dtype=bool)
    if name == "everything":
        a[:] = True
    elif name == "first":
        a[0] = True
    elif name == "last":
        a[n - 1] = True
    elif name == "third":
        a[::3] = True
    elif name == "half":
        a = np.random.default_rng(1000 * seed + n).random(n) < 0.5
    else:
        assert name == "nothing", name
    return a
