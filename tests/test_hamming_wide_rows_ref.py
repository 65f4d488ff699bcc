"""Bit rows of 257 .. 2000 words (Lantern's cap: 2000 x 32 bits, 500 chunks of 16 bytes), without a device.
tests/test_gpu_hamming_wide_rows.py holds every kernel that reads such rows to the oracle, bit for bit; here the oracle itself is held
to an independent reference at these widths: "hamming" to numpy popcounts (integer equality under both summation modes, and the
(distance, slot) order of the brute force), "cos_b1" -- the cosine of the {0, 1} vectors, what a quantization = "b1" cosine index
computes -- to float64 with a tolerance derived from its five f32 roundings, and to its zero-norm rules."""
import numpy as np
import pytest

# 257: the first width past 64 chunks of four words; 1024 / 1025: the last width at which sixteen query rows fit 64 KB of LDS and the first
# word past it; 1792 / 1793: seven load steps of 64 lanes and the first word of the eighth; 2000: the cap
WIDE = [257, 1024, 1025, 1792, 1793, 2000]
NA, NB = 7, 33
COS_B1_TOL = 6 * 2.0 ** -24


def popcounts(queries, rows):
    """[nq][n] int64: np.unpackbits of the XOR, summed in int64"""
    return np.array([[int(np.unpackbits((q ^ r).view(np.uint8)).sum(dtype=np.int64)) for r in rows] for q in queries], dtype=np.int64)


def bit_rows(words):
    """(rows, queries): random words; then duplicates, a complement (every bit differs), one-bit neighbours and zero / all-ones rows, so
    that the brute force has ties for the slot to decide and the distances reach 0 and 32 x words"""
    rng = np.random.default_rng(words)
    rows = rng.integers(0, 2 ** 32, size=(NB, words), dtype=np.uint32)
    queries = rng.integers(0, 2 ** 32, size=(NA, words), dtype=np.uint32)
    rows[20] = rows[3]
    rows[21] = rows[3]
    rows[22] = ~rows[3]
    rows[23] = rows[3]
    rows[23, words - 1] ^= np.uint32(1 << 31)  # the last bit of the last word
    rows[24] = rows[3]
    rows[24, 0] ^= np.uint32(1)
    rows[25] = 0
    rows[26] = 0xFFFFFFFF
    queries[0] = rows[3]
    queries[1] = 0
    queries[2] = 0xFFFFFFFF
    return rows, queries


@pytest.mark.parametrize("words", WIDE)
def test_oracle_hamming_is_the_numpy_popcount(oracle, words):
    rows, queries = bit_rows(words)
    ref = popcounts(queries, rows)
    assert ref.min() == 0 and ref.max() == 32 * words and 32 * words < 2 ** 24  # (every distance is an integer an f32 holds exactly)
    order = np.array([np.lexsort((np.arange(NB), ref[i])) for i in range(NA)])  # by (distance, slot)
    assert any(len(set(r.tolist())) < NB for r in ref), "no tied distances: the slot order is not exercised"
    for mode in (oracle.SUM_WAVE64, oracle.SUM_SEQ):
        got = np.array([[oracle.distance(q, r, "hamming", mode) for r in rows] for q in queries], dtype=np.float64)
        assert np.array_equal(got, ref.astype(np.float64)), (words, mode, np.argwhere(got != ref)[:4].tolist())
        for k in (1, 10, NB):
            ids, dists = oracle.bruteforce(rows, queries, k, "hamming", mode)
            assert np.array_equal(ids.astype(np.int64), order[:, :k]), (words, mode, k)
            assert np.array_equal(dists.astype(np.int64), np.take_along_axis(ref, order[:, :k], axis=1)), (words, mode, k)
            assert np.array_equal(dists, np.floor(dists))


# ---- the cosine over bits --------------------------------------------------------------------------------------------------------
def cos_b1_rows(words):
    """rows of every density between empty and full, zero rows and zero queries among them"""
    rng = np.random.default_rng(100 + words)
    n, nq = 200, 100
    dens = rng.random(n + nq)
    bits = rng.random((n + nq, words * 32)) < dens[:, None]
    packed = np.packbits(bits, axis=1).view(np.uint32)
    rows, queries = packed[:n].copy(), packed[n:].copy()
    rows[[0, 17]] = 0
    rows[1] = 0xFFFFFFFF
    queries[[0, 5]] = 0
    queries[1] = 0xFFFFFFFF
    queries[2] = rows[40]
    return rows, queries


def cos_b1_float64(queries, rows):
    """1 - |a & b| / sqrt(|a| |b|) in float64; both zero: 0, one zero: 1"""
    pop = lambda x: np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).sum(axis=-1, dtype=np.int64)
    ab = np.array([[int(pop(q & r)) for r in rows] for q in queries], dtype=np.float64)
    a2, b2 = pop(queries).astype(np.float64)[:, None], pop(rows).astype(np.float64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = 1.0 - ab / np.sqrt(a2 * b2)
    d = np.where((a2 == 0) & (b2 == 0), 0.0, np.where((a2 == 0) | (b2 == 0), 1.0, d))
    return d, a2, b2


@pytest.mark.parametrize("words", [1, 33, 63])
def test_oracle_cos_b1_is_within_its_roundings_of_float64(oracle, words):
    """the f32 form rounds five times -- two square roots, their product, the quotient, the difference -- on quantities that are at most 1
    (|a & b| <= sqrt(|a| |b|), Cauchy-Schwarz; the popcounts themselves are integers below 2^24, exact in f32): at most 5 x 2^-24 plus
    second-order terms, held at 6 x 2^-24.  The largest error seen over 20 000 pairs at 63 words is 1.51 x 2^-24."""
    rows, queries = cos_b1_rows(words)
    ref, a2, b2 = cos_b1_float64(queries, rows)
    got = np.array([[oracle.distance(q, r, "cos_b1", oracle.SUM_SEQ) for r in rows] for q in queries], dtype=np.float32)
    assert not np.any(np.isnan(got))
    err = np.abs(got.astype(np.float64) - ref)
    assert err.max() <= COS_B1_TOL, (words, float(err.max() / 2.0 ** -24), np.unravel_index(err.argmax(), err.shape))
    # the zero-norm rules, to the bit
    both, one = (a2 == 0) & (b2 == 0), (a2 == 0) ^ (b2 == 0)
    assert both.sum() >= 4 and one.sum() >= 100
    assert np.all(got[both] == 0.0) and np.all(got[one] == 1.0)
    # the brute force returns these distances in (distance, slot) order
    ids, dists = oracle.bruteforce(rows, queries, 10, "cos_b1", oracle.SUM_SEQ)
    for i in range(queries.shape[0]):
        order = np.lexsort((np.arange(rows.shape[0]), got[i]))[:10]
        assert np.array_equal(ids[i].astype(np.int64), order) and np.array_equal(dists[i].view(np.uint32), got[i, order].view(np.uint32)), (words, i)
