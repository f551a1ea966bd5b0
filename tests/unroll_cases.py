"""Cases and the reference of tests/test_unroll_edges.py: gf_history_unroll at the edges of its index arithmetic.

The reference is the definition, in numpy: ``out[n] = ring[n, [(k + j) % H for j in range(H)], :].reshape(H * O)``.  A ring holds
distinct int32 bit patterns (flat index plus an offset) that the kernel sees as float32, with a handful of NaN payloads, -0.0, a
denormal and inf among them; every comparison is on the int32 view, so a misplaced element or a canonicalised NaN shows.

Constants of csrc/gf_unroll.hip that the case groups are built around (restated, not imported: a change there must be met by a change
here)."""
import numpy as np

CHUNK = 2048                 # gf_unroll.hip: kUnrollChunk = 256 lanes x 2 units x 4 floats per workgroup
STREAM_BYTES = 64 << 20      # gf_unroll.hip: kStreamBytes; the launch streams when 4*N*O*H*(3 with out2, else 2), summed over its gathers, is >= this
RANGE_LIMIT = 1 << 17        # gf_unroll.hip: unroll_prep refuses O*H >= 2^17 (the exact range of the multiply-shift divisions)
EC_SPAN = 2056               # gf_unroll.hip: UnrollMap.src is asked for ec <= c0 + 4*511 + 3 with c0 <= O*H - 1, so ec < O*H + 2 056

GF_E_NULL, GF_E_RANGE, GF_E_UNSUPPORTED = -1, -2, -5

BASE_BITS = 0x3F000000       # flat index + this: distinct normal floats in [0.5, 2) for rings below 2^24 elements
SPECIALS = (0x7FC01234, 0xFFA00001, 0x7F800001, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000)   # quiet / signalling NaN payloads, -0.0, denormal, +-inf


def make_ring(n, O, H):
    """[n, H, O] int32 bit patterns, all distinct."""
    total = n * H * O
    assert total < (1 << 24)
    ring = np.arange(total, dtype=np.int64) + BASE_BITS
    at = sorted({0, total - 1, total // 2, total // 3, (2 * total) // 3, min(total - 1, O), max(0, total - O - 1)})
    for i, e in enumerate(at):
        ring[e] = SPECIALS[i % len(SPECIALS)] + (i // len(SPECIALS))   # (still distinct from each other and from the plain ones)
    return ring.astype(np.uint32).view(np.int32).reshape(n, H, O)


def want(ring, k):
    """The restatement: newest frame (slot k) first."""
    n, H, O = ring.shape
    return ring[:, [(k + j) % H for j in range(H)], :].reshape(n, H * O)


def streams(*gathers):
    """The streaming rule for a launch of these (n, O, H, with_out2) gathers."""
    return sum(4 * n * O * H * (3 if two else 2) for n, O, H, two in gathers) >= STREAM_BYTES


def slots_all(H):
    return list(range(1, H + 1))


def slots_few(H):
    return sorted({s for s in (1, 2, H // 2 + 1, H) if 1 <= s <= H})


# ---- case groups: (n, O, H) -------------------------------------------------------------------------------------------------------
NARROW = [(n, O, H) for O in (1, 2, 3) for H in (1, 2, 3, 4, 5, 7) for n in (1, 2, 3, 5)]      # total & 3 takes all four values; units across rows
NARROW_CHUNK = [(2047, 1, 1), (683, 3, 1), (512, 4, 1)]                                           # 2 047, 2 049 and 2 048 floats: around one chunk
assert [n * O * H for n, O, H in NARROW_CHUNK] == [CHUNK - 1, CHUNK + 1, CHUNK]
assert {(n * O * H) & 3 for n, O, H in NARROW} == {0, 1, 2, 3} and any(O * H < 4 and n == 1 for n, O, H in NARROW)

WIDE_SMALL = [(n, O, H) for O in (4, 5, 6, 7) for H in (1, 2, 3) for n in (1, 3, 65)]            # every lead of 1, 2, 3; the unit across the row edge
LONG_ROWS = [(3, 1024, 3), (5, 310, 7), (9, 45, 50)]                                               # O*H = 3 072, 2 170, 2 250 > CHUNK: c0 up to O*H - 1
assert all(O * H > CHUNK for _n, O, H in LONG_ROWS)

RANGE_EDGE = [(3, 131071, 1), (2, 1, 131071), (3, 1024, 127), (3, 4369, 30)]                     # O*H = 131 071, 131 071, 130 048, 131 070
assert all(RANGE_LIMIT - 1024 <= O * H < RANGE_LIMIT for _n, O, H in RANGE_EDGE)
RANGE_REFUSED = [(131072, 1), (1, 131072), (1024, 128)]                                           # (O, H) with O*H = 2^17
assert all(O * H == RANGE_LIMIT for O, H in RANGE_REFUSED)

RING_OFFSETS = [((70, 62, 5), 1), ((130, 16, 5), 2), ((33, 7, 6), 3)]                            # ring starts 4, 8, 12 bytes past a 16-byte boundary

# (n, O, H, with_out2, streams): each pair differs in one thing only
STREAMING = [
    (18041, 62, 5, True, True), (18041, 62, 5, False, False), (18040, 62, 5, True, False),
    (1398102, 3, 2, False, True), (1398101, 3, 2, False, False),
    (93207, 45, 2, False, True), (93206, 45, 2, False, False),
]
assert all(streams((n, O, H, two)) == s for n, O, H, two, s in STREAMING)
PAIR_STREAMING = [(9021, True), (9020, False)]                                                     # two (n, 62, 5) gathers with out2 each
assert all(not streams((n, 62, 5, True)) and streams((n, 62, 5, True), (n, 62, 5, True)) == s for n, s in PAIR_STREAMING)


# ---- the two multiply-shift divisions of UnrollMap.src ----------------------------------------------------------------------------
def magic(d):
    """ceil(2^40 / d), as unroll_consts computes it."""
    d = np.asarray(d, dtype=np.uint64)
    return ((np.uint64(1) << np.uint64(40)) + d - np.uint64(1)) // d


def mulshift_div(i, d):
    """i / d as the kernel forms it: (uint32 i * ceil(2^40 / d)) >> 40 in 64 bits."""
    return (np.asarray(i, dtype=np.uint64) * magic(d)) >> np.uint64(40)


def multiples_up_to(limit):
    """(d, k*d) for every d in [1, 2^17) and every k >= 1 with k*d <= limit[d]."""
    d = np.arange(1, RANGE_LIMIT, dtype=np.int64)
    counts = limit(d) // d
    dd = np.repeat(d, counts)
    first = np.cumsum(counts) - counts
    k = np.arange(dd.size, dtype=np.int64) - np.repeat(first, counts) + 1
    return dd, k * dd
