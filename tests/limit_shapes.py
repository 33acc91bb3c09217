"""Shapes at the edges of the device eliminations' memory budgets, and the inputs that reach them cheaply.

The size formulas of the device sources are restated here in Python and the shape lists are derived from them; the
restatements are pinned to the library by tests/test_elimination_limits_host.py (the workspace size of rank_large.hip,
which fixes its block size too) and by tests/test_gpu_elimination_limits.py (the two LDS formulas, by which shapes the
library accepts).  Plain module: no GPU, no library."""
import numpy as np

from oracle import np_oracle as npo
from tests.gpu_util import np_matmul

MUL = npo.mul_table()
MAX_LDS = 160 * 1024  # kRrefMaxLds (rref.hpp)


# ---- rank_large.hip (rank_state.hpp) ---------------------------------------------------------------------------------
LARGE_MAX_K, LARGE_MAX_M, LARGE_MAX_B = 4096, 8192, 32
LARGE_STEP_FIXED = 8192 + 1024  # kLargeStepFixedBytes: the multiplier table, the small arrays


def large_row_dwords(k, m):
    return (k + 3) // 4 + (m + 3) // 4


def large_block(k, m):
    """Pieces per block; 0 outside the limits."""
    if k <= 0 or m <= 0 or k > LARGE_MAX_K or m > LARGE_MAX_M:
        return 0
    B = min(LARGE_MAX_B, (MAX_LDS - LARGE_STEP_FIXED) // (4 * large_row_dwords(k, m))) & ~3
    return B if B >= 4 else 0


def large_step_lds_bytes(k, m):
    return LARGE_STEP_FIXED + 4 * large_block(k, m) * large_row_dwords(k, m)


def _up4(v):
    return (v + 3) & ~3


def large_layout(k, m):
    """rank_state.hpp's large_layout, one object's state in dwords: the four state words, piv[k], St[m], Q[k][8],
    X[B][D], R[k][D], each array from a multiple of 4.  The offsets from the state words, D and the total."""
    D, B = large_row_dwords(k, m), large_block(k, m)
    piv = 4
    st = _up4(piv + k)
    q = _up4(st + m)
    x = q + k * (LARGE_MAX_B // 4)
    r = _up4(x + B * D)
    return dict(piv=piv, st=st, q=q, x=x, r=r, total=_up4(r + k * D), D=D)


def large_layout_total(k, m):
    return large_layout(k, m)["total"]


# ---- rank.hip --------------------------------------------------------------------------------------------------------
def rank_lds_bytes(k, m):
    kd, D = (k + 3) // 4, large_row_dwords(k, m)
    n = k * D + 2 * D + m * kd + m + 2 * k + kd
    return 8192 + 4 * _up4(n)


def rank_row_bytes(k, m):
    return 4 * large_row_dwords(k, m)


# ---- rref.hip (rref_kernels.hpp) -------------------------------------------------------------------------------------
def rref_row_dwords(k, m):
    d = (k + m + 3) // 4
    if d >= 64:
        return d
    p = 1
    while p < d:
        p <<= 1
    return p


def rref_lds_bytes(k, m):
    return 512 * 8 * 4 + (k + 1) * 4 * rref_row_dwords(k, m) + 4 * _up4(m)


def rref_lds_bytes_staged(k, m):
    return rref_lds_bytes(k, m) + ((k * m + 15) & ~15) + 2 * 4 * 64 * 4


def rref_row_bytes(k, m):
    return 4 * rref_row_dwords(k, m)


# ---- the narrow product (kernels.hip) --------------------------------------------------------------------------------
NARROW_MAX_LDS = 64 * 1024


def narrow_lds_bytes(n_in):
    return n_in * 4 * 20


def narrow_max_n_in():
    n = 1
    while narrow_lds_bytes(n + 1) <= NARROW_MAX_LDS:
        n += 1
    return n


# ---- the largest shapes a formula admits -----------------------------------------------------------------------------
def max_m(lds, k):
    """The largest m >= k with lds(k, m) <= MAX_LDS (every formula here is non-decreasing in m)."""
    m = k
    assert lds(k, m) <= MAX_LDS
    while lds(k, m + 1) <= MAX_LDS:
        m += 1
    return m


def max_k(lds, extra):
    """The largest k with lds(k, k + extra) <= MAX_LDS."""
    k = 1
    while lds(k + 1, k + 1 + extra) <= MAX_LDS:
        k += 1
    return k


def _edges(lds, fixed_k, extras):
    """[(fitting shape, first shape beyond it)]: one more piece where k is given, one more k where m - k is."""
    out = []
    for k in fixed_k:
        m = max_m(lds, k)
        out.append(((k, m), (k, m + 1)))
    for e in extras:
        k = max_k(lds, e)
        out.append(((k, k + e), (k + 1, k + 1 + e)))
    return out


RANK_EDGES = _edges(rank_lds_bytes, (16, 200, 64), (4,))            # rank mode 1, rank.hip
RREF_STAGED_EDGES = _edges(rref_lds_bytes_staged, (200, 130), (2,))  # rank mode 0, headers staged in LDS
RREF_EDGES = _edges(rref_lds_bytes, (130,), (2,))                   # rank mode 0, the matrix only; beyond: the host


def slack(lds, shape):
    return MAX_LDS - lds(*shape)


# ---- rank_large.hip off B = 32 ---------------------------------------------------------------------------------------
def _last_m_of_block(k, B):
    m = k
    while large_block(k, m + 1) >= B:
        m += 1
    return m


def _last_k_of_block(m, B):
    k = 1
    while large_block(k + 1, m) >= B:
        k += 1
    return k


_M32 = _last_m_of_block(40, 32)          # (40, 4792): the step kernel's 160 KiB to the byte at B = 32
_K16 = _last_k_of_block(LARGE_MAX_M, 16)  # (1472, 8192): the same at B = 16
# (k, m, B, objects)
LARGE_NARROW = [
    (40, _M32, 32, 2),
    (40, _M32 + 4, 28, 3),  # the next row width
    (40, 6000, 24, 2),
    (40, 7000, 20, 2),
    (40, LARGE_MAX_M, 16, 2),
    (_K16, LARGE_MAX_M, 16, 1),
    (_K16 + 4, LARGE_MAX_M, 12, 1),
    (LARGE_MAX_K, LARGE_MAX_M, 12, 1),  # the documented limit
    (LARGE_MAX_K - 1, 4837, 16, 1),     # k = 3 mod 4, m odd, a partial last block
    (LARGE_MAX_K, 4, 32, 1),            # m far below B, a long pivot scan
    (2000, 8, 32, 1),
]
LARGE_ZERO_SLACK = [(40, _M32), (_K16, LARGE_MAX_M)]
# the other rank_large shapes of tests/test_gpu_elimination_limits.py (the ragged decode, the shapes beyond rank.hip)
LARGE_OTHER = [(300, 304), (300, 310), (24, 67), (16, 20)] + [beyond for _, beyond in RANK_EDGES]


# ---- inputs ----------------------------------------------------------------------------------------------------------
def sparse_basis(rng, k, nb, nnz=6):
    """nb linearly independent vectors of about nnz nonzeros each, spread over all k columns.  Independent by
    construction: vector i is nonzero in column cols[i] and otherwise only in columns cols[j], j > i (a triangular
    system in the column order cols).  cols holds column 0, and column k - 1 last, so one vector is a multiple of the
    unit vector of column k - 1.  The vectors come back in a random order with that one at index 1 and one that is
    nonzero in column 0 at index 0."""
    nb = min(nb, k)
    assert k >= 2 and nb >= 2
    head = np.array([0] + [int(c) for c in rng.permutation(np.arange(1, k - 1))[:nb - 2]])
    rng.shuffle(head)
    cols = [int(c) for c in head] + [k - 1]
    basis = np.zeros((nb, k), np.uint8)
    for i, c in enumerate(cols):
        basis[i, c] = rng.integers(1, 256)
        later = cols[i + 1:]
        if later:
            pick = rng.choice(len(later), size=min(nnz - 1, len(later)), replace=False)
            basis[i, np.array(later)[pick]] = rng.integers(1, 256, pick.size)
    order = list(rng.permutation(nb))
    first = [int(np.nonzero(basis[:, 0])[0][0]), nb - 1]
    order = first + [int(i) for i in order if i not in first]
    return basis[order]


def trickle(rng, k, m, B, nb, last_at=None):
    """'Burst then trickle' coding vectors [m][k] over a sparse basis of nb vectors (sparse_basis).
    Pieces 0 .. burst - 1 (burst = min(2.5 blocks, nb - 8, m)) reveal one new basis vector each: the new vector plus a
    combination of 3 - 5 revealed ones.  The other basis vectors are revealed at random later pieces, the last one at
    piece last_at (default m - 1).  Every other piece is a combination of 3 - 5 revealed vectors, except a zero piece
    (burst + 1), an exact duplicate of piece 2 (burst + 3) and a scalar multiple of piece 1 two blocks later.
    The model's cost stays at seconds: few stored rows, few nonzero quotients per piece."""
    basis = sparse_basis(rng, k, nb)
    nb = basis.shape[0]
    last_at = m - 1 if last_at is None else last_at
    burst = max(1, min(2 * B + B // 2, nb - 8, m)) if m > 16 else min(nb, m)
    later = nb - burst
    reveal = {p: p for p in range(burst)}
    multiple_at = min(burst + 2 * B + 1, last_at - 1)
    if later > 0:
        free = np.setdiff1d(np.arange(burst + 8, last_at), [multiple_at])
        assert free.size >= later - 1, "no room for the trickle"
        at = np.sort(rng.choice(free, size=later - 1, replace=False))
        for i, p in enumerate(list(at) + [last_at]):
            reveal[int(p)] = burst + i
    co = np.zeros((m, k), np.uint8)
    known = 0
    for p in range(m):
        if known:
            pick = rng.choice(known, size=min(known, int(rng.integers(3, 6))), replace=False)
            co[p] = np_matmul(rng.integers(1, 256, (1, pick.size), dtype=np.uint8), basis[pick])[0]
        if p in reveal:
            co[p] ^= MUL[int(rng.integers(1, 256))][basis[reveal[p]]]
            known += 1
    if m > 16:
        co[burst + 1] = 0
        co[burst + 3] = co[2]
        co[multiple_at] = MUL[0x1D][co[1]]
    elif m >= 8:
        co[3] = 0
        co[m - 2] = co[0]
    elif m >= 4:
        co[m - 2] = co[0]
    return co


def planted(rng, k, m):
    """Dense vectors with planted duplicates, multiples and sums of earlier pieces."""
    co = rng.integers(0, 256, (m, k), dtype=np.uint8)
    for i in range(3, m, 7):
        a, b = rng.integers(0, i, 2)
        co[i] = [co[a], MUL[int(rng.integers(2, 256))][co[a]], co[a] ^ co[b]][i % 3]
    return co


def planted3(rng, k, m):
    """Dense vectors with three planted dependencies (a duplicate, a sum, a multiple): for shapes with m - k >= 4."""
    co = rng.integers(0, 256, (m, k), dtype=np.uint8)
    co[5] = co[2]
    co[m // 3] = co[7] ^ co[m // 5]
    co[2 * m // 3] = MUL[0x1D][co[m // 2]]
    return co


def combos(rng, basis, n):
    """n random GF(2^8) combinations of the basis rows."""
    return np_matmul(rng.integers(0, 256, (n, basis.shape[0]), dtype=np.uint8), basis)


def block_cases(rng, k, m, B):
    """Three objects of m pieces whose dependencies sit on the block boundaries (pieces B at a time):
    a  block 0 spans only 8 dimensions (a zero piece, a duplicate inside the block); block 1 is useless as a whole
       (c = 0: combinations, a multiple of an earlier block's piece, a zero piece); later blocks are dense;
    b  dense with a zero piece and a duplicate: rank k is reached inside block 0, ReceivedAllPieces from there on;
    c  block 0 spans 15 dimensions; block 1 starts with a multiple of an earlier block's piece, a new piece, the XOR
       of that new piece and a stored one, a zero piece, then dense pieces: rank k is reached inside block 1."""
    n = max(m, 3 * B)
    a = np.zeros((n, k), np.uint8)
    basis = rng.integers(0, 256, (8, k), dtype=np.uint8)
    a[:B] = combos(rng, basis, B)
    a[1] = 0
    a[5] = a[2]
    a[B:2 * B] = combos(rng, basis, B)
    a[B] = MUL[0x1D][a[3]]
    a[B + 2] = 0
    a[2 * B:] = rng.integers(0, 256, (n - 2 * B, k), dtype=np.uint8)
    b = rng.integers(0, 256, (n, k), dtype=np.uint8)
    b[3] = 0
    b[6] = b[4]
    b[B] = MUL[7][b[1]]
    c = np.zeros((n, k), np.uint8)
    c[:B] = combos(rng, rng.integers(0, 256, (15, k), dtype=np.uint8), B)
    c[B:] = rng.integers(0, 256, (n - B, k), dtype=np.uint8)
    c[B] = MUL[0x53][c[2]]
    c[B + 2] = c[3] ^ c[B + 1]
    c[B + 3] = 0
    return np.stack([a[:m], b[:m], c[:m]])


def blocks_of(statuses, B):
    return [statuses[i:i + B] for i in range(0, len(statuses), B)]


def pivot_columns(Cm):
    """The pivot columns of the model's reduced rows C [rank][k]."""
    return [int(np.nonzero(r)[0][0]) for r in Cm]
