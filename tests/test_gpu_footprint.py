"""GPU: every device call writes exactly the bytes it documents -- all of them, nothing else -- leaves its inputs alone
and leaves nothing behind for the next call on the context.

Every output sits in an arena (tests/footprint.py: seeded non-constant prefill, guards of >= 8 KiB and two row strides
on both sides, a mask of the documented footprint); after the call the whole arena is read back: every footprint byte
equals the numpy / oracle image, every other byte still holds its prefill, and the inputs are byte-identical to their
host copies.  tests/test_footprint_host.py shows on numpy images that the check reports a stray or missing byte.

Which parametrisation reaches which program (rlnc_amd/csrc/kernels.hip, launch_matmul; the perm, narrow, stream and
nibble kernels themselves are in perm_kernels.hpp, the ragged ones in ragged.hip, the scan kernel in elementwise.hip; on a device with unaligned vector
access, rlnc_device_unaligned_vector_access = 1, every operand counts as aligned, so the branch depends on the variant,
n_out, n_in and the width alone; elsewhere the misaligned cases run the same branches on realigned scratch rows):

  variants 6, 7, 8 (jump_variant):
    n_out 1, 2, 3, width >= 4096     launch_stream<n_out>: n_in = 1, 13 (<= kKC = 32) the stream3 form, which also takes
                                     the < 4 KiB tail (width 8211); n_in = 33 gf_matmul_stream_kernel + the perm tail
                                     (launch_nt<1 | 2 | 4>, variant perm) -- the "*x33x8211" cases
    n_out 4, 8                       bsj 1-wave program (gf_matmul_bsj_kernel<1>) + perm tail at width 8211
    n_out 9, 16                      bsj 2-wave program + perm tail
    n_out 17, 32                     4 waves: variants 7, 8 the shared-set program <4, true>, variant 6 <4>
    n_out 33, 64                     variant 8: the 8-wave program <8, true>, one 64-row tile; variants 6, 7: two 32-row
                                     tiles (33: the second with one live row)
    n_out 65                         variant 8: two 64-row tiles, the second with one live row (the all-zero row of
                                     object 0, the all-ones row of object 1)
    width < 4096                     n_out 5, 40 (or n_in <= 32): the narrow kernel (launch_narrow); n_out = 2 with
                                     n_in = 33: launch_nt<2>, the perm kernel over two chunks of kKC = 32 sources
  variant 0 (perm): the narrow kernel below 4096 bytes, else launch_nt<1 .. 32> by n_out; variant 1 (nibble): launch_nt
    at every width (launch_nt<2> for n_out > 2 below 4096 bytes).
  The A/B build's variants (2-5, 9) run the same grid through launch_matmul_ab.

The marker scan (decoder.rs:162-177) has three device homes; test_marker_scan_sweep reaches
    final_len_scan_kernel      decode_batch, decode_batch_device (k = 1: no payload-tail answer, so the scan kernel runs
                               over all 33 objects: workgroups of 16, 16 and 1) and Decoder.get_decoded_data_device
    ragged_final_len_kernel    decode_ragged (one 64-lane workgroup an object)
and test_marker_scan_in_tile[2049] reaches
    bsj_tile_scan              decode_batch_device at k = 4, L = 4096 over 2,049 objects (k % 4 == 0, one 4 KiB column
                               block, the 1-wave program, and >= 2,048 objects so that the small-object elimination
                               kernel runs and writes the product's address stream): the objects whose last 64 payload
                               bytes are zero are scanned by their tile, the others (rank < k among them) answered by
                               the elimination kernel from the payload tail.  With 33 objects the same payloads go to
                               final_len_scan_kernel.
"""
import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import np_oracle as npo
from oracle.oracle import OracleDecoder
from tests.footprint import Arena, assert_inputs_unchanged
from tests.gpu_util import MUL, np_matmul, variants

pytestmark = pytest.mark.gpu

DEFAULT_VARIANT = 8
OK, NOT_USEFUL, RECEIVED_ALL, NOT_ALL_YET, INVALID_FORMAT = 0, 8, 9, 10, 11
MARKER = 0x81


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    c = rlnc_amd.Context(0)
    yield c
    c.set_kernel_variant(DEFAULT_VARIANT, 0)
    c.set_decode_path(0)


def up(a):
    """A fresh device copy of a host array (the host array stays the test's own copy of the input)."""
    import torch

    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def ro(a):
    a.setflags(write=False)
    return a


# ======================================================================================================================
# a. rlnc_gf256_matmul through the raw descriptor
# ======================================================================================================================
N_OBJ = 2
PADS, OFFS, GAPS = (0, 16, 1), (0, 1, 15), (0, 48)


@dataclass(frozen=True)
class MatmulCase:
    n_out: int
    n_in: int
    W: int
    pad: int      # bytes after each output row: 0 (rows adjacent), 16, 1 (every later row misaligned)
    off: int      # the region's offset from a 16-byte boundary
    gap: int      # bytes between the objects beyond n_out x row stride
    hdr: bool = True    # a 64-byte header slot before each row receives the coefficient row
    zero: bool = False  # the whole coefficient matrix is zero: the output is overwritten with zeros

    @property
    def id(self):
        return (f"{self.n_out}x{self.n_in}x{self.W}-pad{self.pad}-off{self.off}-gap{self.gap}" +
                ("" if self.hdr else "-nohdr") + ("-zero" if self.zero else ""))


def _matmul_cases():
    shapes = [(n_out, n_in, W) for n_out in (1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65) for n_in in (1, 13)
              for W in (4096, 8192 + 16 + 3)]
    shapes += [(n_out, n_in, W) for W in (1, 15, 17, 4095) for n_out in (2, 5, 40) for n_in in (3, 33)]
    shapes += [(n_out, 33, 8192 + 16 + 3) for n_out in (1, 2, 3)]  # more than kKC sources: the perm tail
    # every pad, offset and gap value meets every branch: the four shapes of one n_out take all three pads and all
    # three offsets, paired differently from one n_out to the next, and the gap alternates against the width
    cases = [MatmulCase(n_out, n_in, W, PADS[i % 3], OFFS[(i + i // 4) % 3], GAPS[(i // 4 + i) % 2])
             for i, (n_out, n_in, W) in enumerate(shapes)]
    # no header slot: with pad 0 and no gap the rows and the objects are adjacent byte for byte
    cases += [MatmulCase(4, 13, 4096, 0, 0, 0, hdr=False), MatmulCase(33, 13, 8192 + 16 + 3, 0, 1, 0, hdr=False),
              MatmulCase(3, 13, 4096, 0, 15, 0, hdr=False), MatmulCase(5, 3, 15, 0, 0, 0, hdr=False),
              MatmulCase(65, 1, 4096, 1, 0, 0, hdr=False), MatmulCase(17, 13, 4096, 0, 0, 0, hdr=False)]
    cases += [MatmulCase(8, 13, 4096, 0, 1, 48, zero=True), MatmulCase(65, 13, 8192 + 16 + 3, 1, 0, 0, zero=True),
              MatmulCase(2, 3, 17, 16, 15, 0, zero=True), MatmulCase(3, 13, 8192 + 16 + 3, 0, 0, 48, zero=True),
              MatmulCase(3, 33, 8192 + 16 + 3, 1, 1, 0, zero=True), MatmulCase(32, 1, 4096, 0, 15, 0, zero=True)]
    return cases


MATMUL_CASES = _matmul_cases()


@functools.lru_cache(maxsize=None)
def matmul_operands(n_out, n_in, W, zero):
    """(coef [obj][n_out][n_in], inp [obj][n_in][W], product [obj][n_out][W]), computed once per shape and shared by
    every variant (read-only).  Object 0: row 0 all ones, the last row all zeros; object 1 the other way round (with
    one row: object 0 zeros, object 1 ones)."""
    rng = np.random.default_rng(n_out * 100003 + n_in * 1009 + W)
    coef = rng.integers(0, 256, (N_OBJ, n_out, n_in), dtype=np.uint8)
    coef[0, 0], coef[1, -1] = 1, 1
    coef[0, -1], coef[1, 0] = 0, 0
    if n_out == 1:
        coef[1, 0] = 1
    if zero:
        coef[:] = 0
    inp = rng.integers(0, 256, (N_OBJ, n_in, W), dtype=np.uint8)
    inp[:, 0, : min(W, 256)] = np.arange(min(W, 256), dtype=np.uint8)
    want = np.stack([np_matmul(coef[o], inp[o]) for o in range(N_OBJ)])
    return ro(coef), ro(inp), ro(want)


def run_matmul_case(ctx, c: MatmulCase, variant=DEFAULT_VARIANT):
    """One product on an arena, checked: the arena's image after the call."""
    from rlnc_amd._lib import MatmulDesc
    from rlnc_amd.errors import check

    coef, inp, want = matmul_operands(c.n_out, c.n_in, c.W, c.zero)
    slot = 64 if c.hdr else 0
    row = slot + c.W + c.pad
    obj = c.n_out * row + c.gap
    a = Arena(N_OBJ * obj, seed=c.n_out * 31 + c.n_in * 7 + c.W + c.pad + c.off, base_off=c.off, largest_row_stride=row)
    if c.hdr:
        a.operand("hdr", 0, N_OBJ, obj, c.n_out, row, c.n_in)
        a.expect("hdr", coef)
    a.operand("out", slot, N_OBJ, obj, c.n_out, row, c.W)
    a.expect("out", want)
    a.device()
    d_coef, d_inp = up(coef), up(inp)
    d = MatmulDesc(d_inp.data_ptr(), c.n_in * c.W, c.W, d_coef.data_ptr(), c.n_out * c.n_in, c.n_in,
                   a.ptr("out"), obj, row, a.ptr("hdr") if c.hdr else None, obj if c.hdr else 0, row if c.hdr else 0,
                   c.n_out, c.n_in, c.W, N_OBJ)
    ctx.set_kernel_variant(variant, 0)
    try:
        check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)
        after = a.after()
    finally:
        ctx.set_kernel_variant(DEFAULT_VARIANT, 0)
    a.check(after)
    assert_inputs_unchanged({"coef": (coef, d_coef), "in": (inp, d_inp)})
    return after


@pytest.mark.parametrize("variant", variants(8, 0, 1, 6, 7, 2, 3, 4, 5, 9))
@pytest.mark.parametrize("case", MATMUL_CASES, ids=lambda c: c.id)
def test_matmul_footprint(ctx, case, variant):
    run_matmul_case(ctx, case, variant)


# ======================================================================================================================
# b. the batch wrappers
# ======================================================================================================================
def _batch_lengths(k):
    return (8224 - k, 4096 + 17)  # k + L on a 16-byte boundary (8224), and off one (k = 5, 16, 33: 4118, 4129, 4146)


@functools.lru_cache(maxsize=None)
def encode_operands(k, L):
    n = {5: 8, 16: 20, 33: 40}[k]
    rng = np.random.default_rng(k * 131 + L)
    src = rng.integers(0, 256, (N_OBJ, k, L), dtype=np.uint8)
    co = rng.integers(0, 256, (N_OBJ, n, k), dtype=np.uint8)
    co[:, 1], co[:, -1] = 0, 1
    data = np.stack([np_matmul(co[o], src[o]) for o in range(N_OBJ)])
    return n, ro(src), ro(co), ro(data)


def pieces_arena(n, k, L, seed, hdr, data, n_obj=N_OBJ):
    """[obj][n][k + L] contiguous coded pieces: the header and the data parts as two operands; a part that the call
    does not write (None) stays outside the footprint, so it must keep its prefill."""
    full = k + L
    a = Arena(n_obj * n * full, seed=seed, largest_row_stride=full)
    if hdr is not None:
        a.operand("hdr", 0, n_obj, n * full, n, full, k)
        a.expect("hdr", hdr)
    if data is not None:
        a.operand("data", k, n_obj, n * full, n, full, L)
        a.expect("data", data)
    return a


def whole(a, n, k, L, n_obj=N_OBJ):
    full = k + L
    return a.region().view(n_obj, n, full)


@pytest.mark.parametrize("on16", [True, False], ids=["on16", "off16"])
@pytest.mark.parametrize("k", [5, 16, 33])
def test_encode_batch_footprints(ctx, k, on16):
    from rlnc_amd import batch

    L = _batch_lengths(k)[0 if on16 else 1]
    assert ((k + L) % 16 == 0) == on16
    n, src, co, data = encode_operands(k, L)
    d_src, d_co = up(src), up(co)
    inputs = {"src": (src, d_src), "coeffs": (co, d_co)}

    a = pieces_arena(n, k, L, 1, co, data)
    a.device()
    batch.encode_batch(d_src, d_co, whole(a, n, k, L), ctx)
    a.check_device()
    assert_inputs_unchanged(inputs)

    h = pieces_arena(n, k, L, 2, co, None)  # headers alone: every data byte keeps its prefill
    h.device()
    batch.encode_batch_headers(d_co, whole(h, n, k, L), ctx)
    h.check_device()
    assert_inputs_unchanged(inputs)

    d = pieces_arena(n, k, L, 3, None, data)  # data alone: every header byte keeps its prefill
    d.device()
    batch.encode_batch_data(d_src, d_co, whole(d, n, k, L), ctx)
    d.check_device()
    assert_inputs_unchanged(inputs)

    both = pieces_arena(n, k, L, 1, co, data)  # the two together == encode_batch (same seed: the same whole image)
    both.device()
    batch.encode_batch_headers(d_co, whole(both, n, k, L), ctx)
    batch.encode_batch_data(d_src, d_co, whole(both, n, k, L), ctx)
    after = both.after()
    both.check(after)
    assert np.array_equal(after, a.after())
    assert_inputs_unchanged(inputs)

    # the address stream written ahead into a plan buffer that sits in an arena of its own
    plan_bytes = batch.encode_plan_bytes(k, N_OBJ, n)
    pa = Arena(plan_bytes, seed=4)
    pa.device()
    plan = pa.region()
    p = pieces_arena(n, k, L, 5, None, data)
    p.device()
    batch.encode_batch_prepare(d_src, d_co, whole(p, n, k, L), plan, ctx)
    prepared = p.after()
    assert np.array_equal(prepared, p.fill), "the prepare wrote into the pieces"
    batch.encode_batch_data_planned(d_src, d_co, whole(p, n, k, L), plan, ctx)
    p.check_device()
    pa.check_guards(pa.after())
    assert_inputs_unchanged(inputs)


@pytest.mark.parametrize("on16", [True, False], ids=["on16", "off16"])
@pytest.mark.parametrize("k", [5, 16, 33])
def test_recode_batch_footprint(ctx, k, on16):
    from rlnc_amd import batch

    L = _batch_lengths(k)[0 if on16 else 1]
    n, src, co, data = encode_operands(k, L)
    pieces = np.concatenate([co, data], axis=2)
    count = {5: 3, 16: 12, 33: 36}[k]
    rng = np.random.default_rng(k + L)
    r = rng.integers(0, 256, (N_OBJ, count, n), dtype=np.uint8)
    r[:, 0], r[:, -1] = 0, 1
    want = np.stack([np_matmul(r[o], pieces[o]) for o in range(N_OBJ)])
    a = pieces_arena(count, k, L, 6, want[:, :, :k], want[:, :, k:])
    a.device()
    d_pieces, d_r = up(pieces), up(r)
    batch.recode_batch(d_pieces, d_r, whole(a, count, k, L), k, ctx)
    a.check_device()
    assert_inputs_unchanged({"pieces": (pieces, d_pieces), "r": (r, d_r)})


# ======================================================================================================================
# c. reference-mode decode: constructed objects whose ranks and statuses are known in advance
# ======================================================================================================================
@dataclass(frozen=True)
class DecodeObject:
    k: int
    m: int
    L: int
    pieces: np.ndarray        # [m][k + L]
    statuses: tuple           # planned status of each decode() call (the oracle confirms it)
    rank: int
    T: np.ndarray             # [k][m]: decoded rows = T x received data rows, rows >= rank zero
    decoded: np.ndarray       # [k][L]
    status: int               # get_decoded_data
    data_len: int             # 0 unless Ok


@functools.lru_cache(maxsize=None)
def decode_object(kind, k, m, L, seed=0):
    """kind "complete": k independent pieces, then m - k more (ReceivedAllPieces); "useless": two dependent pieces (a
    repeat and a sum of two earlier ones) in the middle of independent ones -- complete when m - 2 >= k, else rank
    m - 2; "deficient": k - 1 independent pieces, one of them repeated in the middle and at the end: rank k - 1.  The
    coding vectors are the rows of a lower-triangular matrix with a nonzero diagonal, in a fixed permutation."""
    rng = np.random.default_rng(k * 1000 + m * 10 + L + seed + sum(map(ord, kind)))
    tri = np.tril(rng.integers(1, 256, (k, k), dtype=np.uint8))
    basis = tri[[(i * 3 + 1) % k if k % 3 else (i * 5 + 1) % k for i in range(k)]]
    assert len({r.tobytes() for r in basis}) == k
    rows, plan = [], []
    if kind == "complete":
        for i in range(m):
            rows.append(basis[i % k])
            plan.append(OK if i < k else RECEIVED_ALL)
    elif kind == "useless":
        h = max(3, k // 2)
        nxt = 0
        for i in range(m):
            if i == h:
                rows.append(rows[0].copy())
            elif i == h + 1:
                rows.append(rows[1] ^ rows[2])
            else:
                rows.append(basis[nxt % k])
                nxt += 1
            independent = i not in (h, h + 1)
            plan.append(RECEIVED_ALL if plan.count(OK) == k else OK if independent else NOT_USEFUL)
    else:
        assert kind == "deficient"
        nxt = 0
        for i in range(m):
            if i == 2 or nxt == k - 1:
                rows.append(rows[i % 2].copy())
                plan.append(NOT_USEFUL)
            else:
                rows.append(basis[nxt])
                nxt += 1
                plan.append(OK)
    co = np.stack(rows)
    rank = plan.count(OK)
    if rank == k:
        src = npo.pad(rng.integers(0, 256, k * L - 3, dtype=np.uint8), k)
    else:
        src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    assert src.shape == (k, L)
    data = np_matmul(co, src)
    pieces = np.concatenate([co, data], axis=1)
    # the oracle on the pieces: statuses, rows, get_decoded_data; and on [coefficients | identity]: the same row
    # operations applied to unit vectors are T (the elimination reads the coefficient columns alone)
    od, ot = OracleDecoder(L, k), OracleDecoder(m, k)
    got = [od.decode(p) for p in pieces]
    assert got == plan, (kind, k, m, got, plan)
    assert [ot.decode(p) for p in np.concatenate([co, np.eye(m, dtype=np.uint8)], axis=1)] == plan
    T = np.zeros((k, m), np.uint8)
    T[:rank] = ot.matrix()[:, k:]
    decoded = np_matmul(T, data)
    assert np.array_equal(decoded[:rank], od.padded_payload()) and not decoded[rank:].any()
    st, payload = od.get_decoded_data()
    assert st == (OK if rank == k else NOT_ALL_YET)
    if rank == k:
        assert np.array_equal(decoded, src) and payload.size == k * L - 3
    return DecodeObject(k, m, L, ro(pieces), tuple(plan), rank, ro(T), ro(decoded), st, payload.size if st == OK else 0)


DECODE_SHAPES = [(5, 7), (16, 16), (33, 40)]
DECODE_LENGTHS = [48, 4096 + 17]
EXTRA_PIECES = 3  # the pieces are passed as a [:, :m] view of m + 3: the object stride exceeds m x (k + L)


def decode_batch_objects(k, m, L):
    return [decode_object(kind, k, m, L) for kind in ("complete", "useless", "deficient")]


class DecodeOutputs:
    """Arenas for the outputs of the decode calls over `objs` (uniform k, m, L)."""

    def __init__(self, objs, seed, *, decoded=True, T=False, pst=False, ost=True, dl=True, rank=False):
        import torch

        k, m, L, n = objs[0].k, objs[0].m, objs[0].L, len(objs)
        self.arenas = {}

        def make(name, on, region, args, values, s):
            if not on:
                return None
            a = Arena(region, seed=seed * 16 + s, largest_row_stride=args[4])
            a.operand(name, *args)
            a.expect(name, values)
            a.device()
            self.arenas[name] = a
            return a

        make("decoded", decoded, n * k * L, (0, n, k * L, k, L, L), np.stack([o.decoded for o in objs]), 1)
        make("T", T, n * k * m, (0, n, k * m, k, m, m), np.stack([o.T for o in objs]), 2)
        make("piece_status", pst, n * m * 4, (0, n, m * 4, m, 4, 4), np.array([o.statuses for o in objs], np.int32), 3)
        make("object_status", ost, n * 4, (0, 1, 0, n, 4, 4), np.array([o.status for o in objs], np.int32), 4)
        make("data_len", dl, n * 8, (0, 1, 0, n, 8, 8), np.array([o.data_len for o in objs], np.int64), 5)
        make("rank", rank, n * 4, (0, 1, 0, n, 4, 4), np.array([o.rank for o in objs], np.int32), 6)
        shapes = {"decoded": ((n, k, L), None), "T": ((n, k, m), None), "piece_status": ((n, m), torch.int32),
                  "object_status": ((n,), torch.int32), "data_len": ((n,), torch.int64), "rank": ((n,), torch.int32)}
        for name, a in self.arenas.items():
            setattr(self, name, a.tensor(name, *shapes[name]))

    def check(self):
        for a in self.arenas.values():
            a.check_device()


def upload_pieces(objs):
    """(host copy [obj][m + extra][k + L], device tensor, its [:, :m] view): the extra pieces are random bytes."""
    k, m, L = objs[0].k, objs[0].m, objs[0].L
    rng = np.random.default_rng(k + m + L)
    allp = rng.integers(0, 256, (len(objs), m + EXTRA_PIECES, k + L), dtype=np.uint8)
    for i, o in enumerate(objs):
        allp[i, :m] = o.pieces
    t = up(allp)
    return allp, t, t[:, :m]


@pytest.mark.parametrize("path", [0, 1, 2, 5])
@pytest.mark.parametrize("L", DECODE_LENGTHS)
@pytest.mark.parametrize("k,m", DECODE_SHAPES)
def test_decode_footprints(ctx, k, m, L, path):
    """decode_batch_device, decode_batch_eliminate, decode_batch_apply, decode_batch_apply_prepare + _planned and the
    synchronous decode_batch over three objects: complete; useless pieces in the middle (complete where m - 2 >= k: at
    (16, 16) it ends at rank 14); rank-deficient.  (Decode path 1 moves the elimination of decode_batch to the host;
    the device calls take it as path 0.)"""
    from rlnc_amd import batch

    objs = decode_batch_objects(k, m, L)
    n = len(objs)
    allp, d_all, view = upload_pieces(objs)
    inputs = {"pieces": (allp, d_all)}
    ctx.set_decode_path(path)
    try:
        o1 = DecodeOutputs(objs, 1, pst=True)
        batch.decode_batch_device(view, k, o1.decoded, o1.piece_status, o1.object_status, o1.data_len, ctx)
        o1.check()
        assert_inputs_unchanged(inputs)

        o2 = DecodeOutputs(objs, 2, decoded=False, ost=False, dl=False, T=True, pst=True, rank=True)
        batch.decode_batch_eliminate(view, k, o2.T, o2.piece_status, o2.rank, ctx)
        o2.check()
        assert_inputs_unchanged(inputs)

        T = np.stack([o.T for o in objs])
        rank = np.array([o.rank for o in objs], np.int32)
        d_T, d_rank = up(T), up(rank)
        inputs.update(T=(T, d_T), rank=(rank, d_rank))
        o3 = DecodeOutputs(objs, 3)
        batch.decode_batch_apply(view, k, d_T, d_rank, o3.decoded, o3.object_status, o3.data_len, ctx)
        o3.check()
        assert_inputs_unchanged(inputs)

        o4 = DecodeOutputs(objs, 4)
        pa = Arena(batch.decode_apply_plan_bytes(k, m, n), seed=44)
        pa.device()
        plan = pa.region()
        batch.decode_batch_apply_prepare(view, k, d_T, o4.decoded, plan, ctx)
        for a in o4.arenas.values():
            assert np.array_equal(a.after(), a.fill), "the prepare wrote into an output"
        batch.decode_batch_apply_planned(view, k, d_T, d_rank, o4.decoded, o4.object_status, o4.data_len, plan, ctx)
        o4.check()
        pa.check_guards(pa.after())
        assert_inputs_unchanged(inputs)

        o5 = DecodeOutputs(objs, 5, ost=False, dl=False)
        pst, ost, dl = decode_batch_raw(ctx, view, k, o5.decoded)
        o5.check()
        assert pst.tolist() == [list(o.statuses) for o in objs]
        assert ost.tolist() == [o.status for o in objs] and dl.tolist() == [o.data_len for o in objs]
        assert_inputs_unchanged(inputs)
    finally:
        ctx.set_decode_path(0)


# ======================================================================================================================
# d. ragged calls: four objects of different wave classes, outputs packed back to back in one arena
# ======================================================================================================================
RAGGED_ROWS = (5, 12, 20, 40)          # output rows: the 1-, 2-, 4- and 8-wave programs
RAGGED_L = (4096 + 17, 4096, 48, 8192 + 16)


def packed_arena(shapes, pad, seed):
    """Objects of (rows, width) at row stride width + pad, one right after the other: operand "o<i>" each."""
    offs, at = [], 0
    for rows, width in shapes:
        offs.append(at)
        at += (rows - 1) * (width + pad) + width  # the next object starts right behind the last row's last byte
    a = Arena(at, seed=seed, base_off=seed % 16, largest_row_stride=max(w for _, w in shapes) + pad)
    for i, ((rows, width), off) in enumerate(zip(shapes, offs)):
        a.operand(f"o{i}", off, 1, 0, rows, width + pad, width)
    return a


@pytest.mark.parametrize("pad", [1, 16])
def test_encode_ragged_footprint(ctx, pad):
    from rlnc_amd import batch

    rng = np.random.default_rng(40 + pad)
    ks = (7, 16, 33, 12)
    hosts = []
    for k, L, n in zip(ks, RAGGED_L, RAGGED_ROWS):
        src = rng.integers(0, 256, (k, L), dtype=np.uint8)
        co = rng.integers(0, 256, (n, k), dtype=np.uint8)
        co[0], co[-1] = 0, 1
        hosts.append((src, co))
    a = packed_arena([(n, k + L) for k, L, n in zip(ks, RAGGED_L, RAGGED_ROWS)], pad, 3 + pad)
    for i, (src, co) in enumerate(hosts):
        a.expect(f"o{i}", np.concatenate([co, np_matmul(co, src)], axis=1))
    a.device()
    devs = [(up(src), up(co)) for src, co in hosts]
    batch.encode_ragged([(s, c, a.rows(f"o{i}")) for i, (s, c) in enumerate(devs)], ctx)
    a.check_device()
    assert_inputs_unchanged({f"{nm}{i}": (h, d) for i, (hs, ds) in enumerate(zip(hosts, devs))
                             for nm, h, d in (("src", hs[0], ds[0]), ("coeffs", hs[1], ds[1]))})


@pytest.mark.parametrize("pad", [1, 16])
def test_recode_ragged_footprint(ctx, pad):
    from rlnc_amd import batch

    rng = np.random.default_rng(50 + pad)
    ks = (7, 16, 33, 12)
    ns = (9, 16, 40, 3)
    hosts = []
    for k, L, n, count in zip(ks, RAGGED_L, ns, RAGGED_ROWS):
        stride = k + L + pad
        buf = rng.integers(0, 256, (n, stride), dtype=np.uint8)  # received pieces at a padded row stride
        r = rng.integers(0, 256, (count, n), dtype=np.uint8)
        r[0], r[-1] = 0, 1
        hosts.append((buf, r, k))
    a = packed_arena([(count, k + L) for k, L, count in zip(ks, RAGGED_L, RAGGED_ROWS)], pad, 5 + pad)
    for i, (buf, r, k) in enumerate(hosts):
        a.expect(f"o{i}", np_matmul(r, buf[:, : buf.shape[1] - pad]))
    a.device()
    devs = [(up(buf), up(r)) for buf, r, _ in hosts]
    batch.recode_ragged([(b[:, : b.shape[1] - pad], r, a.rows(f"o{i}"), hosts[i][2]) for i, (b, r) in enumerate(devs)],
                        ctx)
    a.check_device()
    assert_inputs_unchanged({f"{nm}{i}": (h, d) for i, (hs, ds) in enumerate(zip(hosts, devs))
                             for nm, h, d in (("pieces", hs[0], ds[0]), ("r", hs[1], ds[1]))})


def decode_batch_raw(ctx, view, k, decoded):
    """rlnc_decode_batch with host status arrays that are prefilled, not zeroed (batch.decode_batch hands the library
    np.zeros): an unwritten status or length keeps a value no call returns."""
    from rlnc_amd.errors import check

    nobj, m, full = view.shape
    ctx.use_torch_stream()
    ps = np.full((nobj, m), -0x55, np.int32)
    os_ = np.full(nobj, -0x55, np.int32)
    dl = np.full(nobj, 0xAAAAAAAAAAAAAAAA, np.uint64)
    check(ctx.lib.rlnc_decode_batch(ctx.h, C.c_void_p(view.data_ptr()), view.stride(0), k, full - k, m, nobj,
                                    C.c_void_p(decoded.data_ptr()), ps.ctypes.data_as(C.POINTER(C.c_int32)),
                                    os_.ctypes.data_as(C.POINTER(C.c_int32)), dl.ctypes.data_as(C.POINTER(C.c_uint64))),
          ctx.lib)
    return ps, os_, dl


def decode_ragged_raw(ctx, objs, pst, ost, dl):
    """rlnc_decode_ragged with caller-owned status arrays: objs = (pieces ptr, row stride, decoded ptr, k, L, m)."""
    from rlnc_amd._lib import DecodeObjDesc
    from rlnc_amd.errors import check

    ctx.use_torch_stream()
    arr = (DecodeObjDesc * len(objs))(*[DecodeObjDesc(*o) for o in objs])
    check(ctx.lib.rlnc_decode_ragged(ctx.h, arr, len(objs), C.c_void_p(pst.data_ptr()), C.c_void_p(ost.data_ptr()),
                                     C.c_void_p(dl.data_ptr())), ctx.lib)


@pytest.mark.parametrize("pad", [1, 16])
def test_decode_ragged_footprint(ctx, pad):
    """Four objects (1-, 2-, 4- and 8-wave products; complete, useless pieces, deficient, complete), their decoded rows
    packed back to back; the received pieces sit at a row stride of k + L + pad."""
    import torch

    objs = [decode_object("complete", 5, 7, 4096 + 17), decode_object("useless", 12, 16, 4096),
            decode_object("deficient", 20, 24, 48), decode_object("complete", 40, 44, 8192 + 16)]
    rng = np.random.default_rng(60 + pad)
    bufs = []
    for o in objs:
        b = rng.integers(0, 256, (o.m, o.k + o.L + pad), dtype=np.uint8)
        b[:, : o.k + o.L] = o.pieces
        bufs.append(b)
    d_bufs = [up(b) for b in bufs]
    # decoded [k][L] is contiguous per object (the descriptor has no stride for it): objects back to back
    a = packed_arena([(o.k, o.L) for o in objs], 0, 7 + pad)
    for i, o in enumerate(objs):
        a.expect(f"o{i}", o.decoded)
    a.device()
    total_m = sum(o.m for o in objs)
    n = len(objs)
    st = {}
    for s, (name, count, width, vals) in enumerate([
            ("piece_status", total_m, 4, np.concatenate([np.array(o.statuses, np.int32) for o in objs])),
            ("object_status", n, 4, np.array([o.status for o in objs], np.int32)),
            ("data_len", n, 8, np.array([o.data_len for o in objs], np.int64))]):
        sa = Arena(count * width, seed=70 + s + pad)
        sa.operand(name, 0, 1, 0, count, width, width)
        sa.expect(name, vals)
        sa.device()
        st[name] = sa
    decode_ragged_raw(ctx, [(d_bufs[i].data_ptr(), o.k + o.L + pad, a.ptr(f"o{i}"), o.k, o.L, o.m)
                            for i, o in enumerate(objs)],
                      st["piece_status"].tensor("piece_status", (total_m,), torch.int32),
                      st["object_status"].tensor("object_status", (n,), torch.int32),
                      st["data_len"].tensor("data_len", (n,), torch.int64))
    a.check_device()
    for sa in st.values():
        sa.check_device()
    assert_inputs_unchanged({f"pieces{i}": (b, d) for i, (b, d) in enumerate(zip(bufs, d_bufs))})


# ======================================================================================================================
# e. the vector primitives on a sub-range
# ======================================================================================================================
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 4095, 4096, 4097])
def test_primitives_footprint(ctx, n):
    """Start offsets 0..15 x scalars {0, 1, 0x53}: the n bytes hold the result, the bytes on both sides and src do not
    change.  (Scalar 0 zero-fills / leaves dst alone, scalar 1 leaves the vector alone / plain XOR: the reference's
    early-outs -- a byte that the call leaves alone is expected to hold its prefill.)"""
    from rlnc_amd import batch

    rng = np.random.default_rng(n)
    for off in range(16):
        src_off = (off * 7 + 3) % 16
        src_buf = rng.integers(0, 256, n + 32, dtype=np.uint8)
        src = src_buf[src_off: src_off + n]
        d_src = up(src_buf)
        for c in (0, 1, 0x53):
            for op in ("mul", "add", "muladd"):
                a = Arena(n, seed=n * 64 + off * 4 + c % 3, base_off=off, largest_row_stride=n)
                a.operand("dst", 0, 1, 0, 1, 0, n)
                before = a.fill[a.start: a.end].copy()
                a.expect("dst", MUL[c][before] if op == "mul" else before ^ src if op == "add"
                         else before ^ MUL[c][src])
                a.device(seal=False)  # the in-place calls read dst: its prefill is part of the input
                dst = a.tensor("dst", (n,))
                if op == "mul":
                    batch.mul_vec_by_scalar(dst, c, ctx)
                elif op == "add":
                    batch.add_vectors(dst, d_src[src_off: src_off + n], ctx)
                else:
                    batch.mul_vec_by_scalar_then_add_into_vec(dst, d_src[src_off: src_off + n], c, ctx)
                a.check_device()
        assert_inputs_unchanged({"src": (src_buf, d_src)})


# ======================================================================================================================
# f. the object API's device outputs
# ======================================================================================================================
@pytest.mark.parametrize("k,size,pad", [(5, 20001, 1), (16, 4096 * 16 - 1, 16), (33, 33 * 4113 - 7, 0)])
def test_object_api_device_outputs(ctx, k, size, pad):
    from rlnc_amd.full import Decoder, Encoder, Recoder

    rng = np.random.default_rng(size)
    data = rng.integers(0, 256, size, dtype=np.uint8)
    src = npo.pad(data, k)
    L = src.shape[1]
    full = k + L
    n = k + 4
    co = np.tril(rng.integers(1, 256, (n, k), dtype=np.uint8))[::-1].copy()  # the last k rows: triangular, independent
    co[0] = 0
    enc = Encoder.new(data, k, ctx)
    a = Arena(n * (full + pad), seed=size + 1, base_off=pad % 16, largest_row_stride=full + pad)
    a.operand("pieces", 0, 1, 0, n, full + pad, full)
    pieces = np.concatenate([co, np_matmul(co, src)], axis=1)
    a.expect("pieces", pieces)
    a.device()
    d_co = up(co)
    enc.code_batch_device(d_co.data_ptr(), n, a.ptr("pieces"), full + pad)
    a.check_device()
    assert_inputs_unchanged({"coeffs": (co, d_co)})

    count = 9
    r = rng.integers(0, 256, (count, n), dtype=np.uint8)
    r[0], r[-1] = 0, 1
    rec = Recoder.new(pieces.reshape(-1), full, k, ctx)
    b = Arena(count * full, seed=size + 2, base_off=1, largest_row_stride=full)
    b.operand("recoded", 0, 1, 0, count, full, full)
    b.expect("recoded", np_matmul(r, pieces))
    b.device()
    d_r = up(r)
    rec.recode_batch_device(d_r.data_ptr(), count, b.ptr("recoded"))
    b.check_device()
    assert_inputs_unchanged({"r": (r, d_r)})

    dec = Decoder.new(L, k, ctx)
    for p in pieces[n - k:]:
        dec.decode(p)
    assert dec.is_already_decoded()
    cap = k * L + 4096 + 5  # out_cap larger than the data: the bytes past k x L keep their prefill
    c = Arena(cap, seed=size + 3, base_off=15, largest_row_stride=L)
    c.operand("decoded", 0, 1, 0, k, L, L)
    c.expect("decoded", src)
    c.device()
    assert dec.get_decoded_data_device(c.ptr("decoded"), cap) == size
    c.check_device()


# ======================================================================================================================
# g. call sequences on one context: nothing of one call is left behind for the next
# ======================================================================================================================
def run_encode_case(ctx, k, L):
    from rlnc_amd import batch

    n, src, co, data = encode_operands(k, L)
    a = pieces_arena(n, k, L, 9, co, data)
    a.device()
    d_src, d_co = up(src), up(co)
    batch.encode_batch(d_src, d_co, whole(a, n, k, L), ctx)
    after = a.after()
    a.check(after)
    assert_inputs_unchanged({"src": (src, d_src), "coeffs": (co, d_co)})
    return after


def run_decode_case(ctx, k, m, L):
    from rlnc_amd import batch

    objs = decode_batch_objects(k, m, L)
    allp, d_all, view = upload_pieces(objs)
    o = DecodeOutputs(objs, 9, pst=True)
    batch.decode_batch_device(view, k, o.decoded, o.piece_status, o.object_status, o.data_len, ctx)
    o.check()
    assert_inputs_unchanged({"pieces": (allp, d_all)})
    return np.concatenate([a.after() for a in o.arenas.values()])


W3 = 8192 + 16 + 3
SEQUENCE = [
    ("matmul", MatmulCase(65, 13, W3, 0, 1, 48)),      # large: two 64-row tiles, a long address stream
    ("matmul", MatmulCase(4, 13, 4096, 1, 0, 0)),      # small: one 8-row tile with four live rows behind it
    ("matmul", MatmulCase(33, 3, W3, 16, 15, 0)),      # 33 rows over fewer sources
    ("encode", (33, 4096 + 17)),
    ("decode", (33, 40, 4096 + 17)),
    ("matmul", MatmulCase(9, 1, 4096, 0, 0, 0)),       # 2-wave tile, 7 rows of padding in the stream
    ("decode", (5, 7, 48)),
    ("encode", (5, 4096 + 17)),
    ("matmul", MatmulCase(64, 13, W3, 1, 1, 48)),      # large again
    ("matmul", MatmulCase(17, 13, 4096, 0, 0, 0, hdr=False)),
    ("matmul", MatmulCase(65, 1, 4096, 16, 0, 0)),
]


def test_call_sequence_leaves_nothing_behind():
    """Large -> small -> large on one fresh context, every call under its full footprint check; the sequence replayed
    on the same context gives the same images (a stale address stream or workspace would change the second round)."""
    import rlnc_amd

    c = rlnc_amd.Context(0)
    try:
        rounds = []
        for _ in range(2):
            images = []
            for kind, arg in SEQUENCE:
                if kind == "matmul":
                    images.append(run_matmul_case(c, arg))
                elif kind == "encode":
                    images.append(run_encode_case(c, *arg))
                else:
                    images.append(run_decode_case(c, *arg))
            rounds.append(images)
        for i, (x, y) in enumerate(zip(*rounds)):
            assert np.array_equal(x, y), (i, SEQUENCE[i][0])
    finally:
        c.close()


# ======================================================================================================================
# h. the marker scan: the last nonzero byte on and around the 1 KiB chunk edges
# ======================================================================================================================
SCAN_OBJECTS = 33  # workgroups of 16, 16 and 1 objects in final_len_scan_kernel


def scan_positions(L):
    """Last-nonzero-byte positions (None: an all-zero payload), clipped to the payload."""
    raw = [None, 0, 1, 15, 16, 1022, 1023, 1024, 1025, L - 1025, L - 1024, L - 2, L - 1]
    return [None if p is None else min(max(p, 0), L - 1) for p in raw]


@functools.lru_cache(maxsize=None)
def scan_payloads(L):
    """33 k = 1 payloads and what OracleDecoder.get_decoded_data answers for each: (payloads [33][L], status, length).
    Object o takes position o % 13, so the objects of one workgroup end in different chunks; the last nonzero byte is
    0x81 in objects 0-12 and 26-32, 0x40 in objects 13-25: every position meets both."""
    rng = np.random.default_rng(L)
    pos = scan_positions(L)
    pay = np.zeros((SCAN_OBJECTS, L), np.uint8)
    status, length = [], []
    for o in range(SCAN_OBJECTS):
        p = pos[o % len(pos)]
        if p is not None:
            pay[o, :p] = rng.integers(0, 256, p, dtype=np.uint8)
            pay[o, p] = MARKER if (o // len(pos)) % 2 == 0 else 0x40
        od = OracleDecoder(L, 1)
        assert od.decode(np.concatenate([[1], pay[o]]).astype(np.uint8)) == OK
        st, data = od.get_decoded_data()
        status.append(st)
        length.append(data.size if st == OK else 0)
    assert OK in status and INVALID_FORMAT in status
    return ro(pay), tuple(status), tuple(length)


def status_arenas(status, length, seed):
    import torch

    n = len(status)
    sa, la = Arena(n * 4, seed=seed), Arena(n * 8, seed=seed + 1)
    sa.operand("object_status", 0, 1, 0, n, 4, 4)
    sa.expect("object_status", np.array(status, np.int32))
    la.operand("data_len", 0, 1, 0, n, 8, 8)
    la.expect("data_len", np.array(length, np.int64))
    sa.device()
    la.device()
    return sa, la, sa.tensor("object_status", (n,), torch.int32), la.tensor("data_len", (n,), torch.int64)


@pytest.mark.parametrize("L", [1023, 1024, 1025, 2055, 5000])
def test_marker_scan_sweep(ctx, L):
    """k = 1 pieces with coefficient 1 decode to exactly their payload: any payload reaches the scan kernels, through
    decode_batch, decode_batch_device (its payload base misaligned by 1), decode_ragged and
    Decoder.get_decoded_data_device."""
    import torch

    from rlnc_amd import batch
    from rlnc_amd.errors import RLNCError
    from rlnc_amd.full import Decoder

    pay, status, length = scan_payloads(L)
    n = SCAN_OBJECTS
    pieces = np.concatenate([np.ones((n, 1, 1), np.uint8), pay[:, None, :]], axis=2)
    d_pieces = up(pieces)
    inputs = {"pieces": (pieces, d_pieces)}

    def decoded_arena(seed, base_off):
        a = Arena(n * L, seed=seed, base_off=base_off, largest_row_stride=L)
        a.operand("decoded", 0, n, L, 1, 0, L)
        a.expect("decoded", pay)
        a.device()
        return a

    # decode_batch (host statuses, prefilled)
    a = decoded_arena(1, 0)
    pst, ost, dl = decode_batch_raw(ctx, d_pieces, 1, a.tensor("decoded", (n, 1, L)))
    a.check_device()
    assert ost.tolist() == list(status) and dl.tolist() == list(length) and not pst.any()
    assert_inputs_unchanged(inputs)

    # decode_batch_device, the decoded payloads (what the scan kernel reads) one byte off a 16-byte boundary
    a = decoded_arena(2, 1)
    sa, la, d_ost, d_dl = status_arenas(status, length, 20)
    pa = Arena(n * 4, seed=22)
    pa.operand("piece_status", 0, n, 4, 1, 0, 4)
    pa.expect("piece_status", np.zeros((n, 1), np.int32))
    pa.device()
    batch.decode_batch_device(d_pieces, 1, a.tensor("decoded", (n, 1, L)), pa.tensor("piece_status", (n, 1), torch.int32),
                              d_ost, d_dl, ctx)
    for x in (a, sa, la, pa):
        x.check_device()
    assert_inputs_unchanged(inputs)

    # decode_ragged: ragged_final_len_kernel
    a = decoded_arena(3, 0)
    sa, la, d_ost, d_dl = status_arenas(status, length, 30)
    pa = Arena(n * 4, seed=32)
    pa.operand("piece_status", 0, 1, 0, n, 4, 4)
    pa.expect("piece_status", np.zeros(n, np.int32))
    pa.device()
    op = a.operands["decoded"]
    decode_ragged_raw(ctx, [(d_pieces[o].data_ptr(), 1 + L, a.ptr("decoded") + o * op.obj_stride, 1, L, 1)
                            for o in range(n)], pa.tensor("piece_status", (n,), torch.int32), d_ost, d_dl)
    for x in (a, sa, la, pa):
        x.check_device()
    assert_inputs_unchanged(inputs)

    # the object API: one decoder per payload, the output with room to spare
    cap = L + 100
    a = Arena(n * cap, seed=4, base_off=1, largest_row_stride=cap)
    a.operand("decoded", 0, n, cap, 1, 0, L)
    a.expect("decoded", pay)
    a.device()
    for o in range(n):
        d = Decoder.new(L, 1, ctx)
        d.decode(pieces[o, 0])
        try:
            got = (OK, d.get_decoded_data_device(a.ptr("decoded") + o * cap, cap))
        except RLNCError as e:
            got = (e.code, 0)
        assert got == (status[o], length[o]), (o, got)
    a.check_device()


IN_TILE_MIN_OBJECTS = 2048  # rref_kernels.hpp kSmallMinObjects: from here on the small-object elimination kernel runs


@functools.lru_cache(maxsize=None)
def in_tile_objects(nobj):
    """k = 4, L = 4096 objects as (pieces, decoded rows, piece statuses, object status, data length), all from the
    oracle.  Four coding vectors that are a row permutation of a diagonal matrix; the payload ends at and around the row
    edges and around the last 64 bytes (a nonzero byte there is answered by the elimination from the payload tail; all
    zero there, the product's tile scans the object).  Every eleventh object is rank-deficient instead (decode_object:
    a repeated coding vector, rank 3): NotAllPiecesReceivedYet and length 0, written by the elimination itself."""
    k, L = 4, 4096
    n = k * L
    pos = [None, 0, 1, 4095, 4096, 4097, 8191, 8192, 3 * 4096 - 1, 3 * 4096, n - 4096, n - 66, n - 65, n - 64, n - 2,
           n - 1]
    rng = np.random.default_rng(4)
    objs = []
    for o in range(nobj):
        if o % 11 == 7:
            d = decode_object("deficient", k, k, L, seed=o % 5)
            objs.append((d.pieces, d.decoded, d.statuses, d.status, d.data_len))
            continue
        p = pos[o % len(pos)]
        src = np.zeros(n, np.uint8)
        if p is not None:
            src[:p] = rng.integers(0, 256, p, dtype=np.uint8)
            src[p] = MARKER if (o // len(pos)) % 2 == 0 else 0x40
        perm = [(i + 1 + o) % k for i in range(k)]
        co = np.zeros((k, k), np.uint8)
        co[np.arange(k), perm] = rng.integers(1, 256, k, dtype=np.uint8)
        pieces = np.concatenate([co, np_matmul(co, src.reshape(k, L))], axis=1)
        od = OracleDecoder(L, k)
        assert [od.decode(x) for x in pieces] == [OK] * k
        st, data = od.get_decoded_data()
        assert np.array_equal(od.padded_payload(), src.reshape(k, L))
        objs.append((pieces, src.reshape(k, L), (OK,) * k, st, data.size if st == OK else 0))
    return objs


@pytest.mark.parametrize("nobj", [33, IN_TILE_MIN_OBJECTS + 1])
def test_marker_scan_in_tile(ctx, nobj):
    """decode_batch_device at k = 4, L = 4096.  With 33 objects the blocked elimination runs and final_len_scan_kernel
    answers every object (four 1 KiB chunks a row).  From 2,048 objects on (here 2,049) the small-object elimination
    kernel answers the objects of rank < k and those with a nonzero byte in the last 64 payload bytes itself, and flags
    the rest for bsj_tile_scan in the product's 1-wave tile (launch_rref_one's small-object branch; batch.cpp, written &&
    want_tail).  That case moves 2 x 33 MiB, beyond the 2 MiB the other cases keep to: the kernel is not reached with
    fewer objects."""
    import torch

    from rlnc_amd import batch

    objs = in_tile_objects(nobj)
    k, L, n = 4, 4096, len(objs)
    assert {o[3] for o in objs} == {OK, NOT_ALL_YET, INVALID_FORMAT}
    pieces = np.stack([o[0] for o in objs])
    d_pieces = up(pieces)
    a = Arena(n * k * L, seed=8, largest_row_stride=L)
    a.operand("decoded", 0, n, k * L, k, L, L)
    a.expect("decoded", np.stack([o[1] for o in objs]))
    a.device()
    sa, la, d_ost, d_dl = status_arenas([o[3] for o in objs], [o[4] for o in objs], 80)
    pa = Arena(n * k * 4, seed=82)
    pa.operand("piece_status", 0, n, k * 4, k, 4, 4)
    pa.expect("piece_status", np.array([o[2] for o in objs], np.int32))
    pa.device()
    batch.decode_batch_device(d_pieces, k, a.tensor("decoded", (n, k, L)),
                              pa.tensor("piece_status", (n, k), torch.int32), d_ost, d_dl, ctx)
    for x in (a, sa, la, pa):
        x.check_device()
    assert_inputs_unchanged({"pieces": (pieces, d_pieces)})
