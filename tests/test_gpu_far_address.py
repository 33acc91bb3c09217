"""GPU: device calls on operands more than 4 GiB from their base -- object strides of FAR = 2^32 + delta, row strides
at and past 2^31 and 2^32, vectors that straddle byte 2^32 -- bit-exact against the numpy / oracle image.

Every operand is a window into one module-scoped arena of uninitialised device memory (tests/far_address.py: its size,
the guards, the prefill and why delta = 4096 + 16 / 4096 + 1 keeps a 32-bit-truncated offset inside the arena: object 1
would land delta bytes into object 0's window, which the check reports as object 0 damaged and object 1 unwritten).
Only the windows are uploaded and read back, a few MiB a test.  tests/test_far_address_host.py shows on numpy images
that the check reports exactly that.  Two objects unless stated, object 1 far.

Which test puts which operand far, and the program it reaches (rlnc_amd/csrc/kernels.hip launch_matmul; on a device with
unaligned vector access every operand counts as aligned, so the branch depends on the variant and the shape alone):

  call                        far operand                                  test
  rlnc_gf256_matmul           in_obj | out_obj | hdr_obj | coef_obj | all  test_matmul_far_object_stride[branch-far-variant]
      branch stream1          1 x 2 x 4096          launch_stream<1> (variants 8, 6); launch_nt<1> (variant 0)
      branch stream3-tail     3 x 2 x 4115          launch_stream<3>, the stream3 form with its < 4 KiB tail
      branch stream2-permtail 2 x 33 x 4115         gf_matmul_stream_kernel + the perm tail (launch_nt<2>)
      branch bsj1-permtail    4 x 2 x 4115          the 1-wave bit-sliced program + perm tail
      branch bsj2             9 x 2 x 4096          the 2-wave program
      branch bsj4             17 x 2 x 4096         4 waves: variant 8 the shared-set program, variant 6 the unshared
      branch bsj8             33 x 2 x 4096         variant 8 the 8-wave program; variant 6 two 32-row tiles
      branch persist          33 x 12 x 7 * 4096    gf_matmul_bsj_persist_kernel (set_persistent_tiles(2, 8)): 14 tiles on
                                                    8 workgroups, counter 3 owns tiles 6 and 7, the last column block of
                                                    object 0 and the first of object 1, so its claim wraps by in_wrap /
                                                    out_wrap (variant 8 only: the other variants run it as bsj8 / perm)
      branch narrow           5 x 3 x 17            launch_narrow
      branch perm33           2 x 33 x 100          launch_nt<2>, the perm kernel over two chunks of 32 sources
      all of these with delta odd, in and out     test_matmul_far_odd_stride (every operand counts as aligned here) and,
                                                    in a child process with RLNC_ASSUME_ALIGNED_ONLY=1,
                                                    test_realigned_far_forced: realign_rows_kernel around the product
                                                    (and test_stream_far at L = 4097: the compaction's single-byte move)
  rlnc_gf256_matmul           in_row = FAR (n_in 2, n_out 4)               test_matmul_far_row_stride[in_row-far]: not
                                                    bit-sliced (bsj_eligible refuses it), launch_nt<4> perm
                              in_row = 2^32 - 4096 (n_in 2, n_out 4)       [in_row-below-2^32]: the 1-wave program
                              out_row = 2^31 + delta (n_out 4)             [out_row-2^31]: the 1-wave program, rows at up to
                                                                           3 * 2^31 (one object near, the second 8 KiB on)
                              out_row = FAR (n_out 2)                      [out_row-far]: launch_stream<2> / perm 2-row tile
                              hdr_row = FAR (n_out 2), 2^31 + delta (4)    [hdr_row-far], [hdr_row-2^31]
  rlnc_gf256_sparse_matmul    in_obj | out_obj | hdr_obj | idx_obj | val_obj | all, in_row = FAR with rows 0 and 1
                                                    test_sparse_far[...], width 4115: the vector body and the byte tail
  decode_batch_eliminate / _apply / _device         pieces_obj_stride = FAR, decoded / T far in the arena
                                                    test_decode_far[mode-path-L]: rank mode 0 under paths 1, 2, 5, rank
                                                    mode 1 under paths 2, 7, 8; k = 8, m = 12, L = 4112 and 4097; object 0
                                                    has a useless piece, object 1 is rank deficient
  DecodeStream push (both forms), compact, deliver, apply, snapshot     pieces_obj_stride = FAR; decoded and T far
                                                    test_stream_far[form-L]
  rlnc_encode_ragged / _recode_ragged / _decode_ragged   object 1 past FAR; piece_row_stride = FAR (k = 2), src_row_stride
                                                    = FAR: test_ragged_far_objects, test_ragged_far_row_strides
  rlnc_encoder_from_device    row_stride = FAR (k = 2)                     test_object_api_far
  rlnc_encoder_code_batch_device, _code_sparse_batch_device   out_row_stride = FAR (n = 2)   test_object_api_far
  rlnc_pad_device             out_row_stride = FAR (k = 2)                 test_pad_device_far
  the three L1 calls          a vector of 4133 bytes across byte 2^32      test_primitives_straddle

Not covered: decode_batch's small-object elimination (>= 2,048 objects of k = 4 x 4 KiB) at a far object stride: 2,049
objects FAR apart span 9 TiB.  Object counts past 65,535 are in tests/test_gpu_object_counts.py, the stride contract of
the raw descriptors in tests/test_gpu_stride_contract.py.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.far_address import DELTA_ALIGNED, FAR, FAR_ODD, FarArena, FarLayout
from tests.gpu_util import MUL, np_matmul

pytestmark = pytest.mark.gpu

DEFAULT_VARIANT = 8
MiB = 1 << 20
# object 0's zones (the far object of each is FAR further on; the largest object is under 1 MiB)
Z_OUT, Z_HDR, Z_IN, Z_COEF, Z_AUX = 1 * MiB, 24 * MiB, 32 * MiB, 44 * MiB, 48 * MiB
N_OBJ = 2


def ro(a):
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    c = rlnc_amd.Context(0)
    yield c
    c.set_kernel_variant(DEFAULT_VARIANT, 0)
    c.set_persistent_tiles(0, 0)
    c.set_decode_path(0)


@pytest.fixture(scope="module")
def arena():
    import torch

    torch.cuda.empty_cache()  # what earlier modules left cached does not count against this one
    a = FarArena()
    yield a
    a.t = None
    torch.cuda.empty_cache()


# ======================================================================================================================
# the realigned form, in a child process of its own (first in the file: it runs before this process holds the arena)
# ======================================================================================================================
def test_realigned_far_forced():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RLNC_ASSUME_ALIGNED_ONLY="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--forced"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "forced realigned far ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ======================================================================================================================
# a. rlnc_gf256_matmul, object strides
# ======================================================================================================================
BRANCHES = {
    "stream1": (1, 2, 4096), "stream3-tail": (3, 2, 4096 + 19), "stream2-permtail": (2, 33, 4096 + 19),
    "bsj1-permtail": (4, 2, 4096 + 19), "bsj2": (9, 2, 4096), "bsj4": (17, 2, 4096), "bsj8": (33, 2, 4096),
    "persist": (33, 12, 7 * 4096), "narrow": (5, 3, 17), "perm33": (2, 33, 100),
}
FAR_SETS = {"in": ("in",), "out": ("out",), "hdr": ("hdr",), "coef": ("coef",), "all": ("in", "out", "hdr", "coef")}


@functools.lru_cache(maxsize=None)
def matmul_operands(n_out, n_in, W, n_obj=N_OBJ):
    """(coef [obj][n_out][n_in], inp [obj][n_in][W], product), computed once per shape, read-only.  Object 0's first
    row is all ones; the last object's last row all zeros where it has another (a far object whose only row is zero
    would not show from where its sources were read)."""
    rng = np.random.default_rng(n_out * 100003 + n_in * 1009 + W)
    coef = rng.integers(1, 256, (n_obj, n_out, n_in), dtype=np.uint8)
    coef[0, 0] = 1
    if n_out > 1:
        coef[-1, -1] = 0
    inp = rng.integers(0, 256, (n_obj, n_in, W), dtype=np.uint8)
    want = np.stack([np_matmul(coef[o], inp[o]) for o in range(n_obj)])
    return ro(coef), ro(inp), ro(want)


def matmul_call(ctx, d, variant, persist=False):
    from rlnc_amd.errors import check

    ctx.set_kernel_variant(variant, 0)
    if persist:
        ctx.set_persistent_tiles(2, 8)
    try:
        check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)
    finally:
        ctx.set_kernel_variant(DEFAULT_VARIANT, 0)
        ctx.set_persistent_tiles(0, 0)


def run_far_matmul(ctx, arena, shape, far_ops, variant, far=FAR, persist=False, pad=16, in_row=None, out_row=None,
                   hdr_row=None, obj_gap=48, n_obj=N_OBJ):
    """One product whose operands are windows of the arena.  An operand named in far_ops has the object stride `far`,
    the others their natural one; in_row / out_row / hdr_row replace a row stride (the object stride of that operand is
    then one row, W + pad or a header slot: the second object lies beside the first)."""
    from rlnc_amd._lib import MatmulDesc

    n_out, n_in, W = shape
    coef, inp, want = matmul_operands(n_out, n_in, W, n_obj)
    slot = 64 + (far & 1)
    rows = {"in": in_row or W + pad, "out": out_row or W + pad, "hdr": hdr_row or slot, "coef": n_in}
    count = {"in": n_in, "out": n_out, "hdr": n_out, "coef": n_out}
    objs = {}
    for name, given in (("in", in_row), ("out", out_row), ("hdr", hdr_row), ("coef", None)):
        if name in far_ops:
            objs[name] = far
        elif given:
            objs[name] = 2 * (W + pad if name != "hdr" else slot)
        else:
            objs[name] = count[name] * rows[name] + (obj_gap if name != "coef" else 0)
    lay = FarLayout(seed=n_out * 31 + n_in * 7 + W + variant + len(far_ops))
    lay.read("coef", Z_COEF, n_obj, objs["coef"], n_out, n_in, n_in, coef)
    lay.read("in", Z_IN + (far & 1), n_obj, objs["in"], n_in, rows["in"], W, inp)
    lay.write("hdr", Z_HDR, n_obj, objs["hdr"], n_out, rows["hdr"], n_in, coef)
    lay.write("out", Z_OUT + (far & 1), n_obj, objs["out"], n_out, rows["out"], W, want)
    lay.build()
    assert lay.moved_bytes < 16 * MiB
    d = MatmulDesc(lay.ptr(arena, "in"), objs["in"], rows["in"], lay.ptr(arena, "coef"), objs["coef"], n_in,
                   lay.ptr(arena, "out"), objs["out"], rows["out"], lay.ptr(arena, "hdr"), objs["hdr"], rows["hdr"],
                   n_out, n_in, W, n_obj)
    arena.run(lay, lambda: matmul_call(ctx, d, variant, persist))


@pytest.mark.parametrize("variant", [8, 0, 6])
@pytest.mark.parametrize("far", list(FAR_SETS))
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_matmul_far_object_stride(ctx, arena, branch, far, variant):
    run_far_matmul(ctx, arena, BRANCHES[branch], FAR_SETS[far], variant, persist=branch == "persist")


@pytest.mark.parametrize("variant", [8, 0, 6])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_matmul_far_odd_stride(ctx, arena, branch, variant):
    """Object strides of 2^32 + 4097 on the sources and the outputs, every base odd, rows at an odd stride."""
    run_far_matmul(ctx, arena, BRANCHES[branch], ("in", "out", "hdr"), variant, far=FAR_ODD, pad=1,
                   persist=branch == "persist")


# ======================================================================================================================
# b. rlnc_gf256_matmul, row strides
# ======================================================================================================================
BELOW_2_32 = (1 << 32) - 4096
PAST_2_31 = (1 << 31) + DELTA_ALIGNED
ROW_CASES = {
    "in_row-far": ((4, 2, 4096), dict(in_row=FAR)),
    "in_row-below-2^32": ((4, 2, 4096), dict(in_row=BELOW_2_32)),
    "out_row-2^31": ((4, 2, 4096), dict(out_row=PAST_2_31)),
    "out_row-far": ((2, 2, 4096 + 19), dict(out_row=FAR)),
    "hdr_row-far": ((2, 2, 4096 + 19), dict(hdr_row=FAR)),
    "hdr_row-2^31": ((4, 2, 4096), dict(hdr_row=PAST_2_31)),
}


@pytest.mark.parametrize("variant", [8, 0, 6])
@pytest.mark.parametrize("case", list(ROW_CASES))
def test_matmul_far_row_stride(ctx, arena, case, variant):
    shape, strides = ROW_CASES[case]
    run_far_matmul(ctx, arena, shape, (), variant, **strides)


# ======================================================================================================================
# c. rlnc_gf256_sparse_matmul
# ======================================================================================================================
SPARSE_FAR = {"in": ("in",), "out": ("out",), "hdr": ("hdr",), "idx": ("idx",), "val": ("val",),
              "all": ("in", "out", "hdr", "idx", "val"), "in_row": ()}


@functools.lru_cache(maxsize=None)
def sparse_operands(n_in):
    from rlnc_amd import sparse

    n_out, w, W = 5, 2, 4096 + 19
    rng = np.random.default_rng(n_in + 77)
    idx = rng.integers(0, n_in, (N_OBJ, n_out, w)).astype(np.int32)
    idx[:, 0] = (0, 1 % n_in)  # both gathered rows in one output row
    idx[:, 1] = (n_in - 1, n_in - 1)  # a repeated index: the values add
    val = rng.integers(1, 256, (N_OBJ, n_out, w), dtype=np.uint8)
    inp = rng.integers(0, 256, (N_OBJ, n_in, W), dtype=np.uint8)
    dense = np.stack([sparse.to_dense(idx[o], val[o], n_in) for o in range(N_OBJ)])
    want = np.stack([np_matmul(dense[o], inp[o]) for o in range(N_OBJ)])
    return n_out, w, W, ro(idx), ro(val), ro(inp), ro(dense), ro(want)


@pytest.mark.parametrize("far", list(SPARSE_FAR))
def test_sparse_far(ctx, arena, far):
    from rlnc_amd._lib import SparseMatmulDesc
    from rlnc_amd.errors import check

    n_in = 2 if far == "in_row" else 3
    n_out, w, W, idx, val, inp, dense, want = sparse_operands(n_in)
    in_row = FAR if far == "in_row" else W + 13
    nat = {"in": 2 * (W + 13) if far == "in_row" else n_in * in_row + 48, "out": n_out * (W + 13) + 48, "hdr": n_out * 64,
           "idx": n_out * w * 4, "val": n_out * w}
    objs = {k: (FAR if k in SPARSE_FAR[far] else v) for k, v in nat.items()}
    lay = FarLayout(seed=len(far) + n_in)
    lay.read("idx", Z_AUX, N_OBJ, objs["idx"], n_out, w * 4, w * 4, idx)
    lay.read("val", Z_COEF, N_OBJ, objs["val"], n_out, w, w, val)
    lay.read("in", Z_IN + 1, N_OBJ, objs["in"], n_in, in_row, W, inp)
    lay.write("hdr", Z_HDR, N_OBJ, objs["hdr"], n_out, 64, n_in, dense)
    lay.write("out", Z_OUT + 3, N_OBJ, objs["out"], n_out, W + 13, W, want)
    lay.build()
    d = SparseMatmulDesc(lay.ptr(arena, "in"), objs["in"], in_row, lay.ptr(arena, "idx"), objs["idx"], w * 4,
                         lay.ptr(arena, "val"), objs["val"], w, lay.ptr(arena, "out"), objs["out"], W + 13,
                         lay.ptr(arena, "hdr"), objs["hdr"], 64, n_out, n_in, w, N_OBJ, W)
    arena.run(lay, lambda: check(ctx.lib.rlnc_gf256_sparse_matmul(ctx.h, C.byref(d)), ctx.lib))


# ======================================================================================================================
# h. the L1 primitives on a vector across byte 2^32 of the arena
# ======================================================================================================================
@pytest.mark.parametrize("op", ["mul", "add", "mul_add"])
@pytest.mark.parametrize("which", ["dst", "src"])
def test_primitives_straddle(ctx, arena, op, which):
    from rlnc_amd.errors import check

    n = 4096 + 37
    straddle, near = (1 << 32) - 2001, Z_AUX + 5
    rng = np.random.default_rng(n + len(op))
    a = rng.integers(0, 256, (1, 1, n), dtype=np.uint8)
    b = rng.integers(0, 256, (1, 1, n), dtype=np.uint8)
    scalar = 0x53
    want = {"mul": MUL[scalar][a], "add": a ^ b, "mul_add": a ^ MUL[scalar][b]}[op]
    d_off, s_off = (straddle, near) if which == "dst" else (near, straddle)
    lay = FarLayout(seed=n)
    lay.read("dst_in", d_off, 1, 0, 1, 0, n, a)
    if op != "mul":
        lay.read("src", s_off, 1, 0, 1, 0, n, b)
    lay.write("dst", d_off, 1, 0, 1, 0, n, want)
    lay.build()
    dst, src = C.c_void_p(arena.ptr + d_off), C.c_void_p(arena.ptr + s_off)
    ctx.use_torch_stream()

    def call():
        if op == "mul":
            check(ctx.lib.rlnc_gf256_inplace_mul_vec_by_scalar(ctx.h, dst, n, scalar), ctx.lib)
        elif op == "add":
            check(ctx.lib.rlnc_gf256_inplace_add_vectors(ctx.h, dst, src, n), ctx.lib)
        else:
            check(ctx.lib.rlnc_gf256_mul_vec_by_scalar_then_add_into_vec(ctx.h, dst, src, n, scalar), ctx.lib)

    arena.run(lay, call)  # in place: the output's prefill is its input


# ======================================================================================================================
# d. decoding with pieces_obj_stride = FAR
# ======================================================================================================================
DK, DM = 8, 12
OK, NOT_ALL_YET = 0, 10
Z_FAR_OUT = (1 << 32) + 200 * MiB   # contiguous outputs (decoded, T) placed past byte 2^32 of the arena
MODE_PATHS = [(0, 1), (0, 2), (0, 5), (1, 2), (1, 7), (1, 8)]
DECODE_L = {4096 + 16: FAR, 4096 + 1: FAR_ODD}


@pytest.fixture(scope="module")
def ctx1():
    from tests.stream_util import true_rank_context

    c = true_rank_context()
    yield c
    c.set_decode_path(0)
    c.set_stream_form(0)


@functools.lru_cache(maxsize=None)
def decode_far_expected(L, mode, m=DM):
    """Object 0 has useless pieces in the middle and completes, object 1 is rank deficient (the constructed objects of
    tests/test_gpu_footprint.py, which the oracle confirms there).  (pieces [2][m][k + L], statuses, rank, T, decoded,
    object status, data length): mode 0 by the oracle, mode 1 by the true-rank model on the first m pieces."""
    from tests.test_gpu_footprint import decode_object
    from tests.true_rank import true_rank_model

    objs = [decode_object("useless", DK, DM, L), decode_object("deficient", DK, DM, L)]
    pieces = np.stack([o.pieces for o in objs])
    if mode == 0:
        assert m == DM
        return (ro(pieces), [list(o.statuses) for o in objs], [o.rank for o in objs], ro(np.stack([o.T for o in objs])),
                ro(np.stack([o.decoded for o in objs])), [o.status for o in objs], [o.data_len for o in objs])
    st, rank, T, dec, ost, dl = [], [], [], [], [], []
    for o in objs:
        s, r, Tm, _ = true_rank_model(DK, o.pieces[:m, :DK])
        Tf = np.zeros((DK, DM), np.uint8)
        Tf[:, :m] = Tm
        st.append(s), rank.append(r), T.append(Tf), dec.append(np_matmul(Tf, o.pieces[:, DK:]))
        ost.append(OK if r == DK else NOT_ALL_YET), dl.append(DK * L - 3 if r == DK else 0)
    assert rank[0] == DK and rank[1] < DK and np.array_equal(dec[0], objs[0].decoded)
    return ro(pieces), st, rank, ro(np.stack(T)), ro(np.stack(dec)), ost, dl


def pieces_layout(seed, pieces, far, extra=()):
    """The pieces [2][m][k + L] as an input at object stride `far` (odd: an odd base too), plus `extra` operands
    (method, name, base, n_obj, obj_stride, n_rows, row_stride, width, values)."""
    n, m, full = pieces.shape
    lay = FarLayout(seed=seed)
    lay.read("pieces", Z_IN + (far & 1), n, far, m, full, full, pieces)
    for method, *args in extra:
        getattr(lay, method)(*args)
    return lay.build()


def contiguous(arena, lay, name, dtype=None):
    """A contiguous operand [n_obj][n_rows][width] as a torch view of the arena."""
    op = lay.operands[name]
    assert op.row_stride == op.width and (op.n_obj == 1 or op.obj_stride == op.n_rows * op.width)
    return arena.t[op.base: op.base + op.n_obj * op.n_rows * op.width].view(op.n_obj, op.n_rows, op.width)


def i32(*shape, fill=-7):
    import torch

    return torch.full(shape, fill, dtype=torch.int32, device="cuda:0")


def i64(*shape, fill=-7):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda:0")


@pytest.mark.parametrize("L", list(DECODE_L))
@pytest.mark.parametrize("mode,path", MODE_PATHS)
def test_decode_far(ctx, ctx1, arena, mode, path, L):
    from rlnc_amd import batch
    from tests.gpu_util import dev

    c = ctx1 if mode else ctx
    far = DECODE_L[L]
    pieces, st, rank, T, dec, ost, dl = decode_far_expected(L, mode)
    dec_op = ("write", "decoded", Z_FAR_OUT + (far & 1), 2, DK * L, DK, L, L, dec)
    c.set_decode_path(path)
    try:
        lay = pieces_layout(L + path, pieces, far, [dec_op])
        ps, os_, dl_ = i32(2, DM), i32(2), i64(2)
        arena.run(lay, lambda: batch.decode_batch_device(arena.strided(lay, "pieces"), DK, contiguous(arena, lay, "decoded"),
                                                         ps, os_, dl_, c))
        assert ps.tolist() == st and os_.tolist() == ost and dl_.tolist() == dl

        lay = pieces_layout(L + path + 1, pieces, far, [("write", "T", Z_FAR_OUT + 1, 2, DK * DM, DK, DM, DM, T)])
        ps, rk = i32(2, DM), i32(2)
        arena.run(lay, lambda: batch.decode_batch_eliminate(arena.strided(lay, "pieces"), DK, contiguous(arena, lay, "T"),
                                                            ps, rk, c))
        assert ps.tolist() == st and rk.tolist() == rank

        lay = pieces_layout(L + path + 2, pieces, far, [dec_op])
        d_T, d_rank, os_, dl_ = dev(T), i32(2), i32(2), i64(2)
        d_rank.copy_(i32(2).new_tensor(rank))
        arena.run(lay, lambda: batch.decode_batch_apply(arena.strided(lay, "pieces"), DK, d_T, d_rank,
                                                        contiguous(arena, lay, "decoded"), os_, dl_, c))
        assert os_.tolist() == ost and dl_.tolist() == dl
    finally:
        c.set_decode_path(0)


# ======================================================================================================================
# e. decode streams with pieces_obj_stride = FAR
# ======================================================================================================================
@pytest.mark.parametrize("L", list(DECODE_L))
@pytest.mark.parametrize("form", [1, 2], ids=["workspace", "lds"])
def test_stream_far(ctx1, arena, form, L):
    """push (both forms), snapshot into a far T, deliver and apply into a far decoded, compact with the pieces moved
    in place: on pieces FAR apart, against the true-rank model and against a second stream fed the same pieces from a
    contiguous tensor.  m - 1 slots are pushed (a compaction follows a strict prefix): object 0 finishes with useless
    arrivals among its slots, object 1 stays below rank k with a useless arrival at slot 2, so slots of both move."""
    import torch

    from rlnc_amd import batch
    from tests.gpu_util import dev
    from tests.stream_util import compact_model

    far, done = DECODE_L[L], DM - 1
    pieces, st, rank, T, dec, ost, dl = decode_far_expected(L, 1, done)
    full = DK + L
    ctx1.set_stream_form(form)
    try:
        near = dev(pieces)
        avail = i32(2, fill=done)
        streams = {"far": batch.DecodeStream(DK, DM, 2, ctx1), "near": batch.DecodeStream(DK, DM, 2, ctx1)}
        got = {}

        # push: reads the pieces only
        lay = pieces_layout(L + form, pieces, far)
        rk, an = i32(2), i32(2)
        arena.run(lay, lambda: streams["far"].push(arena.strided(lay, "pieces"), avail, rank=rk, answered=an))
        assert rk.tolist() == rank and an.tolist() == [done, done]
        streams["near"].push(near, avail)

        # snapshot into a far T
        lay = pieces_layout(L + form + 1, pieces, far, [("write", "T", Z_FAR_OUT + 1, 2, DK * DM, DK, DM, DM, T)])
        ps, rk = i32(2, DM), i32(2)
        arena.run(lay, lambda: streams["far"].snapshot(contiguous(arena, lay, "T"), ps, rk))
        assert [r[:done] for r in ps.tolist()] == st and (ps[:, done:] == -1).all() and rk.tolist() == rank
        nT, nps, nrk = torch.empty((2, DK, DM), dtype=torch.uint8, device="cuda:0"), i32(2, DM), i32(2)
        streams["near"].snapshot(nT, nps, nrk)
        assert torch.equal(nps, ps) and torch.equal(nrk, rk) and np.array_equal(nT.cpu().numpy(), T)

        # deliver: the finished object only; no byte of the unfinished one's payload
        lay = pieces_layout(L + form + 2, pieces, far,
                            [("write", "decoded", Z_FAR_OUT + (far & 1), 1, 0, DK, L, L, dec[:1])])
        os_, dl_ = i32(2), i64(2)
        dview = arena.t[Z_FAR_OUT + (far & 1):][: 2 * DK * L].view(2, DK, L)
        arena.run(lay, lambda: streams["far"].deliver(arena.strided(lay, "pieces"), dview, os_, dl_))
        assert os_.tolist() == ost and dl_.tolist() == dl
        nd, nos, ndl = torch.full((2, DK, L), 0xA5, dtype=torch.uint8, device="cuda:0"), i32(2), i64(2)
        streams["near"].deliver(near, nd, nos, ndl)
        assert torch.equal(nos, os_) and torch.equal(ndl, dl_) and np.array_equal(nd[0].cpu().numpy(), dec[0])
        assert int((nd[1] != 0xA5).count_nonzero()) == 0

        # apply: T x data of both objects
        lay = pieces_layout(L + form + 3, pieces, far, [("write", "decoded", Z_FAR_OUT + (far & 1), 2, DK * L, DK, L, L, dec)])
        os_, dl_ = i32(2), i64(2)
        arena.run(lay, lambda: streams["far"].apply(arena.strided(lay, "pieces"), contiguous(arena, lay, "decoded"),
                                                    os_, dl_))
        assert os_.tolist() == ost and dl_.tolist() == dl

        # compact: slot j takes slot u_j, whole pieces, in place
        moved = pieces.copy()
        kept_want = np.full((2, DK), -1, np.int32)
        for o in range(2):
            u, r, _, _ = compact_model(DK, pieces[o, :done, :DK])
            assert r == rank[o] and u != list(range(r))
            kept_want[o, :r] = u
            moved[o, :r] = pieces[o, u]
        lay = pieces_layout(L + form + 4, pieces, far, [("write", "moved", Z_IN + (far & 1), 2, far, DM, full, full, moved)])
        kept, an = i32(2, DK), i32(2)
        arena.run(lay, lambda: streams["far"].compact(arena.strided(lay, "pieces"), None, kept, an))
        assert np.array_equal(kept.cpu().numpy(), kept_want) and an.tolist() == rank
        nkept = i32(2, DK)
        streams["near"].compact(near, None, nkept, None)
        assert torch.equal(nkept, kept) and np.array_equal(near.cpu().numpy(), moved)
        # ... and the compacted stream is a fresh stream's after a push of the kept pieces
        T2, ps2, rk2 = torch.empty((2, DK, DM), dtype=torch.uint8, device="cuda:0"), i32(2, DM), i32(2)
        streams["far"].snapshot(T2, ps2, rk2)
        streams["near"].snapshot(nT, nps, nrk)
        assert torch.equal(T2, nT) and torch.equal(ps2, nps) and torch.equal(rk2, nrk) and rk2.tolist() == rank
        assert [r[:k] for r, k in zip(ps2.tolist(), rank)] == [[OK] * k for k in rank]
    finally:
        ctx1.set_stream_form(0)


# ======================================================================================================================
# f. ragged calls: object 0 at the arena's start, object 1 past FAR; row strides of FAR
# ======================================================================================================================
def rows2d(arena, lay, name, obj=0):
    op = lay.operands[name]
    return arena.t.as_strided((op.n_rows, op.width), (op.row_stride, 1), op.base + obj * op.obj_stride)


@pytest.mark.parametrize("delta", ["aligned", "odd"])
def test_ragged_far_objects(ctx, arena, delta):
    """encode, recode and decode of two objects of different shapes, every operand of object 1 more than FAR past
    object 0's (the 2-wave and the 1-wave bit-sliced programs with their perm tails)."""
    from rlnc_amd import batch
    from tests.gpu_util import dev
    from tests.test_gpu_footprint import decode_object

    far = FAR if delta == "aligned" else FAR_ODD
    odd = far & 1
    rng = np.random.default_rng(far % 1000)
    shapes = [(7, 4096 + 17, 12), (16, 4096, 5)]  # (k, L, coded pieces)
    srcs = [rng.integers(0, 256, (k, L), dtype=np.uint8) for k, L, _ in shapes]
    cos = [rng.integers(0, 256, (n, k), dtype=np.uint8) for k, _, n in shapes]
    coded = [np.concatenate([co, np_matmul(co, s)], axis=1) for co, s in zip(cos, srcs)]
    lay = FarLayout(seed=1 + odd)
    for o, ((k, L, n), s, p) in enumerate(zip(shapes, srcs, coded)):
        lay.read(f"src{o}", Z_IN + odd + o * far, 1, 0, k, L + 3, L, s[None])
        lay.write(f"pieces{o}", Z_OUT + odd + o * far, 1, 0, n, k + L + 5, k + L, p[None])
    lay.build()
    d_cos = [dev(c) for c in cos]
    arena.run(lay, lambda: batch.encode_ragged([(rows2d(arena, lay, f"src{o}"), d_cos[o], rows2d(arena, lay, f"pieces{o}"))
                                                for o in range(2)], ctx))

    rs = [rng.integers(0, 256, (cnt, n), dtype=np.uint8) for cnt, (_, _, n) in zip((5, 9), shapes)]
    recoded = [np_matmul(r, p) for r, p in zip(rs, coded)]
    lay = FarLayout(seed=2 + odd)
    for o, (p, rc) in enumerate(zip(coded, recoded)):
        lay.read(f"pieces{o}", Z_IN + odd + o * far, 1, 0, p.shape[0], p.shape[1] + 5, p.shape[1], p[None])
        lay.write(f"out{o}", Z_OUT + odd + o * far, 1, 0, rc.shape[0], rc.shape[1] + 1, rc.shape[1], rc[None])
    lay.build()
    d_rs = [dev(r) for r in rs]
    arena.run(lay, lambda: batch.recode_ragged([(rows2d(arena, lay, f"pieces{o}"), d_rs[o], rows2d(arena, lay, f"out{o}"),
                                                 shapes[o][0]) for o in range(2)], ctx))

    objs = [decode_object("useless", 5, 7, 4096 + 17), decode_object("complete", 16, 16, 4096 + 17)]
    lay = FarLayout(seed=3 + odd)
    for o, ob in enumerate(objs):
        full = ob.k + ob.L
        lay.read(f"pieces{o}", Z_IN + odd + o * far, 1, 0, ob.m, full + 7, full, ob.pieces[None])
        lay.write(f"decoded{o}", Z_OUT + odd + o * far, 1, 0, ob.k, ob.L, ob.L, ob.decoded[None])
    lay.build()
    out = {}

    def decode():
        out["r"] = batch.decode_ragged([(rows2d(arena, lay, f"pieces{o}"), ob.k,
                                         contiguous(arena, lay, f"decoded{o}")[0]) for o, ob in enumerate(objs)], ctx)

    arena.run(lay, decode)
    ps, ost, dl = out["r"]
    assert ps.tolist() == [s for ob in objs for s in ob.statuses]
    assert ost.tolist() == [ob.status for ob in objs] and dl.tolist() == [ob.data_len for ob in objs]


def test_ragged_far_row_strides(ctx, arena):
    """piece_row_stride = FAR on the pieces a recode reads (k = 2, five recoded pieces of 4 KiB + 17: ragged_bsj_eligible
    refuses the stride, the perm ragged kernel takes the object) and on the two pieces a decode reads (k = m = 2, the
    oracle's statuses and payload);
    src_row_stride = FAR on an encode's source (k = 2, five coded pieces) and piece_row_stride = FAR on the two pieces
    another encode writes."""
    from oracle import np_oracle as npo
    from oracle.oracle import OracleDecoder
    from rlnc_amd import batch
    from tests.gpu_util import dev

    rng = np.random.default_rng(12)
    k, L = 2, 4096 + 17
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    co5, co2 = rng.integers(1, 256, (5, k), dtype=np.uint8), rng.integers(1, 256, (2, k), dtype=np.uint8)
    coded5, coded2 = (np.concatenate([c, np_matmul(c, src)], axis=1) for c in (co5, co2))

    lay = FarLayout(seed=21)
    lay.read("src", Z_IN, 1, 0, k, FAR, L, src[None])
    lay.write("pieces", Z_OUT, 1, 0, 5, k + L + 14, k + L, coded5[None])
    lay.read("src_b", Z_IN + 4 * MiB, 1, 0, k, L, L, src[None])
    lay.write("pieces_b", Z_OUT + 4 * MiB, 1, 0, 2, FAR, k + L, coded2[None])
    lay.build()
    d5, d2 = dev(co5), dev(co2)
    arena.run(lay, lambda: batch.encode_ragged([(rows2d(arena, lay, "src"), d5, rows2d(arena, lay, "pieces")),
                                                (rows2d(arena, lay, "src_b"), d2, rows2d(arena, lay, "pieces_b"))], ctx))

    r = rng.integers(0, 256, (5, 2), dtype=np.uint8)
    lay = FarLayout(seed=22)
    lay.read("pieces", Z_IN, 1, 0, 2, FAR, k + L, coded2[None])
    lay.write("out", Z_OUT, 1, 0, 5, k + L + 14, k + L, np_matmul(r, coded2)[None])
    lay.build()
    d_r = dev(r)
    arena.run(lay, lambda: batch.recode_ragged([(rows2d(arena, lay, "pieces"), d_r, rows2d(arena, lay, "out"), k)], ctx))

    data = rng.integers(0, 256, k * L - 1, dtype=np.uint8)
    padded = npo.pad(data, k)
    received = np.concatenate([co2, np_matmul(co2, padded)], axis=1)
    od = OracleDecoder(L, k)
    statuses = [od.decode(p) for p in received]
    status, payload = od.get_decoded_data()
    assert padded.shape == (k, L) and statuses == [0, 0] and status == 0 and np.array_equal(payload, data)
    lay = FarLayout(seed=23)
    lay.read("pieces", Z_IN, 1, 0, 2, FAR, k + L, received[None])
    lay.write("decoded", Z_OUT, 1, 0, k, L, L, od.padded_payload()[None])
    lay.build()
    out = {}
    arena.run(lay, lambda: out.update(r=batch.decode_ragged([(rows2d(arena, lay, "pieces"), k,
                                                              contiguous(arena, lay, "decoded")[0])], ctx)))
    ps, ost, dl = out["r"]
    assert ps.tolist() == statuses and ost.tolist() == [status] and dl.tolist() == [data.size]


# ======================================================================================================================
# g. the object API and the padded image
# ======================================================================================================================
def test_object_api_far(ctx, arena):
    """rlnc_encoder_from_device on two source rows FAR apart; rlnc_encoder_code_batch_device and
    _code_sparse_batch_device writing two coded pieces FAR apart."""
    import torch

    from rlnc_amd import sparse
    from rlnc_amd.full import Encoder
    from tests.gpu_util import dev

    rng = np.random.default_rng(31)
    k, L, n = 2, 4096 + 17, 5
    src = rng.integers(0, 256, (k, L), dtype=np.uint8)
    co = rng.integers(0, 256, (n, k), dtype=np.uint8)
    lay = FarLayout(seed=31)
    lay.read("src", Z_IN + 1, 1, 0, k, FAR, L, src[None])
    lay.write("pieces", Z_OUT, 1, 0, n, k + L, k + L, np.concatenate([co, np_matmul(co, src)], axis=1)[None])
    lay.build()
    d_co = dev(co)
    ctx.use_torch_stream()

    def from_device():
        enc = Encoder.from_device(lay.ptr(arena, "src"), k, L, FAR, ctx)
        assert (enc.get_piece_count(), enc.get_piece_byte_len()) == (k, L)
        enc.code_batch_device(d_co.data_ptr(), n, lay.ptr(arena, "pieces"))
        torch.cuda.synchronize()

    arena.run(lay, from_device)

    k3 = 3
    src3 = rng.integers(0, 256, (k3, L), dtype=np.uint8)
    co2 = rng.integers(0, 256, (2, k3), dtype=np.uint8)
    idx = np.array([[0, 2], [1, 1]], np.int32)
    val = rng.integers(1, 256, (2, 2), dtype=np.uint8)
    dense = sparse.to_dense(idx, val, k3)
    d_src3, d_co2, d_idx, d_val = dev(src3), dev(co2), torch.from_numpy(idx).to("cuda:0"), dev(val)
    enc = Encoder.from_device(d_src3.data_ptr(), k3, L, L, ctx)
    lay = FarLayout(seed=32)
    lay.write("dense", Z_OUT + 1, 1, 0, 2, FAR, k3 + L, np.concatenate([co2, np_matmul(co2, src3)], axis=1)[None])
    lay.write("sparse", Z_OUT + 4 * MiB, 1, 0, 2, FAR, k3 + L, np.concatenate([dense, np_matmul(dense, src3)], axis=1)[None])
    lay.build()

    def code():
        enc.code_batch_device(d_co2.data_ptr(), 2, lay.ptr(arena, "dense"), FAR)
        enc.code_sparse_batch_device(d_idx.data_ptr(), d_val.data_ptr(), 2, 2, lay.ptr(arena, "sparse"), FAR)
        torch.cuda.synchronize()

    arena.run(lay, code)


def test_pad_device_far(ctx, arena):
    """rlnc_pad_device: Encoder::new's padded image of a byte string, its two rows FAR apart."""
    from oracle import np_oracle as npo
    from rlnc_amd.errors import check
    from tests.gpu_util import dev

    k, n = 2, 2 * (4096 + 17) - 5
    data = np.random.default_rng(33).integers(0, 256, n, dtype=np.uint8)
    want = npo.pad(data, k)
    L = want.shape[1]
    lay = FarLayout(seed=33)
    lay.write("out", Z_OUT + 1, 1, 0, k, FAR, L, want[None])
    lay.build()
    d = dev(data)
    ctx.use_torch_stream()
    arena.run(lay, lambda: check(ctx.lib.rlnc_pad_device(ctx.h, C.c_void_p(d.data_ptr()), n, k,
                                                         C.c_void_p(lay.ptr(arena, "out")), FAR), ctx.lib))


# ======================================================================================================================
def _forced_main():
    """Child process (RLNC_ASSUME_ALIGNED_ONLY=1): object strides of 2^32 + 4097 through the realigned form of the
    stream and bit-sliced branches and a decode stream on odd rows, on an arena of this process's own (the object
    strides alone: 2^32 + 256 MiB)."""
    import rlnc_amd

    c = rlnc_amd.Context(0)
    assert c.lib.rlnc_device_unaligned_vector_access(0) == 0
    a = FarArena((1 << 32) + 256 * MiB)
    for branch in ("stream3-tail", "stream2-permtail", "bsj1-permtail", "bsj4", "bsj8"):
        for far in (("in",), ("out", "hdr"), ("in", "out", "hdr")):
            run_far_matmul(c, a, BRANCHES[branch], far, 8, far=FAR_ODD, pad=1)
    # the decode stream on odd rows: the delivery's realigned product and the compaction's single-byte move
    from tests.stream_util import true_rank_context

    test_stream_far(true_rank_context(), a, 1, 4096 + 1)
    print("forced realigned far ok")


if __name__ == "__main__" and "--forced" in sys.argv:
    _forced_main()
