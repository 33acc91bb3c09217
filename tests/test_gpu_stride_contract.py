"""GPU: the stride contract of the raw product descriptors (include/rlnc_hip.h, rlnc_matmul_desc and
rlnc_sparse_matmul_desc).

Rejected before any launch, with RLNC_ERR_INVALID_ARGUMENT and every byte of the output arena still its prefill: a
negative stride of any operand; an `out` or `hdr` whose rows overlap (a row stride below the row's bytes with more than
one row, an object stride below them with more than one object, objects that reach into each other's rows).  Accepted
and equal to the oracle: a zero stride on an input -- one source object, one source row, one coefficient matrix or one
coefficient row for all -- each on its own and all together, at 40 output rows (the shared 4-wave program, two tiles)
and 70 (the 8-wave program, two tiles) in variant 8 and in variant 0 (perm).
"""
import ctypes as C

import numpy as np
import pytest

from tests.footprint import Arena
from tests.gpu_util import dev, np_matmul

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 100
N_OBJ, N_OUT, N_IN, W = 2, 4, 3, 4096
ROW = 64 + W + 16
OBJ = N_OUT * ROW + 48


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    c = rlnc_amd.Context(0)
    yield c
    c.set_kernel_variant(8, 0)


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(41)
    coef = rng.integers(1, 256, (N_OBJ, N_OUT, N_IN), dtype=np.uint8)
    inp = rng.integers(0, 256, (N_OBJ, N_IN, W), dtype=np.uint8)
    idx = rng.integers(0, N_IN, (N_OBJ, N_OUT, 2)).astype(np.int32)
    val = rng.integers(1, 256, (N_OBJ, N_OUT, 2), dtype=np.uint8)
    import torch

    return dev(coef), dev(inp), torch.from_numpy(idx).to("cuda:0"), dev(val)


# field -> value; the good descriptor has every stride of `GOOD`
GOOD = dict(in_obj_stride=N_IN * W, in_row_stride=W, coef_obj_stride=N_OUT * N_IN, coef_row_stride=N_IN,
            out_obj_stride=OBJ, out_row_stride=ROW, hdr_obj_stride=OBJ, hdr_row_stride=ROW)
REJECTED = {
    "in_obj<0": dict(in_obj_stride=-N_IN * W), "in_row<0": dict(in_row_stride=-W), "in_row=-1": dict(in_row_stride=-1),
    "coef_obj<0": dict(coef_obj_stride=-N_OUT * N_IN), "coef_row<0": dict(coef_row_stride=-N_IN),
    "out_obj<0": dict(out_obj_stride=-OBJ), "out_row<0": dict(out_row_stride=-ROW),
    "out_row=-2^32+row": dict(out_row_stride=ROW - (1 << 32)),
    "hdr_obj<0": dict(hdr_obj_stride=-OBJ), "hdr_row<0": dict(hdr_row_stride=-ROW),
    "out_row=0": dict(out_row_stride=0), "out_row<width": dict(out_row_stride=W - 1),
    "out_obj=0": dict(out_obj_stride=0), "out_obj<width": dict(out_obj_stride=W - 1),
    "out_obj<extent": dict(out_obj_stride=(N_OUT - 1) * ROW + W - 1),
    "hdr_row=0": dict(hdr_row_stride=0), "hdr_row<n_in": dict(hdr_row_stride=N_IN - 1),
    "hdr_obj=0": dict(hdr_obj_stride=0), "hdr_obj<extent": dict(hdr_obj_stride=(N_OUT - 1) * ROW + N_IN - 1),
}
SPARSE_ONLY = {
    "idx_obj<0": dict(idx_obj_stride=-N_OUT * 8), "idx_row<0": dict(idx_row_stride=-8),
    "val_obj<0": dict(val_obj_stride=-N_OUT * 2), "val_row<0": dict(val_row_stride=-2),
}


def out_arena(seed):
    a = Arena(N_OBJ * OBJ, seed=seed, largest_row_stride=ROW)
    a.device(seal=False)
    return a


def assert_untouched(a):
    after = a.after()
    assert np.array_equal(after, a.fill), f"a rejected call wrote byte {int(np.flatnonzero(after != a.fill)[0])}"


@pytest.mark.parametrize("variant", [8, 0])
@pytest.mark.parametrize("case", list(REJECTED))
def test_dense_descriptor_rejected(ctx, inputs, case, variant):
    from rlnc_amd._lib import MatmulDesc

    coef, inp, _, _ = inputs
    a = out_arena(len(case))
    base = a.region().data_ptr()
    s = dict(GOOD, **REJECTED[case])
    d = MatmulDesc(inp.data_ptr(), s["in_obj_stride"], s["in_row_stride"], coef.data_ptr(), s["coef_obj_stride"],
                   s["coef_row_stride"], base + 64, s["out_obj_stride"], s["out_row_stride"], base, s["hdr_obj_stride"],
                   s["hdr_row_stride"], N_OUT, N_IN, W, N_OBJ)
    ctx.set_kernel_variant(variant, 0)
    try:
        assert ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)) == INVALID_ARGUMENT
    finally:
        ctx.set_kernel_variant(8, 0)
    assert_untouched(a)


@pytest.mark.parametrize("case", [c for c in REJECTED if not c.startswith("coef")] + list(SPARSE_ONLY))
def test_sparse_descriptor_rejected(ctx, inputs, case):
    from rlnc_amd._lib import SparseMatmulDesc

    _, inp, idx, val = inputs
    a = out_arena(len(case) + 100)
    base = a.region().data_ptr()
    s = dict(GOOD, idx_obj_stride=N_OUT * 8, idx_row_stride=8, val_obj_stride=N_OUT * 2, val_row_stride=2)
    s.update(REJECTED.get(case) or SPARSE_ONLY[case])
    d = SparseMatmulDesc(inp.data_ptr(), s["in_obj_stride"], s["in_row_stride"], idx.data_ptr(), s["idx_obj_stride"],
                         s["idx_row_stride"], val.data_ptr(), s["val_obj_stride"], s["val_row_stride"], base + 64,
                         s["out_obj_stride"], s["out_row_stride"], base, s["hdr_obj_stride"], s["hdr_row_stride"],
                         N_OUT, N_IN, 2, N_OBJ, W)
    assert ctx.lib.rlnc_gf256_sparse_matmul(ctx.h, C.byref(d)) == INVALID_ARGUMENT
    assert_untouched(a)


def test_unused_strides_and_interleaved_outputs_accepted(ctx, inputs):
    """A single row's or a single object's stride is never used, so 0 there is no overlap; and objects may lie inside
    the rows' stride (out[o][i] at i * R + o * S with n_obj * S <= R) as well as rows inside the objects'."""
    from rlnc_amd._lib import MatmulDesc
    from rlnc_amd.errors import check

    coef, inp, _, _ = inputs
    hc, hi = coef.cpu().numpy(), inp.cpu().numpy()
    want = np.stack([np_matmul(hc[o], hi[o]) for o in range(N_OBJ)])
    S, R = W + 32, N_OBJ * (W + 32) + 16
    a = Arena(N_OUT * R, seed=5, largest_row_stride=R)
    a.operand("out", 0, N_OBJ, S, N_OUT, R, W)
    a.expect("out", want)
    a.device()
    d = MatmulDesc(inp.data_ptr(), N_IN * W, W, coef.data_ptr(), N_OUT * N_IN, N_IN, a.ptr("out"), S, R, None, -1, -1,
                   N_OUT, N_IN, W, N_OBJ)  # no hdr: its strides are not looked at
    check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)
    a.check_device()
    one = Arena(W, seed=6)
    one.operand("out", 0, 1, 0, 1, 0, W)
    one.expect("out", want[:1, :1])
    one.device()
    d = MatmulDesc(inp.data_ptr(), 0, W, coef.data_ptr(), 0, 0, one.ptr("out"), 0, 0, None, 0, 0, 1, N_IN, W, 1)
    check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)
    one.check_device()


# ---- broadcasts ------------------------------------------------------------------------------------------------------
BROADCASTS = {"in_obj": ("in_obj",), "coef_obj": ("coef_obj",), "coef_row": ("coef_row",), "in_row": ("in_row",),
              "all": ("in_obj", "coef_obj", "coef_row", "in_row")}
BW = 4096 + 19


@pytest.mark.parametrize("variant", [8, 0])
@pytest.mark.parametrize("zero", list(BROADCASTS))
@pytest.mark.parametrize("n_out", [40, 70])
def test_input_broadcast(ctx, n_out, zero, variant):
    from rlnc_amd._lib import MatmulDesc
    from rlnc_amd.errors import check

    z = BROADCASTS[zero]
    rng = np.random.default_rng(n_out + len(zero))
    coef = rng.integers(0, 256, (N_OBJ, n_out, N_IN), dtype=np.uint8)
    inp = rng.integers(0, 256, (N_OBJ, N_IN, BW), dtype=np.uint8)
    # what the device reads through the zero strides
    ec = coef[:1].repeat(N_OBJ, 0) if "coef_obj" in z else coef.copy()
    if "coef_row" in z:
        ec = ec[:, :1].repeat(n_out, 1)
    ei = inp[:1].repeat(N_OBJ, 0) if "in_obj" in z else inp.copy()
    if "in_row" in z:
        ei = ei[:, :1].repeat(N_IN, 1)
    want = np.stack([np_matmul(ec[o], ei[o]) for o in range(N_OBJ)])
    row = 64 + BW + 13
    obj = n_out * row
    a = Arena(N_OBJ * obj, seed=n_out + variant, largest_row_stride=row)
    a.operand("hdr", 0, N_OBJ, obj, n_out, row, N_IN)
    a.expect("hdr", ec)
    a.operand("out", 64, N_OBJ, obj, n_out, row, BW)
    a.expect("out", want)
    a.device()
    d_coef, d_inp = dev(coef), dev(inp)
    d = MatmulDesc(d_inp.data_ptr(), 0 if "in_obj" in z else N_IN * BW, 0 if "in_row" in z else BW, d_coef.data_ptr(),
                   0 if "coef_obj" in z else n_out * N_IN, 0 if "coef_row" in z else N_IN, a.ptr("out"), obj, row,
                   a.ptr("hdr"), obj, row, n_out, N_IN, BW, N_OBJ)
    ctx.set_kernel_variant(variant, 0)
    try:
        check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)
        after = a.after()
    finally:
        ctx.set_kernel_variant(8, 0)
    a.check(after)


@pytest.mark.parametrize("zero", ["in_obj", "in_row", "idx_obj", "idx_row", "val_obj", "val_row", "all"])
def test_sparse_input_broadcast(ctx, zero):
    from rlnc_amd import sparse
    from rlnc_amd._lib import SparseMatmulDesc
    from rlnc_amd.errors import check
    import torch

    z = ("in_obj", "in_row", "idx_obj", "idx_row", "val_obj", "val_row") if zero == "all" else (zero,)
    n_out, w = 5, 2
    rng = np.random.default_rng(len(zero))
    idx = rng.integers(0, N_IN, (N_OBJ, n_out, w)).astype(np.int32)
    val = rng.integers(1, 256, (N_OBJ, n_out, w), dtype=np.uint8)
    inp = rng.integers(0, 256, (N_OBJ, N_IN, BW), dtype=np.uint8)

    def seen(x, obj, row):
        x = x[:1].repeat(N_OBJ, 0) if obj in z else x.copy()
        return x[:, :1].repeat(x.shape[1], 1) if row in z else x

    ex, ev, ei = seen(idx, "idx_obj", "idx_row"), seen(val, "val_obj", "val_row"), seen(inp, "in_obj", "in_row")
    dense = np.stack([sparse.to_dense(ex[o], ev[o], N_IN) for o in range(N_OBJ)])
    want = np.stack([np_matmul(dense[o], ei[o]) for o in range(N_OBJ)])
    row = 64 + BW + 13
    obj = n_out * row
    a = Arena(N_OBJ * obj, seed=len(zero), largest_row_stride=row)
    a.operand("hdr", 0, N_OBJ, obj, n_out, row, N_IN)
    a.expect("hdr", dense)
    a.operand("out", 64, N_OBJ, obj, n_out, row, BW)
    a.expect("out", want)
    a.device()
    d_idx, d_val, d_inp = torch.from_numpy(idx).to("cuda:0"), dev(val), dev(inp)
    st = lambda name, v: 0 if name in z else v  # noqa: E731
    d = SparseMatmulDesc(d_inp.data_ptr(), st("in_obj", N_IN * BW), st("in_row", BW), d_idx.data_ptr(),
                         st("idx_obj", n_out * w * 4), st("idx_row", w * 4), d_val.data_ptr(), st("val_obj", n_out * w),
                         st("val_row", w), a.ptr("out"), obj, row, a.ptr("hdr"), obj, row, n_out, N_IN, w, N_OBJ, BW)
    check(ctx.lib.rlnc_gf256_sparse_matmul(ctx.h, C.byref(d)), ctx.lib)
    a.check_device()
