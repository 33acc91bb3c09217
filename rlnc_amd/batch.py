"""Multi-object, device-resident batch API on torch tensors (torch is plumbing: HBM + streams only).

Layouts (uint8, contiguous, on the context's device):
    src     [obj][k][L]          source pieces (Encoder::new's padded image per object)
    coeffs  [obj][n][k]          coding vectors
    pieces  [obj][n][k+L]        full coded pieces, coeffs ‖ data (encoder.rs:246-248)
    decoded [obj][k][L]          padded payload rows (decoder.rs:141-153)
All launches go to torch's current stream of the tensors' device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import MatmulDesc, SparseMatmulDesc
from .context import Context, stream_context
from .errors import check


def _ctx_for(t, ctx: Context | None) -> Context:
    """The context a batch call launches with, on torch's current stream.  Without an explicit ctx each
    (device, stream) pair gets its own default context: a context's workspaces are stream-ordered, so two
    streams sharing one would overwrite each other's in-flight index stream / transform (include/rlnc_hip.h,
    Threading)."""
    import torch

    dev = t.device.index or 0
    if ctx is None:
        ctx = stream_context(dev, torch.cuda.current_stream(dev).cuda_stream)
    else:
        ctx.use_torch_stream()
    if torch.cuda.is_current_stream_capturing():
        ctx.graph_bound = True  # the graph holds its workspace addresses: never evicted (context.stream_context)
    return ctx


def _chk(t, shape=None):
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), "uint8 contiguous device tensor required"
    if shape is not None:
        assert tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)


def encode_batch(src, coeffs, out, ctx: Context | None = None) -> None:
    """out[o][i] = coeffs[o][i] ‖ Σ_j coeffs[o][i][j]·src[o][j]  (n coded pieces per object)."""
    nobj, k, L = src.shape
    n = coeffs.shape[1]
    _chk(src)
    _chk(coeffs, (nobj, n, k))
    _chk(out, (nobj, n, k + L))
    ctx = _ctx_for(src, ctx)
    check(ctx.lib.rlnc_encode_batch(ctx.h, C.c_void_p(src.data_ptr()), k, L, nobj, C.c_void_p(coeffs.data_ptr()), n,
                                    C.c_void_p(out.data_ptr())), ctx.lib)


def encode_batch_headers(coeffs, out, ctx: Context | None = None) -> None:
    """The coefficient headers of encode_batch alone: out[o][i][0..k) = coeffs[o][i] (encoder.rs:246-248)."""
    nobj, n, k = coeffs.shape
    _chk(coeffs)
    _chk(out)
    assert out.shape[0] == nobj and out.shape[1] == n and out.shape[2] > k
    ctx = _ctx_for(out, ctx)
    check(ctx.lib.rlnc_encode_batch_headers(ctx.h, C.c_void_p(coeffs.data_ptr()), k, out.shape[2] - k, nobj, n,
                                            C.c_void_p(out.data_ptr())), ctx.lib)


def encode_batch_data(src, coeffs, out, ctx: Context | None = None) -> None:
    """The data part of encode_batch alone: out[o][i][k..) = Σ_j coeffs[o][i][j]·src[o][j]."""
    nobj, k, L = src.shape
    n = coeffs.shape[1]
    _chk(src)
    _chk(coeffs, (nobj, n, k))
    _chk(out, (nobj, n, k + L))
    ctx = _ctx_for(src, ctx)
    check(ctx.lib.rlnc_encode_batch_data(ctx.h, C.c_void_p(src.data_ptr()), k, L, nobj,
                                         C.c_void_p(coeffs.data_ptr()), n, C.c_void_p(out.data_ptr())), ctx.lib)


def encode_plan_bytes(k: int, nobj: int, n: int) -> int:
    """Device bytes of an encode plan buffer (encode_batch_prepare)."""
    from ._lib import load

    return int(load().rlnc_encode_batch_plan_bytes(k, nobj, n))


def encode_batch_prepare(src, coeffs, out, plan, ctx: Context | None = None) -> None:
    """The code-block address stream of encode_batch_data(src, coeffs, out) written ahead into `plan` (a uint8 device
    tensor of encode_plan_bytes bytes) on this context's stream -- e.g. a side stream, so that the encode launch
    itself does not wait for it (encode_batch_data_planned)."""
    nobj, k, L = src.shape
    n = coeffs.shape[1]
    _chk(src)
    _chk(coeffs, (nobj, n, k))
    _chk(out, (nobj, n, k + L))
    _chk(plan)
    ctx = _ctx_for(src, ctx)
    check(ctx.lib.rlnc_encode_batch_prepare(ctx.h, C.c_void_p(src.data_ptr()), k, L, nobj,
                                            C.c_void_p(coeffs.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(plan.data_ptr()), plan.numel()), ctx.lib)


def encode_batch_data_planned(src, coeffs, out, plan, ctx: Context | None = None) -> None:
    """encode_batch_data with the address stream prepared by encode_batch_prepare (same arguments); the caller
    orders this launch after the prepare."""
    nobj, k, L = src.shape
    n = coeffs.shape[1]
    _chk(src)
    _chk(coeffs, (nobj, n, k))
    _chk(out, (nobj, n, k + L))
    ctx = _ctx_for(src, ctx)
    check(ctx.lib.rlnc_encode_batch_data_planned(ctx.h, C.c_void_p(src.data_ptr()), k, L, nobj,
                                                 C.c_void_p(coeffs.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(plan.data_ptr())), ctx.lib)


def recode_batch(pieces, r, out, k: int, ctx: Context | None = None) -> None:
    """out[o][c] = Σ_i r[o][c][i]·pieces[o][i] (coefficient header and data alike, recoder.rs:122-153)."""
    nobj, n, full = pieces.shape
    count = r.shape[1]
    _chk(pieces)
    _chk(r, (nobj, count, n))
    _chk(out, (nobj, count, full))
    ctx = _ctx_for(pieces, ctx)
    check(ctx.lib.rlnc_recode_batch(ctx.h, C.c_void_p(pieces.data_ptr()), k, full - k, n, nobj,
                                    C.c_void_p(r.data_ptr()), count, C.c_void_p(out.data_ptr())), ctx.lib)


def decode_batch(pieces, k: int, decoded, ctx: Context | None = None):
    """Feed pieces[o][0..m) to a fresh Decoder per object; returns (piece_status[obj][m],
    object_status[obj], data_len[obj]) as numpy arrays (status codes: rlnc_amd.errors.STATUS_NAMES).
    `pieces` may be a view pieces_all[:, :m] of more coded pieces (rows contiguous, objects strided)."""
    import torch

    nobj, m, full = pieces.shape
    L = full - k
    assert pieces.is_cuda and pieces.dtype == torch.uint8
    # strides of size-1 dimensions are arbitrary in torch; only real ones are checked
    obj_stride = pieces.stride(0) if nobj > 1 else m * full
    assert (full == 1 or pieces.stride(2) == 1) and (m == 1 or pieces.stride(1) == full) and obj_stride >= m * full
    _chk(decoded, (nobj, k, L))
    ctx = _ctx_for(pieces, ctx)
    ps = np.zeros((nobj, m), np.int32)
    os_ = np.zeros(nobj, np.int32)
    dl = np.zeros(nobj, np.uint64)
    check(ctx.lib.rlnc_decode_batch(ctx.h, C.c_void_p(pieces.data_ptr()), obj_stride, k, L, m, nobj,
                                    C.c_void_p(decoded.data_ptr()),
                                    ps.ctypes.data_as(C.POINTER(C.c_int32)), os_.ctypes.data_as(C.POINTER(C.c_int32)),
                                    dl.ctypes.data_as(C.POINTER(C.c_uint64))), ctx.lib)
    return ps, os_, dl


def decode_batch_device(pieces, k: int, decoded, piece_status, object_status, data_len, ctx: Context | None = None):
    """Asynchronous decode_batch with device outputs: piece_status int32 [obj][m], object_status int32 [obj],
    data_len int64 [obj] (all device tensors)."""
    import torch

    nobj, m, full = pieces.shape
    L = full - k
    obj_stride = pieces.stride(0) if nobj > 1 else m * full
    assert (m == 1 or pieces.stride(1) == full) and obj_stride >= m * full
    _chk(decoded, (nobj, k, L))
    assert piece_status.dtype == torch.int32 and tuple(piece_status.shape) == (nobj, m)
    assert object_status.dtype == torch.int32 and data_len.dtype == torch.int64
    ctx = _ctx_for(pieces, ctx)
    check(ctx.lib.rlnc_decode_batch_device(ctx.h, C.c_void_p(pieces.data_ptr()), obj_stride, k, L, m, nobj,
                                           C.c_void_p(decoded.data_ptr()), C.c_void_p(piece_status.data_ptr()),
                                           C.c_void_p(object_status.data_ptr()), C.c_void_p(data_len.data_ptr())),
          ctx.lib)


def _pieces_view(pieces, k):
    nobj, m, full = pieces.shape
    obj_stride = pieces.stride(0) if nobj > 1 else m * full
    assert (m == 1 or pieces.stride(1) == full) and obj_stride >= m * full
    return nobj, m, full - k, obj_stride


def decode_batch_eliminate(pieces, k: int, T, piece_status, rank, ctx: Context | None = None):
    """The elimination half of decode_batch_device (reads only the coefficient bytes): T uint8 [obj][k][m],
    piece_status int32 [obj][m], rank int32 [obj] (device tensors), asynchronous on the current stream."""
    import torch

    nobj, m, L, obj_stride = _pieces_view(pieces, k)
    _chk(T, (nobj, k, m))
    assert piece_status.dtype == torch.int32 and tuple(piece_status.shape) == (nobj, m)
    assert rank.dtype == torch.int32 and rank.numel() == nobj
    ctx = _ctx_for(pieces, ctx)
    check(ctx.lib.rlnc_decode_batch_eliminate(ctx.h, C.c_void_p(pieces.data_ptr()), obj_stride, k, L, m, nobj,
                                              C.c_void_p(T.data_ptr()), C.c_void_p(piece_status.data_ptr()),
                                              C.c_void_p(rank.data_ptr())), ctx.lib)


def decode_batch_apply(pieces, k: int, T, rank, decoded, object_status, data_len, ctx: Context | None = None):
    """The data half of decode_batch_device: decoded = T × received data, then the marker scan."""
    import torch

    nobj, m, L, obj_stride = _pieces_view(pieces, k)
    _chk(T, (nobj, k, m))
    _chk(decoded, (nobj, k, L))
    assert object_status.dtype == torch.int32 and data_len.dtype == torch.int64
    ctx = _ctx_for(pieces, ctx)
    check(ctx.lib.rlnc_decode_batch_apply(ctx.h, C.c_void_p(pieces.data_ptr()), obj_stride, k, L, m, nobj,
                                          C.c_void_p(T.data_ptr()), C.c_void_p(rank.data_ptr()),
                                          C.c_void_p(decoded.data_ptr()), C.c_void_p(object_status.data_ptr()),
                                          C.c_void_p(data_len.data_ptr())), ctx.lib)


def decode_apply_plan_bytes(k: int, m: int, nobj: int) -> int:
    """Device bytes of a decode plan buffer (decode_batch_apply_prepare)."""
    from ._lib import load

    return int(load().rlnc_decode_batch_apply_plan_bytes(k, m, nobj))


def decode_large_workspace_bytes(k: int, m: int, nobj: int) -> int:
    """Device bytes decode paths 7 and 8 keep in the context for nobj objects of k x m (0: outside their limits,
    k <= 4096 and m <= 8192).  Needs no GPU."""
    from ._lib import load

    return int(load().rlnc_decode_large_workspace_bytes(k, m, nobj))


def decode_batch_apply_prepare(pieces, k: int, T, decoded, plan, ctx: Context | None = None):
    """The code-block address stream of decode_batch_apply(pieces, k, T, ..., decoded) written ahead into `plan` (a
    uint8 device tensor of decode_apply_plan_bytes bytes) on this context's stream, once T is final -- e.g. behind
    decode_batch_eliminate on its side stream, so that the data side does not wait for it
    (decode_batch_apply_planned)."""
    nobj, m, L, obj_stride = _pieces_view(pieces, k)
    _chk(T, (nobj, k, m))
    _chk(decoded, (nobj, k, L))
    _chk(plan)
    ctx = _ctx_for(pieces, ctx)
    check(ctx.lib.rlnc_decode_batch_apply_prepare(ctx.h, C.c_void_p(pieces.data_ptr()), obj_stride, k, L, m, nobj,
                                                  C.c_void_p(T.data_ptr()), C.c_void_p(decoded.data_ptr()),
                                                  C.c_void_p(plan.data_ptr()), plan.numel()), ctx.lib)


def decode_batch_apply_planned(pieces, k: int, T, rank, decoded, object_status, data_len, plan,
                               ctx: Context | None = None):
    """decode_batch_apply with the address stream prepared by decode_batch_apply_prepare (same arguments); the caller
    orders this launch after the prepare."""
    import torch

    nobj, m, L, obj_stride = _pieces_view(pieces, k)
    _chk(T, (nobj, k, m))
    _chk(decoded, (nobj, k, L))
    assert object_status.dtype == torch.int32 and data_len.dtype == torch.int64
    ctx = _ctx_for(pieces, ctx)
    check(ctx.lib.rlnc_decode_batch_apply_planned(ctx.h, C.c_void_p(pieces.data_ptr()), obj_stride, k, L, m, nobj,
                                                  C.c_void_p(T.data_ptr()), C.c_void_p(rank.data_ptr()),
                                                  C.c_void_p(decoded.data_ptr()),
                                                  C.c_void_p(object_status.data_ptr()),
                                                  C.c_void_p(data_len.data_ptr()), C.c_void_p(plan.data_ptr())),
          ctx.lib)


def matmul(coef, inp, out, ctx: Context | None = None) -> None:
    """out[o] = coef[o] ⊗ inp[o] over GF(2^8); coef [obj][n_out][n_in], inp [obj][n_in][W], out [obj][n_out][W]."""
    nobj, n_out, n_in = coef.shape
    W = inp.shape[2]
    _chk(coef)
    _chk(inp, (nobj, n_in, W))
    _chk(out, (nobj, n_out, W))
    ctx = _ctx_for(inp, ctx)
    d = MatmulDesc(inp.data_ptr(), n_in * W, W, coef.data_ptr(), n_out * n_in, n_in, out.data_ptr(), n_out * W, W,
                   None, 0, 0, n_out, n_in, W, nobj)
    check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)


def _chk_sparse(idx, val, rows_shape):
    """idx int32 / val uint8 [obj][rows][w], contiguous, on the device; returns w."""
    import torch

    assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous(), "int32 contiguous device tensor required"
    assert idx.dim() == 3 and tuple(idx.shape[:2]) == tuple(rows_shape), (tuple(idx.shape), rows_shape)
    _chk(val, tuple(idx.shape))
    return idx.shape[2]


def _ptr_or_null(t):
    return C.c_void_p(t.data_ptr() if t.numel() else None)


def encode_batch_sparse(src, idx, val, out, ctx: Context | None = None) -> None:
    """encode_batch from sparse coding vectors (rlnc_amd.sparse; include/rlnc_hip.h "Sparse coding vectors"):
    idx int32 / val uint8 [obj][n][w] -> out[o][i] = dense header ‖ Σ_t val[o][i][t]·src[o][idx[o][i][t]]."""
    nobj, k, L = src.shape
    n = idx.shape[1]
    _chk(src)
    w = _chk_sparse(idx, val, (nobj, n))
    _chk(out, (nobj, n, k + L))
    ctx = _ctx_for(src, ctx)
    check(ctx.lib.rlnc_encode_batch_sparse(ctx.h, C.c_void_p(src.data_ptr()), k, L, nobj, _ptr_or_null(idx),
                                           _ptr_or_null(val), w, n, C.c_void_p(out.data_ptr())), ctx.lib)


def recode_batch_sparse(pieces, idx, val, out, k: int, ctx: Context | None = None) -> None:
    """recode_batch from sparse recoding vectors over the n received pieces: idx / val [obj][count][w] ->
    out[o][c] = Σ_t val[o][c][t]·pieces[o][idx[o][c][t]] (coefficient header and data alike)."""
    nobj, n, full = pieces.shape
    count = idx.shape[1]
    _chk(pieces)
    w = _chk_sparse(idx, val, (nobj, count))
    _chk(out, (nobj, count, full))
    ctx = _ctx_for(pieces, ctx)
    check(ctx.lib.rlnc_recode_batch_sparse(ctx.h, C.c_void_p(pieces.data_ptr()), k, full - k, n, nobj,
                                           _ptr_or_null(idx), _ptr_or_null(val), w, count,
                                           C.c_void_p(out.data_ptr())), ctx.lib)


def sparse_matmul(idx, val, inp, out, ctx: Context | None = None) -> None:
    """out[o][i] = Σ_t val[o][i][t]·inp[o][idx[o][i][t]] over GF(2^8); idx / val [obj][n_out][w], inp [obj][n_in][W],
    out [obj][n_out][W]."""
    nobj, n_in, W = inp.shape
    n_out = idx.shape[1]
    _chk(inp)
    w = _chk_sparse(idx, val, (nobj, n_out))
    _chk(out, (nobj, n_out, W))
    ctx = _ctx_for(inp, ctx)
    d = SparseMatmulDesc(inp.data_ptr(), n_in * W, W, idx.data_ptr() if w else None, n_out * w * 4, w * 4,
                         val.data_ptr() if w else None, n_out * w, w, out.data_ptr(), n_out * W, W, None, 0, 0,
                         n_out, n_in, w, nobj, W)
    check(ctx.lib.rlnc_gf256_sparse_matmul(ctx.h, C.byref(d)), ctx.lib)


def mul_vec_by_scalar(vec, scalar: int, ctx: Context | None = None) -> None:
    """gf256_inplace_mul_vec_by_scalar (simd/mod.rs:18-47) on a device vector."""
    _chk(vec)
    ctx = _ctx_for(vec, ctx)
    check(ctx.lib.rlnc_gf256_inplace_mul_vec_by_scalar(ctx.h, C.c_void_p(vec.data_ptr()), vec.numel(), scalar),
          ctx.lib)


def add_vectors(dst, src, ctx: Context | None = None) -> None:
    """gf256_inplace_add_vectors (simd/mod.rs:58-76)."""
    _chk(dst)
    _chk(src, tuple(dst.shape))
    ctx = _ctx_for(dst, ctx)
    check(ctx.lib.rlnc_gf256_inplace_add_vectors(ctx.h, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()),
                                                 dst.numel()), ctx.lib)


def mul_vec_by_scalar_then_add_into_vec(dst, src, scalar: int, ctx: Context | None = None) -> None:
    """gf256_mul_vec_by_scalar_then_add_into_vec (simd/mod.rs:89-119)."""
    _chk(dst)
    _chk(src, tuple(dst.shape))
    ctx = _ctx_for(dst, ctx)
    check(ctx.lib.rlnc_gf256_mul_vec_by_scalar_then_add_into_vec(ctx.h, C.c_void_p(dst.data_ptr()),
                                                                 C.c_void_p(src.data_ptr()), dst.numel(), scalar),
          ctx.lib)


# ------------------------------------------------------------------------------------------------------------------
# ragged batches (include/rlnc_hip.h: rlnc_encode_ragged / rlnc_recode_ragged / rlnc_decode_ragged): objects of
# different shapes and buffers, one launch per kernel stage
# ------------------------------------------------------------------------------------------------------------------
def _rows(t):
    """(pointer, row stride) of a 2-D uint8 device view whose rows are contiguous."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def encode_ragged(objs, ctx: Context | None = None) -> None:
    """objs: (src [k][L], coeffs [n][k], pieces [n][k+L]) per object -> n coded pieces coeffs ‖ data each."""
    from ._lib import ObjectDesc

    if not objs:
        return
    ctx = _ctx_for(objs[0][0], ctx)
    descs = []
    for src, co, pc in objs:
        k, L = src.shape
        n = co.shape[0]
        assert tuple(co.shape) == (n, k) and tuple(pc.shape) == (n, k + L) and co.is_contiguous()
        sp, ss = _rows(src)
        pp, ps = _rows(pc)
        descs.append(ObjectDesc(sp, ss, co.data_ptr(), pp, ps, k, L, n))
    arr = (ObjectDesc * len(descs))(*descs)
    check(ctx.lib.rlnc_encode_ragged(ctx.h, arr, len(descs)), ctx.lib)


def recode_ragged(objs, ctx: Context | None = None) -> None:
    """objs: (pieces [n][k+L], r [count][n], out [count][k+L], k) per object (recoder.rs:122-153 × count)."""
    from ._lib import RecodeObjDesc

    if not objs:
        return
    ctx = _ctx_for(objs[0][0], ctx)
    descs = []
    for pieces, r, out, k in objs:
        n, full = pieces.shape
        count = r.shape[0]
        assert tuple(r.shape) == (count, n) and r.is_contiguous() and tuple(out.shape) == (count, full)
        pp, ps = _rows(pieces)
        op, os_ = _rows(out)
        descs.append(RecodeObjDesc(pp, ps, r.data_ptr(), op, os_, k, full - k, n, count))
    arr = (RecodeObjDesc * len(descs))(*descs)
    check(ctx.lib.rlnc_recode_ragged(ctx.h, arr, len(descs)), ctx.lib)


def decode_ragged(objs, ctx: Context | None = None):
    """objs: (pieces [m][k+L], k, decoded [k][L]) per object.  Returns device tensors (piece_status int32 [sum m]
    in object order, object_status int32 [count], data_len int64 [count]); asynchronous like decode_batch_device."""
    import torch

    from ._lib import DecodeObjDesc

    dev = objs[0][0].device
    ctx = _ctx_for(objs[0][0], ctx)
    descs = []
    for pieces, k, dec in objs:
        m, full = pieces.shape
        L = full - k
        assert tuple(dec.shape) == (k, L) and dec.is_contiguous()
        pp, ps = _rows(pieces)
        descs.append(DecodeObjDesc(pp, ps, dec.data_ptr(), k, L, m))
    total_m = sum(d.m for d in descs)
    ps_t = torch.empty(total_m, dtype=torch.int32, device=dev)
    os_t = torch.empty(len(descs), dtype=torch.int32, device=dev)
    dl_t = torch.empty(len(descs), dtype=torch.int64, device=dev)
    arr = (DecodeObjDesc * len(descs))(*descs)
    check(ctx.lib.rlnc_decode_ragged(ctx.h, arr, len(descs), C.c_void_p(ps_t.data_ptr()), C.c_void_p(os_t.data_ptr()),
                                     C.c_void_p(dl_t.data_ptr())), ctx.lib)
    return ps_t, os_t, dl_t


# ------------------------------------------------------------------------------------------------------------------
# decode streams (include/rlnc_hip.h, "Decode streams"): the device decode, resumable -- pieces pushed as they arrive,
# per object
# ------------------------------------------------------------------------------------------------------------------
def state_bytes(k: int, m: int, num_objects: int) -> int:
    """Device bytes of a decode stream's state for num_objects objects of generation size k with m piece slots each
    (0: outside the limits, k <= 4096 and m <= 8192).  Needs no GPU."""
    from ._lib import load

    return int(load().rlnc_decode_stream_state_bytes(k, m, num_objects))


def stream_lds_fits(k: int, m: int) -> bool:
    """Whether the one-launch LDS form of a decode stream's push (Context.set_stream_form(2)) takes generation size k
    with m piece slots: the LDS condition of the true-rank device kernel.  False for k = 0 or m = 0.  Needs no GPU."""
    from ._lib import load

    return bool(load().rlnc_decode_stream_lds_fits(k, m))


def stream_deliver_plan_bytes(k: int, m: int, num_objects: int) -> int:
    """Device bytes of DecodeStream.deliver's plan buffer (rlnc_decode_stream_deliver_plan_bytes): a multiple of 16, 0
    exactly where state_bytes is 0.  Needs no GPU."""
    from ._lib import load

    return int(load().rlnc_decode_stream_deliver_plan_bytes(k, m, num_objects))


def stream_recode_plan_bytes(k: int, m: int, count: int, num_objects: int) -> int:
    """Device bytes of DecodeStream.recode's plan buffer for count recoded pieces per object
    (rlnc_decode_stream_recode_plan_bytes): a multiple of 16, non-decreasing in count, 0 exactly where state_bytes is 0
    or count is outside [1, 4096].  Needs no GPU."""
    from ._lib import load

    return int(load().rlnc_decode_stream_recode_plan_bytes(k, m, count, num_objects))


def stream_accept_plan_bytes(n: int, num_objects: int) -> int:
    """Device bytes of DecodeStream.accept's plan buffer for up to n arrivals per call
    (rlnc_decode_stream_accept_plan_bytes): a multiple of 16, non-decreasing in both arguments, 0 for n = 0,
    n > 1,048,576 and num_objects = 0.  Needs no GPU."""
    from ._lib import load

    return int(load().rlnc_decode_stream_accept_plan_bytes(n, num_objects))


class DecodeStream:
    """The true-rank decoder state of num_objects objects (generation size k, m piece slots each) kept on the device
    between calls.  Slot t of object o is pieces[o][t] of the caller's pieces [obj][m][k+L] tensor; the caller fills
    slots in order as pieces arrive and says in `avail` (int32 [obj], device) how many of each object are filled.
    After any sequence of pushes the state is a fresh mode-1 decoder's after decode() of the same slots in order.

    ctx: a context in rank mode 1 (a context in mode 0 is refused); None: a context of the stream's own, in rank mode 1
    on torch's current device.  push runs the form of that context (Context.set_stream_form).  Every call launches on torch's current stream and none synchronises."""

    def __init__(self, k: int, m: int, num_objects: int, ctx: Context | None = None):
        import torch

        self.k, self.m, self.num_objects = int(k), int(m), int(num_objects)
        nbytes = state_bytes(self.k, self.m, self.num_objects)
        assert nbytes > 0, f"a decode stream takes k <= 4096, m <= 8192 and at least one object: {(k, m, num_objects)}"
        if ctx is None:
            ctx = Context(torch.cuda.current_device())
            ctx.set_rank_mode(1)
        self.ctx = ctx
        dev = torch.device("cuda", ctx.device)
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert self.state.data_ptr() % 16 == 0
        self._T = None
        self._rank = None
        self._plan = None
        self._recode_plan = None
        self._accept_plan = None
        c = _ctx_for(self.state, self.ctx)
        check(c.lib.rlnc_decode_stream_init(c.h, C.c_void_p(self.state.data_ptr()), nbytes, self.k, self.m,
                                            self.num_objects), c.lib)

    def _i32(self, t, shape, name):
        import torch

        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
            f"{name}: int32 contiguous device tensor of shape {tuple(shape)} required"
        return C.c_void_p(t.data_ptr())

    def _pieces(self, pieces):
        nobj, m, L, obj_stride = _pieces_view(pieces, self.k)
        import torch

        assert pieces.is_cuda and pieces.dtype == torch.uint8 and (pieces.shape[2] == 1 or pieces.stride(2) == 1)
        assert (nobj, m) == (self.num_objects, self.m) and L > 0, (tuple(pieces.shape), self.num_objects, self.m)
        return L, obj_stride

    def push(self, pieces, avail, max_new: int | None = None, rank=None, answered=None) -> None:
        """Object o advances from the slots answered so far, done_o, to min(max(avail[o], done_o), m, done_o +
        max_new) (max_new=None: m).  avail may be overwritten as soon as this returns.  rank / answered (int32 [obj]
        device tensors, optional) receive every object's rank and done_o after the push; with max_new=0 nothing is launched
        and neither is written."""
        L, obj_stride = self._pieces(pieces)
        n = (self.num_objects,)
        av = self._i32(avail, n, "avail")
        rk = self._i32(rank, n, "rank") if rank is not None else None
        an = self._i32(answered, n, "answered") if answered is not None else None
        max_new = self.m if max_new is None else int(max_new)
        assert max_new >= 0
        c = _ctx_for(self.state, self.ctx)
        check(c.lib.rlnc_decode_stream_push(c.h, C.c_void_p(self.state.data_ptr()), self.state.numel(),
                                            C.c_void_p(pieces.data_ptr()), obj_stride, self.k, L, self.m,
                                            self.num_objects, av, max_new, rk, an), c.lib)

    def compact(self, pieces=None, retire=None, kept=None, answered=None) -> None:
        """Reclaims the slots of useless arrivals and retires objects in place (rlnc_decode_stream_compact), after the
        last push.  Object o with retire[o] != 0 (int32 [obj], optional) restarts empty: a new generation may be
        written into its slots.  Every other object keeps the slots below done_o whose status is Ok, u_0 < ... <
        u_{r-1}: piece u_j moves to slot j (pieces=None: only the state is compacted, the caller moves its pieces by
        `kept`), and the stream is a fresh stream's after a push of the kept pieces.  kept (int32 [obj][k], optional)
        receives u (-1 from r on, and for a retired object); answered (int32 [obj], optional) r, the slot of the
        object's next arrival, 0 for a retired object: avail restarts from there."""
        L, obj_stride = self._pieces(pieces) if pieces is not None else (0, 0)
        n = (self.num_objects,)
        rt = self._i32(retire, n, "retire") if retire is not None else None
        kp = self._i32(kept, (self.num_objects, self.k), "kept") if kept is not None else None
        an = self._i32(answered, n, "answered") if answered is not None else None
        c = _ctx_for(self.state, self.ctx)
        check(c.lib.rlnc_decode_stream_compact(c.h, C.c_void_p(self.state.data_ptr()), self.state.numel(),
                                               C.c_void_p(pieces.data_ptr()) if pieces is not None else None,
                                               obj_stride, self.k, L, self.m, self.num_objects, rt, kp, an), c.lib)

    def snapshot(self, T=None, piece_status=None, rank=None) -> None:
        """What the stream holds now (each output optional; the state is not modified): T uint8 [obj][k][m] as
        decode_batch_eliminate writes it (columns >= done_o zero), piece_status int32 [obj][m] (RLNC_STATUS_PENDING,
        -1, for the slots not yet answered), rank int32 [obj]."""
        if T is not None:
            _chk(T, (self.num_objects, self.k, self.m))
        ps = self._i32(piece_status, (self.num_objects, self.m), "piece_status") if piece_status is not None else None
        rk = self._i32(rank, (self.num_objects,), "rank") if rank is not None else None
        c = _ctx_for(self.state, self.ctx)
        check(c.lib.rlnc_decode_stream_snapshot(c.h, C.c_void_p(self.state.data_ptr()), self.state.numel(), self.k,
                                                self.m, self.num_objects,
                                                C.c_void_p(T.data_ptr()) if T is not None else None, ps, rk), c.lib)

    def apply(self, pieces, decoded, object_status, data_len) -> None:
        """The data of what was pushed so far: a snapshot into the stream's own T and rank, then decode_batch_apply
        (decoded [obj][k][L]; object_status int32 [obj]: Ok, NotAllPiecesReceivedYet below rank k, or
        InvalidDecodedDataFormat; data_len int64 [obj])."""
        import torch

        self._pieces(pieces)
        if self._T is None:
            self._T = torch.empty((self.num_objects, self.k, self.m), dtype=torch.uint8, device=self.state.device)
            self._rank = torch.empty((self.num_objects,), dtype=torch.int32, device=self.state.device)
        self.snapshot(T=self._T, rank=self._rank)
        decode_batch_apply(pieces, self.k, self._T, self._rank, decoded, object_status, data_len, self.ctx)

    def deliver(self, pieces, decoded, object_status, data_len, select=None) -> None:
        """The finished objects only, chosen on the device (rlnc_decode_stream_deliver): object o with rank k gets
        decoded[o] ([obj][k][L]) = T_o x the data rows of its answered slots, object_status[o] Ok or
        InvalidDecodedDataFormat and data_len[o]; an object below rank k gets NotAllPiecesReceivedYet and length 0, no
        byte of decoded[o] and no product work; an object with select[o] == 0 (int32 [obj], optional) gets nothing
        written at all.  The state and the pieces are only read.  The product takes done_o source rows: after
        compact() that is k, the minimum -- a receiver with many useless arrivals compacts first.  The stream owns
        the plan buffer and allocates it on the first call: call deliver once before capturing (push, deliver,
        compact) into a graph -- that call also looks up the 32- and 64-row programs' block table, which a capture
        cannot."""
        import torch

        L, obj_stride = self._pieces(pieces)
        _chk(decoded, (self.num_objects, self.k, L))
        n = (self.num_objects,)
        os_ = self._i32(object_status, n, "object_status")
        assert data_len.is_cuda and data_len.dtype == torch.int64 and data_len.is_contiguous() and \
            tuple(data_len.shape) == n, "data_len: int64 contiguous device tensor of shape [obj] required"
        sel = self._i32(select, n, "select") if select is not None else None
        if self._plan is None:
            nbytes = stream_deliver_plan_bytes(self.k, self.m, self.num_objects)
            self._plan = torch.empty(nbytes, dtype=torch.uint8, device=self.state.device)
            assert self._plan.data_ptr() % 16 == 0
        c = _ctx_for(self.state, self.ctx)
        check(c.lib.rlnc_decode_stream_deliver(c.h, C.c_void_p(self.state.data_ptr()), self.state.numel(),
                                               C.c_void_p(pieces.data_ptr()), obj_stride, self.k, L, self.m,
                                               self.num_objects, sel, C.c_void_p(decoded.data_ptr()), os_,
                                               C.c_void_p(data_len.data_ptr()), C.c_void_p(self._plan.data_ptr()),
                                               self._plan.numel()), c.lib)

    def recode_reserve(self, count: int) -> None:
        """Grows the stream's recode plan buffer to what recode() of count pieces per object needs (never shrinks it).
        recode() calls this itself; a buffer cannot grow inside a capture, so a graph's largest count is reserved, or
        recoded once eagerly, before capturing."""
        import torch

        nbytes = stream_recode_plan_bytes(self.k, self.m, int(count), self.num_objects)
        assert nbytes > 0, f"a stream recode takes 1 <= count <= 4096: {count}"
        if self._recode_plan is None or self._recode_plan.numel() < nbytes:
            assert not torch.cuda.is_current_stream_capturing(), \
                "the recode's plan buffer cannot grow inside a capture: recode_reserve(count) before capturing"
            self._recode_plan = torch.empty(nbytes, dtype=torch.uint8, device=self.state.device)
            assert self._recode_plan.data_ptr() % 16 == 0

    def recode(self, pieces, r, out, status, used=None, select=None) -> None:
        """The relay's call (rlnc_decode_stream_recode): count = r.shape[1] recoded pieces per selected object over the
        useful pieces it holds -- the slots below done_o whose status is Ok, u_0 < ... < u_{rank-1}, the ones compact()
        keeps -- found on the device.  r uint8 [obj][count][k], the random bytes (row i's first rank bytes are used);
        out uint8 [obj][count][k+L]: out[o][i] = sum_j r[o][i][j] * pieces[o][u_j], header and data alike; status int32
        [obj]: Ok, or NotEnoughPiecesToRecode (6) for an object of rank 0, of which no byte of out[o] is written; used
        int32 [obj], optional: the rank; an object with select[o] == 0 (int32 [obj], optional) gets nothing written at
        all.  The state and the pieces are only read.  The product takes done_o source rows: after compact() that is the
        rank, the minimum.  The stream owns the plan buffer and grows it for a larger count, eagerly and never inside a
        capture (recode_reserve): call recode once with the largest count before capturing (push, recode) into a graph
        -- that call also looks up the 32- and 64-row programs' block table, which a capture cannot."""
        L, obj_stride = self._pieces(pieces)
        _chk(r)
        assert r.dim() == 3 and tuple(r.shape) == (self.num_objects, r.shape[1], self.k) and r.shape[1] >= 1, \
            (tuple(r.shape), self.num_objects, self.k)
        count = int(r.shape[1])
        _chk(out, (self.num_objects, count, self.k + L))
        n = (self.num_objects,)
        st = self._i32(status, n, "status")
        us = self._i32(used, n, "used") if used is not None else None
        sel = self._i32(select, n, "select") if select is not None else None
        self.recode_reserve(count)
        c = _ctx_for(self.state, self.ctx)
        check(c.lib.rlnc_decode_stream_recode(c.h, C.c_void_p(self.state.data_ptr()), self.state.numel(),
                                              C.c_void_p(pieces.data_ptr()), obj_stride, self.k, L, self.m,
                                              self.num_objects, sel, C.c_void_p(r.data_ptr()), count,
                                              C.c_void_p(out.data_ptr()), st, us,
                                              C.c_void_p(self._recode_plan.data_ptr()), self._recode_plan.numel()), c.lib)

    def accept_reserve(self, n: int) -> None:
        """Grows the stream's accept plan buffer to what accept() of up to n arrivals needs (never shrinks it).
        accept() calls this itself; a buffer cannot grow inside a capture, so a graph's largest n is reserved, or
        accepted once eagerly, before capturing."""
        import torch

        nbytes = stream_accept_plan_bytes(int(n), self.num_objects)
        assert nbytes > 0, f"a stream accept takes 1 <= n <= 1,048,576 arrivals per call: {n}"
        if self._accept_plan is None or self._accept_plan.numel() < nbytes:
            assert not torch.cuda.is_current_stream_capturing(), \
                "the accept's plan buffer cannot grow inside a capture: accept_reserve(n) before capturing"
            self._accept_plan = torch.empty(nbytes, dtype=torch.uint8, device=self.state.device)
            assert self._accept_plan.data_ptr() % 16 == 0

    def accept(self, arrivals, objects, pieces, avail, slot=None, refused=None, count=None, finished=False) -> None:
        """The step before push (rlnc_decode_stream_accept): mixed arrivals go into their objects' next free slots in
        arrival order, decided on the device.  arrivals uint8 [n][k+L] on the device, stride(1) == 1 and any row stride
        of at least k + L, at any byte address; objects int32 [n], arrival i's object; avail int32 [obj], read and
        rewritten: arrival j of object o in the call goes to slot a + j of pieces[o], a = avail[o] clamped to [0, m],
        and avail[o] becomes min(a + its arrivals, m), what push takes next.  slot int32 [n], optional: the slot of
        each arrival, or RLNC_ACCEPT_NO_ROOM (-1) from slot m on, RLNC_ACCEPT_NO_OBJECT (-2) for an id outside [0, obj),
        RLNC_ACCEPT_FINISHED (-3), RLNC_ACCEPT_ABSENT (-4) for an index at or beyond count; refused int32 [obj],
        optional: the object's arrivals that found no room.  count int32 [1] on the device, optional: only the first
        min(max(count, 0), n) arrivals are taken, so a captured call replays with another number each time.
        finished=True passes the stream's state: the arrivals of an object whose rank is k are answered
        RLNC_ACCEPT_FINISHED, nothing of it is written and its avail keeps its value.  The stream owns the plan buffer
        and grows it for a larger n, eagerly and never inside a capture (accept_reserve)."""
        import torch

        L, obj_stride = self._pieces(pieces)
        S = self.k + L
        assert arrivals.is_cuda and arrivals.dtype == torch.uint8 and arrivals.dim() == 2 and arrivals.shape[1] == S, \
            (tuple(arrivals.shape), S)
        n = int(arrivals.shape[0])
        assert n >= 1 and (S == 1 or arrivals.stride(1) == 1) and (n == 1 or arrivals.stride(0) >= S), arrivals.stride()
        arrival_stride = int(arrivals.stride(0)) if n > 1 else S
        ob = self._i32(objects, (n,), "objects")
        av = self._i32(avail, (self.num_objects,), "avail")
        sl = self._i32(slot, (n,), "slot") if slot is not None else None
        rf = self._i32(refused, (self.num_objects,), "refused") if refused is not None else None
        ct = self._i32(count, (1,), "count") if count is not None else None
        self.accept_reserve(n)
        c = _ctx_for(self.state, self.ctx)
        check(c.lib.rlnc_decode_stream_accept(c.h, C.c_void_p(self.state.data_ptr()) if finished else None,
                                              self.state.numel() if finished else 0,
                                              C.c_void_p(arrivals.data_ptr()), arrival_stride, ob, n, ct,
                                              C.c_void_p(pieces.data_ptr()), obj_stride, self.k, L, self.m,
                                              self.num_objects, av, sl, rf,
                                              C.c_void_p(self._accept_plan.data_ptr()), self._accept_plan.numel()), c.lib)


def encode_emit_plan_bytes(k: int, max_per_object: int, num_objects: int, n: int) -> int:
    """Device bytes of EncodeEmitter's plan buffer (rlnc_encode_emit_plan_bytes): a multiple of 16, non-decreasing in
    each argument inside the limits, 0 for a zero argument, k > 4096, max_per_object > 4096, num_objects > 1,048,576
    and n > 1,048,576.  Needs no GPU."""
    from ._lib import load

    return int(load().rlnc_encode_emit_plan_bytes(k, max_per_object, num_objects, n))


class EncodeEmitter:
    """The sender's side of a decode stream (rlnc_encode_emit): per-object piece counts read on the device, coded
    pieces written as one packed run of packets with an object id per packet and a device-side count -- what
    DecodeStream.accept takes as (arrivals, objects, count=count).

    k, L: the generation; num_objects objects; max_per_object: the cap of one object's packets per call, which also
    selects the product's program for the whole call (a sender in its late rounds builds an emitter with a small cap);
    n: the packet capacity of out / objects / r.  The emitter owns the plan buffer, allocated here and never inside a
    capture.  ctx=None: the default context of torch's current stream, created on first use -- a capture on a stream
    that has none yet takes a context made beforehand.  emit launches on torch's current stream and never synchronises;
    call it once eagerly before capturing it into a graph (that call looks up the 32- and 64-row programs' block table,
    which a capture cannot; a first call inside a capture runs every column in the slower perm product, the same
    bytes)."""

    def __init__(self, k: int, L: int, num_objects: int, max_per_object: int, n: int, ctx: Context | None = None):
        self.k, self.L, self.num_objects = int(k), int(L), int(num_objects)
        self.max_per_object, self.n = int(max_per_object), int(n)
        nbytes = encode_emit_plan_bytes(self.k, self.max_per_object, self.num_objects, self.n)
        assert nbytes > 0 and self.L >= 1, \
            f"an emit takes 1 <= k <= 4096, L >= 1, 1 <= max_per_object <= 4096, 1 <= num_objects <= 1,048,576 and " \
            f"1 <= n <= 1,048,576: {(k, L, num_objects, max_per_object, n)}"
        import torch

        assert not torch.cuda.is_current_stream_capturing(), "the emit's plan buffer cannot be allocated inside a capture"
        self.ctx = ctx
        dev = torch.device("cuda", ctx.device if ctx is not None else torch.cuda.current_device())
        self._plan = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert self._plan.data_ptr() % 16 == 0

    def _i32(self, t, shape, name):
        import torch

        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.is_cuda, \
            f"{name}: int32 contiguous device tensor of shape {tuple(shape)} required"
        return C.c_void_p(t.data_ptr())

    def emit(self, src, want, r, out, objects, count, granted=None) -> None:
        """src uint8 [obj][k][L] on the device (stride(2) == 1, rows k*L-dense, any object stride >= k*L); want int32
        [obj]: object o gets w = min(max(want[o], 0), max_per_object) packets, in object order, while the n packets
        last (the low-numbered objects first); r uint8 [n][k], packet i's random bytes; out uint8 [n][k+L] with any row
        stride >= k+L at any byte address: packet i = r[i] || sum_j r[i][j] * src[o][j]; objects int32 [n]: packet i's
        object, RLNC_EMIT_NONE (-1) from the emitted count on; count int32 [1]: the emitted count; granted int32 [obj],
        optional: the packets each object got.  No byte of out from packet count on is written.  (out, objects, count)
        go to the transport, or straight into DecodeStream.accept(out, objects, pieces, avail, count=count)."""
        import torch

        k, L, nobj, n = self.k, self.L, self.num_objects, self.n
        assert src.dtype == torch.uint8 and tuple(src.shape) == (nobj, k, L), (tuple(src.shape), (nobj, k, L))
        assert (L == 1 or src.stride(2) == 1) and (k == 1 or src.stride(1) == L) and \
            (nobj == 1 or src.stride(0) >= k * L), src.stride()
        src_obj_stride = int(src.stride(0)) if nobj > 1 else k * L
        assert r.dtype == torch.uint8 and tuple(r.shape) == (n, k) and r.is_contiguous(), (tuple(r.shape), (n, k))
        S = k + L
        assert out.dtype == torch.uint8 and tuple(out.shape) == (n, S), (tuple(out.shape), (n, S))
        assert out.stride(1) == 1 and (n == 1 or out.stride(0) >= S), out.stride()
        out_stride = int(out.stride(0)) if n > 1 else S
        assert src.is_cuda and r.is_cuda and out.is_cuda, "src, r, out: device tensors required"
        wt = self._i32(want, (nobj,), "want")
        ob = self._i32(objects, (n,), "objects")
        ct = self._i32(count, (1,), "count")
        gr = self._i32(granted, (nobj,), "granted") if granted is not None else None
        c = _ctx_for(self._plan, self.ctx)
        check(c.lib.rlnc_encode_emit(c.h, C.c_void_p(src.data_ptr()), src_obj_stride, k, L, nobj, wt,
                                     self.max_per_object, C.c_void_p(r.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                     out_stride, ob, ct, gr, C.c_void_p(self._plan.data_ptr()), self._plan.numel()),
              c.lib)
