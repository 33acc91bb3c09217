"""GPU: the sparse product (rlnc_amd/csrc/sparse.hip) through every entry point that reaches it.  The contract is one
sentence: a sparse call writes, byte for byte, what the dense call writes on the expanded matrix.  The checker is the
numpy model (tests.gpu_util.np_matmul / oracle.np_oracle) on rlnc_amd.sparse.to_dense, never the device's dense path,
except in the one equivalence test that says so.  Every comparison is exact.  Output buffers start as 0xAA so that
unwritten bytes show."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_oracle as npo
from rlnc_amd import sparse
from tests.gpu_util import dev, host, np_matmul

pytestmark = pytest.mark.gpu

ROWS = 4  # kSparseRows: output rows per workgroup (rlnc_amd/csrc/sparse_kernels.hpp)
FILL = 0xAA
INVALID_ARGUMENT = 100


@pytest.fixture(scope="module")
def ctx():
    import rlnc_amd

    return rlnc_amd.Context(0)


def idev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")


def filled(shape):
    import torch

    return torch.full(shape, FILL, dtype=torch.uint8, device="cuda:0")


def random_entries(rng, shape, n_in):
    """idx / val of `shape` = (..., w): indices with repeats, values 0..255 (a few zeros: padding)."""
    idx = rng.integers(0, n_in, shape).astype(np.int32)
    val = rng.integers(0, 256, shape, dtype=np.uint8)
    return idx, val


def sparse_desc_call(ctx, *fields):
    import torch

    from rlnc_amd import _lib
    from rlnc_amd.errors import check

    d = _lib.SparseMatmulDesc(*fields)
    check(ctx.lib.rlnc_gf256_sparse_matmul(ctx.h, C.byref(d)), ctx.lib)
    torch.cuda.synchronize()


# (n_obj, n_in, n_out, w, width, with header): a pruned product -- every n_in of {1, 2, 33, 300}, every w of
# {0, 1, 3, 8, 40 on 33 sources}, n_out one below / at / one above the rows per workgroup and 70, every width of
# {1, 15, 16, 17, 4095, 4096, 4097, 8192 + 48}, 1 and 3 objects; the large widths at small n_out
MATMUL_CASES = [
    (1, 1, ROWS - 1, 0, 1, True),
    (1, 1, ROWS, 1, 15, False),
    (3, 2, ROWS + 1, 3, 16, True),
    (1, 33, ROWS, 40, 17, True),
    (1, 300, 70, 8, 4095, False),
    (3, 33, ROWS - 1, 3, 4096, False),
    (1, 2, ROWS + 1, 1, 4097, True),
    (1, 300, ROWS, 8, 8192 + 48, False),
    (3, 300, 70, 3, 17, True),
]


@pytest.mark.parametrize("n_obj,n_in,n_out,w,width,with_hdr", MATMUL_CASES)
def test_sparse_matmul_against_numpy(ctx, n_obj, n_in, n_out, w, width, with_hdr):
    rng = np.random.default_rng(n_in * 1000 + n_out * 10 + w + width)
    inp = rng.integers(0, 256, (n_obj, n_in, width), dtype=np.uint8)
    idx, val = random_entries(rng, (n_obj, n_out, w), n_in)
    dense = sparse.to_dense(idx, val, n_in)
    if w == 40:
        assert any(len(set(r)) < w for r in idx[0].tolist())  # 40 entries over 33 sources: duplicates
    dinp, didx, dval = dev(inp), idev(idx), dev(val)
    out = filled((n_obj, n_out, width))
    if with_hdr:
        hdr = filled((n_obj, n_out, n_in))
        sparse_desc_call(ctx, dinp.data_ptr(), n_in * width, width, didx.data_ptr() if w else None, n_out * w * 4,
                         w * 4, dval.data_ptr() if w else None, n_out * w, w, out.data_ptr(), n_out * width, width,
                         hdr.data_ptr(), n_out * n_in, n_in, n_out, n_in, w, n_obj, width)
        assert np.array_equal(host(hdr), dense)
    else:
        from rlnc_amd import batch

        batch.sparse_matmul(didx, dval, dinp, out, ctx)
    got = host(out)
    for o in range(n_obj):
        assert np.array_equal(got[o], np_matmul(dense[o], inp[o])), o


def test_every_multiplier(ctx):
    """One output row of 255 entries, the values 1..255 over distinct sources."""
    from rlnc_amd import batch

    rng = np.random.default_rng(255)
    n_in = w = 255
    width = 4096 + 7
    inp = rng.integers(0, 256, (1, n_in, width), dtype=np.uint8)
    idx = rng.permutation(n_in).astype(np.int32).reshape(1, 1, w)
    val = np.arange(1, 256, dtype=np.uint8).reshape(1, 1, w)
    out = filled((1, 1, width))
    batch.sparse_matmul(idev(idx), dev(val), dev(inp), out, ctx)
    assert np.array_equal(host(out)[0], np_matmul(sparse.to_dense(idx, val, n_in)[0], inp[0]))


def test_padding_and_degenerate_rows(ctx):
    from rlnc_amd import batch

    rng = np.random.default_rng(6)
    k, L, w = 5, 100, 6
    rows = [
        ([0, 1, 2, 3, 4, 0], [0, 0, 0, 0, 0, 0]),   # all padding (valid indices, zero values)
        ([2, 2, 2, 2, 2, 2], [9, 9, 9, 9, 9, 9]),   # an even number of copies: zero
        ([2, 2, 2, 2, 2, 0], [9, 9, 9, 9, 9, 0]),   # an odd number of copies: one product
        ([0, 0, 1, 3, 4, 2], [0, 0, 4, 9, 1, 7]),   # padding first
        ([1, 3, 4, 2, 0, 0], [4, 9, 1, 7, 0, 0]),   # padding last
        ([4, 1, 4, 3, 0, 4], [0, 4, 0, 9, 0, 1]),   # padding interleaved
    ]
    idx = np.array([[r[0] for r in rows]], np.int32)
    val = np.array([[r[1] for r in rows]], np.uint8)
    src = rng.integers(1, 256, (1, k, L), dtype=np.uint8)
    dense = sparse.to_dense(idx, val, k)
    assert not dense[0, 0].any() and not dense[0, 1].any() and dense[0, 2].tolist() == [0, 0, 9, 0, 0]
    out = filled((1, len(rows), k + L))
    batch.encode_batch_sparse(dev(src), idev(idx), dev(val), out, ctx)
    got = host(out)[0]
    assert np.array_equal(got, npo.encode(src[0], dense[0]))
    assert not got[0].any() and not got[1].any()  # zero header and zero data
    assert np.array_equal(got[2, k:], npo.gf_mul_vec(src[0, 2], 9))


def test_index_guard(ctx):
    """Out-of-range entries are dropped without a read.  The source is rows 2 .. 2 + k of a (k + 4)-row tensor of
    nonzero bytes and the bad indices are -2, -1, k and k + 1 only: a missing guard reads rows of that tensor and shows
    as wrong bytes, never as an access outside it.  The header rows sit in a wider buffer for the same reason."""
    rng = np.random.default_rng(12)
    k, width, n_out, w = 9, 4096 + 16, ROWS + 2, 5
    big = rng.integers(1, 256, (k + 4, width), dtype=np.uint8)
    idx = rng.integers(0, k, (1, n_out, w)).astype(np.int32)
    val = rng.integers(1, 256, (1, n_out, w), dtype=np.uint8)
    for i, bad in enumerate([-2, -1, k, k + 1, -1, k]):
        idx[0, i, (2 * i) % w] = bad
    idx[0, 0, 3] = k  # two bad entries in one row
    dense = sparse.to_dense(idx, val, k)
    dbig, didx, dval = dev(big), idev(idx), dev(val)
    out = filled((n_out, width))
    hdr = filled((n_out, k + 4))
    sparse_desc_call(ctx, dbig.data_ptr() + 2 * width, 0, width, didx.data_ptr(), n_out * w * 4, w * 4,
                     dval.data_ptr(), n_out * w, w, out.data_ptr(), 0, width, hdr.data_ptr() + 2, 0, k + 4,
                     n_out, k, w, 1, width)
    assert np.array_equal(host(out), np_matmul(dense[0], big[2:2 + k]))
    h = host(hdr)
    assert np.array_equal(h[:, 2:2 + k], dense[0])
    assert (h[:, :2] == FILL).all() and (h[:, 2 + k:] == FILL).all()


@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_base_and_odd_strides(ctx, off):
    """Source and output at a byte offset, rows at odd strides larger than the rows, objects at odd strides; the gap
    bytes stay as they were."""
    rng = np.random.default_rng(off)
    n_obj, n_in, n_out, w, width = 2, 7, ROWS + 1, 3, 4096 + 33
    in_row, out_row, hdr_row = width + 4, width + 6, n_in + 2
    in_obj, out_obj, hdr_obj = n_in * in_row + 1, n_out * out_row + 7, n_out * hdr_row + 1
    assert in_row % 2 == 1 and out_row % 2 == 1
    inp = rng.integers(0, 256, off + n_obj * in_obj, dtype=np.uint8)
    idx, val = random_entries(rng, (n_obj, n_out, w), n_in)
    dense = sparse.to_dense(idx, val, n_in)
    dinp, didx, dval = dev(inp), idev(idx), dev(val)
    out = filled((off + n_obj * out_obj,))
    hdr = filled((off + n_obj * hdr_obj,))
    sparse_desc_call(ctx, dinp.data_ptr() + off, in_obj, in_row, didx.data_ptr(), n_out * w * 4, w * 4,
                     dval.data_ptr(), n_out * w, w, out.data_ptr() + off, out_obj, out_row,
                     hdr.data_ptr() + off, hdr_obj, hdr_row, n_out, n_in, w, n_obj, width)
    got, gh = host(out), host(hdr)
    want = np.full_like(got, FILL)
    want_h = np.full_like(gh, FILL)
    for o in range(n_obj):
        src = np.stack([inp[off + o * in_obj + j * in_row:][:width] for j in range(n_in)])
        res = np_matmul(dense[o], src)
        for i in range(n_out):
            want[off + o * out_obj + i * out_row:][:width] = res[i]
            want_h[off + o * hdr_obj + i * hdr_row:][:n_in] = dense[o, i]
    assert np.array_equal(got, want)
    assert np.array_equal(gh, want_h)


ENCODE_CASES = [(1, 1, 1, 1, 1), (16, 4096, 16, 2, 5), (33, 4097, 9, 3, 2), (300, 64, 70, 8, 1), (2048, 16, 4, 8, 1)]


@pytest.mark.parametrize("k,L,n,w,nobj", ENCODE_CASES)
def test_encode_batch_sparse(ctx, k, L, n, w, nobj):
    """Header bytes included; with odd k the data starts at an odd byte of the piece row."""
    from rlnc_amd import batch

    rng = np.random.default_rng(k + L)
    src = rng.integers(0, 256, (nobj, k, L), dtype=np.uint8)
    ent = [sparse.draw(rng, n, k, w) for _ in range(nobj)]
    idx, val = np.stack([e[0] for e in ent]), np.stack([e[1] for e in ent])
    dense = sparse.to_dense(idx, val, k)
    out = filled((nobj, n, k + L))
    batch.encode_batch_sparse(dev(src), idev(idx), dev(val), out, ctx)
    got = host(out)
    for o in range(nobj):
        assert np.array_equal(got[o], npo.encode(src[o], dense[o])), o
    if (k, L) == (16, 4096):  # the one equivalence case: the dense call on the expanded coefficients
        ref = filled((nobj, n, k + L))
        batch.encode_batch(dev(src), dev(dense), ref, ctx)
        assert np.array_equal(host(ref), got)


@pytest.mark.parametrize("k,L,n,count,w", [(8, 5, 3, 2, 2), (32, 4096, 20, 33, 4), (33, 1000, 64, 5, 8)])
def test_recode_batch_sparse(ctx, k, L, n, count, w):
    from rlnc_amd import batch

    rng = np.random.default_rng(k + n)
    nobj = 2
    pieces = rng.integers(0, 256, (nobj, n, k + L), dtype=np.uint8)
    idx, val = random_entries(rng, (nobj, count, w), n)
    dense = sparse.to_dense(idx, val, n)
    out = filled((nobj, count, k + L))
    batch.recode_batch_sparse(dev(pieces), idev(idx), dev(val), out, k, ctx)
    got = host(out)
    for o in range(nobj):
        assert np.array_equal(got[o], np_matmul(dense[o], pieces[o])), o


def test_encoder_code_sparse_batch_device(ctx):
    """An Encoder::new object (odd L: its rows sit at a padded stride) and a non-default output row stride."""
    from rlnc_amd.full import Encoder

    rng = np.random.default_rng(3)
    k, n, w = 7, 6, 3
    data = rng.integers(0, 256, k * 33 - 1, dtype=np.uint8)
    src = npo.pad(data, k).reshape(k, -1)
    L = src.shape[1]
    assert L == 33
    enc = Encoder.new(data, k, ctx)
    idx, val = sparse.draw(rng, n, k, w)
    idx[1, 1], val[1, 1] = idx[1, 0], val[1, 0]  # a duplicate that cancels
    didx, dval = idev(idx), dev(val)
    row = k + L + 5
    out = filled((n, row))
    enc.code_sparse_batch_device(didx.data_ptr(), dval.data_ptr(), w, n, out.data_ptr(), row)
    got = host(out)
    assert np.array_equal(got[:, :k + L], npo.encode(src, sparse.to_dense(idx, val, k)))
    assert (got[:, k + L:] == FILL).all()
    out2 = filled((n, k + L))
    enc.code_sparse_batch_device(didx.data_ptr(), dval.data_ptr(), w, n, out2.data_ptr())
    assert np.array_equal(host(out2), got[:, :k + L])


def test_round_trip_with_a_true_rank_receiver():
    """A sparse sender and a rank-mode-1 receiver: 3 nonzeros per vector over k = 33, where dependent pieces are
    common.  The model reaches rank 33 at piece 46 with 13 PieceNotUseful before it."""
    import rlnc_amd
    from rlnc_amd import batch
    from tests.true_rank import sparse_vectors, true_rank_model

    k, L, m = 33, 257, 132
    vectors = sparse_vectors(np.random.default_rng(0), k, m, 3)
    st, rank, _, _ = true_rank_model(k, vectors)
    assert rank == k and st.index(9) == 46 and st[:46].count(8) == 13 and st[:46].count(0) == k
    idx, val = sparse.from_dense(vectors)
    assert idx.shape == (m, 3)
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, k * L - 5, dtype=np.uint8)
    src = npo.pad(data, k).reshape(1, k, L)
    ctx = rlnc_amd.Context(0)
    ctx.set_rank_mode(1)
    pieces = filled((1, m, k + L))
    batch.encode_batch_sparse(dev(src), idev(idx[None]), dev(val[None]), pieces, ctx)
    assert np.array_equal(host(pieces)[0, :, :k], vectors)
    decoded = filled((1, k, L))
    pst, ost, dl = batch.decode_batch(pieces, k, decoded, ctx)
    assert pst[0].tolist() == st
    assert np.array_equal(host(decoded), src)
    assert ost[0] == 0 and int(dl[0]) == data.size


def test_error_order_follows_the_dense_twins(ctx):
    lib, h = ctx.lib, ctx.h
    k, L, n, w = 4, 32, 3, 2
    src, co, pieces = dev(np.ones((1, k, L))), dev(np.ones((1, n, k))), filled((1, n, k + L))
    idx, val = idev(np.zeros((1, n, w))), dev(np.ones((1, n, w)))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = 0x80000000
    # (k, L, objects, n, null source): the dense call and the sparse call answer alike
    for kk, LL, no, nn, null_src in [(0, 0, 1, n, False), (0, L, 1, n, True), (k, 0, 1, n, True), (k, L, 0, n, True),
                                     (k, L, 1, 0, True), (k, L, 1, n, True), (big, L, 1, n, False),
                                     (k, L, big, n, False), (k, L, 1, big, False)]:
        s = None if null_src else p(src)
        want = lib.rlnc_encode_batch(h, s, kk, LL, no, p(co), nn, p(pieces))
        assert lib.rlnc_encode_batch_sparse(h, s, kk, LL, no, p(idx), p(val), w, nn, p(pieces)) == want, (kk, LL, no, nn)
    # recode: n received == 0, k == 0, L == 0, nothing to do, null pointers
    for nr, kk, LL, cnt, null_in in [(0, 0, 0, 1, False), (3, 0, 0, 1, False), (3, k, 0, 1, False), (3, k, L, 0, True),
                                     (3, k, L, 1, True), (big, k, L, 1, False), (3, k, L, big, False)]:
        s = None if null_in else p(pieces)
        want = lib.rlnc_recode_batch(h, s, kk, LL, nr, 1, p(co), cnt, p(pieces))
        got = lib.rlnc_recode_batch_sparse(h, s, kk, LL, nr, 1, p(idx), p(val), w, cnt, p(pieces))
        assert got == want, (nr, kk, LL, cnt)
    # the entries: null with w > 0, w out of range, idx misaligned by 2 bytes
    args = (h, p(src), k, L, 1)
    assert lib.rlnc_encode_batch_sparse(*args, None, p(val), w, n, p(pieces)) == INVALID_ARGUMENT
    assert lib.rlnc_encode_batch_sparse(*args, p(idx), None, w, n, p(pieces)) == INVALID_ARGUMENT
    assert lib.rlnc_encode_batch_sparse(*args, p(idx), p(val), big, n, p(pieces)) == INVALID_ARGUMENT
    assert lib.rlnc_encode_batch_sparse(*args, C.c_void_p(idx.data_ptr() + 2), p(val), w, n, p(pieces)) == INVALID_ARGUMENT
    assert lib.rlnc_recode_batch_sparse(h, p(pieces), k, L, n, 1, C.c_void_p(idx.data_ptr() + 2), p(val), w, 1,
                                        p(pieces)) == INVALID_ARGUMENT
    from rlnc_amd import _lib

    d = _lib.SparseMatmulDesc(src.data_ptr(), k * L, L, idx.data_ptr() + 2, n * w * 4, w * 4, val.data_ptr(), n * w, w,
                              pieces.data_ptr(), n * (k + L), k + L, None, 0, 0, n, k, w, 1, L)
    assert lib.rlnc_gf256_sparse_matmul(h, C.byref(d)) == INVALID_ARGUMENT
    d.idx, d.idx_row_stride = idx.data_ptr(), w * 4 + 2
    assert lib.rlnc_gf256_sparse_matmul(h, C.byref(d)) == INVALID_ARGUMENT
    d.idx_row_stride, d.idx_obj_stride = w * 4, n * w * 4 + 1
    assert lib.rlnc_gf256_sparse_matmul(h, C.byref(d)) == INVALID_ARGUMENT
    # w == 0 needs no arrays
    assert lib.rlnc_encode_batch_sparse(*args, None, None, 0, n, p(pieces)) == 0
    import torch

    torch.cuda.synchronize()
    assert not host(pieces).any()


def test_encode_batch_sparse_under_graph_capture():
    """One captured call on a single stream; the graph holds pointers, not coefficients: a replay after idx / val were
    overwritten in place encodes the new vectors."""
    import torch

    import rlnc_amd
    from rlnc_amd import batch

    ctx = rlnc_amd.Context(0)
    rng = np.random.default_rng(4)
    nobj, k, L, n, w = 2, 20, 4096 + 48, 10, 3
    src = rng.integers(0, 256, (nobj, k, L), dtype=np.uint8)
    first = random_entries(rng, (nobj, n, w), k)
    second = random_entries(rng, (nobj, n, w), k)
    dsrc, didx, dval = dev(src), idev(first[0]), dev(first[1])
    out = filled((nobj, n, k + L))
    batch.encode_batch_sparse(dsrc, didx, dval, out, ctx)  # eager warm-up
    torch.cuda.synchronize()
    out.fill_(FILL)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            batch.encode_batch_sparse(dsrc, didx, dval, out, ctx)
    for entries in (first, second):
        didx.copy_(idev(entries[0]))
        dval.copy_(dev(entries[1]))
        out.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        got = host(out)
        dense = sparse.to_dense(entries[0], entries[1], k)
        for o in range(nobj):
            assert np.array_equal(got[o], npo.encode(src[o], dense[o])), o


def _forced_main():
    """Child process (RLNC_ASSUME_ALIGNED_ONLY=1): misaligned rows take the byte-granular kernel for every slot, aligned
    ones the vector kernel; the same checks as above."""
    import rlnc_amd

    c = rlnc_amd.Context(0)
    assert rlnc_amd._lib.load().rlnc_device_unaligned_vector_access(0) == 0
    test_misaligned_base_and_odd_strides(c, 1)
    test_misaligned_base_and_odd_strides(c, 3)
    test_encode_batch_sparse(c, 33, 4097, 9, 3, 2)    # data at an odd byte of the piece row
    test_encode_batch_sparse(c, 16, 4096, 16, 2, 5)   # aligned rows
    test_recode_batch_sparse(c, 33, 1000, 64, 5, 8)
    test_index_guard(c)
    print("forced byte-granular path ok")


def test_byte_granular_path_forced():
    """The device here reads misaligned 16-byte vectors, so the tests above reach the byte-granular kernel only for a
    row's last partial slot; with the probe overridden it carries whole misaligned rows."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RLNC_ASSUME_ALIGNED_ONLY="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--forced"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "forced byte-granular path ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__" and "--forced" in sys.argv:
    _forced_main()
