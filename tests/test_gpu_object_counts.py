"""GPU: batches of 65,535, 65,536 and 65,537 objects -- the counts around what one grid dimension holds.

The bit-sliced product writes its block-address stream with a kernel whose grid.y is the object (kernels.hip
bsj_offset_kernel), launched in ranges of 65,535 objects; pad_kernel (wire.hip) takes the descriptor from grid.y and
rlnc_pad_batch_device documents 65,535 descriptors as its limit.  Everything else indexes objects in grid.x.

The product shape is n_out = 4, n_in = 1, width 4,096 (256 MiB of source, 1 GiB out), generated on the device.
Coefficient row 0 is 1 for every object, so out[:, 0] must equal the source for *all* objects (compared on the device:
any folding of the object index shows); the other rows are random and are checked against tests.gpu_util.np_matmul for
objects 0, 1, 65,534, 65,535, 65,536 where present, the last one and 64 seeded random ones; the header copy is compared
for all objects.  Variant 8 (the bit-sliced default, which refused 65,536 objects with a device error before the ranges)
and variant 0 (perm, the control).  The decode tests build their pieces with the variant-0 encode, construct every
object's coding vectors so that its statuses and rank are known (one object in 997 is rank deficient), assert the status,
rank and length arrays of all objects on the device, the payload of every finished object against its source, and the
sampled objects against the oracle / the true-rank model.  No test holds more than 6 GiB.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import np_oracle as npo
from oracle.oracle import OracleDecoder
from tests.gpu_util import np_matmul
from tests.true_rank import true_rank_model

pytestmark = pytest.mark.gpu

COUNTS = [65535, 65536, 65537]
N_MAX = COUNTS[-1]
N_OUT, W = 4, 4096
OK, NOT_USEFUL, RECEIVED_ALL, NOT_ALL_YET, INVALID_ARGUMENT = 0, 8, 9, 10, 100
FILL = 0xA5
K, L = 4, 4096
DATA_LEN = K * L - 1  # the marker is the payload's last byte


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    c = rlnc_amd.Context(0)
    yield c
    c.set_kernel_variant(8, 0)


def gen(seed):
    import torch

    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return g


def rand_u8(shape, g, low=0):
    import torch

    return torch.randint(low, 256, shape, dtype=torch.uint8, device="cuda:0", generator=g)


def filled(shape):
    import torch

    return torch.full(shape, FILL, dtype=torch.uint8, device="cuda:0")


def sampled(n):
    rng = np.random.default_rng(n)
    fixed = [o for o in (0, 1, 65534, 65535, 65536, n - 1) if o < n]
    return sorted(set(fixed) | set(int(o) for o in rng.integers(0, n, 64)))


@pytest.fixture(scope="module")
def product_inputs():
    """(src [N_MAX][1][W], coef [N_MAX][4][1]) on the device; every test takes its first n objects."""
    import torch

    g = gen(65537)
    src = rand_u8((N_MAX, 1, W), g)
    coef = rand_u8((N_MAX, N_OUT, 1), g)
    coef[:, 0] = 1
    yield src, coef
    del src, coef
    torch.cuda.empty_cache()


def check_product(n, src, coef, out, hdr):
    """out [n][4][W] and hdr [n][4][1] (strided views allowed) against the source and the coefficients."""
    import torch

    torch.cuda.synchronize()
    assert torch.equal(out[:, 0], src[:n, 0]), "row 0 (coefficient 1) is not the source for every object"
    assert torch.equal(hdr, coef[:n]), "the header copy differs from the coefficients"
    idx = torch.tensor(sampled(n), device="cuda:0")
    h_out, h_src, h_coef = out[idx].cpu().numpy(), src[idx].cpu().numpy(), coef[idx].cpu().numpy()
    for i, o in enumerate(idx.tolist()):
        assert np.array_equal(h_out[i], np_matmul(h_coef[i], h_src[i])), f"object {o}"


@pytest.mark.parametrize("variant", [8, 0])
@pytest.mark.parametrize("n", COUNTS)
def test_matmul_object_counts(ctx, product_inputs, n, variant):
    from rlnc_amd._lib import MatmulDesc
    from rlnc_amd.errors import check

    src, coef = product_inputs
    out, hdr = filled((n, N_OUT, W)), filled((n, N_OUT, 1))
    d = MatmulDesc(src.data_ptr(), W, W, coef.data_ptr(), N_OUT, 1, out.data_ptr(), N_OUT * W, W, hdr.data_ptr(), N_OUT, 1,
                   N_OUT, 1, W, n)
    ctx.use_torch_stream()
    ctx.set_kernel_variant(variant, 0)
    try:
        check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)
    finally:
        ctx.set_kernel_variant(8, 0)
    check_product(n, src, coef, out, hdr)


@pytest.mark.parametrize("variant", [8, 0])
@pytest.mark.parametrize("n", COUNTS)
def test_encode_batch_object_counts(ctx, product_inputs, n, variant):
    from rlnc_amd import batch

    src, coef = product_inputs
    pieces = filled((n, N_OUT, 1 + W))
    ctx.set_kernel_variant(variant, 0)
    try:
        batch.encode_batch(src[:n], coef[:n], pieces, ctx)
    finally:
        ctx.set_kernel_variant(8, 0)
    check_product(n, src, coef, pieces[:, :, 1:], pieces[:, :, :1])


def test_planned_encode_object_count(ctx, product_inputs):
    """The address stream of 65,537 objects written ahead (rlnc_encode_batch_prepare), then the planned product: the
    data as above, every header byte still its prefill."""
    import torch

    from rlnc_amd import batch

    n = N_MAX
    src, coef = product_inputs
    pieces = filled((n, N_OUT, 1 + W))
    plan = torch.empty(batch.encode_plan_bytes(1, n, N_OUT), dtype=torch.uint8, device="cuda:0")
    batch.encode_batch_prepare(src, coef, pieces, plan, ctx)
    torch.cuda.synchronize()
    assert int((pieces != FILL).count_nonzero()) == 0, "the prepare wrote into the pieces"
    batch.encode_batch_data_planned(src, coef, pieces, plan, ctx)
    torch.cuda.synchronize()
    assert int((pieces[:, :, 0] != FILL).count_nonzero()) == 0, "the planned data product wrote a header byte"
    check_product(n, src, coef, pieces[:, :, 1:], coef[:n])


# ---- decode ----------------------------------------------------------------------------------------------------------
def deficient_objects(n):
    import torch

    return torch.arange(n, device="cuda:0") % 997 == 5


def coded_pieces(ctx, n, m, seed):
    """(src [n][K][L] with the marker as its last byte, coef [n][m][K], pieces [n][m][K + L]): the first K coding
    vectors are lower triangular with a nonzero diagonal, the others dense; in a deficient object the last column of
    every vector is zero (rank K - 1: vector K - 1 and all later ones lie in the span of the first K - 1).  The pieces
    come from the variant-0 encode, which test_encode_batch_object_counts checks."""
    from rlnc_amd import batch

    g = gen(seed)
    src = rand_u8((n, K, L), g)
    src[:, K - 1, L - 1] = 0x81
    coef = rand_u8((n, m, K), g, low=1)
    coef[:, :K] = coef[:, :K].tril()
    coef[deficient_objects(n), :, K - 1] = 0
    pieces = filled((n, m, K + L))
    ctx.set_kernel_variant(0, 0)
    try:
        batch.encode_batch(src, coef, pieces, ctx)
    finally:
        ctx.set_kernel_variant(8, 0)
    return src, coef, pieces


def expect_rows(n, full_row, deficient_row, dtype):
    """[n][len(row)]: full_row for every object, deficient_row for the deficient ones."""
    import torch

    t = torch.tensor(full_row, dtype=dtype, device="cuda:0").repeat(n, 1)
    t[deficient_objects(n)] = torch.tensor(deficient_row, dtype=dtype, device="cuda:0")
    return t


def test_decode_batch_device_object_count(ctx):
    import torch

    from rlnc_amd import batch

    n, m = N_MAX, K
    src, coef, pieces = coded_pieces(ctx, n, m, 1)
    decoded = filled((n, K, L))
    ps = torch.full((n, m), -7, dtype=torch.int32, device="cuda:0")
    ost = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    dl = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    batch.decode_batch_device(pieces, K, decoded, ps, ost, dl, ctx)
    torch.cuda.synchronize()
    bad = deficient_objects(n)
    assert int(bad.sum()) == len(range(5, n, 997))
    assert torch.equal(ps, expect_rows(n, [OK] * K, [OK] * (K - 1) + [NOT_USEFUL], torch.int32))
    assert torch.equal(ost, expect_rows(n, [OK], [NOT_ALL_YET], torch.int32)[:, 0])
    assert torch.equal(dl, expect_rows(n, [DATA_LEN], [0], torch.int64)[:, 0])
    assert torch.equal(decoded[~bad], src[~bad]), "a finished object's payload is not its source"
    for o in sampled(n) + [5, 997 + 5]:
        od = OracleDecoder(L, K)
        hp = pieces[o].cpu().numpy()
        assert [od.decode(p) for p in hp] == ps[o].tolist(), o
        st, payload = od.get_decoded_data()
        assert st == int(ost[o]), o
        if st == OK:
            assert payload.size == int(dl[o]) and np.array_equal(decoded[o].cpu().numpy(), od.padded_payload()), o


def test_decode_stream_object_count():
    """push + deliver + apply over 65,537 objects of k = 4, m = 6 (rank mode 1)."""
    import torch

    from rlnc_amd import batch
    from tests.stream_util import true_rank_context

    ctx1 = true_rank_context()
    n, m = N_MAX, 6
    src, coef, pieces = coded_pieces(ctx1, n, m, 2)
    bad = deficient_objects(n)
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda:0")  # noqa: E731
    stream = batch.DecodeStream(K, m, n, ctx1)
    avail = torch.full((n,), m, dtype=torch.int32, device="cuda:0")
    rank, answered = i32(n), i32(n)
    stream.push(pieces, avail, rank=rank, answered=answered)
    T, ps, rk = filled((n, K, m)), i32(n, m), i32(n)
    stream.snapshot(T, ps, rk)
    torch.cuda.synchronize()
    want_rank = expect_rows(n, [K], [K - 1], torch.int32)[:, 0]
    assert torch.equal(rank, want_rank) and torch.equal(rk, want_rank)
    assert torch.equal(answered, avail)
    assert torch.equal(ps, expect_rows(n, [OK] * K + [RECEIVED_ALL] * (m - K), [OK] * (K - 1) + [NOT_USEFUL] * (m - K + 1),
                                       torch.int32))
    h_coef = coef.cpu().numpy()
    for o in sampled(n) + [5, 997 + 5]:
        st, r, Tm, _ = true_rank_model(K, h_coef[o])
        assert st == ps[o].tolist() and r == int(rk[o]) and np.array_equal(T[o].cpu().numpy(), Tm), o

    want_status = expect_rows(n, [OK], [NOT_ALL_YET], torch.int32)[:, 0]
    want_len = expect_rows(n, [DATA_LEN], [0], torch.int64)[:, 0]
    decoded, ost, dl = filled((n, K, L)), i32(n), torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    stream.deliver(pieces, decoded, ost, dl)
    torch.cuda.synchronize()
    assert torch.equal(ost, want_status) and torch.equal(dl, want_len)
    assert torch.equal(decoded[~bad], src[~bad]), "a finished object's payload is not its source"
    assert int((decoded[bad] != FILL).count_nonzero()) == 0, "the delivery wrote into an unfinished object"

    decoded.fill_(FILL)
    ost.fill_(-7)
    dl.fill_(-7)
    stream.apply(pieces, decoded, ost, dl)
    torch.cuda.synchronize()
    assert torch.equal(ost, want_status) and torch.equal(dl, want_len)
    assert torch.equal(decoded[~bad], src[~bad])
    # an unfinished object: T x received data, rows >= rank zero
    h_T, h_dec, h_pc = T[5].cpu().numpy(), decoded[5].cpu().numpy(), pieces[5].cpu().numpy()
    assert np.array_equal(h_dec, npo.matmul(h_T, h_pc[:, K:]))


# ---- rlnc_pad_batch_device -------------------------------------------------------------------------------------------
PAD_K, PAD_LEN = 2, 5
PAD_L = (PAD_LEN + 1 + PAD_K - 1) // PAD_K


def pad_descs(n, data, out):
    from rlnc_amd._lib import PadDesc

    arr = (PadDesc * n)()
    dp, op = data.data_ptr(), out.data_ptr()
    for o in range(n):
        arr[o] = PadDesc(dp + o, PAD_LEN, PAD_K, op + o * PAD_K * PAD_L, 0)
    return arr


def test_pad_batch_65535_descriptors(ctx):
    """The most descriptors one call takes: descriptor o pads the 5 bytes at data + o into out[o] [2][3]."""
    import torch

    from rlnc_amd.errors import check

    n = 65535
    data = rand_u8((n + PAD_LEN,), gen(3))
    out = filled((n, PAD_K, PAD_L))
    ctx.use_torch_stream()
    check(ctx.lib.rlnc_pad_batch_device(ctx.h, pad_descs(n, data, out), n), ctx.lib)
    torch.cuda.synchronize()
    h = data.cpu().numpy()
    want = np.zeros((n, PAD_K * PAD_L), np.uint8)
    want[:, :PAD_LEN] = np.lib.stride_tricks.sliding_window_view(h, PAD_LEN)[:n]
    want[:, PAD_LEN] = 0x81
    assert np.array_equal(want[7].reshape(PAD_K, PAD_L), npo.pad(h[7: 7 + PAD_LEN], PAD_K))
    assert np.array_equal(out.cpu().numpy().reshape(n, -1), want)


def test_pad_batch_65536_descriptors_refused(ctx):
    """One more than the documented limit (include/rlnc_hip.h): RLNC_ERR_INVALID_ARGUMENT, nothing written."""
    import torch

    n = 65536
    data = rand_u8((n + PAD_LEN,), gen(4))
    out = filled((n, PAD_K, PAD_L))
    ctx.use_torch_stream()
    assert ctx.lib.rlnc_pad_batch_device(ctx.h, pad_descs(n, data, out), n) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert int((out != FILL).count_nonzero()) == 0
