"""GPU: the persistent-tile form of the 64-row product (kernels.hip gf_matmul_bsj_persist_kernel, the generated program
RLNC_BSJ_ASM_W8P of bitslice_jump_persist.inc): one workgroup per compute unit stays for the whole launch and claims its next column block from
per-XCD counters in the context's workspace; the last workgroup to finish zeroes them.

Every product here is compared byte for byte with tests.gpu_util.np_matmul (the oracle's GF(2^8) table).  The launcher
takes the persistent form by itself from two tiles per compute unit on, for 12 or more sources and up to 64 output rows;
`set_persistent_tiles(2, W)` makes it take it for every such launch however few its tiles, with at most W workgroups
instead of one per compute unit.  The tile-count tests run with the device's own grid (W = 0); every other test runs 8
workgroups over 26 or more tiles, so each workgroup makes three or more successful claims: pointer moves, tile
switches at different positions of the 12-row ring, wraps into the next object with more than one column block per
object, and next-tile DMA entries all happen (k < 12 keeps the one-tile-per-workgroup grid by construction and must
stay right).

Shapes: 33 output rows and 12 sources are the smallest the program takes.  The two largest tile counts (2 CU + 3 and
8 CU + 5 tiles of 4 KiB) would cost numpy seconds as full random products, so above 300 tiles the sources are built for
a cheap exact reference: source rows 0 and k - 1 are random per tile, the rows between are one random 4 KiB block
repeated in every tile, and by linearity the product is np_matmul of the repeated block plus the table products of the
two per-tile rows; 16 sampled tiles are also checked against np_matmul of their actual sources.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.footprint import Arena, assert_inputs_unchanged
from tests.gpu_util import MUL, np_matmul

pytestmark = pytest.mark.gpu

BLK = 4096
AUTO, OFF, ALWAYS = 0, 1, 2
FULL_RANDOM_TILES = 300


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    c = rlnc_amd.Context(0)
    c.set_kernel_variant(8, 0)
    c.set_persistent_tiles(ALWAYS, 0)
    yield c
    c.set_persistent_tiles(AUTO, 0)


WGS = 8  # workgroups of the capped launches: one per counter


@pytest.fixture
def capped(ctx):
    """The context with at most WGS workgroups per persistent launch."""
    ctx.set_persistent_tiles(ALWAYS, WGS)
    yield ctx
    ctx.set_persistent_tiles(ALWAYS, 0)


@functools.lru_cache(maxsize=None)
def compute_units():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def operands(n_obj, blocks, k, n_out):
    """(coef [obj][n_out][k], inp [obj][k][blocks * 4 KiB], want [obj][n_out][blocks * 4 KiB]), read-only, shared."""
    rng = np.random.default_rng(((n_obj * 1009 + blocks) * 1013 + k) * 1019 + n_out)
    W = blocks * BLK
    tiles = n_obj * blocks
    if tiles <= FULL_RANDOM_TILES:
        coef = rng.integers(0, 256, (n_obj, n_out, k), dtype=np.uint8)
        coef[0, 0], coef[-1, -1] = 1, 0
        inp = rng.integers(0, 256, (n_obj, k, W), dtype=np.uint8)
        want = np.stack([np_matmul(coef[o], inp[o]) for o in range(n_obj)])
        return ro(coef), ro(inp), ro(want)
    assert k >= 2
    c1 = rng.integers(1, 256, (n_out, k), dtype=np.uint8)  # one coefficient matrix, every entry nonzero
    coef = np.broadcast_to(c1, (n_obj, n_out, k)).copy()
    base = rng.integers(0, 256, (k, BLK), dtype=np.uint8)
    base[0] = base[k - 1] = 0
    inp = np.broadcast_to(np.tile(base, (1, blocks))[None], (n_obj, k, W)).copy()
    first = rng.integers(0, 256, (n_obj, W), dtype=np.uint8)
    last = rng.integers(0, 256, (n_obj, W), dtype=np.uint8)
    inp[:, 0], inp[:, k - 1] = first, last
    want = np.broadcast_to(np.tile(np_matmul(c1, base), (1, blocks))[None], (n_obj, n_out, W)).copy()
    for i in range(n_out):
        want[:, i] ^= MUL[c1[i, 0]][first] ^ MUL[c1[i, k - 1]][last]
    for t in rng.choice(tiles, 16, replace=False):  # the shortcut against the plain product
        o, b = divmod(int(t), blocks)
        assert np.array_equal(want[o][:, b * BLK:(b + 1) * BLK], np_matmul(c1, inp[o][:, b * BLK:(b + 1) * BLK]))
    return ro(coef), ro(inp), ro(want)


def up(a):
    import torch

    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def desc(d_inp, d_coef, out_ptr, n_obj, n_out, k, W, in_row=None, out_row=None):
    from rlnc_amd._lib import MatmulDesc

    in_row = W if in_row is None else in_row
    out_row = W if out_row is None else out_row
    return MatmulDesc(d_inp if isinstance(d_inp, int) else d_inp.data_ptr(), k * in_row, in_row, d_coef.data_ptr(),
                      n_out * k, k, out_ptr, n_out * out_row, out_row, None, 0, 0, n_out, k, W, n_obj)


def launch(ctx, d):
    from rlnc_amd.errors import check

    check(ctx.lib.rlnc_gf256_matmul(ctx.h, C.byref(d)), ctx.lib)


def product(ctx, n_obj, blocks, k, n_out):
    """One product on fresh device buffers, compared on the device with the expected image."""
    import torch

    coef, inp, want = operands(n_obj, blocks, k, n_out)
    d_coef, d_inp, d_want = up(coef), up(inp), up(want)
    out = torch.full(want.shape, 0xA5, dtype=torch.uint8, device="cuda:0")
    launch(ctx, desc(d_inp, d_coef, out.data_ptr(), n_obj, n_out, k, blocks * BLK))
    torch.cuda.synchronize()
    if not torch.equal(out, d_want):
        bad = torch.nonzero(out != d_want)
        o, i, c = (int(x) for x in bad[0])
        raise AssertionError(f"{bad.shape[0]} bytes differ, first at object {o} row {i} column {c} (column block "
                             f"{c // BLK}): got {int(out[o, i, c]):#04x}, want {int(d_want[o, i, c]):#04x}")
    assert_inputs_unchanged({"coef": (coef, d_coef), "in": (inp, d_inp)})


def tile_count_cases():
    """(objects, column blocks) with objects x blocks = 1, 2, CU - 1, CU, CU + 1, 2 CU + 3, 8 CU + 5 as functions of
    the compute-unit count, blocks in {1, 2, 3, 9}: the largest and the smallest divisor of each count, and one object
    of 1, 2, 3 and 9 blocks."""
    def cases(cu):
        out = [(1, 1), (1, 2), (1, 3), (1, 9)]
        for tiles in (2, cu - 1, cu, cu + 1, 2 * cu + 3, 8 * cu + 5):
            divs = [b for b in (1, 2, 3, 9) if tiles % b == 0]
            for b in {divs[0], divs[-1]}:
                if (tiles // b, b) not in out:
                    out.append((tiles // b, b))
        return out
    return cases


# The case list depends on the device, which a collection without a GPU does not have: the parameter is the index into
# the list of a 256-CU device (the MI355X), and the test recomputes the list for the device it runs on.
N_TILE_CASES = len(tile_count_cases()(256))


@pytest.mark.parametrize("idx", range(N_TILE_CASES))
def test_tile_counts_around_the_grid(ctx, idx):
    cases = tile_count_cases()(compute_units())
    if idx >= len(cases):  # a device whose counts share more divisors has fewer distinct cases
        idx = len(cases) - 1
    n_obj, blocks = cases[idx]
    product(ctx, n_obj, blocks, 12, 33)


def test_automatic_choice_takes_it_from_two_tiles_per_unit(ctx):
    ctx.set_persistent_tiles(AUTO, 0)
    try:
        product(ctx, 2 * compute_units() + 3, 1, 12, 33)
    finally:
        ctx.set_persistent_tiles(ALWAYS, 0)


@pytest.mark.parametrize("n_out", [40, 64])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 9, 11, 12, 13, 25, 32])
def test_source_counts_around_the_pipeline_depths(capped, k, n_out):
    """5 objects of 7 column blocks = 35 tiles on 8 workgroups: with k = 13, 25, 32 successive tiles of a workgroup end
    in different bodies of the 12-row ring (k mod 12 = 1, 1, 8), with k = 12 always in the last."""
    product(capped, 5, 7, k, n_out)


@pytest.mark.parametrize("n_out", [33, 39, 40, 57, 64])
def test_partial_row_tiles(capped, n_out):
    """The epilogue's row count on claimed tiles: 9 objects of 3 column blocks on 8 workgroups."""
    product(capped, 9, 3, 13, n_out)


def test_tile_switch_at_every_ring_position(capped):
    """180 tiles of 13 sources on 8 workgroups: about 22 consecutive tiles per workgroup, each ending one body later in
    the 12-row ring than the one before, so the continuation after every body is taken."""
    product(capped, 20, 9, 13, 40)


POISON = 0x5A


def test_back_to_back_launches_and_graph_replays(capped):
    """Two shapes launched back to back on one context without a synchronisation between them, then one captured launch
    replayed three times, the outputs poisoned before every launch: 27 and 36 tiles on 8 workgroups, so most tiles are
    claims, and a launch that found a counter nonzero would skip tiles and leave their poison."""
    import torch

    ctx = capped
    a, b = (9, 3, 13, 40), (4, 9, 12, 64)
    (ca, ia, wa), (cb, ib, wb) = operands(*a), operands(*b)
    dca, dia, dcb, dib = up(ca), up(ia), up(cb), up(ib)
    dwa, dwb = up(wa), up(wb)
    outs_a = [torch.full(wa.shape, POISON, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    ob = torch.full(wb.shape, POISON, dtype=torch.uint8, device="cuda:0")
    das = [desc(dia, dca, o.data_ptr(), a[0], a[3], a[2], a[1] * BLK) for o in outs_a]
    db = desc(dib, dcb, ob.data_ptr(), b[0], b[3], b[2], b[1] * BLK)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        try:
            launch(ctx, das[0])
            launch(ctx, db)
            launch(ctx, das[1])
            s.synchronize()
            assert torch.equal(outs_a[0], dwa), "first launch"
            assert torch.equal(ob, dwb), "second launch, behind the first without a synchronisation"
            assert torch.equal(outs_a[1], dwa), "third launch"
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                launch(ctx, db)
            for r in range(3):
                ob.fill_(POISON)
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(ob, dwb), f"replay {r}"
        finally:
            ctx.use_own_stream()


def test_two_contexts_on_two_streams(capped):
    """Different shapes on two contexts at once, twice, every launch into a poisoned output of its own: each context
    claims from its own counters (shared ones would hand a context the other's indices: skipped tiles keep their
    poison)."""
    import torch

    import rlnc_amd

    ctx = capped
    other = rlnc_amd.Context(0)
    other.set_kernel_variant(8, 0)
    other.set_persistent_tiles(ALWAYS, WGS)
    a, b = (2 * compute_units() + 3, 1, 12, 33), (40, 9, 25, 57)
    (ca, ia, wa), (cb, ib, wb) = operands(*a), operands(*b)
    dca, dia, dcb, dib = up(ca), up(ia), up(cb), up(ib)
    oas = [torch.full(wa.shape, POISON, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    obs = [torch.full(wb.shape, POISON, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    for oa, ob in zip(oas, obs):
        launch(ctx, desc(dia, dca, oa.data_ptr(), a[0], a[3], a[2], a[1] * BLK))
        launch(other, desc(dib, dcb, ob.data_ptr(), b[0], b[3], b[2], b[1] * BLK))
    ctx.synchronize()
    other.synchronize()
    dwa, dwb = up(wa), up(wb)
    for r, (oa, ob) in enumerate(zip(oas, obs)):
        assert torch.equal(oa, dwa), f"first context, launch {r}"
        assert torch.equal(ob, dwb), f"second context, launch {r}"
    other.close()


@pytest.mark.parametrize("hdr", [False, True], ids=["nohdr", "hdr"])
@pytest.mark.parametrize("shape", [(9, 3, 13, 40), (13, 2, 12, 33)], ids=["27tiles-40rows", "26tiles-33rows"])
def test_footprint(capped, shape, hdr):
    """Outputs in a seeded arena with guards on both sides, rows padded by 48 bytes and objects 4 KiB + 16 apart: every
    documented byte written, nothing else changed, inputs unchanged.  hdr: a 64-byte slot before each row receives the
    row's coefficients (the persistent kernel's workgroups share the objects' header copies among them)."""
    from rlnc_amd._lib import MatmulDesc

    n_obj, blocks, k, n_out = shape
    coef, inp, want = operands(*shape)
    W = blocks * BLK
    slot = 64 if hdr else 0
    row = slot + W + 48
    obj = n_out * row + BLK + 16
    a = Arena(n_obj * obj, seed=sum(shape) + slot, largest_row_stride=row)
    if hdr:
        a.operand("hdr", 0, n_obj, obj, n_out, row, k)
        a.expect("hdr", coef)
    a.operand("out", slot, n_obj, obj, n_out, row, W)
    a.expect("out", want)
    a.device()
    d_coef, d_inp = up(coef), up(inp)
    launch(capped, MatmulDesc(d_inp.data_ptr(), k * W, W, d_coef.data_ptr(), n_out * k, k, a.ptr("out"), obj, row,
                              a.ptr("hdr") if hdr else None, obj if hdr else 0, row if hdr else 0, n_out, k, W, n_obj))
    a.check(a.after())
    assert_inputs_unchanged({"coef": (coef, d_coef), "in": (inp, d_inp)})


def test_misaligned_rows(capped):
    """The source at byte offset 1 and the pieces at offset 17 (where the device has unaligned vector access the product
    runs on them as they are, elsewhere on realigned copies): 27 tiles on 8 workgroups."""
    import torch

    n_obj, blocks, k, n_out = shape = (9, 3, 13, 40)
    coef, inp, want = operands(*shape)
    W = blocks * BLK
    d_coef = up(coef)
    src = torch.zeros(inp.size + 64, dtype=torch.uint8, device="cuda:0")
    src[1:1 + inp.size] = up(inp).reshape(-1)
    out = torch.full((want.size + 64,), 0x3C, dtype=torch.uint8, device="cuda:0")
    launch(capped, desc(src.data_ptr() + 1, d_coef, out.data_ptr() + 17, n_obj, n_out, k, W))
    torch.cuda.synchronize()
    assert torch.equal(out[17:17 + want.size], up(want).reshape(-1))
    assert bool((out[:17] == 0x3C).all()) and bool((out[17 + want.size:] == 0x3C).all())
    assert torch.equal(src[1:1 + inp.size], up(inp).reshape(-1))
