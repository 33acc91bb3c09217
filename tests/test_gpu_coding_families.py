"""GPU: every elimination kernel on the structured coding-vector families of tests/coding_families.py.

Rank mode 0 (the reference's diagonal-pivot elimination) against the reference oracle, piece by piece: the two
small-object kernels, the blocked run (its dirty step of at most 8 rows on `gf2`; the many-dirty-rows fallback and the
re-extension of the clean prefix from 0 to k in one piece on `reversed` and its kin), the two-pass split, the one-wave
kernel with its headers staged in LDS and read from global memory, the host engine, and the ragged decode.  Rank mode 1
against true_rank_model: one workgroup and one wave per object, the workspace kernels of decode path 8, and both forms
of a decode stream's push.  Which shape reaches which kernel is read from launch_rref_one / launch_rref_batch
(rref.hip), launch_rank_batch (rank.hip) and the stream's launches, and asserted here from the size formulas of
tests/limit_shapes.py (the kernels one run launched: profiles/r15_family_kernels.txt); what each family does to the
matrix is asserted from the oracle (tests/coding_families.py, profile).  All comparisons are exact."""
import numpy as np
import pytest

from oracle import np_oracle as npo
from oracle.oracle import OracleDecoder
from tests import coding_families as cf
from tests import limit_shapes as ls
from tests.gpu_util import dev, host, np_matmul
from tests.stream_util import Prefixes, advance, check_snapshot, i32, true_rank_context
from tests.test_gpu_true_rank import check_decoded, check_eliminate
from tests.true_rank import RECEIVED_ALL, true_rank_model

pytestmark = pytest.mark.gpu

SMALL_MIN_OBJECTS, SMALL_NW = 2048, 4  # kSmallMinObjects, kSmallNW (rref_kernels.hpp)
WAVE_MIN_OBJECTS = 1024                # rank.hip launch_rank_batch: one wave per object from here on
DIRTY_STEP_ROWS = 8                    # kBlkB: more dirty rows than this take the blocked run's generic fallback
UNSTAGED = ls.RREF_STAGED_EDGES[0][1]  # (200, 260): the first m at k = 200 whose headers do not fit beside the matrix
WORKSPACE, LDS = 1, 2                  # rlnc_set_stream_form
LARGE = 8                              # RLNC_DECODE_PATH_LARGE
WHOLE_MATRIX = ("reversed", "shift", "upper_rev")


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    return rlnc_amd.Context(0)


@pytest.fixture(scope="module")
def ctx1():
    return true_rank_context()


# ---- the cases: one object per (family, shape, L, seed), its references computed once and left unchanged ------------
class Case:
    def __init__(self, name, k, m, L, seed):
        self.name, self.k, self.m, self.L = name, k, m, L
        self.co = cf.vectors(name, k, m, seed)
        rng = np.random.default_rng([cf.NAMES.index(name), k, m, L])
        self.data = rng.integers(0, 256, k * L - 1 - cf.NAMES.index(name) % min(k, L), dtype=np.uint8)
        self.src = npo.pad(self.data, k)
        assert self.src.shape == (k, L)
        self.pieces = np.concatenate([self.co, np_matmul(self.co, self.src)], axis=1)
        self._ref = self._model = self._profile = None

    @property
    def ref(self):
        """The reference decoder over the pieces: (statuses, padded payload rows, get_decoded_data status, length)."""
        if self._ref is None:
            od = OracleDecoder(self.L, self.k)
            st = [od.decode(p) for p in self.pieces]
            fin, data = od.get_decoded_data()
            self._ref = (st, od.padded_payload(), fin, data.size if fin == 0 else None)
        return self._ref

    @property
    def model(self):
        if self._model is None:
            self._model = true_rank_model(self.k, self.co)
        return self._model

    @property
    def profile(self):
        if self._profile is None:
            self._profile = cf.profile(cf.reference_trace(self.k, self.pieces), self.model)
        return self._profile


_cases = {}


def case(name, k, m, L=8, seed=None):
    key = (name, k, m, L, seed)
    if key not in _cases:
        _cases[key] = Case(name, k, m, L, seed)
    return _cases[key]


def all_families(k, m, L=8):
    return [case(n, k, m, L) for n in cf.NAMES]


def seeded(k, m, count, seeds=4):
    """count objects: the families over `seeds` seeds, repeated.  Returns (cases per object, distinct)."""
    base = [case(n, k, m, 8, s) for s in range(seeds) for n in cf.NAMES]
    return [base[o % len(base)] for o in range(count)], len(base)


# ---- rank mode 0 -----------------------------------------------------------------------------------------------------
def check_mode0(ctx, cases, path):
    """decode_batch over the cases (one shape) == the reference decoder: every status, the payload rows, zeros after
    them, the final status and length."""
    import torch

    from rlnc_amd import batch

    k, L = cases[0].k, cases[0].L
    seqs = dev(np.stack([c.pieces for c in cases]))
    decoded = torch.full((len(cases), k, L), 0xAA, dtype=torch.uint8, device="cuda:0")
    ctx.set_decode_path(path)
    try:
        pst, ost, dl = batch.decode_batch(seqs, k, decoded, ctx)
    finally:
        ctx.set_decode_path(0)
    got = host(decoded)
    for o, c in enumerate(cases):
        st, pay, fin, size = c.ref
        assert list(pst[o]) == st, (o, c.name, list(pst[o]), st)
        assert np.array_equal(got[o, : pay.shape[0]], pay), (o, c.name)
        assert not got[o, pay.shape[0]:].any(), (o, c.name)
        assert ost[o] == fin, (o, c.name, ost[o], fin)
        if fin == 0:
            assert int(dl[o]) == size, (o, c.name)


def assert_block_states(cases):
    """The states of the blocked run that the families are there for, from the oracle alone."""
    k = cases[0].k
    by = {c.name: c.profile for c in cases}
    for n in ("identity", "upper", "lower"):  # the clean run alone
        assert by[n]["dirty_pieces"] == 0
    for n in WHOLE_MATRIX:  # the fallback beyond 8 dirty rows, then the prefix re-extended from 0 to k in one piece
        assert by[n]["max_dirty_rows"] == k - 1 > DIRTY_STEP_ROWS and by[n]["reclean"] == [k - 1]
    for n in ("perm", "band", "halves"):
        assert 2 * by[n]["max_dirty_rows"] >= k > DIRTY_STEP_ROWS
    g = by["gf2"]  # in and out of the clean state within the dirty step
    assert 2 <= g["max_dirty_rows"] <= DIRTY_STEP_ROWS and len(g["reclean"]) >= 3
    for n in ("highspan", "fixture_blocks"):
        assert by[n]["differ"]


@pytest.mark.parametrize("k,m,groups", [(8, 12, 8), (16, 40, 4)])
def test_mode0_small_object_kernels(ctx, k, m, groups):
    """2,051 objects of k <= 16: gf_rref_small_kernel<4,8,2> for rows of at most 8 dwords (the last workgroup holds
    three objects), gf_rref_small_kernel<1,4,4> for rows of up to 16."""
    nobj = SMALL_MIN_OBJECTS + 3
    D = ls.rref_row_dwords(k, m)
    assert k <= 16 and (D <= 8 if groups == 8 else 8 < D <= 16) and nobj % SMALL_NW == 3
    cases, distinct = seeded(k, m, nobj)
    assert any(c.profile["max_dirty_rows"] == k - 1 for c in cases[:distinct])
    assert any(c.profile["differ"] for c in cases[:distinct])
    check_mode0(ctx, cases, 0)


@pytest.mark.parametrize("path", [0, 5])
@pytest.mark.parametrize("k,m", [(16, 40), (24, 40), (64, 72), (100, 130)])
def test_mode0_blocked_run(ctx, k, m, path):
    """gf_rref_block_kernel, one object per family (too few objects for the small-object kernel at k = 16)."""
    assert ls.rref_row_dwords(k, m) <= 64 and len(cf.NAMES) < SMALL_MIN_OBJECTS
    cases = all_families(k, m)
    assert_block_states(cases)
    check_mode0(ctx, cases, path)


def test_mode0_two_pass_split(ctx):
    """(128, 130): the blocked run over the first 256 - k = 128 pieces, the one-wave kernel over all 130 for the objects
    still short of rank k."""
    k, m = 128, 130
    assert ls.rref_row_dwords(k, m) > 64 and ls.rref_row_dwords(k, 256 - k) <= 64 and 256 - k == k
    cases = all_families(k, m)
    assert_block_states(cases)
    by = {c.name: c for c in cases}
    for n in ("lowrank", "fixture_blocks"):  # the second pass has work to do
        assert by[n].ref[0][:k].count(0) < k
    st = by["reversed"].ref[0]  # complete on the first pass's last piece
    assert st[:k] == [0] * k and st[k:] == [RECEIVED_ALL] * (m - k)
    check_mode0(ctx, cases, 0)


@pytest.mark.parametrize("k,m,staged", [(130, 132, True), UNSTAGED + (False,)])
def test_mode0_one_wave_kernel(ctx, k, m, staged):
    """gf_rref_batch_kernel (decode path 2, k > 128), the piece headers staged in LDS or read from global memory."""
    assert k > 128 and ls.rref_row_dwords(k, m) > 64 and ls.rref_lds_bytes(k, m) <= ls.MAX_LDS
    assert (ls.rref_lds_bytes_staged(k, m) <= ls.MAX_LDS) == staged
    cases = all_families(k, m)
    assert_block_states(cases)
    check_mode0(ctx, cases, 2)


def test_mode0_host_engine_behind_decode_batch(ctx):
    cases = all_families(64, 72)
    check_mode0(ctx, cases, 1)


def test_mode0_decode_ragged(ctx):
    """One ragged decode of every family at every shape up to the two-pass and one-wave ones, interleaved: the blocked
    launch and the general launch of rref_ragged_object (wire.hip)."""
    import torch

    from rlnc_amd import batch

    shapes = [(8, 12), (16, 40), (24, 40), (64, 72), (100, 130), (128, 130), (130, 132)]
    cases = [c for k, m in shapes for c in all_families(k, m)]
    cases = [cases[i] for i in np.random.default_rng(0xFA).permutation(len(cases))]
    objs = [(dev(c.pieces), c.k, torch.full((c.k, c.L), 0xAA, dtype=torch.uint8, device="cuda:0")) for c in cases]
    ps, ost, dl = batch.decode_ragged(objs, ctx)
    ps, ost, dl = host(ps), host(ost), host(dl)
    off = 0
    for i, (c, (_, _, dec)) in enumerate(zip(cases, objs)):
        st, pay, fin, size = c.ref
        assert list(ps[off: off + c.m]) == st, (i, c.name, c.k)
        off += c.m
        assert int(ost[i]) == fin, (i, c.name, c.k)
        if pay.shape[0] == c.k:
            assert np.array_equal(host(dec), pay), (i, c.name, c.k)
        if fin == 0:
            assert int(dl[i]) == size, (i, c.name, c.k)


def test_mode0_scaled_permutation_product(ctx):
    """k = 24 unit-vector families with L = 4096 + 16: T is a scaled permutation, so every row of the bit-sliced
    T x data product has 23 zero coefficients and one nonzero.  The decoded rows are the source."""
    k, L = 24, 4096 + 16
    cases = [case(n, k, k, L) for n in ("identity", "reversed", "perm", "shift")]
    for c in cases:
        assert ((c.co != 0).sum(0) == 1).all() and ((c.co != 0).sum(1) == 1).all()
        assert np.array_equal(c.ref[1], c.src) and c.ref[2] == 0
    check_mode0(ctx, cases, 0)


# ---- rank mode 1 -----------------------------------------------------------------------------------------------------
def vectors_of(cases):
    return np.stack([c.co for c in cases])


def assert_pivot_orders(cases):
    """What the families are to mode 1: in `reversed` every new pivot column sorts before all earlier ones; the
    rank-deficient ones answer PieceNotUseful."""
    by = {c.name: c for c in cases}
    k = cases[0].k
    _, rank, T, _ = by["reversed"].model
    assert rank == k and np.array_equal(T[:, :k], np.eye(k, dtype=np.uint8)[::-1])
    for n in ("lowrank", "dupzero", "highspan", "fixture_blocks"):
        assert 8 in by[n].model[0]


@pytest.mark.parametrize("k,m", [(24, 40), (64, 72), UNSTAGED])
def test_mode1_one_workgroup_per_object(ctx1, k, m):
    assert ls.rank_lds_bytes(k, m) <= ls.MAX_LDS and k > 16
    cases = all_families(k, m)
    assert_pivot_orders(cases)
    check_eliminate(ctx1, vectors_of(cases))


@pytest.mark.parametrize("k,m", [(8, 12), (16, 40)])
def test_mode1_one_wave_per_object(ctx1, k, m):
    nobj = WAVE_MIN_OBJECTS + 3
    assert k <= 16 and ls.large_row_dwords(k, m) <= 16
    cases, distinct = seeded(k, m, nobj)
    check_eliminate(ctx1, vectors_of(cases), distinct=distinct)


@pytest.mark.parametrize("k,m,blocks", [(8, 12, [12]), (16, 40, [32, 8]), (24, 40, [32, 8]), (64, 72, [32, 32, 8])])
def test_mode1_workspace_kernels(ctx1, k, m, blocks):
    """Decode path 8: gf_rank_large_reduce / _step / _update per block of pieces, then gf_rank_large_final."""
    B = ls.large_block(k, m)
    assert [min(B, m - at) for at in range(0, m, B)] == blocks
    cases = all_families(k, m)
    assert_pivot_orders(cases)
    ctx1.set_decode_path(LARGE)
    try:
        check_eliminate(ctx1, vectors_of(cases))
    finally:
        ctx1.set_decode_path(0)


_prefixes = {}


@pytest.mark.parametrize("max_new", [None, 5, 1])
@pytest.mark.parametrize("form", [WORKSPACE, LDS])
def test_mode1_decode_stream(ctx1, form, max_new):
    """Both forms of a push at (24, 40): the latch / reduce / step / update launches over the workspace, and
    gf_rank_stream_push in LDS -- everything in one push, five pieces per push, one piece per push.  After every push
    the snapshot is the model of each object's prefix."""
    import torch

    from rlnc_amd import batch

    k, m = 24, 40
    assert batch.stream_lds_fits(k, m)
    cases = all_families(k, m)
    co = vectors_of(cases)
    nobj = len(cases)
    if "model" not in _prefixes:
        _prefixes["model"] = Prefixes(k, co)
    model = _prefixes["model"]
    pieces = dev(np.stack([c.pieces for c in cases]))
    stream = batch.DecodeStream(k, m, nobj, ctx1)
    done = [0] * nobj
    rounds = 1 if max_new is None else -(-m // max_new)
    ctx1.set_stream_form(form)
    try:
        for r in range(rounds):
            av = torch.full((nobj,), m, dtype=torch.int32, device="cuda:0")
            rank, answered = i32(nobj), i32(nobj)
            stream.push(pieces, av, max_new, rank, answered)
            done = advance(done, [m] * nobj, m, max_new)
            assert list(host(answered)) == done, (r, done)
            assert list(host(rank)) == [model(o, done[o])[1] for o in range(nobj)], r
            check_snapshot(stream, model, done, r)
    finally:
        ctx1.set_stream_form(0)
    assert done == [m] * nobj
    for o, c in enumerate(cases):  # the last snapshot was the one-shot model's
        assert model(o, m)[0] == c.model[0] and model(o, m)[1] == c.model[1]


def test_mode1_decode_batch_device(ctx1):
    """decode_batch_device at (24, 40), L = 64: where the rank is k the decoded bytes are the source."""
    import torch

    from rlnc_amd import batch

    k, m, L = 24, 40, 64
    cases = all_families(k, m, L)
    objs = [(c.data, c.src, c.pieces, c.model) for c in cases]
    n = len(cases)
    pieces = dev(np.stack([c.pieces for c in cases]))
    decoded = torch.full((n, k, L), 0xAA, dtype=torch.uint8, device="cuda:0")
    ps = torch.full((n, m), -1, dtype=torch.int32, device="cuda:0")
    os_ = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    dl = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    batch.decode_batch_device(pieces, k, decoded, ps, os_, dl, ctx1)
    full = check_decoded(objs, k, host(decoded), host(ps), host(os_), host(dl))
    assert full == sum(c.model[1] == k for c in cases) >= 10


# ---- both modes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,L", [(24, 40, 64), (64, 72, 8)])
def test_cross_mode_decoded_bytes(ctx, ctx1, k, m, L):
    """Where the two modes' statuses agree and the rank is k, both modes' decode_batch return the same decoded bytes:
    the source."""
    import torch

    from rlnc_amd import batch

    cases = [c for c in all_families(k, m, L) if not c.profile["differ"] and c.model[1] == k]
    assert len(cases) >= 9 and {"reversed", "gf2", "band"} <= {c.name for c in cases}
    pieces = dev(np.stack([c.pieces for c in cases]))
    out = []
    for c in (ctx, ctx1):
        dec = torch.full((len(cases), k, L), 0xAA, dtype=torch.uint8, device="cuda:0")
        pst, ost, dl = batch.decode_batch(pieces, k, dec, c)
        out.append((host(dec), pst, ost, dl))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    for o, c in enumerate(cases):
        assert np.array_equal(out[0][0][o], c.src), c.name
        assert out[0][2][o] == 0 and int(out[0][3][o]) == c.data.size, c.name
