"""GPU: the device eliminations at the edges of their memory budgets (shapes and inputs: tests/limit_shapes.py).

  rank_large.hip  off 32 pieces per block (B = 28 .. 12), at the two shapes that use the block step's 160 KiB to the
                  byte, at the documented limit k = 4096, m = 8192, with pivots in the first and last column, and as
                  several objects of different layouts one after another in the one workspace of a ragged decode;
  rank.hip        at the largest shapes its LDS formula admits, and the first shapes beyond them;
  rref.hip        on both sides of its two borders: headers staged in LDS / the matrix only / the host;
  the product     T x data of a large-generation decode (n_in = m in the thousands), and on both sides of the narrow
                  kernel's own LDS cap.

A region undersized by a few dwords gives wrong bytes, not a fault, so every comparison is exact equality against a
checker that is no device code: the numpy model of tests/true_rank.py in rank mode 1, OracleDecoder in rank
mode 0, tests.gpu_util.np_matmul for products.  Output buffers start as 0xAA or -1."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import np_oracle as npo
from oracle.oracle import OracleDecoder
from tests import limit_shapes as ls
from tests.gpu_util import dev, host, np_matmul
from tests.test_gpu_parity import S, _sequences
from tests.stream_util import true_rank_context
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL, sparse_vectors, true_rank_model

pytestmark = pytest.mark.gpu
NOT_ALL_YET = 10
AUTO, DEVICE, DEVICE_ANY, LARGE = 0, 2, 7, 8


def _context(rank_mode):
    import torch

    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import rlnc_amd

    c = rlnc_amd.Context(0)
    c.set_rank_mode(rank_mode)
    return c


@pytest.fixture(scope="module")
def ctx1():
    """A context in rank mode 1 (tests set its decode path through `path` and get path 0 back)."""
    return true_rank_context()


@pytest.fixture(scope="module")
def ctx0():
    return _context(0)


@contextlib.contextmanager
def path(ctx, p):
    ctx.set_decode_path(p)
    try:
        yield ctx
    finally:
        ctx.set_decode_path(0)


@contextlib.contextmanager
def invalid_argument():
    from rlnc_amd.errors import RLNCError

    with pytest.raises(RLNCError) as ei:
        yield
    assert ei.value == RLNCError.InvalidArgument


def eliminate(ctx, pieces_t, k):
    import torch

    from rlnc_amd import batch

    nobj, m, _ = pieces_t.shape
    T = torch.full((nobj, k, m), 0xAA, dtype=torch.uint8, device="cuda:0")
    ps = torch.full((nobj, m), -1, dtype=torch.int32, device="cuda:0")
    rk = torch.full((nobj,), -1, dtype=torch.int32, device="cuda:0")
    batch.decode_batch_eliminate(pieces_t, k, T, ps, rk, ctx)
    return host(T), host(ps), host(rk)


def header_pieces(co, L=4):
    """co [nobj][m][k] -> pieces [nobj][m][k + L] with random payload bytes (the elimination reads the headers only)."""
    nobj, m, k = co.shape
    pieces = np.random.default_rng(k * 1000 + m).integers(0, 256, (nobj, m, k + L), dtype=np.uint8)
    pieces[:, :, :k] = co
    return pieces


def check_eliminate(ctx, co, models):
    """Mode-1 elimination of co [nobj][m][k] on the device == the model, object by object."""
    k = co.shape[2]
    T, ps, rk = eliminate(ctx, dev(header_pieces(co)), k)
    for o, (st, rank, Tm, _) in enumerate(models):
        assert list(ps[o]) == st, o
        assert rk[o] == rank, o
        assert np.array_equal(T[o], Tm), o


def coded(rng, co, st, src):
    """Pieces co || data: a useful piece carries its combination of the source rows, every other piece random garbage
    (in rank mode 1 T's column of such a piece is zero, so the decoded rows must not depend on it)."""
    useful = np.array(st) == OK
    data = rng.integers(0, 256, (co.shape[0], src.shape[1]), dtype=np.uint8)
    data[useful] = np_matmul(co[useful], src)
    return np.concatenate([co, data], axis=1)


def decode_both_ways(ctx, pieces, k, L):
    """decode_batch_device and decode_batch of one object -> [(statuses, object status, data length, rows)] x 2."""
    import torch

    from rlnc_amd import batch

    m = pieces.shape[0]
    pieces_t = dev(pieces[None])
    decoded = torch.full((1, k, L), 0xAA, dtype=torch.uint8, device="cuda:0")
    ps_d = torch.full((1, m), -1, dtype=torch.int32, device="cuda:0")
    os_d = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    dl_d = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    batch.decode_batch_device(pieces_t, k, decoded, ps_d, os_d, dl_d, ctx)
    first = (list(host(ps_d)[0]), int(host(os_d)[0]), int(host(dl_d)[0]), host(decoded)[0])
    decoded2 = torch.full((1, k, L), 0xAA, dtype=torch.uint8, device="cuda:0")
    pst, ost, dl = batch.decode_batch(pieces_t, k, decoded2, ctx)
    return [first, (list(pst[0]), int(ost[0]), int(dl[0]), host(decoded2)[0])]


# ---- rank_large.hip off B = 32 (decode path 8) -----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def narrow_objects(k, m):
    """The objects of one shape of ls.LARGE_NARROW and their models, computed once and left unchanged.
    Object 0: fewer basis vectors than k where k = 40 (the last piece brings the last of them); object 1 (k = 40):
    all 40, the last one in the middle of the pieces, so rank k is reached inside a later block and the rest answers
    ReceivedAllPieces; object 2: all 40, the last one with the last piece."""
    (B, nobj), = [(B, n) for kk, mm, B, n in ls.LARGE_NARROW if (kk, mm) == (k, m)]
    rng = np.random.default_rng(k * 10000 + m)
    if m <= 16:
        co = [ls.trickle(rng, k, m, B, m)]
    elif k == 40:
        co = [ls.trickle(rng, k, m, B, 36), ls.trickle(rng, k, m, B, 40, last_at=m // 2 + 3),
              ls.trickle(rng, k, m, B, 40)][:nobj]
    else:
        co = [ls.trickle(rng, k, m, B, 2 * B + B // 2 + 12)]
    assert len(co) == nobj
    for c in co:
        c.setflags(write=False)
    return B, np.stack(co), [true_rank_model(k, c) for c in co]


@pytest.mark.parametrize("k,m", [(k, m) for k, m, _, _ in ls.LARGE_NARROW])
def test_narrow_blocks(ctx1, k, m):
    from rlnc_amd import batch

    B, co, models = narrow_objects(k, m)
    assert batch.decode_large_workspace_bytes(k, m, 1) == 4 * ls.large_layout_total(k, m)  # B is the library's
    # the inputs reach the cases (asserted on the model)
    st, rank, _, Cm = models[0]
    piv = ls.pivot_columns(Cm)
    assert piv[0] == 0 and piv[-1] == k - 1  # the first and the last column (k = 4095: byte 2 of the last dword)
    assert st[-1] == OK  # the last piece is useful
    if m > 16:
        blocks = ls.blocks_of(st, B)
        assert blocks[0] == [OK] * B or (k == 40 and B > 28)  # a whole block of useful pieces
        assert any(OK not in b for b in blocks) and NOT_USEFUL in st  # a block with none
        burst = min(2 * B + B // 2, rank - 8)
        assert [st[burst + 1], st[burst + 3], st[burst + 2 * B + 1]] == [NOT_USEFUL] * 3  # zero, duplicate, multiple
        assert 32 <= rank <= 105
    else:
        assert st[m - 2] == NOT_USEFUL and rank == m - 1 - (m >= 8)
    if k == 40:
        st1, rank1, _, _ = models[1]
        full_at = st1.index(RECEIVED_ALL) - 1
        assert rank1 == k and full_at // B > 0 and st1[full_at] == OK  # rank k inside a block other than the first,
        assert all(set(b) == {RECEIVED_ALL} for b in ls.blocks_of(st1, B)[full_at // B + 1:])  # then whole such blocks
        assert len(ls.blocks_of(st1, B)) > full_at // B + 2
    if len(models) > 2:
        assert models[2][1] == k and models[2][0][-1] == OK
    with path(ctx1, LARGE):
        check_eliminate(ctx1, co, models)


def test_decode_through_a_narrow_block(ctx1):
    """Decode path 7 end to end at k = 40, m = 4796 (B = 28): rank 40 comes with the last piece."""
    k, m = ls.LARGE_NARROW[1][:2]
    B, co, models = narrow_objects(k, m)
    assert B == 28 and ls.rank_lds_bytes(k, m) > ls.MAX_LDS
    st, rank, _, _ = models[2]
    assert rank == k and st[-1] == OK
    L = 4096 + 16
    rng = np.random.default_rng(4796)
    data = rng.integers(0, 256, k * L - 7, dtype=np.uint8)
    src = npo.pad(data, k)
    pieces = coded(rng, co[2], st, src)
    with path(ctx1, DEVICE_ANY):
        for pst, ost, dl, rows in decode_both_ways(ctx1, pieces, k, L):
            assert pst == st
            assert ost == 0 and dl == data.size
            assert np.array_equal(rows, src)


# ---- rank.hip at its LDS edge (decode path 0, rank mode 1) -----------------------------------------------------------

def rank_edge_input(rng, k, m, kind):
    if kind == "trickle":
        return ls.trickle(rng, k, m, 2, k)
    if kind == "planted":
        return ls.planted3(rng, k, m)
    return sparse_vectors(rng, k, m, 3)


@pytest.mark.parametrize("fit,beyond", ls.RANK_EDGES, ids=[f"{k}-{m}" for (k, m), _ in ls.RANK_EDGES])
def test_rank_lds_edge(ctx1, fit, beyond):
    k, m = fit
    rng = np.random.default_rng(k * 10000 + m)
    kinds = (["trickle"] if k == 16 else []) + ["planted", "sparse"]
    co = np.stack([rank_edge_input(rng, k, m, kind) for kind in kinds])
    models = [true_rank_model(k, c) for c in co]
    if k == 16:
        assert models[0][0][-1] == OK and models[0][1] == k  # the last piece (of the widest row) is useful
    assert ls.slack(ls.rank_lds_bytes, fit) < ls.rank_row_bytes(*fit)
    check_eliminate(ctx1, co, models)  # the LDS kernel takes the largest shape of the formula ...
    kb, mb = beyond
    with invalid_argument():  # ... and nothing beyond it
        eliminate(ctx1, dev(np.zeros((1, mb, kb + 4), np.uint8)), kb)


@pytest.mark.parametrize("k,m", [(16, 4085), (224, 228)])
def test_first_shapes_beyond_rank_lds(ctx1, k, m):
    assert (k, m) in [beyond for _, beyond in ls.RANK_EDGES]
    rng = np.random.default_rng(k * 10000 + m)
    co = rank_edge_input(rng, k, m, "trickle" if k == 16 else "planted")
    model = true_rank_model(k, co)
    st, rank, _, _ = model
    assert rank == k
    L = 8
    data = rng.integers(0, 256, k * L - 3, dtype=np.uint8)
    src = npo.pad(data, k)
    pieces = coded(rng, co, st, src)
    from rlnc_amd import batch

    decoded = dev(np.full((1, k, L), 0xAA, np.uint8))
    pst, ost, dl = batch.decode_batch(dev(pieces[None]), k, decoded, ctx1)  # path 0: the host elimination
    assert list(pst[0]) == st and ost[0] == 0 and int(dl[0]) == data.size
    assert np.array_equal(host(decoded)[0], src)
    with path(ctx1, DEVICE_ANY):  # path 7: rank_large.hip
        check_eliminate(ctx1, co[None], [model])
        for pst, ost, dl, rows in decode_both_ways(ctx1, pieces, k, L):
            assert pst == st and ost == 0 and dl == data.size
            assert np.array_equal(rows, src)
    with invalid_argument():  # path 0 does not eliminate it on the device
        check_eliminate(ctx1, co[None], [model])


# ---- rref.hip across its two borders (rank mode 0) -------------------------------------------------------------------

RREF_SHAPES = [s for pair in ls.RREF_STAGED_EDGES + ls.RREF_EDGES for s in pair]


@pytest.mark.parametrize("k,m", RREF_SHAPES)
def test_rref_lds_borders(ctx0, k, m):
    from rlnc_amd import batch

    fits = ls.rref_lds_bytes(k, m) <= ls.MAX_LDS
    assert fits == ((k, m) not in [beyond for _, beyond in ls.RREF_EDGES])
    L, nobj = 8, 2
    for sparsity, dep in [(0.0, 0.0), (0.5, 0.03)]:
        rng = np.random.default_rng(k * 1000 + m + int(100 * sparsity))
        seqs = _sequences(rng, nobj, k, m, L, sparsity, dep)
        want = []
        for o in range(nobj):
            od = OracleDecoder(L, k)
            want.append(([S[od.decode(p)] for p in seqs[o]], od.padded_payload(), od.get_decoded_data()))
        pieces_t = dev(seqs)
        for p in (AUTO, DEVICE):
            decoded = dev(np.zeros((nobj, k, L), np.uint8))
            with path(ctx0, p):
                if p == DEVICE and not fits:  # beyond the general kernel: an error, not the host
                    with invalid_argument():
                        batch.decode_batch(pieces_t, k, decoded, ctx0)
                    continue
                pst, ost, dl = batch.decode_batch(pieces_t, k, decoded, ctx0)
            got = host(decoded)
            for o, (sts, pay, (st, data)) in enumerate(want):
                assert [S[x] for x in pst[o]] == sts, (p, o)
                assert np.array_equal(got[o, : pay.shape[0]], pay), (p, o)
                assert not got[o, pay.shape[0]:].any()
                assert S[ost[o]] == S[st], (p, o)
                if st == 0:
                    assert int(dl[o]) == data.size
    # the formula by behaviour: the device elimination takes the shape exactly when the mirror says it fits
    if fits:
        eliminate(ctx0, pieces_t, k)
    else:
        with invalid_argument():
            eliminate(ctx0, pieces_t, k)


# ---- rref.hip: one case per outcome of its dispatch (launch_rref_one and the two-pass wrapper; rank mode 0) -----------

SMALL_MIN_OBJECTS = 2048  # kSmallMinObjects (rref_kernels.hpp)
# name -> (k, m, objects)
RREF_OUTCOMES = {
    "blocked": (16, 18, 3),
    "small-8-dwords": (8, 10, SMALL_MIN_OBJECTS),
    "small-16-dwords": (16, 40, SMALL_MIN_OBJECTS),
    "two-pass": (128, 130, 2),
    "lds-staged": (130, 132, 2),
    "lds-unstaged": (224, 228, 2),
}


@functools.lru_cache(maxsize=None)
def outcome_case(name):
    """(pieces [nobj][m][k + m], per object (statuses, rank, T)) of one shape of RREF_OUTCOMES, computed once and left
    unchanged.  Piece j carries the unit vector e_j as its data, so the oracle's payload rows are T's rows.  Every
    object has a piece that is a combination of two earlier ones: piece 5 in odd objects, piece k / 2 in even ones (in
    the two-pass shape the last piece, so that the first 128 pieces alone reach rank k); every fourth object (the
    second, where there are two) has half of its coefficients zero, which takes the matrix out of the clean state."""
    k, m, nobj = RREF_OUTCOMES[name]
    rng = np.random.default_rng(k * 1000 + m)
    co = rng.integers(0, 256, (nobj, m, k), dtype=np.uint8)
    for o in range(nobj):
        if o % 4 == 1:
            co[o][rng.random((m, k)) < 0.5] = 0
        d = 5 if o % 2 else m - 1 if name == "two-pass" else k // 2
        co[o, d] = co[o, 1] ^ ls.MUL[int(rng.integers(2, 256))][co[o, 3]]
    pieces = np.concatenate([co, np.broadcast_to(np.eye(m, dtype=np.uint8), (nobj, m, m))], axis=2)
    want = []
    for o in range(nobj):
        od = OracleDecoder(m, k)
        st = [od.decode(p) for p in pieces[o]]
        rows = od.padded_payload()
        T = np.zeros((k, m), np.uint8)
        T[:rows.shape[0]] = rows
        want.append((st, rows.shape[0], T))
    pieces.setflags(write=False)
    return pieces, want


@pytest.mark.parametrize("name", list(RREF_OUTCOMES))
def test_rref_dispatch_outcomes(ctx0, name):
    """decode_batch_eliminate on decode path 0, one shape per kernel choice of rref.hip, exact against the oracle on
    statuses, rank and T.  Which choice a shape reaches is asserted on the mirrors of tests/limit_shapes.py: the
    small-object kernel from 2,048 objects of k <= 16 on, in its 8-dword and 16-dword row shapes; the blocked run while
    a row fits one wave (k + m <= 256); beyond that the two-pass split up to k = 128 (the first object reaches rank k
    within the blocked pass, the second does not and is redone by the general pass); else the one-wave LDS kernel, with
    the headers staged in LDS where they fit beside the matrix and without where only the matrix fits.  The borders of
    the two LDS forms themselves are test_rref_lds_borders' (other shapes); none of these six runs elsewhere in this
    module."""
    k, m, nobj = RREF_OUTCOMES[name]
    D = ls.rref_row_dwords(k, m)
    small = k <= 16 and nobj >= SMALL_MIN_OBJECTS and D <= 16
    reached = ("small-8-dwords" if small and D <= 8 else "small-16-dwords" if small else "blocked" if D <= 64 else
               "two-pass" if k <= 128 else
               "lds-staged" if ls.rref_lds_bytes_staged(k, m) <= ls.MAX_LDS else "lds-unstaged")
    assert reached == name
    assert ls.rref_lds_bytes(k, m) <= ls.MAX_LDS
    pieces, want = outcome_case(name)
    if name == "two-pass":  # pass 1 replays the first 256 - k = 128 pieces
        assert want[0][0] == [OK] * 128 + [RECEIVED_ALL] * 2 and NOT_USEFUL in want[1][0][:128]
    else:
        # the dependent piece of every dense object (the diagonal-pivot elimination may keep a sparse one's)
        assert all(NOT_USEFUL in st for o, (st, _, _) in enumerate(want) if o % 4 != 1)
    assert any(rank == k for _, rank, _ in want)
    T, ps, rk = eliminate(ctx0, dev(pieces.copy()), k)
    for o, (st, rank, Tw) in enumerate(want):
        assert list(ps[o]) == st, o
        assert rk[o] == rank, o
        assert np.array_equal(T[o], Tw), o


# ---- several beyond-LDS objects in the one workspace of a ragged decode ----------------------------------------------

@functools.lru_cache(maxsize=None)
def ragged_objects():
    """(k, m, data, source rows, pieces, model) per object, in the order that reuses the workspace by a larger layout,
    then a smaller one, then across a change of B."""
    rng = np.random.default_rng(5)
    L = 16
    k40, m40 = ls.LARGE_NARROW[1][:2]
    deficient = np_matmul(rng.integers(0, 256, (310, 290), dtype=np.uint8),
                          rng.integers(0, 256, (290, 300), dtype=np.uint8))  # 310 pieces of a 290-dimensional span
    deficient[7] = 0
    vectors = [rng.integers(0, 256, (304, 300), dtype=np.uint8), sparse_vectors(rng, 16, 20, 2),
               narrow_objects(k40, m40)[1][2], ls.planted(rng, 24, 67), deficient]
    out = []
    for i, co in enumerate(vectors):
        m, k = co.shape
        model = narrow_objects(k40, m40)[2][2] if i == 2 else true_rank_model(k, co)
        data = rng.integers(0, 256, k * L - 2, dtype=np.uint8)
        src = npo.pad(data, k)
        out.append((k, m, data, src, coded(rng, co, model[0], src), model))
    return out


def test_ragged_objects_share_the_workspace(ctx1):
    import torch

    from rlnc_amd import batch

    objs = ragged_objects()
    assert [(k, m) for k, m, *_ in objs] == [(300, 304), (16, 20), (40, 4796), (24, 67), (300, 310)]
    assert [ls.large_block(k, m) for k, m, *_ in objs] == [32, 32, 28, 32, 32]
    sizes = [ls.large_layout_total(k, m) for k, m, *_ in objs]
    assert len(set(sizes)) == 5 and sizes[2] == max(sizes) and sizes[4] > sizes[0]  # five layouts, up and down
    assert [mdl[1] for *_, mdl in objs] == [300, objs[1][5][1], 40, 24, 290]
    for p in (DEVICE_ANY, LARGE):  # path 8: the LDS-sized objects go through the workspace too
        tensors = [(dev(pieces), k, torch.full((k, 16), 0xAA, dtype=torch.uint8, device="cuda:0"))
                   for k, m, _, _, pieces, _ in objs]
        with path(ctx1, p):
            ps, os_, dl = batch.decode_ragged(tensors, ctx1)
            ps, os_, dl = host(ps), host(os_), host(dl)
        at = 0
        for i, (k, m, data, src, _, (st, rank, _, _)) in enumerate(objs):
            assert list(ps[at:at + m]) == st, (p, i)
            at += m
            if rank == k:
                assert os_[i] == 0 and dl[i] == data.size, (p, i)
                assert np.array_equal(host(tensors[i][2]), src), (p, i)
            else:
                assert os_[i] == NOT_ALL_YET, (p, i)
    # the workspace is left in the (300, 310) layout: a batch of another shape must not see it
    k, m, _, _, pieces, model = objs[3]
    with path(ctx1, LARGE):
        check_eliminate(ctx1, pieces[None, :, :k], [model])


# ---- the wide products behind a large-generation decode --------------------------------------------------------------

_CAP = ls.narrow_max_n_in()  # the narrow kernel's tables fill its 64 KiB at n_in = 819


@pytest.mark.parametrize("n_out,n_in,W,nobj", [(5, ls.LARGE_MAX_M, 4096 + 16, 1), (33, 4832, 4096, 1),
                                               (3, 2000, 8192, 1), (40, _CAP, 100, 1), (40, _CAP + 1, 100, 1),
                                               (40, 1100, 16, 2)])
def test_wide_products(ctx0, n_out, n_in, W, nobj):
    import torch

    from rlnc_amd import batch

    assert (_CAP, ls.narrow_lds_bytes(_CAP), ls.narrow_lds_bytes(_CAP + 1)) == (819, 65520, 65600)
    rng = np.random.default_rng(n_out * 1000 + n_in * 10 + W + nobj)
    coef = rng.integers(0, 256, (nobj, n_out, n_in), dtype=np.uint8)
    coef[:, 0, :] = 1
    coef[:, n_out // 2, :] = 0
    inp = rng.integers(0, 256, (nobj, n_in, W), dtype=np.uint8)
    inp[:, n_in - 1, :min(256, W)] = np.arange(min(256, W), dtype=np.uint8)
    out = torch.full((nobj, n_out, W), 0xAA, dtype=torch.uint8, device="cuda:0")
    batch.matmul(dev(coef), dev(inp), out, ctx0)
    got = host(out)
    for o in range(nobj):
        assert np.array_equal(got[o], np_matmul(coef[o], inp[o])), o
