"""CPU: the size formulas of the device eliminations as tests/limit_shapes.py restates them, the shapes derived from
them, and the input family of tests/test_gpu_elimination_limits.py -- without a GPU.

The large-generation mirror is pinned to the library through rlnc_decode_large_workspace_bytes (a block size off by one
step of 4 moves that figure by 16 x D bytes, so the equality fixes the block size as well).  The two LDS mirrors are
pinned on the GPU by which shapes the library accepts; here their slack figures are checked."""
import numpy as np
import pytest

from rlnc_amd import batch
from tests import limit_shapes as ls
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL, host_run, true_rank_model

WIDER_THAN_A_ROW = {(130, 482), (269, 271)}  # test_lds_edges
LARGE_SHAPES = sorted({(k, m) for k, m, _, _ in ls.LARGE_NARROW} | set(ls.LARGE_OTHER))


@pytest.mark.parametrize("k,m", LARGE_SHAPES)
def test_large_workspace_mirror(k, m):
    assert batch.decode_large_workspace_bytes(k, m, 1) == 4 * ls.large_layout_total(k, m)
    assert batch.decode_large_workspace_bytes(k, m, 3) == 3 * 4 * ls.large_layout_total(k, m)


def test_a_block_size_off_by_one_step_shows_in_the_workspace_size(monkeypatch):
    for k, m, B, _ in ls.LARGE_NARROW:
        want = batch.decode_large_workspace_bytes(k, m, 1)
        for off in (-4, 4):
            with monkeypatch.context() as mp:
                mp.setattr(ls, "large_block", lambda k_, m_, B_=B + off: B_)
                assert 4 * ls.large_layout_total(k, m) == want + off * 4 * ls.large_row_dwords(k, m), (k, m, off)


def test_narrow_block_shapes():
    assert [(k, m) for k, m, _, _ in ls.LARGE_NARROW] == [
        (40, 4792), (40, 4796), (40, 6000), (40, 7000), (40, 8192), (1472, 8192), (1476, 8192), (4096, 8192),
        (4095, 4837), (4096, 4), (2000, 8)]
    for k, m, B, _ in ls.LARGE_NARROW:
        assert ls.large_block(k, m) == B, (k, m)
        assert ls.large_step_lds_bytes(k, m) <= ls.MAX_LDS
        assert ls.LARGE_STEP_FIXED + 4 * (B + 4) * ls.large_row_dwords(k, m) > ls.MAX_LDS or B == ls.LARGE_MAX_B
    assert {B for _, _, B, _ in ls.LARGE_NARROW} == {12, 16, 20, 24, 28, 32}
    assert ls.large_row_dwords(40, 4792) == 1208 and ls.large_row_dwords(1472, 8192) == 2416
    for k, m in ls.LARGE_ZERO_SLACK:  # the step kernel's LDS to the byte; one more dword per row costs a step of B
        assert ls.large_step_lds_bytes(k, m) == ls.MAX_LDS
        assert ls.large_block(k + (-k % 4) + 1, m) == ls.large_block(k, m) - 4
    # m is no multiple of B, with more than one block
    assert sum(1 for k, m, B, _ in ls.LARGE_NARROW if m > B and m % B) >= 2
    assert ls.large_block(ls.LARGE_MAX_K, ls.LARGE_MAX_M) == 12 and ls.large_block(4097, 8192) == 0


@pytest.mark.parametrize("lds,row,edges,shapes,slacks", [
    (ls.rank_lds_bytes, ls.rank_row_bytes, ls.RANK_EDGES, [(16, 4084), (200, 278), (64, 1124), (223, 227)],
     [16, 176, 224, 176]),
    (ls.rref_lds_bytes_staged, ls.rref_row_bytes, ls.RREF_STAGED_EDGES, [(200, 259), (130, 482), (218, 220)],
     [100, 628, 200]),
    (ls.rref_lds_bytes, ls.rref_row_bytes, ls.RREF_EDGES, [(130, 966), (269, 271)], [8, 568]),
], ids=["rank", "rref-staged", "rref"])
def test_lds_edges(lds, row, edges, shapes, slacks):
    assert [fit for fit, _ in edges] == shapes
    assert [ls.slack(lds, fit) for fit, _ in edges] == slacks
    for fit, beyond in edges:
        assert beyond in ((fit[0], fit[1] + 1), (fit[0] + 1, fit[1] + 1))
        assert 0 <= ls.slack(lds, fit) < lds(*beyond) - lds(*fit), fit  # the largest that fits: the next one does not
        assert lds(*beyond) > ls.MAX_LDS, beyond
        # less than one row to spare -- but for two shapes of rref.hip, whose next shape costs more than a row: at
        # (130, 482) with staged headers one more piece is 130 header bytes and a dword on each of the 131 rows (652 B
        # against the 628 B left, a row is 612 B); at (269, 271) one more k is a row and a dword on every row (1624 B
        # against 568 B, a row is 540 B)
        if fit not in WIDER_THAN_A_ROW:
            assert ls.slack(lds, fit) < row(*fit), fit
        else:
            assert row(*fit) <= ls.slack(lds, fit) < row(*fit) + 32, fit
    # every shape beyond rank.hip is inside rank_large.hip's limits (decode path 7 takes it)
    assert all(ls.large_block(*beyond) == 32 for _, beyond in ls.RANK_EDGES)


def test_staged_shapes_fit_unstaged_and_the_widest_row():
    for fit, beyond in ls.RREF_STAGED_EDGES:
        assert ls.rref_lds_bytes(*beyond) <= ls.MAX_LDS  # beyond the staged form: the matrix-only form, not the host
    assert ls.large_row_dwords(16, 4084) == 1025


def test_rref_row_dwords_rounding():
    assert [ls.rref_row_dwords(k, m) for k, m in [(1, 1), (1, 3), (3, 2), (8, 9), (16, 20), (60, 68), (120, 129),
                                                   (126, 126), (126, 127), (128, 130), (218, 220)]] == \
        [1, 1, 2, 8, 16, 32, 64, 64, 64, 65, 110]


def test_narrow_product_cap():
    n = ls.narrow_max_n_in()
    assert n == 819 and ls.narrow_lds_bytes(n) <= ls.NARROW_MAX_LDS < ls.narrow_lds_bytes(n + 1)


def test_sparse_basis_is_independent():
    rng = np.random.default_rng(4)
    for k, nb in [(40, 40), (40, 33), (4095, 50), (2, 2)]:
        basis = ls.sparse_basis(rng, k, nb)
        assert basis.shape == (nb, k) and (np.count_nonzero(basis, axis=1) <= 6).all()
        assert true_rank_model(k, basis)[1] == nb
        assert basis[0, 0] != 0 and list(np.nonzero(basis[1])[0]) == [k - 1]


@pytest.mark.parametrize("k,m,B,nb,last_at", [(40, 300, 28, 40, None), (40, 300, 28, 40, 150), (45, 211, 12, 30, None),
                                              (64, 8, 32, 8, None), (64, 4, 32, 4, None)])
def test_trickle_family_reaches_its_cases(k, m, B, nb, last_at):
    """The family does what its description says, at shapes small enough for the host elimination to be compared
    with the model as well."""
    co = ls.trickle(np.random.default_rng(m + B), k, m, B, nb, last_at)
    st, rank, T, Cm = true_rank_model(k, co)
    got = host_run(k, co, True)
    assert got[0] == st and got[1] == rank and np.array_equal(got[2], T)
    piv = ls.pivot_columns(Cm)
    assert 0 in piv and k - 1 in piv
    if m <= 16:
        assert rank == m - 1 - (m >= 8) and st[m - 2] == NOT_USEFUL and st[-1] == OK
        return
    blocks = ls.blocks_of(st, B)
    burst = min(2 * B + B // 2, nb - 8)
    assert st[:burst] == [OK] * burst and (burst < B or blocks[0] == [OK] * B)
    assert st[burst + 1] == NOT_USEFUL and st[burst + 3] == NOT_USEFUL and st[burst + 2 * B + 1] == NOT_USEFUL
    assert any(OK not in b for b in blocks)  # a block with no useful piece
    assert rank == nb
    if last_at is None:
        assert st[-1] == OK  # the last piece brings the last dimension
    else:
        assert st[last_at] == OK and last_at // B > 0 and st[last_at + 1:] == [RECEIVED_ALL] * (m - 1 - last_at)
