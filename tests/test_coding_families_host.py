"""CPU: the host elimination on the structured coding-vector families of tests/coding_families.py -- rank mode 0 against
the reference oracle, rank mode 1 against true_rank_model -- and the reach conditions: what each family must do to the
reference's matrix to be worth its place (hold the clean state, leave it for the whole matrix and re-clean in one piece,
go in and out of it below the blocked run's 8-row limit, tell the two rank modes apart).  The conditions are asserted
from the oracle and the model alone; tests/test_gpu_coding_families.py sends the same vectors through every device
kernel.  Every comparison is exact."""
import numpy as np
import pytest

from tests import coding_families as cf
from tests.true_rank import NOT_USEFUL, OK, RECEIVED_ALL, check_against_model

SHAPES = [(6, 8), (8, 12), (16, 40), (24, 40), (64, 72), (126, 130), (130, 132)]
_memo = {}


def case(name, k, m):
    """(vectors, reference trace, true-rank model checked against the host engine's mode 1, profile), once per case."""
    if (name, k, m) not in _memo:
        co = cf.vectors(name, k, m)
        trace = cf.reference_trace(k, co)
        model = check_against_model(k, co)
        _memo[(name, k, m)] = (co, trace, model, cf.profile(trace, model))
    return _memo[(name, k, m)]


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("name", cf.NAMES)
def test_host_engine_both_modes(orc, name, k, m):
    from rlnc_amd.elimination import Elimination

    co, (st, rows, _), model, prof = case(name, k, m)  # mode 1: check_against_model, inside case()
    assert co.shape == (m, k) and co.dtype == np.uint8
    e = Elimination(k, rank_mode=0)
    assert [e.push(h)[0] for h in co] == st
    assert e.rank == rows[-1]
    assert prof["true_rank"] == model[1] <= rows[-1]  # the diagonal-pivot elimination never under-counts


def test_family_layout():
    """What family() promises about the rows: the named structure in rows 0 .. k - 1, dense rows from k on."""
    k, m = 24, 40
    rows = {n: cf.vectors(n, k, m) for n in cf.NAMES}
    eye = np.eye(k, dtype=np.uint8)
    assert np.array_equal(rows["identity"][:k], eye) and np.array_equal(rows["reversed"][:k], eye[::-1])
    for n in ("shift", "perm"):
        assert ((rows[n][:k] != 0).sum(0) == 1).all() and ((rows[n][:k] != 0).sum(1) == 1).all()
    assert all(rows["shift"][i, (i + 1) % k] for i in range(k))
    nz = {n: rows[n][:k] != 0 for n in cf.NAMES}
    assert np.array_equal(nz["upper"], np.triu(np.ones((k, k), bool)))
    assert np.array_equal(nz["lower"], np.tril(np.ones((k, k), bool)))
    for n in ("upper", "lower"):  # the same rows in reverse order, under the same generator
        fwd, rev = (cf.family(n + s, k, m, np.random.default_rng(7)) for s in ("", "_rev"))
        assert np.array_equal(rev[:k], fwd[:k][::-1]) and np.array_equal(rev[k:], fwd[k:])
    first = sorted(int(np.nonzero(r)[0][0]) for r in rows["band"][:k])
    assert first == list(range(k)) and all(r.sum() == min(cf.BAND, k - int(np.nonzero(r)[0][0])) for r in nz["band"])
    assert rows["gf2"][:k].max() == 1
    h = k // 2
    assert not nz["halves"][:h, :h].any() and not nz["halves"][h:, h:].any()
    assert nz["halves"][:h, h:].all() and nz["halves"][h:, :h].all()
    assert not nz["highspan"][:h + 4, :k - h].any() and nz["highspan"][h + 4:].all()
    fb = rows["fixture_blocks"]
    for b in range(k // cf.FIXTURE_K):
        blk = fb[4 * b:4 * b + 4]
        assert np.array_equal(blk[:, 6 * b:6 * b + 6], cf.FIXTURE) and blk.sum() == cf.FIXTURE.sum()
    assert nz["fixture_blocks"][4 * (k // 6):].all()
    assert not rows["dupzero"][0].any() and np.array_equal(rows["dupzero"][1:k - 1:2], rows["dupzero"][2:k:2])
    for n in cf.NAMES:  # rows from k on are dense random, and short objects are the family's first rows
        assert (rows[n][k:] != 0).mean() > 0.95
        short, whole = (cf.family(n, k, mm, np.random.default_rng(9)) for mm in (5, m))
        assert np.array_equal(short, whole[:5])


# ---- reach conditions ------------------------------------------------------------------------------------------------
def dirty_after(trace, p):
    return trace[1][p] - trace[2][p]


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("name", ["identity", "upper", "lower"])
def test_reach_stays_clean(orc, name, k, m):
    _, (st, rows, _), _, prof = case(name, k, m)
    assert prof["dirty_pieces"] == 0 and prof["max_dirty_rows"] == 0
    assert rows[k - 1] == k and st[:k] == [OK] * k and st[k:] == [RECEIVED_ALL] * (m - k)


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("name", ["reversed", "shift", "upper_rev"])
def test_reach_whole_matrix_dirty_then_clean_in_one_piece(orc, name, k, m):
    _, trace, _, prof = case(name, k, m)
    assert prof["max_dirty_rows"] == k - 1 and dirty_after(trace, k - 2) == k - 1
    assert prof["reclean"] == [k - 1] and prof["dirty_pieces"] == k - 1
    assert trace[1][k - 1] == k and prof["true_rank"] == k


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("name", ["perm", "band"])
def test_reach_many_dirty_rows_then_clean(orc, name, k, m):
    _, trace, _, prof = case(name, k, m)
    assert 2 * prof["max_dirty_rows"] >= k
    assert k - 1 in prof["reclean"] and trace[1][k - 1] == k


@pytest.mark.parametrize("k,m", SHAPES)
def test_reach_halves(orc, k, m):
    assert case("halves", k, m)[3]["max_dirty_rows"] >= k // 2


@pytest.mark.parametrize("k,m", [s for s in SHAPES if s[0] >= 16])
def test_reach_gf2_in_and_out_of_the_clean_state(orc, k, m):
    prof = case("gf2", k, m)[3]
    assert len(prof["reclean"]) >= 3 and prof["max_dirty_rows"] <= 16


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("name", ["highspan", "fixture_blocks"])
def test_reach_modes_differ(orc, name, k, m):
    assert len(case(name, k, m)[3]["differ"]) >= 1


@pytest.mark.parametrize("k,m,useful,rank", [(60, 64, 55, 54), (126, 130, 112, 109), (130, 132, 114, 111)])
def test_reach_fixture_blocks_over_counts(orc, k, m, useful, rank):
    """Mode 0 counts each block's fourth vector useful and, with few dense pieces after the blocks,
    ends above the true rank.  (At (64, 72) the eight dense pieces after row k bring both to 62.)"""
    prof = case("fixture_blocks", k, m)[3]
    assert (prof["useful"], prof["true_rank"]) == (useful, rank) and useful > rank


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("name", ["lowrank", "dupzero"])
def test_reach_not_useful_pieces(orc, name, k, m):
    _, (st, _, _), model, _ = case(name, k, m)
    need = k / 2 - (m - k)
    assert st.count(NOT_USEFUL) >= need and model[0].count(NOT_USEFUL) >= need
    assert NOT_USEFUL in st and NOT_USEFUL in model[0]
