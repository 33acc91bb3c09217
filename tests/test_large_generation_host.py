"""CPU: rlnc_decode_large_workspace_bytes, the pure size function of decode paths 7 and 8 (the true-rank elimination
beyond LDS, rlnc_amd/csrc/rank_large.hip): its limits and its lower bound, without a GPU."""
import pytest

from rlnc_amd import _lib, batch


def row_dwords(k, m):
    return (k + 3) // 4 + (m + 3) // 4


def test_declared_everywhere():
    assert "rlnc_decode_large_workspace_bytes" in _lib._SIGS
    assert "rlnc_decode_large_workspace_bytes" in _lib.header_symbols()
    assert hasattr(_lib.load(), "rlnc_decode_large_workspace_bytes")
    assert (_lib.RLNC_DECODE_PATH_DEVICE_ANY, _lib.RLNC_DECODE_PATH_LARGE) == (7, 8)


@pytest.mark.parametrize("k,m", [(0, 8), (4097, 4100), (4096, 8193), (8, 0)])
def test_zero_outside_the_limits(k, m):
    assert batch.decode_large_workspace_bytes(k, m, 1) == 0


@pytest.mark.parametrize("k,m", [(300, 310), (4096, 4200), (4096, 8192), (1, 3), (24, 67)])
def test_holds_every_stored_row(k, m):
    one = batch.decode_large_workspace_bytes(k, m, 1)
    assert one > 0
    for nobj in (1, 2, 7):
        assert batch.decode_large_workspace_bytes(k, m, nobj) >= nobj * k * 4 * row_dwords(k, m)


def test_non_decreasing_in_the_object_count():
    sizes = [batch.decode_large_workspace_bytes(300, 310, n) for n in range(1, 40)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert batch.decode_large_workspace_bytes(300, 310, 0) == 0
