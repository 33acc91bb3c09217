"""CPU: the sparse coding-vector format on the host (rlnc_amd.sparse: the normative expansion, the dense -> ELL
conversion, the sampler) and the sparse entry points of the C ABI as far as they answer without a device (exported,
null arguments rejected, status order of the size checks as in the dense twins)."""
import ctypes as C

import numpy as np
import pytest

from rlnc_amd import sparse

INVALID_ARGUMENT, PIECE_COUNT_ZERO, PIECE_LENGTH_ZERO = 100, 3, 5
NOT_ENOUGH_PIECES_TO_RECODE, PIECE_LENGTH_TOO_SHORT = 6, 7
SPARSE_SYMBOLS = ["rlnc_gf256_sparse_matmul", "rlnc_encode_batch_sparse", "rlnc_recode_batch_sparse",
                  "rlnc_encoder_code_sparse_batch_device"]


@pytest.mark.parametrize("shape,density", [((7, 5), 0.5), ((3, 4, 33), 0.1), ((1, 1), 1.0), ((6, 300), 0.02)])
def test_round_trip(shape, density):
    rng = np.random.default_rng(sum(shape))
    dense = rng.integers(1, 256, shape, dtype=np.uint8) * (rng.random(shape) < density)
    idx, val = sparse.from_dense(dense)
    assert idx.dtype == np.int32 and val.dtype == np.uint8 and idx.shape == val.shape == shape[:-1] + (idx.shape[-1],)
    assert idx.shape[-1] == int((dense != 0).sum(axis=-1).max())
    assert np.array_equal(sparse.to_dense(idx, val, shape[-1]), dense)
    # a wider w pads; the expansion is the same
    idx2, val2 = sparse.from_dense(dense, idx.shape[-1] + 3)
    assert idx2.shape[-1] == idx.shape[-1] + 3
    assert np.array_equal(sparse.to_dense(idx2, val2, shape[-1]), dense)


def test_from_dense_raises_on_a_row_with_more_than_w_nonzeros():
    dense = np.array([[1, 0, 0, 0], [1, 2, 3, 0]], np.uint8)
    with pytest.raises(ValueError):
        sparse.from_dense(dense, 2)
    idx, val = sparse.from_dense(dense, 3)
    assert np.array_equal(sparse.to_dense(idx, val, 4), dense)


def test_from_dense_of_a_zero_matrix_has_no_entries():
    idx, val = sparse.from_dense(np.zeros((3, 5), np.uint8))
    assert idx.shape == val.shape == (3, 0)
    assert np.array_equal(sparse.to_dense(idx, val, 5), np.zeros((3, 5), np.uint8))


def test_to_dense_duplicates_accumulate_by_xor():
    idx = np.array([[2, 2], [2, 2], [1, 1]], np.int32)
    val = np.array([[5, 5], [5, 3], [7, 0]], np.uint8)
    want = np.zeros((3, 4), np.uint8)
    want[1, 2] = 6
    want[2, 1] = 7
    assert np.array_equal(sparse.to_dense(idx, val, 4), want)
    # three copies leave one
    assert np.array_equal(sparse.to_dense([[0, 0, 0]], [[9, 9, 9]], 2), [[9, 0]])


def test_to_dense_zero_value_padding_anywhere():
    want = np.array([[0, 4, 0, 9, 0]], np.uint8)
    for idx, val in [([0, 0, 1, 3], [0, 0, 4, 9]),      # at the start
                     ([1, 0, 2, 3], [4, 0, 0, 9]),      # in the middle (index 2 with value 0 is padding too)
                     ([1, 3, 0, 0], [4, 9, 0, 0]),      # at the end
                     ([4, 1, 4, 3], [0, 4, 0, 9])]:     # interleaved
        assert np.array_equal(sparse.to_dense(np.array([idx], np.int32), np.array([val], np.uint8), 5), want)


def test_to_dense_drops_out_of_range_indices():
    n_in = 6
    idx = np.array([[-1, 2, n_in, 2**31 - 1, 5]], np.int32)
    val = np.array([[7, 3, 8, 9, 1]], np.uint8)
    want = np.zeros((1, n_in), np.uint8)
    want[0, 2] = 3
    want[0, 5] = 1
    assert np.array_equal(sparse.to_dense(idx, val, n_in), want)


def test_draw():
    rng = np.random.default_rng(1)
    idx, val = sparse.draw(rng, 50, 33, 4)
    assert idx.shape == val.shape == (50, 4) and idx.dtype == np.int32 and val.dtype == np.uint8
    assert (val != 0).all() and (idx >= 0).all() and (idx < 33).all()
    assert all(len(set(r)) == 4 for r in idx.tolist())
    assert ((sparse.to_dense(idx, val, 33) != 0).sum(axis=1) == 4).all()
    # w > k: min(w, k) distinct entries, the rest padding
    idx, val = sparse.draw(rng, 20, 3, 8)
    assert idx.shape == (20, 8)
    assert (val[:, :3] != 0).all() and (val[:, 3:] == 0).all()
    assert all(sorted(r[:3]) == [0, 1, 2] for r in idx.tolist())
    assert ((sparse.to_dense(idx, val, 3) != 0).sum(axis=1) == 3).all()


def test_library_exports_the_sparse_symbols_and_rejects_null():
    from rlnc_amd import _lib

    lib = _lib.load()
    for s in SPARSE_SYMBOLS:
        assert hasattr(lib, s) and s in _lib._SIGS and s in _lib.header_symbols(), s
    assert lib.rlnc_gf256_sparse_matmul(None, None) == INVALID_ARGUMENT
    d = _lib.SparseMatmulDesc()
    assert lib.rlnc_gf256_sparse_matmul(None, C.byref(d)) == INVALID_ARGUMENT
    # a null context is rejected before the size checks, as in the dense twins
    assert lib.rlnc_encode_batch_sparse(None, None, 0, 0, 0, None, None, 0, 0, None) == INVALID_ARGUMENT
    assert lib.rlnc_encode_batch(None, None, 0, 0, 0, None, 0, None) == INVALID_ARGUMENT
    assert lib.rlnc_recode_batch_sparse(None, None, 0, 0, 0, 0, None, None, 0, 0, None) == INVALID_ARGUMENT
    assert lib.rlnc_recode_batch(None, None, 0, 0, 0, 0, None, 0, None) == INVALID_ARGUMENT
    assert lib.rlnc_encoder_code_sparse_batch_device(None, None, None, 0, 0, None, 0) == INVALID_ARGUMENT
    assert lib.rlnc_encoder_code_batch_device(None, None, 0, None, 0) == INVALID_ARGUMENT


def test_size_checks_come_before_any_use_of_the_context():
    """k == 0 and L == 0 are answered before the context is touched (no device here), with the dense twins' codes in
    the dense twins' order.  The context handle only has to be non-null for that: these calls return before reading
    it."""
    from rlnc_amd import _lib

    lib = _lib.load()
    stand_in = C.create_string_buffer(64)  # never dereferenced: every call below returns on its size checks
    h = C.cast(stand_in, C.c_void_p)
    for k, L, want in [(0, 0, PIECE_COUNT_ZERO), (0, 8, PIECE_COUNT_ZERO), (4, 0, PIECE_LENGTH_ZERO)]:
        assert lib.rlnc_encode_batch(h, None, k, L, 1, None, 1, None) == want
        assert lib.rlnc_encode_batch_sparse(h, None, k, L, 1, None, None, 2, 1, None) == want
    for n, k, L, want in [(0, 0, 0, NOT_ENOUGH_PIECES_TO_RECODE), (3, 0, 0, PIECE_COUNT_ZERO),
                          (3, 2, 0, PIECE_LENGTH_TOO_SHORT)]:
        assert lib.rlnc_recode_batch(h, None, k, L, n, 1, None, 1, None) == want
        assert lib.rlnc_recode_batch_sparse(h, None, k, L, n, 1, None, None, 2, 1, None) == want
    # nothing to do is Ok and launches nothing
    assert lib.rlnc_encode_batch_sparse(h, None, 4, 8, 0, None, None, 2, 1, None) == 0
    assert lib.rlnc_encode_batch_sparse(h, None, 4, 8, 1, None, None, 2, 0, None) == 0
    assert lib.rlnc_recode_batch_sparse(h, None, 4, 8, 3, 1, None, None, 2, 0, None) == 0
    # then the pointers and sizes
    assert lib.rlnc_encode_batch_sparse(h, None, 4, 8, 1, None, None, 2, 1, None) == INVALID_ARGUMENT
    assert lib.rlnc_recode_batch_sparse(h, None, 4, 8, 3, 1, None, None, 2, 1, None) == INVALID_ARGUMENT
