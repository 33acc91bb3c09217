"""CPU: the stream-form interface without a GPU (include/rlnc_hip.h, rlnc_set_stream_form and
rlnc_decode_stream_lds_fits) -- the symbols in the header, the ctypes table and the library, and the pure predicate
against the restated LDS formula of tests/limit_shapes.py at the edges of the budget.  A context cannot be made
without a device: what set_stream_form accepts on one is in tests/test_gpu_decode_stream_lds.py."""
import re

from tests import limit_shapes as ls

SYMBOLS = ["rlnc_set_stream_form", "rlnc_decode_stream_lds_fits"]
FORMS = {"RLNC_STREAM_FORM_AUTO": 0, "RLNC_STREAM_FORM_WORKSPACE": 1, "RLNC_STREAM_FORM_LDS": 2}


def test_symbols_are_declared_bound_and_exported():
    from rlnc_amd import _lib

    lib = _lib.load()
    declared = _lib.header_symbols()
    header = open(_lib.HEADER_PATH).read()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib._SIGS, s
        assert hasattr(lib, s), s
    for name, value in FORMS.items():
        assert re.search(rf"#define\s+{name}\s+{value}\b", header), name
        assert getattr(_lib, name) == value


def test_lds_fits_is_the_rank_kernel_formula_at_its_edges():
    from rlnc_amd import batch

    for fitting, beyond in ls.RANK_EDGES:
        assert ls.rank_lds_bytes(*fitting) <= ls.MAX_LDS < ls.rank_lds_bytes(*beyond)
        assert batch.stream_lds_fits(*fitting) is True, fitting
        assert batch.stream_lds_fits(*beyond) is False, beyond
    shapes = [(4, 8192), (4, 1100), (1, 1), (5, 7), (32, 32), (200, 210), (300, 310), (256, 256), (4096, 8192),
              (2 ** 31, 8), (8, 2 ** 31), (2 ** 40, 2 ** 40)]
    for k, m in shapes:
        want = k < 2 ** 20 and m < 2 ** 20 and ls.rank_lds_bytes(k, m) <= ls.MAX_LDS
        assert batch.stream_lds_fits(k, m) is want, (k, m)
    assert batch.stream_lds_fits(4, 8192) is True  # rows of more than 256 dwords
    for k, m in [(0, 0), (0, 8), (8, 0)]:
        assert batch.stream_lds_fits(k, m) is False, (k, m)


def test_set_stream_form_refuses_a_null_context():
    from rlnc_amd import _lib

    lib = _lib.load()
    for form in (0, 1, 2, 3):
        assert lib.rlnc_set_stream_form(None, form) == 100
