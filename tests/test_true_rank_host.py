"""CPU: the host elimination in rank mode 1 (RLNC_RANK_MODE_TRUE; include/rlnc_hip.h, "Rank mode") against the numpy
model of tests/true_rank.py, which follows the four steps of the mode's definition literally.  Every comparison is
exact equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests.true_rank import (FIXTURE, FIXTURE_K, MUL, NOT_USEFUL, OK, RECEIVED_ALL, check_against_model,
                             sparse_vectors)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_survey_fixture_true_rank():
    st, rank, T, Cm = check_against_model(FIXTURE_K, FIXTURE)
    assert st == [OK, OK, OK, NOT_USEFUL] and rank == 3
    assert np.array_equal(Cm, np.array([[0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 0, 1]], np.uint8))


def test_survey_fixture_default_mode_unchanged():
    from rlnc_amd.elimination import Elimination

    for e in (Elimination(FIXTURE_K), Elimination(FIXTURE_K, rank_mode=0)):
        assert [e.push(h)[0] for h in FIXTURE] == [OK, OK, OK, OK]
        assert e.rank == 4


def test_new_mode_rejects_other_modes():
    from rlnc_amd.elimination import Elimination
    from rlnc_amd.errors import RLNCError

    for mode in (2, -1):
        with pytest.raises(RLNCError):
            Elimination(4, rank_mode=mode)


@pytest.mark.parametrize("k,density,n", [(8, 2, 24), (16, 2, 48), (32, 3, 64), (64, 4, 128), (130, 3, 260)])
def test_sparse_streams(k, density, n):
    rng = np.random.default_rng(1000 * k + density)
    for _ in range(3 if k <= 32 else 1):
        check_against_model(k, sparse_vectors(rng, k, n, density))


def test_degenerate_pieces():
    rng = np.random.default_rng(7)
    k = 12
    a = rng.integers(0, 256, (5, k), dtype=np.uint8)
    vec = np.vstack([
        np.zeros((1, k), np.uint8),        # all zero
        a[0:1], a[0:1],                    # an exact duplicate
        MUL[0x53][a[0:1]],                 # a scalar multiple
        a[1:2], a[0:1] ^ a[1:2],           # the sum of two earlier pieces
        a[2:3], MUL[7][a[2:3]] ^ MUL[9][a[0:1]],
        a[3:5],
    ])
    st, rank, _, _ = check_against_model(k, vec)
    assert st == [NOT_USEFUL, OK, NOT_USEFUL, NOT_USEFUL, OK, NOT_USEFUL, OK, NOT_USEFUL, OK, OK] and rank == 5


def test_k_one():
    st, rank, T, _ = check_against_model(1, np.array([[0], [5], [7]], np.uint8))
    assert st == [NOT_USEFUL, OK, RECEIVED_ALL] and rank == 1
    assert T[0, 1] == npo.gf_inv(5)


def test_pieces_after_full_rank_answer_received_all():
    rng = np.random.default_rng(3)
    k = 10
    vec = rng.integers(0, 256, (k + 6, k), dtype=np.uint8)
    st, rank, _, Cm = check_against_model(k, vec)
    assert rank == k and st[-3:] == [RECEIVED_ALL] * 3
    assert np.array_equal(Cm, np.eye(k, dtype=np.uint8))


def test_shuffled_unit_vectors_then_dense_repair():
    rng = np.random.default_rng(5)
    k = 20
    units = np.eye(k, dtype=np.uint8)[rng.permutation(k)[: k - 6]]  # systematic pieces, six of them lost
    units = MUL[rng.integers(1, 256)][units]
    repair = rng.integers(0, 256, (10, k), dtype=np.uint8)
    st, rank, _, Cm = check_against_model(k, np.vstack([units, units[:3], repair]))
    assert st[: k - 6] == [OK] * (k - 6) and st[k - 6: k - 3] == [NOT_USEFUL] * 3
    assert rank == k and np.array_equal(Cm, np.eye(k, dtype=np.uint8))


def test_sparse_objects_where_the_reference_mode_differs():
    """k = 16, density 2, 48 pieces: on most objects the reference's status sequence differs from the true one (the
    premise, asserted on the input), and mode 1 gives the true sequence on every object."""
    from oracle.oracle import OracleDecoder

    rng = np.random.default_rng(20240)
    k, n, nobj = 16, 48, 40
    differ = 0
    for _ in range(nobj):
        vec = sparse_vectors(rng, k, n, 2)
        want = check_against_model(k, vec)
        od = OracleDecoder(1, k)
        ref = [od.decode(np.concatenate([h, [0]]).astype(np.uint8)) for h in vec]
        differ += ref != want[0]
    assert 2 * differ >= nobj, (differ, nobj)


_SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "elimination.hpp"
#include "rlnc_hip.h"
using rlnc::Elimination;
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return unsigned(s >> 11); }
#define REQUIRE(c) do { if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
    {
        const unsigned char f[4][6] = {{0, 0, 2, 0, 0, 3}, {0, 0, 0, 2, 2, 0}, {0, 0, 0, 0, 0, 2}, {0, 0, 0, 0, 0, 1}};
        Elimination e(6, 0, 1), ref(6);
        int slot; bool keep;
        for (int p = 0; p < 4; ++p) {
            REQUIRE(e.push(f[p], &slot, &keep) == (p < 3 ? RLNC_OK : RLNC_ERR_PIECE_NOT_USEFUL));
            REQUIRE(ref.push(f[p], &slot, &keep) == RLNC_OK);
        }
        REQUIRE(e.rank() == 3 && ref.rank() == 4);
    }
    for (int fixed = 0; fixed < 2; ++fixed)
        for (size_t k : {1, 5, 16, 33, 130}) {
            const size_t m = 3 * k;
            Elimination e(k, fixed ? 2 : 0, 1);  // fixed: grows from 2 slots
            std::vector<unsigned char> h(k), T;
            size_t useful = 0;
            for (size_t p = 0; p < m; ++p) {
                for (auto &b : h) b = 0;
                for (int d = 0; d < 3; ++d) h[rnd() % k] = (unsigned char)(1 + rnd() % 255);
                int slot = -1; bool keep = false;
                const int st = e.push(h.data(), &slot, &keep);
                REQUIRE(st == RLNC_OK || st == RLNC_ERR_PIECE_NOT_USEFUL || st == RLNC_ERR_RECEIVED_ALL_PIECES);
                if (st == RLNC_OK) ++useful;
                REQUIRE(e.rank() == useful && useful <= k);
                Elimination c(e);  // the decoder's clone
                T.assign(k * c.slots(), 0);
                c.transform(T.data(), c.slots());
                for (size_t r = 0; r < c.rank(); ++r) REQUIRE(c.row(r) != nullptr);
            }
        }
    std::puts("ok");
    return 0;
}
"""


def test_host_elimination_under_sanitizers(tmp_path):
    """The host elimination source and a stand-alone main, built with AddressSanitizer and UBSan and run as a program."""
    csrc = os.path.join(ROOT, "rlnc_amd", "csrc")
    main = tmp_path / "san_main.cpp"
    main.write_text(_SAN_MAIN)
    exe = str(tmp_path / "san_elim")
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__host__=", "-D__device__=", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
           os.path.join(csrc, "elimination.cpp"), str(main), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("sanitize" in b.stderr or "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("the host compiler does not accept -fsanitize=address,undefined: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
