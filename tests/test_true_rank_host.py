"""CPU: the host elimination in rank mode 1 (RLNC_RANK_MODE_TRUE; include/rlnc_hip.h, "Rank mode") against a numpy
model that follows the four steps of the mode's definition literally.  Every comparison is exact equality.

The model (true_rank_model) is also what tests/test_gpu_true_rank.py checks the device kernel against."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as npo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_USEFUL, RECEIVED_ALL = 0, 8, 9
MUL = npo.mul_table()

# the reference's diagonal-pivot elimination answers Ok four times (rank 4); the true rank is 3
FIXTURE_K = 6
FIXTURE = np.array([[0, 0, 2, 0, 0, 3], [0, 0, 0, 2, 2, 0], [0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 1]], np.uint8)


def true_rank_model(k, vectors):
    """The normative steps on rows [c | e], e one byte per pushed piece.  Returns (statuses, rank, T [k][m],
    C [rank][k]): T / C rows in pivot order, T rows >= rank zero."""
    vectors = np.asarray(vectors, np.uint8).reshape(-1, k)
    m = vectors.shape[0]
    rows, piv, st = [], [], []
    for p, h in enumerate(vectors):
        if len(rows) == k:  # step 1
            st.append(RECEIVED_ALL)
            continue
        v = np.zeros(k + m, np.uint8)  # step 2
        v[:k] = h
        v[k + p] = 1
        for r, pc in zip(rows, piv):
            q = int(h[pc])
            if q:
                v ^= MUL[q][r]
        nz = np.nonzero(v[:k])[0]
        if nz.size == 0:  # step 3
            st.append(NOT_USEFUL)
            continue
        pc = int(nz[0])  # step 4
        v = MUL[npo.gf_inv(int(v[pc]))][v]
        for r in rows:
            q = int(r[pc])
            if q:
                r ^= MUL[q][v]
        rows.append(v)
        piv.append(pc)
        st.append(OK)
    rank = len(rows)
    T = np.zeros((k, m), np.uint8)
    Cm = np.zeros((rank, k), np.uint8)
    for i, r in enumerate(np.argsort(piv, kind="stable")):
        T[i] = rows[r][k:]
        Cm[i] = rows[r][:k]
    return st, rank, T, Cm


def sparse_vectors(rng, k, n, density):
    """n coding vectors with `density` random nonzero entries each."""
    v = np.zeros((n, k), np.uint8)
    for i in range(n):
        v[i, rng.choice(k, size=min(density, k), replace=False)] = rng.integers(1, 256, min(density, k))
    return v


def host_run(k, vectors, fixed):
    """Push the vectors through the library's host elimination in mode 1.  Returns (statuses, rank, T [k][m], C) with
    T's columns mapped back from slots to piece indices (a piece that keeps no slot has a zero column)."""
    from rlnc_amd.elimination import Elimination

    vectors = np.asarray(vectors, np.uint8).reshape(-1, k)
    m = vectors.shape[0]
    e = Elimination(k, m if fixed else 0, rank_mode=1)
    st, slot_of = [], {}
    for p, h in enumerate(vectors):
        rank_before = e.rank
        s, slot, keep = e.push(h)
        st.append(s)
        if s == OK:
            assert keep and slot not in slot_of.values()
            slot_of[p] = slot
            assert e.rank == rank_before + 1
        else:
            assert e.rank == rank_before
            if s == NOT_USEFUL:
                assert not keep
        if not fixed:
            assert slot < k and e.slots <= k  # recycled slots never exceed k
        elif s != RECEIVED_ALL:
            assert slot == p
    Ts = e.transform()
    T = np.zeros((k, m), np.uint8)
    for p, s in slot_of.items():
        T[:, p] = Ts[:, s]
    used = sorted(slot_of.values())
    assert not np.delete(Ts, used, axis=1).any()  # columns of no useful piece stay zero for ever
    return st, e.rank, T, e.coefficients()


def check_against_model(k, vectors):
    want = true_rank_model(k, vectors)
    for fixed in (False, True):
        got = host_run(k, vectors, fixed)
        assert got[0] == want[0], (fixed, got[0], want[0])
        assert got[1] == want[1]
        assert np.array_equal(got[2], want[2]), fixed
        assert np.array_equal(got[3], want[3]), fixed
    # the model's own invariants: T x vectors = the RREF rows, which have unit pivot columns
    st, rank, T, Cm = want
    vec = np.asarray(vectors, np.uint8).reshape(-1, k)
    assert np.array_equal(npo.matmul(T[:rank], vec), Cm)
    lead = [int(np.nonzero(r)[0][0]) for r in Cm]
    assert lead == sorted(set(lead)) and np.array_equal(Cm[:, lead], np.eye(rank, dtype=np.uint8))
    return want


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
