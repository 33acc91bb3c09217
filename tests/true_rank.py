"""The numpy model of rank mode 1 (RLNC_RANK_MODE_TRUE; include/rlnc_hip.h, "Rank mode"), which follows the four steps
of the mode's definition literally, and the host elimination run against it.  Every true-rank and decode-stream test,
on the CPU and on the GPU, is measured against true_rank_model.  Plain module: no GPU."""
import numpy as np

from oracle import np_oracle as npo

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
