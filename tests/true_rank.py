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


class TrueRank:
    """The normative steps on rows [c | e], e one byte per pushed piece, one piece at a time: a decoder that has room
    for `slots` pieces.  true_rank_model is this class fed a whole list; the session model (tests/session_model.py)
    keeps one per object, so that a push costs its new pieces only."""

    def __init__(self, k, slots):
        self.k, self.slots = k, slots
        self.R = np.zeros((k, k + slots), np.uint8)  # the stored rows, in the order they were made
        self.piv, self.st = [], []

    def push(self, h):
        k, p = self.k, len(self.st)
        assert p < self.slots
        h = np.asarray(h, np.uint8).reshape(k)
        n = len(self.piv)
        if n == k:  # step 1
            self.st.append(RECEIVED_ALL)
            return RECEIVED_ALL
        v = np.zeros(k + self.slots, np.uint8)  # step 2
        v[:k] = h
        v[k + p] = 1
        if n:  # v ^= h[pivot of r] * r for every stored row r, all rows at once
            v ^= np.bitwise_xor.reduce(MUL[h[self.piv][:, None], self.R[:n]], axis=0)
        nz = np.nonzero(v[:k])[0]
        if nz.size == 0:  # step 3
            self.st.append(NOT_USEFUL)
            return NOT_USEFUL
        pc = int(nz[0])  # step 4
        v = MUL[npo.gf_inv(int(v[pc]))][v]
        if n:  # r ^= r[pc] * v for every stored row r
            self.R[:n] ^= MUL[self.R[:n, pc][:, None], v[None, :]]
        self.R[n] = v
        self.piv.append(pc)
        self.st.append(OK)
        return OK

    @property
    def rank(self):
        return len(self.piv)

    def result(self):
        """(statuses, rank, T [k][pushed], C [rank][k]): T / C rows in pivot order, T rows >= rank zero."""
        k, n = self.k, len(self.st)
        T = np.zeros((k, n), np.uint8)
        Cm = np.zeros((self.rank, k), np.uint8)
        for i, r in enumerate(np.argsort(self.piv, kind="stable")):
            T[i] = self.R[r][k: k + n]
            Cm[i] = self.R[r][:k]
        return list(self.st), self.rank, T, Cm

    def gathered(self, u):
        """The decoder of the pieces u_0 < u_1 < ... alone, u the Ok slots: a useless piece left a zero column of e in
        every row, and the rows are the unique reduced rows of the span, so the columns are renumbered and nothing is
        eliminated again (include/rlnc_hip.h, rlnc_decode_stream_compact, "Equivalence").
        tests/test_stream_session_host.py holds every such decoder to one fed the kept vectors from scratch."""
        k = self.k
        assert list(u) == [t for t, s in enumerate(self.st) if s == OK]
        out = TrueRank(k, self.slots)
        n = len(self.piv)
        out.R[:n, :k] = self.R[:n, :k]
        out.R[:n, k: k + len(u)] = self.R[:n, k:][:, list(u)]
        out.piv, out.st = list(self.piv), [OK] * len(u)
        return out


def true_rank_model(k, vectors):
    """The normative steps on rows [c | e], e one byte per pushed piece.  Returns (statuses, rank, T [k][m],
    C [rank][k]): T / C rows in pivot order, T rows >= rank zero."""
    vectors = np.asarray(vectors, np.uint8).reshape(-1, k)
    d = TrueRank(k, vectors.shape[0])
    for h in vectors:
        d.push(h)
    return d.result()


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
