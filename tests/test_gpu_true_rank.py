"""GPU: rank mode 1 (RLNC_RANK_MODE_TRUE; include/rlnc_hip.h, "Rank mode") through every public layer -- the device
kernel (rank.hip) behind decode_batch_eliminate / decode_batch_device / decode_batch / decode_ragged /
decode_host_stream, the host fallback beyond LDS, the object API and the C++ mirror -- against the numpy model of
tests/true_rank.py.  All comparisons are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as npo
from tests.gpu_util import dev, host
from tests.stream_util import true_rank_context
from tests.true_rank import (FIXTURE, FIXTURE_K, NOT_USEFUL, OK, RECEIVED_ALL, sparse_vectors,
                                       true_rank_model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_ALL_YET = 10


@pytest.fixture(scope="module")
def ctx1():
    """A context in rank mode 1 (tests that change its mode or path put it back)."""
    return true_rank_context()


def eliminate(ctx, pieces_t, k):
    import torch

    from rlnc_amd import batch

    nobj, m, _ = pieces_t.shape
    T = torch.full((nobj, k, m), 0xAA, dtype=torch.uint8, device="cuda:0")
    ps = torch.full((nobj, m), -1, dtype=torch.int32, device="cuda:0")
    rk = torch.full((nobj,), -1, dtype=torch.int32, device="cuda:0")
    batch.decode_batch_eliminate(pieces_t, k, T, ps, rk, ctx)
    return host(T), host(ps), host(rk)


def check_eliminate(ctx, co, distinct=None, L=4, pad_pieces=0):
    """co [nobj][m][k] coefficient vectors -> mode-1 elimination on the device == the model, object by object.
    distinct: only the first `distinct` objects are different (the rest repeat them); pad_pieces: extra pieces per
    object beyond the m decoded (a non-dense object stride)."""
    nobj, m, k = co.shape
    rng = np.random.default_rng(k * 1000 + m)
    pieces = rng.integers(0, 256, (nobj, m + pad_pieces, k + L), dtype=np.uint8)
    pieces[:, :m, :k] = co
    T, ps, rk = eliminate(ctx, dev(pieces)[:, :m], k)
    models = {}
    for o in range(nobj):
        key = o % distinct if distinct else o
        if key not in models:
            models[key] = true_rank_model(k, co[o])
        st, rank, Tm, _ = models[key]
        assert list(ps[o]) == st, o
        assert rk[o] == rank, o
        assert np.array_equal(T[o], Tm), o
    return models


def planted(rng, k, m):
    """Dense vectors with planted duplicates, multiples and sums of earlier pieces."""
    co = rng.integers(0, 256, (m, k), dtype=np.uint8)
    mul = npo.mul_table()
    for i in range(3, m, 7):
        a, b = rng.integers(0, i, 2)
        co[i] = [co[a], mul[int(rng.integers(2, 256))][co[a]], co[a] ^ co[b]][i % 3]
    return co


def test_eliminate_fixture(ctx1):
    co = np.stack([FIXTURE, FIXTURE[::-1], FIXTURE[[2, 3, 0, 1]]])
    models = check_eliminate(ctx1, co)
    assert models[0][0] == [OK, OK, OK, NOT_USEFUL] and models[0][1] == 3


@pytest.mark.parametrize("k,m,nobj,density", [(16, 48, 64, 2), (32, 64, 16, 3)])
def test_eliminate_sparse(ctx1, k, m, nobj, density):
    rng = np.random.default_rng(k)
    check_eliminate(ctx1, np.stack([sparse_vectors(rng, k, m, density) for _ in range(nobj)]))


def test_eliminate_dense_with_planted_dependencies(ctx1):
    rng = np.random.default_rng(64)
    models = check_eliminate(ctx1, np.stack([planted(rng, 64, 80) for _ in range(4)]))
    assert all(NOT_USEFUL in mdl[0] and mdl[1] == 64 for mdl in models.values())


def test_eliminate_rows_wider_than_256_bytes(ctx1):
    rng = np.random.default_rng(128)
    co = np.stack([planted(rng, 128, 140), sparse_vectors(rng, 128, 140, 3)])
    check_eliminate(ctx1, co)


def test_eliminate_near_the_lds_bound(ctx1):
    rng = np.random.default_rng(200)
    co = np.stack([planted(rng, 200, 210), sparse_vectors(rng, 200, 210, 4)])
    check_eliminate(ctx1, co)


def test_eliminate_many_small_objects(ctx1):
    """2,500 objects of k = 16: the one-wave-per-object form.  125 different objects (half of them sparse), repeated."""
    rng = np.random.default_rng(2500)
    k, m, distinct = 16, 20, 125
    base = [sparse_vectors(rng, k, m, 2) if i % 2 else rng.integers(0, 256, (m, k), dtype=np.uint8)
            for i in range(distinct)]
    co = np.stack([base[o % distinct] for o in range(2500)])
    models = check_eliminate(ctx1, co, distinct=distinct)
    assert len({mdl[1] for mdl in models.values()}) > 2  # ranks differ among them


def test_eliminate_k_one_and_few_pieces(ctx1):
    check_eliminate(ctx1, np.array([[[0], [5], [7]], [[9], [0], [1]], [[0], [0], [0]]], np.uint8))
    rng = np.random.default_rng(1)
    models = check_eliminate(ctx1, rng.integers(0, 256, (3, 5, 12), dtype=np.uint8))  # m < k
    assert all(mdl[1] == 5 for mdl in models.values())


def test_eliminate_strided_objects(ctx1):
    rng = np.random.default_rng(33)
    check_eliminate(ctx1, np.stack([sparse_vectors(rng, 24, 30, 3) for _ in range(5)]), L=7, pad_pieces=3)


def make_objects(rng, k, m, L, nobj):
    """Objects alternating sparse (density 2) and dense coding vectors: (data, padded source, pieces, model)."""
    objs = []
    for o in range(nobj):
        data = rng.integers(0, 256, k * L - 1 - int(rng.integers(0, k)), dtype=np.uint8)
        src = npo.pad(data, k)
        assert src.shape == (k, L)
        co = sparse_vectors(rng, k, m, 2) if o % 2 == 0 else rng.integers(0, 256, (m, k), dtype=np.uint8)
        objs.append((data, src, npo.encode(src, co), true_rank_model(k, co)))
    return objs


def check_decoded(objs, k, dec, pst, ost, dl):
    full = 0
    for o, (data, src, _, (st, rank, _, _)) in enumerate(objs):
        assert list(pst[o]) == st, o
        if rank == k:
            full += 1
            assert ost[o] == 0 and int(dl[o]) == data.size, o
            assert np.array_equal(dec[o], src), o
        else:
            assert ost[o] == NOT_ALL_YET, o
    return full


@pytest.mark.parametrize("L", [64, 100, 4096])
def test_decode_batch_and_device(ctx1, L):
    import torch

    from rlnc_amd import batch

    k, m, nobj = 16, 24, 8
    objs = make_objects(np.random.default_rng(L), k, m, L, nobj)
    pieces = dev(np.stack([x[2] for x in objs]))
    decoded = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0")
    pst, ost, dl = batch.decode_batch(pieces, k, decoded, ctx1)
    full = check_decoded(objs, k, host(decoded), pst, ost, dl)
    assert 0 < full < nobj  # both outcomes occur
    decoded2 = torch.zeros_like(decoded)
    ps_d = torch.full((nobj, m), -1, dtype=torch.int32, device="cuda:0")
    os_d = torch.full((nobj,), -1, dtype=torch.int32, device="cuda:0")
    dl_d = torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0")
    batch.decode_batch_device(pieces, k, decoded2, ps_d, os_d, dl_d, ctx1)
    check_decoded(objs, k, host(decoded2), host(ps_d), host(os_d), host(dl_d))
    # path 1: the host elimination behind the same call
    ctx1.set_decode_path(1)
    try:
        decoded3 = torch.zeros_like(decoded)
        pst3, ost3, dl3 = batch.decode_batch(pieces, k, decoded3, ctx1)
    finally:
        ctx1.set_decode_path(0)
    check_decoded(objs, k, host(decoded3), pst3, ost3, dl3)


def test_host_fallback_beyond_lds(ctx1):
    import torch

    from rlnc_amd import batch
    from rlnc_amd.errors import RLNCError

    k, m, L = 300, 310, 16
    rng = np.random.default_rng(300)
    data = rng.integers(0, 256, k * L - 5, dtype=np.uint8)
    src = npo.pad(data, k)
    co = rng.integers(0, 256, (m, k), dtype=np.uint8)
    co[5] = co[2]
    co[100] = co[7] ^ co[50]
    co[200] = npo.mul_table()[0x1D][co[150]]
    model = true_rank_model(k, co)
    assert model[1] == k and model[0].count(NOT_USEFUL) == 3 and model[0][-1] == RECEIVED_ALL
    from tests.gpu_util import np_matmul

    pieces = dev(np.concatenate([co, np_matmul(co, src)], axis=1)[None])
    decoded = torch.zeros((1, k, L), dtype=torch.uint8, device="cuda:0")
    pst, ost, dl = batch.decode_batch(pieces, k, decoded, ctx1)
    assert list(pst[0]) == model[0] and ost[0] == 0 and int(dl[0]) == data.size
    assert np.array_equal(host(decoded)[0], src)
    # the device-only call reports the shape as it does in mode 0
    with pytest.raises(RLNCError) as ei:
        eliminate(ctx1, pieces, k)
    assert ei.value == RLNCError.InvalidArgument


def test_decode_ragged(ctx1):
    import torch

    from rlnc_amd import batch
    from tests.gpu_util import np_matmul

    rng = np.random.default_rng(6)
    shapes = [(6, 4, 8, "fixture"), (16, 20, 100, 2), (32, 40, 64, "planted"), (64, 70, 32, "dense"), (130, 140, 16, 3),
              (300, 304, 16, "dense")]
    objs, want = [], []
    for k, m, L, kind in shapes:
        data = rng.integers(0, 256, k * L - 2, dtype=np.uint8)
        src = npo.pad(data, k)
        co = (FIXTURE if kind == "fixture" else planted(rng, k, m) if kind == "planted" else
              rng.integers(0, 256, (m, k), dtype=np.uint8) if kind == "dense" else sparse_vectors(rng, k, m, kind))
        pieces = np.concatenate([co, np_matmul(co, src)], axis=1)
        objs.append((dev(pieces), k, torch.zeros((k, L), dtype=torch.uint8, device="cuda:0")))
        want.append((data, src, true_rank_model(k, co)))
    ps, os_, dl = batch.decode_ragged(objs, ctx1)
    ps, os_, dl = host(ps), host(os_), host(dl)
    at = 0
    for i, ((k, m, L, _), (data, src, (st, rank, _, _))) in enumerate(zip(shapes, want)):
        assert list(ps[at:at + m]) == st, i
        at += m
        if rank == k:
            assert os_[i] == 0 and dl[i] == data.size, i
            assert np.array_equal(host(objs[i][2]), src), i
        else:
            assert os_[i] == NOT_ALL_YET, i
    assert want[0][2][1] == 3 and want[-1][2][1] == 300


def test_decode_host_stream(ctx1):
    k, m, L, nobj = 16, 24, 64, 5
    objs = make_objects(np.random.default_rng(77), k, m, L, nobj)
    pieces = np.ascontiguousarray(np.stack([x[2] for x in objs]))
    decoded = np.zeros((nobj, k, L), np.uint8)
    ps = np.zeros((nobj, m), np.int32)
    os_ = np.zeros(nobj, np.int32)
    dl = np.zeros(nobj, np.uint64)
    st = ctx1.lib.rlnc_decode_host_stream(ctx1.h, C.c_void_p(pieces.ctypes.data), m * (k + L), k, L, m, nobj,
                                          C.c_void_p(decoded.ctypes.data), ps.ctypes.data_as(C.POINTER(C.c_int32)),
                                          os_.ctypes.data_as(C.POINTER(C.c_int32)),
                                          dl.ctypes.data_as(C.POINTER(C.c_uint64)), 2)
    assert st == 0
    assert 0 < check_decoded(objs, k, decoded, ps, os_, dl) < nobj


def test_object_api():
    import rlnc_amd
    from rlnc_amd.errors import RLNCError
    from rlnc_amd.full import Decoder

    ctx = rlnc_amd.Context(0)
    rng = np.random.default_rng(8)
    k, L = FIXTURE_K, 8
    data = rng.integers(0, 256, k * L - 1, dtype=np.uint8)
    src = npo.pad(data, k)
    before = Decoder.new(L, k, ctx)
    ctx.set_rank_mode(1)
    dec = Decoder.new(L, k, ctx)
    assert before.rank_mode == 0 and dec.rank_mode == 1
    fixture_pieces = npo.encode(src, FIXTURE)
    for p in fixture_pieces[:3]:
        dec.decode(p)
        before.decode(p)
    before.decode(fixture_pieces[3])  # mode 0 kept: the reference counts it useful
    assert before.get_useful_piece_count() == 4
    with pytest.raises(RLNCError) as ei:
        dec.decode(fixture_pieces[3])
    assert ei.value == RLNCError.PieceNotUseful
    assert dec.get_useful_piece_count() == 3 and dec.get_received_piece_count() == 4
    assert dec.get_remaining_piece_count() == 3
    ctx.set_rank_mode(0)  # existing decoders are not touched
    twin = dec.clone()
    assert twin.rank_mode == 1 and twin.get_useful_piece_count() == 3
    for d in (dec, twin):
        while not d.is_already_decoded():
            try:
                d.decode(npo.encode(src, rng.integers(0, 256, (1, k), dtype=np.uint8))[0])
            except RLNCError as e:
                assert e == RLNCError.PieceNotUseful
        assert np.array_equal(d.get_decoded_data(), data)
        with pytest.raises(RLNCError) as ei:
            d.decode(fixture_pieces[0])
        assert ei.value == RLNCError.ReceivedAllPieces


def test_mode_isolation_and_decode_paths():
    import torch

    import rlnc_amd
    from oracle.oracle import OracleDecoder
    from rlnc_amd import batch
    from rlnc_amd.errors import RLNCError

    ctx = rlnc_amd.Context(0)
    with pytest.raises(RLNCError):
        ctx.set_rank_mode(2)
    ctx.set_rank_mode(1)
    rng = np.random.default_rng(21)
    cases = [(FIXTURE_K, FIXTURE), (16, sparse_vectors(rng, 16, 48, 2))]
    inputs = []
    for k, co in cases:
        L = 32
        src = npo.pad(rng.integers(0, 256, k * L - 3, dtype=np.uint8), k)
        inputs.append((k, L, npo.encode(src, co)))
    # in mode 1 the reference-mode kernel named by path 5 is refused (no silent fallback)
    ctx.set_decode_path(5)
    k, L, pieces = inputs[0]
    dec = torch.zeros((1, k, L), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RLNCError) as ei:
        batch.decode_batch(dev(pieces[None]), k, dec, ctx)
    assert ei.value == RLNCError.InvalidArgument
    with pytest.raises(RLNCError) as ei:
        batch.decode_ragged([(dev(pieces), k, dec[0])], ctx)
    assert ei.value == RLNCError.InvalidArgument
    ctx.set_decode_path(0)
    batch.decode_batch(dev(pieces[None]), k, dec, ctx)  # mode 1 runs
    # back in mode 0 the context is the exact replica again
    ctx.set_rank_mode(0)
    differs = 0
    for k, L, pieces in inputs:
        dec = torch.zeros((1, k, L), dtype=torch.uint8, device="cuda:0")
        pst, ost, dl = batch.decode_batch(dev(pieces[None]), k, dec, ctx)
        od = OracleDecoder(L, k)
        want = [od.decode(p) for p in pieces]
        assert list(pst[0]) == want
        pay = od.padded_payload()
        assert np.array_equal(host(dec)[0, : pay.shape[0]], pay)
        st, _ = od.get_decoded_data()
        assert ost[0] == st
        differs += want != true_rank_model(k, pieces[:, :k])[0]
    assert differs >= 1  # the inputs do tell the modes apart


def test_cross_mode_agreement_on_dense_objects():
    import torch

    import rlnc_amd
    from oracle.oracle import OracleDecoder
    from rlnc_amd import batch

    k, m, L, nobj = 32, 36, 64, 6
    rng = np.random.default_rng(3200)
    objs = []
    for _ in range(nobj):
        src = npo.pad(rng.integers(0, 256, k * L - 9, dtype=np.uint8), k)
        co = rng.integers(0, 256, (m, k), dtype=np.uint8)
        pieces = npo.encode(src, co)
        od = OracleDecoder(L, k)
        ref = [od.decode(p) for p in pieces]
        assert ref == true_rank_model(k, co)[0]  # the premise: the two models agree on these inputs
        objs.append(pieces)
    pieces = dev(np.stack(objs))
    ctx = rlnc_amd.Context(0)
    out = []
    for mode in (0, 1):
        ctx.set_rank_mode(mode)
        T, ps, rk = eliminate(ctx, pieces, k)
        dec = torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0")
        pst, ost, dl = batch.decode_batch(pieces, k, dec, ctx)
        out.append((T, ps, rk, host(dec), pst, ost, dl))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_decode_batch_device_under_graph_capture(ctx1):
    import torch

    from rlnc_amd import batch

    k, m, L, nobj = 16, 24, 4096, 8
    objs = make_objects(np.random.default_rng(99), k, m, L, nobj)
    pieces = dev(np.stack([x[2] for x in objs]))

    def outputs():
        return (torch.zeros((nobj, k, L), dtype=torch.uint8, device="cuda:0"),
                torch.full((nobj, m), -1, dtype=torch.int32, device="cuda:0"),
                torch.full((nobj,), -1, dtype=torch.int32, device="cuda:0"),
                torch.full((nobj,), -1, dtype=torch.int64, device="cuda:0"))

    import rlnc_amd

    ctx = rlnc_amd.Context(0)  # its workspaces become bound to the graph
    ctx.set_rank_mode(1)
    eager = outputs()
    batch.decode_batch_device(pieces, k, *eager, ctx)  # the eager run of the shape: workspaces grow here
    torch.cuda.synchronize()
    check_decoded(objs, k, host(eager[0]), host(eager[1]), host(eager[2]), host(eager[3]))
    cap = outputs()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            batch.decode_batch_device(pieces, k, *cap, ctx)
    for _ in range(2):
        for t in cap:
            t.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(cap, eager):
            assert torch.equal(a, b)


def test_cpp_mirror_rank_mode():
    exe = os.path.join(ROOT, "build", "test_true_rank")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_true_rank.cpp"), "-L" + os.path.join(ROOT, "rlnc_amd"),
                           "-lrlnc_hip", "-Wl,-rpath," + os.path.join(ROOT, "rlnc_amd"), "-pthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout
