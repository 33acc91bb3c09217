"""GPU: bench.py's other launch modes run and verify (the default pipelined mode runs in the round-end bench and in
tests/test_gpu_multirank.py).  --graph 1 replays one captured step of the pipeline-1 form; --pipeline 0 / 1, --no-plan
(the products write their own address streams) and --encode-only are the A/B and diagnostic forms the DESIGN.md
records quote.  Reduced in size: 4 objects of config2's shape.
"""
import pytest

from test_gpu_multirank import run_bench

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", [["--graph", "1"], ["--pipeline", "0"], ["--pipeline", "1"], ["--no-plan"],
                                  ["--encode-only"], ["--variant", "7"]], ids=lambda m: "".join(m).strip("-"))
def test_bench_mode(mode):
    line = run_bench(["--full", "--objects", "4", "--steps", "3", "--warmup", "1", "--breakdown-steps", "4",
                      "--no-cpu-baseline", "--no-ceiling"] + mode)
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["breakdown"]["verified"] is True
    assert line["roofline"]["achieved"] > 0
    if "--graph" in mode:
        assert "captured HIP graph" in line["config"]["pipeline"]
        assert line["config"]["pipeline"].startswith("elimination on a side stream")


@pytest.mark.timeout(300)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full the line holds the headline figure and nothing that takes runs of its own; --dump-outputs writes
    the last timed step's outputs: the decoded sample equals the same bytes of the (seeded) source, every object
    decoded from k useful pieces and every byte sum of a decoded row is its source row's."""
    import os

    import numpy as np
    import torch

    import bench

    objs, k, L, n, m = 4, 32, 1 << 20, 64, 32
    line = run_bench(["--objects", str(objs), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["n_gpus"] == 1
    assert line["value"] == pytest.approx(bench.step_bytes(objs, k, L, n) / (line["ms_per_step"] * 1e-3) / bench.GIB,
                                          rel=2e-3)
    for moved in ("roofline", "roofline_decode", "hbm_single_pass_encode", "cpu_baseline", "breakdown"):
        assert moved not in line
    out = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(out) == {"objects", "pieces", "pieces_rowsum", "decoded", "decoded_rowsum", "piece_status",
                        "object_status", "decoded_len"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64e6
    assert out["objects"].tolist() == list(range(objs))
    assert out["pieces"].shape == out["decoded"].shape == (bench.DUMP_SAMPLE,)
    assert out["pieces_rowsum"].shape == (objs, n) and out["decoded_rowsum"].shape == (objs, k)
    assert out["object_status"].shape == out["decoded_len"].shape == (objs,)
    assert out["piece_status"].shape == (objs, m) and ((out["piece_status"] == 0).sum(axis=1) == k).all()
    # the source of rank 0, as bench.py seeds it
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x524C4E43)
    src = torch.randint(0, 256, (objs, k, L), dtype=torch.uint8, device="cuda:0", generator=gen).cpu().numpy()
    idx = bench.sample_index(src.size, bench.DUMP_SAMPLE, bench.DUMP_SEED)
    assert np.array_equal(out["decoded"], src.reshape(-1)[idx].astype(np.float32))
    assert np.array_equal(out["decoded_rowsum"], src.sum(axis=2, dtype=np.int64).astype(np.float64))
