"""bench.py's plain run, --full and --dump-outputs.

CPU: a plain run leaves every extra leg off (--full turns them on);
dump_outputs writes each output as exact 32-bit words in float64, samples a
large output at fixed rows that hold the first and the last, stays within its
byte budget and folds the whole output.
GPU: one small plain run of bench.py itself: --steps sets the timed steps,
the line carries ms_per_step and none of the --full legs, and the dumped
hashes are the oracle's hashes of the keys the run generates.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from oracle_lib import load_oracle, orc_fixed  # noqa: E402
from raikv_amd.workload import STATIC_SEED  # noqa: E402


def test_plain_run_has_every_extra_leg_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def _words(t):
    return t.numpy().reshape(t.shape[0], int(np.prod(t.shape[1:]))).view(np.uint32)


def test_dump_outputs_small_outputs_whole_and_exact(tmp_path):
    g = torch.Generator().manual_seed(5)
    outs = {"hashes": torch.randint(-2**63, 2**63 - 1, (300, 2), dtype=torch.int64, generator=g),
            "multi": torch.randint(-2**63, 2**63 - 1, (40, 4, 2), dtype=torch.int64, generator=g),
            "crc": torch.randint(-2**31, 2**31 - 1, (77,), dtype=torch.int32, generator=g),
            "none": torch.empty((0, 2), dtype=torch.int64)}
    info = bench.dump_outputs(str(tmp_path), outs)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}{s}.npy" for n in outs for s in ("", "_rows", "_fold"))
    for name, t in outs.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and info[name]["rows_written"] == info[name]["rows"] == t.shape[0]
        assert np.array_equal(got, _words(t).astype(np.float64))
        assert np.array_equal(np.load(tmp_path / f"{name}_rows.npy"), np.arange(t.shape[0]))
        fold = np.load(tmp_path / f"{name}_fold.npy").astype(np.uint64)
        total = fold[:, 0] | fold[:, 1] << np.uint64(16) | fold[:, 2] << np.uint64(32) | fold[:, 3] << np.uint64(48)
        want = _words(t).view(np.int32).astype(np.int64).sum(0).view(np.uint64)
        assert np.array_equal(total, want)


def test_dump_outputs_samples_a_large_output_within_its_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    t = torch.arange(2 * 100_000, dtype=torch.int64).reshape(100_000, 2) * 0x100000001
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), {"hashes": t, "items": t[:, 0].contiguous()})
    bench.dump_outputs(str(b), {"hashes": t, "items": t[:, 0].contiguous()})
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 200_000 + 6 * 128  # + the .npy headers
    for f in os.listdir(a):  # the same rows from run to run
        assert np.array_equal(np.load(a / f), np.load(b / f))
    rows = np.load(a / "hashes_rows.npy").astype(np.int64)
    assert rows[0] == 0 and rows[-1] == 99_999 and np.all(np.diff(rows) > 0)
    assert 2000 < len(rows) == info["hashes"]["rows_written"] < 100_000
    assert np.array_equal(np.load(a / "hashes.npy"), _words(t)[rows].astype(np.float64))


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_hashes_of_its_keys(tmp_path):
    n, steps = 70_001, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "2", "--keys", str(n), "--settle-ms", "0", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["full"] is False
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for leg in ("parity", "scaling_anchor", "e2e_pcie", "cpu_baseline"):
        assert leg not in line
    assert "achievable_peak" not in line["roofline"]
    # the keys of a run are fixed by its arguments: rank 0's generator, seed 1000
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000)
    keys = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=gen).cpu().numpy()
    want = orc_fixed(load_oracle(), keys, 16, STATIC_SEED)
    got = np.load(tmp_path / "hashes.npy")
    assert got.dtype == np.float64 and got.shape == (n, 4)
    assert np.array_equal(got, want.view(np.uint32).astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "hashes_rows.npy"), np.arange(n))
