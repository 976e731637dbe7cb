"""bench.py's --dump-outputs and --full.  CPU: the .npy files dump_outputs writes (names, float32,
the seeded sample) from host tensors, and the options on the launcher's dry path.  GPU: one plain
run of the default config -- its result line holds the headline fields and none of the --full legs,
and the dumped checksums are the oracle's on the seeded batch of the last timed step."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from oracle import oracle as O

BENCH = os.path.join(bench.ROOT, "bench.py")
FULL_ONLY = ("verified", "cpu_baseline", "e2e_host_to_host")


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=300)


def test_options_accepted_on_the_dry_path(tmp_path):
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--dump-outputs", str(tmp_path / "d")],
             PICO_BENCH_DRY="1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (tmp_path / "d").exists()                   # the dry path computes nothing to dump


def test_dump_uniform_is_float32_of_the_uint16_results(tmp_path):
    out = torch.tensor([0, 1, -1, -32768, 32767], dtype=torch.int16)      # int16 storage of uint16 checksums
    bench.dump_outputs(str(tmp_path), 0, {"kind": "uniform"}, None, out)
    assert os.listdir(tmp_path) == ["checksum.npy"]
    got = np.load(tmp_path / "checksum.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, [0, 1, 65535, 32768, 32767])


def test_dump_fused_tx_results_and_seeded_frame_sample(tmp_path):
    n = 7
    buf = torch.arange(1000, dtype=torch.int32).to(torch.uint8)
    out = (torch.full((n,), -2, dtype=torch.int16), torch.arange(n, dtype=torch.int16), torch.ones(n, dtype=torch.uint8))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), 0, {"kind": "ipv4", "tx": True}, (buf, None, 0, None), out)
    bench.dump_outputs(str(b), 1, {"kind": "ipv4", "tx": True}, (buf, None, 0, None), out)
    names = ["frames_sample", "net_checksum", "transport_checksum", "verdict"]
    assert sorted(os.listdir(a)) == [f"{x}.npy" for x in names]
    assert sorted(os.listdir(b)) == [f"{x}.rank1.npy" for x in names]
    for x in names:
        u, v = np.load(a / f"{x}.npy"), np.load(b / f"{x}.rank1.npy")
        assert u.dtype == np.float32
        np.testing.assert_array_equal(u, v)                # the same sample positions every time
    np.testing.assert_array_equal(np.load(a / "net_checksum.npy"), np.full(n, 65534.0))
    s = np.load(a / "frames_sample.npy")
    assert s.size == bench.DUMP_SAMPLE and set(np.unique(s)) == set(range(256))
    # RX (and TX without F_WRITE) leaves the frames alone: results only
    bench.dump_outputs(str(tmp_path / "c"), 0, {"kind": "ipv4", "tx": True, "write": False}, (buf, None, 0, None), out)
    assert sorted(os.listdir(tmp_path / "c")) == ["net_checksum.npy", "transport_checksum.npy", "verdict.npy"]


@pytest.mark.gpu
def test_plain_run_line_and_dumped_checksums(tmp_path):
    steps, rot = 4, 3
    r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rotate", str(rot),
              "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u16" and line["steps"] == steps and line["warmup"] == 1
    cfg = bench.CONFIGS["c1"]
    n, ln = cfg["frames"], cfg["frame_bytes"]
    # value and ms_per_step are one measurement (both rounded in the line)
    assert line["value"] == pytest.approx(n * ln / (line["ms_per_step"] / 1e3) / bench.GIB, rel=1e-3)
    assert not any(k in line for k in FULL_ONLY)
    # the last timed step ran on rotation slot (steps - 1) % rot, whose frames main() seeds with 1000 + slot
    frames = bench.make_uniform(n, ln, torch.device("cuda:0"), 1000 + (steps - 1) % rot).cpu().numpy()
    _, want = O.uniform_mt(frames, ln, ln, n, max(1, min(16, len(os.sched_getaffinity(0)))), kind="port")
    got = np.load(tmp_path / "checksum.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want.astype(np.float32))
