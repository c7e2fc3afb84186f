"""CPU: `bench.py --gpus N` starts its own ranks (one child process per GPU through
torch.distributed.run) when called from a plain shell, refuses a launcher that started a different
number of ranks, and keeps the all-gather of the rendered maps inside the timed region.  `--dry`
swaps the HIP render for stand-in maps and RCCL for gloo so the launcher, the rendezvous, the
sharding arithmetic and the collective run here, and `--dump-outputs` writes the last timed step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=240):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True,
                          text=True, timeout=timeout)


def _json_line(r):
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (r.stdout, r.stderr[-2000:])
    return json.loads(lines[0])


@pytest.mark.parametrize("gather,steps,gathers", [("step", 4, 5), ("image", 144, 3)])
def test_bench_starts_its_own_ranks(gather, steps, gathers):
    r = _run(["--dry", "--gpus", "2", "--steps", str(steps), "--warmup", "1", "--gather", gather])
    assert r.returncode == 0, r.stderr[-2000:]
    out = _json_line(r)
    assert out["n_gpus"] == 2 and out["world_size"] == 2 and out["steps"] == steps
    assert out["rows_in_order"] and out["gathers"] == gathers          # warm-up + timed region
    # image mode: 72 calls of 2 x 1024 rays fill one 288 x 512 image; the warm-up call is flushed by the fence
    assert out["gathered_rows"][-1] == (2048 if gather == "step" else 2 * 72 * 1024)


def test_strong_scaling_splits_the_rays():
    r = _run(["--dry", "--gpus", "2", "--steps", "2", "--warmup", "0", "--workload", "zest_val_4096x192",
              "--scaling", "strong", "--gather", "step"])
    assert r.returncode == 0, r.stderr[-2000:]
    out = _json_line(r)
    assert out["scaling"] == "strong" and out["rays_per_gpu"] == 2048 and out["gathered_rows"][0] == 4096


def test_rank_count_mismatch_is_an_error():
    r = _run(["--dry", "--gpus", "2", "--steps", "1", "--warmup", "0"],
             env={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29999"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_dry_dump_outputs_holds_the_last_timed_step(tmp_path):
    """--dump-outputs writes the arrays of the LAST timed step (stand-in maps carry their step number) as float32,
    the same in every run with the same arguments."""
    dumps = []
    for i in range(2):
        out_dir = tmp_path / str(i)
        r = _run(["--dry", "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(out_dir)])
        assert r.returncode == 0, r.stderr[-2000:]
        assert _json_line(r)["steps"] == 3
        assert sorted(os.listdir(out_dir)) == ["zest_packed_maps.npy"]
        dumps.append(np.load(out_dir / "zest_packed_maps.npy"))
    got = dumps[0]
    assert got.dtype == np.float32 and got.shape == (1024, 16)
    want = np.arange(1024, dtype=np.float32)[:, None].repeat(16, 1) + np.float32(0.001 * 4)   # step 4 = 2 + 3 - 1
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(dumps[1], got)


def test_dump_outputs_samples_past_the_size_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 << 20)
    ret = {"a": torch.arange(1 << 20, dtype=torch.float32), "b": torch.ones(2, 1 << 19, dtype=torch.float64), "n": 3}
    bench.dump_outputs(ret, str(tmp_path / "x"))
    bench.dump_outputs(ret, str(tmp_path / "y"))
    a, b = np.load(tmp_path / "x" / "a.npy"), np.load(tmp_path / "x" / "b.npy")
    assert a.dtype == b.dtype == np.float32 and a.size == b.size == (2 << 20) // 8
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x")) <= 3 << 20
    assert (np.diff(a) > 0).all() and (b == 1).all()                 # sorted sample of the flattened elements
    np.testing.assert_array_equal(np.load(tmp_path / "y" / "a.npy"), a)


def test_steps_must_be_positive():
    r = _run(["--dry", "--gpus", "1", "--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_bench_line_and_dump_on_the_gpu(tmp_path):
    """A plain run (no --full) on one GPU: the headline keys only, none of the --full measurements, and the rendered
    maps of its last timed step in --dump-outputs."""
    r = _run(["--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path)], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _json_line(r)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"):
        assert k in out, k
    assert out["steps"] == 5 and out["dtype"] == "bf16" and out["value"] > 1e5 and out["ms_per_step"] > 0
    assert not {"roofline", "modes", "cpu_baseline", "psnr"} & set(out)
    maps = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert {"rgb_map", "depth_map", "acc_map", "zest_packed_maps"} <= set(maps)
    assert maps["rgb_map"].shape == (1, 1024, 3) and maps["zest_packed_maps"].shape[0] == 1024
    for k, x in maps.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), k
    np.testing.assert_array_equal(maps["rgb_map"][0], maps["zest_packed_maps"][:, 0:3])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "f16x3"])
def test_bench_json_line_on_the_gpu(mode):
    """The real (non --dry) bench on one GPU with --full, short: ONE JSON line with the contract's keys, the roofline
    object and the other operand types in `modes` - also when the headline mode is f16x3 (the line used to die on a
    KeyError after all the timing was done)."""
    r = _run(["--full", "--steps", "5", "--warmup", "2", "--mode", mode, "--no-cpu-baseline"], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _json_line(r)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out, k
    assert out["dtype"] == mode and out["n_gpus"] == 1 and out["steps"] == 5 and out["value"] > 1e5
    assert out["roofline"]["bound"] == "mfma" and 0.05 < out["roofline"]["frac"] < 1.0
    assert sorted(out["modes"]) == sorted(m for m in ("bf16", "f16", "f16x3") if m != mode)
    assert out["config"]["workload"] == "nsff_static_1024x128"
