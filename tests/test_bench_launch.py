"""`bench.py --gpus N` must measure N GPUs, never one (VERDICT r03 "What's missing" #1): without a launcher around it the script
re-executes itself under torch.distributed.run; under the driver's own torch.distributed.run it takes WORLD_SIZE from the
environment and refuses a --gpus that disagrees.  Checked here on the CPU with --dry-launch (gloo, stand-in render): N ranks
join one process group and the collectives of the selected mode, and rank 0 prints ONE JSON line with n_gpus = N."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    return env


def _json_lines(out):
    lines = []
    for ln in out.splitlines():
        ln = ln.strip()
        if ln.startswith("{") and ln.endswith("}"):
            try:
                lines.append(json.loads(ln))
            except ValueError:
                pass
    return lines


@pytest.mark.parametrize("mode", [[], ["--weak"], ["--strong"], ["--strong", "--partition", "tiles"], ["--train"]])
def test_gpus_flag_launches_that_many_ranks(mode):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-launch", "--steps", "2", "--warmup", "0"] + mode,
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    js = _json_lines(p.stdout)
    assert len(js) == 1, p.stdout                       # rank 0 only, one line
    j = js[0]
    assert p.stdout.strip().splitlines()[-1].strip().startswith("{")          # ... and it is the last line of stdout
    assert j["n_gpus"] == 2 and j["dry_launch"] is True and j["ok"] is True
    assert j["ranks"]["world_size"] == 2 and j["ranks"]["ranks_counted_by_all_reduce"] == 2
    assert len(j["ranks"]["per_rank_ms_per_step"]) == 2
    assert j["value"] is None                           # a dry launch must not look like a measurement
    assert all(j["checks"].values())
    # N > 1 without a mode flag is the STRONG line (the metric's frame partitioned over the ranks); --weak opts out
    assert j["scaling"] == ("weak" if mode in (["--weak"], ["--train"]) else "strong")
    if j["scaling"] == "strong" and "tiles" not in mode:
        assert j["checks"]["blocks_are_cost_balanced"] is True


def test_under_the_drivers_own_launcher():
    """the driver's N > 1 invocation: python -m torch.distributed.run ... bench.py --gpus N"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--dry-launch"],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    js = _json_lines(p.stdout)
    assert len(js) == 1 and js[0]["n_gpus"] == 2 and js[0]["ranks"]["ranks_counted_by_all_reduce"] == 2
    assert js[0]["ranks"]["launcher"] == "torch.distributed.run"


def test_flag_and_launcher_must_agree():
    env = _env()
    env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dry-launch"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "WORLD_SIZE = 2" in (p.stderr + p.stdout)


def test_one_rank_needs_no_launcher():
    p = subprocess.run([sys.executable, BENCH, "--dry-launch", "--steps", "1"], env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    js = _json_lines(p.stdout)
    assert len(js) == 1 and js[0]["n_gpus"] == 1 and js[0]["ranks"]["launcher"].startswith("none")


def test_more_ranks_than_gpus_is_refused_before_anything_is_launched():
    """(this container has no GPU: a real --gpus 2 must fail loudly, not fall back to one rank)"""
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs here")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1"], env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "GPU(s) visible" in (p.stderr + p.stdout)
    assert not _json_lines(p.stdout)


# ---- preflight of a multi-rank run: every way the first contact can go wrong ends in ONE JSON error line, not a hang ----
def _run_failing(env_extra, timeout=240):
    env = _env()
    env.update(env_extra)
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-launch", "--steps", "1", "--warmup", "0"], env=env, capture_output=True,
                       text=True, timeout=timeout)
    return p, _json_lines(p.stdout)


def test_every_rank_reports_its_device_binding():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-launch", "--steps", "1", "--warmup", "0"], env=_env(), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for r in (0, 1):
        assert f"[bench rank {r}/2] LOCAL_RANK {r} ->" in p.stderr, p.stderr[-2000:]


def test_a_rank_that_never_arrives_gives_an_error_line_not_a_hang():
    """rank 1 sleeps in front of the rendezvous: rank 0's watchdog prints the error line after DSN_BENCH_INIT_TIMEOUT seconds"""
    p, js = _run_failing({"DSN_BENCH_TEST_FAIL": "hang_rank1", "DSN_BENCH_INIT_TIMEOUT": "8"})
    assert p.returncode != 0
    errs = [j for j in js if j.get("error")]
    assert errs and errs[0]["value"] is None and errs[0]["n_gpus"] == 2 and "did not finish within 8 s" in errs[0]["error"], (p.stdout, p.stderr[-1500:])
    assert not [j for j in js if j.get("value") is not None]


def test_a_rank_without_a_device_says_so_in_a_json_line():
    p, js = _run_failing({"DSN_BENCH_TEST_FAIL": "nodev_rank1", "DSN_BENCH_INIT_TIMEOUT": "8"})
    assert p.returncode != 0
    errs = [j for j in js if j.get("error")]
    assert errs and any("has no GPU" in j["error"] and j["failed_rank"] == 1 for j in errs), (p.stdout, p.stderr[-1500:])


def test_ranks_are_counted_before_anything_is_timed():
    """the first collective is an all-reduce of ones: a world the library miscounts stops the run"""
    p, js = _run_failing({"DSN_BENCH_TEST_FAIL": "miscount", "DSN_BENCH_INIT_TIMEOUT": "60"})
    assert p.returncode != 0
    errs = [j for j in js if j.get("error")]
    assert errs and all("counted 1 rank(s)" in j["error"] for j in errs), (p.stdout, p.stderr[-1500:])


# ---- --dump-outputs / --steps: what the timed path computed, and how many steps were timed ----
def test_steps_below_one_are_refused():
    p = subprocess.run([sys.executable, BENCH, "--dry-launch", "--steps", "0"], env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr
    assert not _json_lines(p.stdout)


def test_dump_outputs_refuses_a_mode_it_does_not_dump(tmp_path):
    p = subprocess.run([sys.executable, BENCH, "--dry-launch", "--train", "--steps", "1", "--dump-outputs", str(tmp_path / "d")], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--dump-outputs" in p.stderr
    assert not os.path.exists(tmp_path / "d")


def test_dump_outputs_writes_float_arrays_within_64_mb(tmp_path):
    """render_rays' result at the headline size (512 x 512 rays x 64 samples): every array as float32, the [R, S] one on a fixed seeded
    row sample, and the same rows in every run"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from benchlib.common import DUMP_SAMPLE_ROWS, dump_outputs
    R, S = 512 * 512, 64
    g = torch.Generator().manual_seed(1)
    out = {"color": torch.rand(R, 3, generator=g), "disp_map": torch.rand(R, generator=g), "acc_map": torch.rand(R, generator=g),
           "depth_map": torch.rand(R, generator=g), "z_vals": torch.rand(R, S, generator=g)}
    out["disp_map"][::7] = float("nan")           # (rays with acc_map = 0: 0 / 0, like the reference)
    out["disp_map"][3] = float("inf")
    out["disp_map"][5] = -float("inf")
    shapes = dump_outputs(str(tmp_path / "a"), out)
    dump_outputs(str(tmp_path / "b"), out)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{k}.npy" for k in shapes) and "z_vals_rows.npy" in files
    assert "disp_map_nonfinite.npy" in files and "color_nonfinite.npy" not in files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 2 ** 20
    rows = np.load(tmp_path / "a" / "z_vals_rows.npy")
    assert rows.dtype == np.float64 and rows.shape == (DUMP_SAMPLE_ROWS,) and len(np.unique(rows)) == DUMP_SAMPLE_ROWS
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, b), f
    d, code = out["disp_map"].numpy(), np.load(tmp_path / "a" / "disp_map_nonfinite.npy")
    assert np.array_equal(code == 1, np.isnan(d)) and code[3] == 2 and code[5] == 3 and int((code > 0).sum()) == int((~np.isfinite(d)).sum())
    fin = np.isfinite(d)
    assert np.array_equal(np.load(tmp_path / "a" / "disp_map.npy")[fin], d[fin]) and not np.load(tmp_path / "a" / "disp_map.npy")[~fin].any()
    for k in ("color", "acc_map", "depth_map"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), out[k].numpy()), k
    assert np.array_equal(np.load(tmp_path / "a" / "z_vals.npy"), out["z_vals"].numpy()[rows.astype(np.int64)])


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_frame(tmp_path):
    """a small headline line with --dump-outputs, twice: the result line names the dump, ms_per_step is per timed step, and two runs
    with the same arguments write the same arrays (the inputs are seeded)"""
    import numpy as np
    cmd = [sys.executable, BENCH, "--gpus", "1", "--hw", "128", "--steps", "3", "--warmup", "1", "--no-extras", "--no-roofline",
           "--no-cpu-baseline"]
    js = []
    for d in ("a", "b"):
        p = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        js.append(_json_lines(p.stdout)[-1])
    j = js[0]
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and abs(j["value"] - 128 * 128 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert j["dumped_outputs"]["shapes"]["color"] == [128 * 128, 3]
    files = sorted(os.listdir(tmp_path / "a"))
    assert {"color.npy", "acc_map.npy", "depth_map.npy", "disp_map.npy", "z_vals.npy"} <= set(files)
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, b), f
    acc = np.load(tmp_path / "a" / "acc_map.npy")
    assert float(acc.max()) > 0.05          # the frame shows the body
    # disp_map is NaN exactly on the rays with acc_map = 0 (like the reference): written as 0, coded 1
    code = np.load(tmp_path / "a" / "disp_map_nonfinite.npy") if "disp_map_nonfinite.npy" in files else np.zeros_like(acc)
    assert np.array_equal(code == 1, acc == 0) and not (code > 1).any()


# ---- a plain run measures its headline figure only; --full adds the secondary measurements ----
SECONDARY = ("roofline", "cpu_baseline", "cpu_baseline_c", "eager_gpu_baseline", "train", "train_w4", "ms_per_frame_by_weights")


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_the_secondary_measurements():
    """without --full the line carries the headline figure and what the timed frames counted, nothing measured in runs of its own;
    --full (here without the baselines and the extras) adds the frame alone and the roofline pass, and the headline keys stay"""
    cmd = [sys.executable, BENCH, "--gpus", "1", "--hw", "128", "--steps", "2", "--warmup", "1"]
    js = []
    for extra in ([], ["--full", "--no-cpu-baseline", "--no-extras"]):
        p = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        js.append(_json_lines(p.stdout)[-1])
    plain, full = js
    for j in js:
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "whole_frame"):
            assert k in j, k
        assert j["steps"] == 2 and j["warmup"] == 1 and abs(j["value"] - 128 * 128 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert not [k for k in SECONDARY if k in plain], plain.keys()
    assert "ms_per_frame_alone" not in plain["config"] and "by_weights" not in plain["config"]
    assert full["config"]["ms_per_frame_alone"] > 0 and full["roofline"]["kernel_ms"] > 0
    assert not [k for k in SECONDARY if k in full and k != "roofline"], full.keys()
