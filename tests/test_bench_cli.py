"""bench.py's launcher contract on CPU (no GPU needed): `--gpus N` either runs N
ranks or exits non-zero before touching a device.

  * no launcher and N > 1: bench starts torch.distributed.run with N processes
    itself (checked here by intercepting the child command);
  * a launcher whose WORLD_SIZE differs from --gpus: exit 2;
  * more ranks than visible GPUs without --stack-ranks: exit 2;
  * --single-process under a launcher: exit 2.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=120)


def test_too_few_gpus_exits_2():
    p = _run(["--gpus", "2"])  # this container has no GPU
    assert p.returncode == 2, p.stderr[-2000:]
    assert "needs 2 GPUs" in p.stderr


def test_world_size_mismatch_exits_2():
    p = _run(["--gpus", "2"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2 and "3 ranks are running" in p.stderr, p.stderr[-2000:]


def test_single_process_under_launcher_exits_2():
    p = _run(["--gpus", "2", "--single-process"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2 and "one process" in p.stderr, p.stderr[-2000:]


def test_single_process_too_few_gpus_exits_2():
    p = _run(["--gpus", "2", "--single-process"])
    assert p.returncode == 2 and "needs 2 GPUs" in p.stderr, p.stderr[-2000:]


def _parse(argv, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_leaves_the_secondary_legs_out(monkeypatch):
    """Without --full every leg beyond the timed steps is off, whatever else is given;
    --steps and --warmup are taken as given."""
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_count_work and a.no_draw_frame and a.side_scenes == ""
    a = _parse(["--side-scenes", "csg32_nested"], monkeypatch)
    assert a.side_scenes == ""


def test_full_run_keeps_the_secondary_legs_and_their_switches(monkeypatch):
    a = _parse(["--full"], monkeypatch)
    assert a.full and not (a.no_cpu_baseline or a.no_count_work or a.no_draw_frame)
    assert a.side_scenes == "csg32_nested"
    a = _parse(["--full", "--no-cpu-baseline", "--side-scenes", ""], monkeypatch)
    assert a.no_cpu_baseline and not a.no_count_work and a.side_scenes == ""


def test_dump_outputs_writes_the_frame(tmp_path):
    """A frame within the limit is written whole, as float32."""
    np = pytest.importorskip("numpy")
    sys.path.insert(0, ROOT)
    import bench
    frame = np.arange(5 * 7 * 4, dtype=np.float32).reshape(5, 7, 4)
    bench.dump_outputs(str(tmp_path / "out"), frame)
    assert sorted(os.listdir(tmp_path / "out")) == ["frame.npy"]
    got = np.load(tmp_path / "out" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)


def test_dump_outputs_samples_a_frame_over_the_limit(tmp_path, monkeypatch):
    """Over the limit: the same pixels every time, in order, with their indices, and the
    files together stay under the limit."""
    np = pytest.importorskip("numpy")
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    frame = np.random.default_rng(5).random((33, 17, 4), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame)
    px, idx = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "frame_pixels.npy")
    assert px.dtype == np.float32 and idx.dtype == np.float64 and px.shape == (len(idx), 4)
    assert 0 < len(idx) < 33 * 17 and np.all(np.diff(idx) > 0)
    assert np.array_equal(px, frame.reshape(-1, 4)[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "frame_pixels.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 4096


@pytest.mark.parametrize("n", [2, 8])
def test_self_launch_starts_n_ranks(n, monkeypatch):
    """The command bench starts without a launcher: torch.distributed.run, N processes
    on one node, 127.0.0.1, this script with the same arguments; its exit status is
    bench's."""
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    class Done:
        returncode = 7

    def fake_run(cmd, *a, **k):
        seen["cmd"] = cmd
        return Done()

    monkeypatch.setattr(bench, "visible_devices", lambda: n)
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", str(n), "--steps", "3"])
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert ex.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert f"--nproc-per-node={n}" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", str(n), "--steps", "3"] and cmd[-5].endswith("bench.py")
