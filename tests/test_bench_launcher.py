"""bench.py --gpus N outside torchrun: the parent starts N ranks through
torch.distributed.run as child processes and returns torchrun's status. CPU checks: the launcher command,
and that N rank processes really start (each one reaches the GPU check after joining a gloo group of N and
fails there on this GPU-less host) and a rank's failure is a nonzero exit of the parent."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_launcher_cmd_is_the_driver_form():
    import bench
    cmd = bench.launcher_cmd(4, ["--gpus", "4", "--steps", "3"], 29533)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd and "--master-port=29533" in cmd
    i = cmd.index("--master-addr")
    assert cmd[i + 1] == "127.0.0.1"
    assert cmd[-5:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "3"]


def test_dump_outputs_writes_float32_within_budget(tmp_path, monkeypatch):
    """--dump-outputs: one float32 .npy per field of the step's result; an array over its share of the
    budget is written as the same seeded sample every time."""
    import collections
    import numpy as np
    import torch
    import bench
    Out = collections.namedtuple("Out", ["loss", "embs_norm"])
    out = Out(torch.tensor(1.5, dtype=torch.float64), torch.arange(1000, dtype=torch.float32).reshape(250, 4))
    bench.dump_outputs(str(tmp_path / "a"), out)
    loss, norms = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "embs_norm.npy")
    assert loss.dtype == np.float32 and loss.shape == () and float(loss) == 1.5
    assert norms.dtype == np.float32 and np.array_equal(norms, out.embs_norm.numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4 * 100)   # 100 elements per array
    bench.dump_outputs(str(tmp_path / "b"), out)
    bench.dump_outputs(str(tmp_path / "c"), out)
    s1, s2 = np.load(tmp_path / "b" / "embs_norm.npy"), np.load(tmp_path / "c" / "embs_norm.npy")
    assert s1.shape == (100,) and np.array_equal(s1, s2) and np.all(np.diff(s1) > 0)
    assert np.load(tmp_path / "b" / "loss.npy").shape == ()


def test_plain_run_options():
    """--full is off by default and --dump-outputs takes a directory."""
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
        assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
        sys.argv = ["bench.py", "--full", "--dump-outputs", "d"]
        a = bench.parse()
        assert a.full and a.dump_outputs == "d"
    finally:
        sys.argv = old


def test_gpus_2_starts_two_ranks_and_propagates_failure():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(RQVAE_DIST_BACKEND="gloo", CUDA_VISIBLE_DEVICES="", PYTHONUNBUFFERED="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-extras"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0
    out = r.stdout + r.stderr
    # both ranks ran main() past the process-group join: each exits at the GPU check
    assert out.count("bench.py needs an MI355X") >= 2, out[-3000:]
    assert "{\"metric\"" not in r.stdout
