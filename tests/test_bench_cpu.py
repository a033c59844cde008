"""CPU: `python bench.py --gpus N` (no launcher) must start N fresh ranks itself — before anything touches HIP — through
torch.distributed.run on 127.0.0.1, relay their status, and never exec.  Reference slot: none (harness contract)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_flag_spawns_n_ranks_without_touching_the_gpu(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    calls = {}

    def fake_call(cmd, env=None):
        calls["cmd"], calls["env"] = cmd, env
        return 7
    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    modules_before = set(sys.modules)
    try:
        bench.main()
        raise AssertionError("launch_ranks must exit with the children's status")
    except SystemExit as e:
        assert e.code == 7
    cmd = calls["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert calls["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert "points_matching_amd" not in set(sys.modules) - modules_before      # the parent never loaded the library


def test_dump_outputs_writer_dtypes_budget_and_seeded_sample(tmp_path):
    """--dump-outputs' writer: float32 kept, everything else float64 with the same values; under the budget nothing is
    cut; over it the row arrays are cut to the same seeded rows (recorded in <name>_rows.npy) and the set fits."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    rng = np.random.default_rng(5)
    arrays = {"idx": rng.integers(0, 1 << 20, (100000, 2)).astype(np.int32), "dist": rng.random(100000, np.float32),
              "mask": (rng.random(100000) < 0.5).astype(np.uint8), "F": rng.random((3, 3)), "n": 100000}
    names = bench.write_outputs(str(tmp_path / "all"), arrays)
    assert names == sorted(arrays)
    for k, v in arrays.items():
        got = np.load(str(tmp_path / "all" / (k + ".npy")))
        assert got.dtype == (np.float32 if np.asarray(v).dtype == np.float32 else np.float64)
        assert (got == np.asarray(v)).all()
    limit = 1 << 20
    for d in ("cut_a", "cut_b"):
        bench.write_outputs(str(tmp_path / d), arrays, limit=limit)
    files = sorted(os.listdir(str(tmp_path / "cut_a")))
    assert files == sorted(["%s.npy" % k for k in arrays] + ["%s_rows.npy" % k for k in ("idx", "dist", "mask")])
    assert sum(np.load(str(tmp_path / "cut_a" / f)).nbytes for f in files) <= limit
    rows = np.load(str(tmp_path / "cut_a" / "idx_rows.npy")).astype(np.int64)
    assert rows.size > 1000 and (np.diff(rows) > 0).all()
    for k in ("idx", "dist", "mask"):
        assert (np.load(str(tmp_path / "cut_a" / (k + "_rows.npy"))) == rows).all()
        assert (np.load(str(tmp_path / "cut_a" / (k + ".npy"))) == np.asarray(arrays[k])[rows]).all()
    for f in files:                                       # the sample is seeded: the same cut every time
        assert (np.load(str(tmp_path / "cut_a" / f)) == np.load(str(tmp_path / "cut_b" / f))).all()


def test_rank_process_does_not_respawn(monkeypatch):
    """With WORLD_SIZE set (we ARE a rank) the launcher branch is skipped: with no GPU the rank then stops at the
    explicit 'needs a GPU' error instead of spawning anything.  The GPU is hidden from torch so that the test is the
    same on a machine that has one (there the rank would otherwise wait in init_process_group for a rank 1)."""
    sys.path.insert(0, ROOT)
    import bench
    import subprocess
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(subprocess, "call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("spawned")))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    saved = os.dup(1)
    try:
        bench.main()
        raise AssertionError("expected SystemExit")
    except SystemExit as e:
        assert "needs a GPU" in str(e.code)
    finally:
        os.dup2(saved, 1)
        os.close(saved)
