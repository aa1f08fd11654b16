"""
Launcher tests: everything that starts bench.py / torch.distributed.run child
processes or creates a process group.  The file name sorts after every other
test file so a launcher hiccup can never stand in front of a parity test under
``pytest -x`` (round-2 verdict, item 1).
"""
import os
import sys

import numpy as np
import pytest
import torch

import ngmix_amd as ngmix

pytestmark = pytest.mark.gpu


def test_bench_two_ranks_share_one_gpu(tmp_path):
    """bench.py's N > 1 path (sharding, side-stream all-gather of the result
    records, barriers, max-over-ranks timing, one JSON line from rank 0) with
    two ranks on this one GPU: RCCL refuses two ranks per device, so the
    collectives go over gloo (NGMIX_DIST_BACKEND), everything else is the
    production path"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NGMIX_DIST_BACKEND="gloo")
    # bench.py starts its two ranks itself (no torch.distributed.run)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3",
           "--warmup", "1", "--settle-steps", "2", "--nstamps", "3000", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak"
    # a --full (C2) run carries a leg of every other config at N > 1 too, each
    # with every rank's own time per step; no CPU legs beside them
    oc = d["other_configs"]
    for name in ("C3", "C4", "C5"):
        assert "error" not in oc[name], oc[name]
        assert oc[name]["n_gpus"] == 2 and oc[name]["value"] > 0
        assert len(oc[name]["per_rank_ms_per_step"]) == 2
        assert "cpu_baseline" not in oc[name]
    assert oc["C3"]["bad_status"] == 0 and oc["C3"]["kernels_ms"]["lm_eval"] > 0
    assert d["rccl_ranks"] == 2 and d["backend"] == "gloo"
    assert d["bad_status"] == 0 and d["value"] > 0
    # which of render / loglike is "dominant" at 3,000 stamps x 3 steps is
    # timing noise, and the loglike build is named pixpass_wave_kernel7: any
    # fused pixel-pass symbol is right
    assert "pixpass_wave_kernel" in d["roofline"]["kernel"], d["roofline"]["kernel"]
    assert d["roofline"]["dominant"] in ("loglike", "render")
    assert "cpu_baseline" not in d  # rank 0 at N = 1 only
    # every rank's own time per step rides in rank 0's line (skew at N = 8)
    assert len(d["per_rank_ms_per_step"]) == 2 and min(d["per_rank_ms_per_step"]) > 0
    assert max(d["per_rank_ms_per_step"]) <= d["ms_per_step"] * 1.001
    # the same launch under torch.distributed.run, and for config 4
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29541",
           os.path.join(root, "bench.py"), "--gpus", "2", "--config", "C4", "--steps", "2",
           "--warmup", "1", "--settle-steps", "0", "--nstamps", "2000"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["bad_status"] == 0 and d["admom_flags_nonzero"] == 0
    assert d["roofline"]["bound"] == "fp64_valu" and d["value"] > 0
    # config 3 (complete LM fits), two self-started ranks
    cmd3 = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "C3",
            "--steps", "2", "--warmup", "1", "--nstamps", "1500"]
    p = subprocess.run(cmd3, env=env, capture_output=True, text=True, timeout=280, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["bad_status"] == 0 and d["unit"] == "fits/s"
    assert d["roofline"]["kernel"].startswith("ngmix::lm_eval_kernel<") and d["roofline"]["frac"] > 0
    # config 5 (multi-epoch objects: every epoch of an object on one rank)
    cmd5 = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "C5",
            "--steps", "2", "--warmup", "1", "--settle-steps", "0", "--nstamps", "300"]
    p = subprocess.run(cmd5, env=env, capture_output=True, text=True, timeout=280, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["bad_status"] == 0 and d["value"] > 0
    assert d["roofline"]["bound"] == "hbm" and len(d["per_rank_ms_per_step"]) == 2
    # a world size other than --gpus is refused, not mislabelled
    cmd[cmd.index("--gpus") + 1] = "4"
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=root)
    assert p.returncode != 0 and "refusing" in p.stderr


@pytest.mark.parametrize("spec, leg", [("C4:1:step33", "C4"), ("C3:1:setup", "C3"),
                                       ("C5:0:step1", "C5"), ("C4:0:build", "C4")])
def test_bench_rank_local_failure_in_a_leg_keeps_the_headline(spec, leg):
    """a failure on ONE rank inside an other_configs leg (injected: before the
    leg's workload is built, at the entry of the steps, in a settle step, in a
    timed step; on rank 0 or rank 1): the
    ranks agree on it (bench.run_leg), the failing rank keeps the leg's
    all-gathers matched with empty records, nobody blocks, every other leg and
    the headline line are intact"""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NGMIX_DIST_BACKEND="gloo", NGMIX_BENCH_FAIL=spec)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--settle-steps", "1", "--nstamps", "2000", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["bad_status"] == 0
    oc = d["other_configs"]
    for name in ("C3", "C4", "C5"):
        if name == leg:
            assert "error" in oc[name], oc[name]
            # rank 0 reports its own failure, or that a peer failed
            assert ("injected failure" in oc[name]["error"]) == spec.startswith(leg + ":0:")
            assert "PeerFailure" in oc[name]["error"] or "injected" in oc[name]["error"]
        else:
            assert "error" not in oc[name], oc[name]
            assert oc[name]["value"] > 0 and oc[name]["n_gpus"] == 2


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """a plain run times the steps and prints the headline line, none of the
    --full extras; --dump-outputs writes the last step's loglike records,
    statuses and a sample of the model image, identical from run to run"""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3",
               "--warmup", "1", "--settle-steps", "2", "--nstamps", "3000",
               "--dump-outputs", str(out)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=root)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["unit"] == "pixel-gaussian evals/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f64" and d["bad_status"] == 0
        for extra in ("other_configs", "cpu_baseline", "fresh_render"):
            assert extra not in d, extra
        got = {name: np.load(str(out / (name + ".npy")))
               for name in ("loglike", "status", "image")}
        assert got["loglike"].shape == (3000, 4) and got["loglike"].dtype == np.float64
        assert np.all(got["loglike"][:, 3] == 48 * 48) and np.isfinite(got["loglike"]).all()
        assert got["status"].shape == (3000,) and np.all(got["status"] == 0)
        assert got["image"].shape == (1024, 48, 48) and got["image"].dtype == np.float64
        assert got["image"].max() > 0
        dumps.append(got)
    for name in dumps[0]:
        np.testing.assert_array_equal(dumps[0][name], dumps[1][name])


def test_bench_refuses_more_ranks_than_gpus():
    """RCCL needs one device per rank: bench.py --gpus 2 on this one-GPU box
    stops with a message instead of measuring one GPU"""
    import subprocess
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a one-GPU box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "NGMIX_DIST_BACKEND")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"],
                       env=env, capture_output=True, text=True, timeout=280, cwd=root)
    assert p.returncode == 2
    assert "only 1 GPU(s) are visible" in p.stderr


def test_rccl_allgather_world1():
    """the RCCL backend itself ("nccl" on ROCm), as far as one GPU can take it:
    a one-rank process group, the bench's all-gather helper on device records"""
    import socket
    import torch.distributed as dist
    from ngmix_amd import distributed as nd
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0,
                            world_size=1, device_id=torch.device("cuda", 0))
    try:
        assert dist.get_backend() == "nccl"
        rec = torch.arange(12, dtype=torch.float64, device="cuda").reshape(3, 4)
        full = nd.allgather_records(rec, n_objects=3)
        torch.cuda.synchronize()
        assert torch.equal(full, rec)
        out = nd.gather_object_results(lambda lo, hi: rec[lo:hi], 3, (4,))
        assert torch.equal(out, rec)
        t = torch.tensor([1.5], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        assert float(t) == 1.5
    finally:
        dist.destroy_process_group()


