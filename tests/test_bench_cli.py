"""CPU-only checks of bench.py's command line: `--gpus N` without a launcher starts its own N ranks as child
processes (the driver's invocation form for N = 1 must also work for N > 1), strong / weak
batch arithmetic, and the parser of the in-step timing probes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_gpus_n_builds_the_torchrun_child_command(monkeypatch):
    bench = _bench()
    seen = {}

    class FakeProc:
        stdout = iter(['{"metric": "x"}\n', "launcher chatter\n"])

        def wait(self):
            return 7

    def fake_popen(cmd, **kw):
        seen["cmd"], seen["env"] = cmd, kw["env"]
        return FakeProc()

    monkeypatch.setattr(bench.subprocess, "Popen", fake_popen)
    argv = ["--gpus", "4", "--steps", "3", "--scaling", "strong"]
    rc = bench.spawn_ranks(bench.parse_args(argv), argv)
    assert rc == 7                                            # the child's exit code is the parent's
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-len(argv):] == argv and cmd[-len(argv) - 1].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


@pytest.mark.timeout(300)
def test_gpus_2_really_starts_two_ranks_and_returns_their_failure_here():
    """No GPU in this container: both ranks must get as far as the device check and refuse (there is no CPU path), and the
    parent must hand their failure back as its own exit code -- after having decided to spawn from argv alone."""
    import torch
    if torch.cuda.is_available():             # (decided BEFORE anything is started: on a GPU box the two ranks would go for the card)
        pytest.skip("meant for the CPU-only container")
    env = dict(os.environ, MASTER_PORT="29611")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--master-port", "29611"], capture_output=True, text=True, env=env, timeout=280)
    assert r.returncode != 0
    # (the launcher ends the other rank as soon as one has failed: the second refusal may or may not reach stderr)
    assert r.stderr.count("bench.py needs an MI355X") >= 1, r.stderr[-2000:]


def test_probe_parser_pairs_stamps_and_subtracts_the_calibration():
    bench = _bench()
    T63 = 1 << 63

    def tag(kind, layer, t, end):
        v = kind | layer << 8 | t << 16 | end << 31 | T63
        return v - (1 << 64)                                   # as the int64 tensor holds it

    w = np.zeros(64, dtype=np.int64)
    rows = [(0, 0, 0, 0, 1000), (0, 0, 0, 1, 1300),            # calibration pair: 3 us
            (1, 0, 0, 0, 2000), (1, 0, 0, 1, 12300),           # gate layer 0 t=0: 103 us - 3
            (1, 2, 5, 0, 20000), (1, 2, 5, 1, 22900)]          # gate layer 2 t=5: 29 us - 3
    for i, (k, l, t, e, ticks) in enumerate(rows):
        w[2 * i], w[2 * i + 1] = tag(k, l, t, e), ticks
    d = bench.probe_durations(w, np.zeros(8, dtype=np.int64))
    assert d[(1, 0)] == [(0, 100.0)] and d[(1, 2)] == [(5, 26.0)] and d["cal_us"] == [3.0]


def test_strong_scaling_divides_the_global_batch():
    bench = _bench()
    a = bench.parse_args(["--gpus", "8", "--scaling", "strong"])
    assert a.batch == 8 and a.scaling == "strong"             # 8 in all -> 1 per GPU (main() divides by the world size)
    assert bench.parse_args([]).scaling == "weak" and bench.parse_args([]).long_steps == 200


# ------------------------------------------------------------------------------------------ the probe pass under a process group
def _probe_worker(rank, world, port, out):
    import datetime
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=30))
    bench = _bench()

    class StubTrainer:                        # what FusedTrainer.step does under a process group: ONE all-reduce per step
        def __init__(self):
            self.steps, self.bucket, self.probed = 0, torch.ones(1000), 0

        def set_probe(self, buf, mask=0):
            self.probed += buf is not None

        def step(self, X, y):
            dist.all_reduce(self.bucket, op=dist.ReduceOp.SUM)
            self.bucket.mul_(1.0 / world)
            self.steps += 1

    tr = StubTrainer()
    pbuf = torch.zeros(2 * 64, dtype=torch.int64) if rank == 0 else None
    dur, step_ms = bench.probe_steps(tr, None, None, rank, pbuf, 0x7E, 3, 64)
    t = torch.tensor([float(tr.steps)])
    dist.all_reduce(t)                        # pairs up only if both ranks left the pass with the same number of collectives
    dist.barrier()
    torch.save({"steps": tr.steps, "sum": float(t), "probed": tr.probed, "dur": dur is not None}, f"{out}.{rank}")
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_probe_pass_keeps_collectives_symmetric_across_ranks(tmp_path):
    """bench.py's in-step pricing pass runs extra trainer.step() calls, each ending in the gradient all-reduce: every rank
    must run them (rank 0 alone stamps), or rank 0's collectives have no peer and `--gpus N` never prints its line
    (round-3 advisor finding).  Two gloo ranks, a stub step that is just the all-reduce: with a rank-0-only pass this
    test dies in the 30 s collective timeout."""
    import socket
    import torch
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "probe")
    mp.spawn(_probe_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert r0["steps"] == r1["steps"] == 4 and r0["sum"] == 8.0          # 3 probed steps + 1 plain one, on both ranks
    assert r0["dur"] and not r1["dur"] and r0["probed"] == 1 and r1["probed"] == 0


def test_extra_measurements_need_full():
    """A plain run measures the headline alone; --full adds the long window, the all-reduce by itself (under a process group),
    the kernel rooflines and the CPU baseline (one rank), each of which its own --no-* / --long-steps 0 still turns off."""
    bench = _bench()
    off = {"long_steps": 0, "allreduce": False, "rooflines": False, "cpu_baseline": False}
    plain = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    assert bench.parse_args(plain).full is False
    assert bench.extras(bench.parse_args(plain), 1) == off
    assert bench.extras(bench.parse_args(plain + ["--force-dist", "--phase-events", "3"]), 1) == off
    assert bench.extras(bench.parse_args(["--gpus", "2"]), 2) == off
    assert bench.extras(bench.parse_args(plain + ["--full"]), 1) == {"long_steps": 200, "allreduce": False, "rooflines": True,
                                                                     "cpu_baseline": True}
    assert bench.extras(bench.parse_args(plain + ["--full", "--force-dist"]), 1)["allreduce"] is True
    assert bench.extras(bench.parse_args(["--gpus", "2", "--full"]), 2) == {"long_steps": 200, "allreduce": True, "rooflines": True,
                                                                            "cpu_baseline": False}
    assert bench.extras(bench.parse_args(plain + ["--full", "--no-cpu-baseline", "--no-kernel-rooflines", "--long-steps", "0"]), 1) == off


def test_steps_must_be_positive():
    bench = _bench()
    assert bench.parse_args(["--steps", "7"]).steps == 7
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_loss_parameters_and_gradients(tmp_path):
    """--dump-outputs: the loss, every updated parameter and its gradient as float32 .npy files named after the parameter."""
    import torch
    bench = _bench()
    assert bench.parse_args([]).dump_outputs is None and bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    net = torch.nn.Conv2d(3, 4, 3)
    for p in net.parameters():
        p.grad = torch.full_like(p, 0.5)
    arrays = bench.step_outputs(torch.tensor(1.25), net)
    assert sorted(arrays) == ["grad.bias", "grad.weight", "loss", "param.bias", "param.weight"]
    bench.write_outputs(str(tmp_path / "out"), arrays)
    assert np.load(tmp_path / "out" / "loss.npy").tolist() == [1.25]
    w = np.load(tmp_path / "out" / "param.weight.npy")
    assert w.dtype == np.float32 and np.array_equal(w, net.weight.detach().numpy())
    assert np.array_equal(np.load(tmp_path / "out" / "grad.bias.npy"), np.full(4, 0.5, dtype=np.float32))


def test_dump_outputs_refuses_more_than_the_limit(tmp_path):
    bench = _bench()
    big = {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, dtype=np.float32)}
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "out"), big)
    assert not (tmp_path / "out").exists()
