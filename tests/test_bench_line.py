"""The line `bench.py` prints is the record the driver keeps: it has to be ONE JSON object, small enough for the driver to hold
(round 5's 30 KB line came back as `parsed: null`), and carry the contract's keys + `roofline` + `cpu_baseline`.  The full result goes to a
detail file.  CPU only: the assembly is run on a stored full result and through `--dry-run` (kernels replaced by a sleep)."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("stored", ["r05_bench_c3.json", "r04_bench_c3.json", "r05_bench_c5.json"])
def test_headline_line_of_a_full_result_is_small_and_complete(stored, tmp_path):
    bench = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", stored)))
    assert len(json.dumps(full)) > 2000
    line = bench.headline_line(full, "gpurun_out/bench_detail.json")
    assert "\n" not in line and len(line) < bench.LINE_MAX_BYTES < 8000
    res = json.loads(line)
    for k in CONTRACT:
        assert k in res, k
    assert res["value"] == pytest.approx(full["value"], rel=1e-5) and res["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert res["config"]["workload"] == full["config"]["workload"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in res["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in res["cpu_baseline"], k
    assert all(len(v) <= bench.LINE_STR_MAX for v in res["config"].values() if isinstance(v, str))
    # emit(): the full result lands in the detail file, stdout gets the line only
    import io, contextlib
    buf = io.StringIO()
    path = str(tmp_path / "d" / "detail.json")
    with contextlib.redirect_stdout(buf):
        bench.emit(full, path)
    printed = buf.getvalue()
    assert printed.count("\n") == 1 and json.loads(printed)["detail"] == path
    assert json.load(open(path))["value"] == full["value"]


def test_headline_line_survives_an_oversized_block():
    """Whatever a block grows to, the printed line stays under the bound (optional blocks are dropped, the contract keys stay)."""
    bench = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_c3.json")))
    full["ser"] = dict(per_mode_rank0=[0.0] * 4000)
    full["tier_b"]["checks"] = {("k%d" % i): True for i in range(2000)}
    line = bench.headline_line(full, None)
    assert len(line) < bench.LINE_MAX_BYTES
    res = json.loads(line)
    assert all(k in res for k in CONTRACT) and "roofline" in res and "cpu_baseline" in res


def test_two_rank_line_parses_and_is_small(tmp_path):
    """`bench.py --gpus 2 --dry-run` end to end over the socket backend: rank 0's line is the compact one, with the per-rank step times."""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    detail = str(tmp_path / "detail.json")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1", "--detail-out", detail],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 8000
    res = json.loads(lines[0])
    for k in CONTRACT:
        assert k in res, k
    assert res["n_gpus"] == 2 and res["ranks_seen"] == 2 and len(res["ms_per_step_per_rank"]) == 2 and res["comm_backend"] == "tcp"
    assert res["detail"] == detail and json.load(open(detail))["n_gpus"] == 2


def test_two_rank_line_under_torchrun_as_the_driver_starts_it(tmp_path):
    """The driver's own command for N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P
    bench.py --gpus N --steps K --warmup W` (here with --dry-run: no GPU).  Exactly ONE JSON line on stdout, from rank 0, compact, with both ranks seen."""
    pytest.importorskip("torch")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    detail = str(tmp_path / "detail.json")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run", "--detail-out", detail]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 8000, lines
    res = json.loads(lines[0])
    for k in CONTRACT:
        assert k in res, k
    assert res["n_gpus"] == 2 and res["ranks_seen"] == 2 and res["steps"] == 3 and res["warmup"] == 1 and len(res["ms_per_step_per_rank"]) == 2
    assert res["value"] == pytest.approx(2 * res["config"]["nsym_per_channel"] * 3 / (res["ms_per_step"] * 3e-3) / 1e6, rel=1e-3)


def test_full_flag_is_accepted_and_leaves_the_contract_alone(tmp_path):
    """`--full` (everything beyond the headline) is an option of every run; the dry run's line carries the contract's keys with or without it."""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    for extra in ([], ["--full"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "1",
                              "--detail-out", str(tmp_path / "detail.json")] + extra, capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        res = json.loads(lines[0])
        assert all(k in res for k in CONTRACT) and res["steps"] == 2 and res["warmup"] == 1


@pytest.mark.gpu
def test_plain_run_certifies_its_headline_and_stops_there(tmp_path):
    """A plain run on the GPU: the headline, certified against the exact path in the same run, and nothing that only `--full` measures."""
    detail = str(tmp_path / "detail.json")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nsym", str(2 ** 18), "--steps", "2", "--warmup", "1",
                          "--detail-out", detail], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert all(k in res for k in CONTRACT) and res["value"] > 0 and res["ms_per_step"] > 0
    checks = res["tier_b"]["checks"]
    assert res["tier_b"]["certified"] == all(v for k, v in checks.items() if k != "tol") and "errors_within_3" in checks
    assert res["headline_tier"] == ("b" if res["tier_b"]["certified"] else "a") and res["tier_a"]["steps"] == 2
    full = json.load(open(detail))
    for k in ("roofline", "cpu_baseline", "parity_vs_cpu", "tier_b_tight", "ns", "c2", "channel_bank", "one_capture_at_a_time"):
        assert k not in full, k
    assert "pass_ms_all_launches" not in full["tier_b"]["stages"][0]


def test_dump_files_are_float_bounded_and_the_same_every_run(tmp_path):
    """`--dump-outputs`: what ResidentReceiver.fetch() returns at the C3 shape (2^22 symbols, two stages) becomes float32 / float64 files within
    64 MB; long arrays are kept at a seeded sample of positions that does not change from run to run."""
    import numpy as np
    bench = _bench()
    rng = np.random.default_rng(0)

    def c(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    n = 2 ** 22 - 20
    res = dict(wxy=c(2, 2, 41), err=(c(2, n - 20), c(2, n - 20)), eq=c(2, n), mu=(np.float32(2e-4), np.float32(2e-4)), out=c(2, n),
               ph=rng.standard_normal((2, n)).astype(np.float32), idx=rng.integers(0, 64, (2, n)).astype(np.int32))
    files = bench.dump_files(res)
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert files["wxy"].shape == (2, 2, 41, 2) and np.array_equal(files["wxy"][..., 1], res["wxy"].imag)
    assert files["mu"].shape == (2,) and set(files) >= {"err1", "err2", "eq", "out", "ph", "idx"}
    pos = files["out_sample_index"].astype(np.int64)
    assert np.all(np.diff(pos) > 0) and pos[-1] < n
    assert np.array_equal(files["out"][..., 0], res["out"][:, pos].real) and np.array_equal(files["idx"], res["idx"][:, pos].astype(np.float64))
    again = bench.dump_files(res)
    assert sorted(again) == sorted(files) and all(np.array_equal(again[k], files[k]) for k in files)
    bench.write_dump(files, str(tmp_path / "d"))
    assert np.array_equal(np.load(str(tmp_path / "d" / "eq.npy")), files["eq"])
