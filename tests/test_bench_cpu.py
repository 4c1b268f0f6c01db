"""CPU: bench.py's launch contract (the driver runs `python bench.py --gpus N`): without a launcher in the environment the
script starts one rank per GPU as CHILD processes before anything touches the GPU, relays rank 0's JSON line -- and only
that -- to stdout, and passes the children's failure on."""
import importlib.util
import io
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if getattr(mod, "_BLAS_LIMIT", None) is not None:  # (bench.py limits the BLAS pool of ITS process at import: not of this one)
        mod._BLAS_LIMIT.restore_original_limits()
    return mod


def test_self_launch_relays_exactly_one_json_line(monkeypatch, capsys):
    bench = _bench()
    line = json.dumps({"metric": "emulated signals/sec (batched predict)", "value": 1.0, "n_gpus": 2})
    noise = "[Gloo] Rank 0 is connected to 1 peer ranks.\n{\"not\": \"the line\"}\nsome banner\n"
    seen = {}

    def fake_run(cmd, stdout=None, env=None, timeout=None):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=0, stdout=(noise + line + "\n").encode())
    monkeypatch.setattr(subprocess, "run", fake_run)
    with pytest.raises(SystemExit) as e:
        bench._self_launch(2, ["--gpus", "2", "--steps", "5"])
    assert e.value.code == 0
    out, err = capsys.readouterr()
    assert out.strip() == line and "Gloo" in err and "the line" in err          # stdout: the line alone; chatter: stderr
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "2"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "2", "--steps", "5"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"

    # a child that fails, or prints no line, fails the run
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: types.SimpleNamespace(returncode=3, stdout=(line + "\n").encode()))
    with pytest.raises(SystemExit) as e:
        bench._self_launch(2, [])
    assert e.value.code == 3
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: types.SimpleNamespace(returncode=0, stdout=b"no json here\n"))
    with pytest.raises(SystemExit) as e:
        bench._self_launch(2, [])
    assert e.value.code == 4


def test_main_self_launches_when_no_launcher_is_in_the_environment(monkeypatch):
    bench = _bench()
    called = {}
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])

    def fake_launch(n, argv):
        called["n"], called["argv"] = n, list(argv)
        raise SystemExit(0)
    monkeypatch.setattr(bench, "_self_launch", fake_launch)
    with pytest.raises(SystemExit):
        bench.main()
    assert called == {"n": 4, "argv": ["--gpus", "4", "--steps", "3"]}


def test_dump_outputs_writes_the_same_bounded_sample_every_run(tmp_path):
    """--dump-outputs: the timed step's output as float32 .npy (a seeded row sample when it is larger than DUMP_ROWS, with the
    row numbers beside it), the same rows on every run, at most 64 MB in all."""
    bench = _bench()
    y = np.random.default_rng(5).normal(size=(bench.BATCH, bench.DIMS[-1])).astype(np.float32)
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), y)
    bench.dump_outputs(str(b), y)
    files = sorted(os.listdir(a))
    assert files == ["signal_rows.npy", "signals.npy"] and info["signals"] == [bench.DUMP_ROWS, bench.DIMS[-1]]
    assert sum(os.path.getsize(a / f) for f in files) <= 64 << 20
    s, rows = np.load(a / "signals.npy"), np.load(a / "signal_rows.npy")
    assert s.dtype == np.float32 and rows.dtype == np.float64 and s.shape == (bench.DUMP_ROWS, bench.DIMS[-1])
    assert np.all(np.diff(rows) > 0) and rows[-1] < len(y)
    np.testing.assert_array_equal(s, y[rows.astype(np.int64)])
    for f in files:
        np.testing.assert_array_equal(np.load(a / f), np.load(b / f))
    # an output that fits is written whole
    small = y[:100]
    bench.dump_outputs(str(tmp_path / "c"), small)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "signals.npy"), small)


def test_steps_must_be_positive(monkeypatch):
    bench = _bench()
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


class _FakeNative:
    """Stands in for 21cmvae_amd._native inside bench.main(): no GPU, every launch recorded in order."""
    FWD_IN_TRANSFORM, FWD_OUT_TRANSFORM = 1, 2

    def __init__(self):
        self.launches = []
        fake = self

        class Context:
            def __init__(self, device=0):
                self.next = 1 << 20

            def malloc(self, nbytes):
                self.next += nbytes + 256
                return self.next - nbytes - 256

            def d2h(self, arr, dptr):
                arr[...] = 0

            def event(self):
                return object()

            def elapsed_ms(self, a, b):
                return 0.05

            h2d = memset = lambda self, *a: None
            sync = free = record = lambda self, *a: None

        class Stack:
            def __init__(self, ctx, dims, act):
                pass

            set_weights = set_input_transform = set_output_transform = lambda self, *a: None

            def forward_dev(self, d_x, ldx, n, d_y, ldy, prec, flags):
                fake.launches.append(("forward", prec, n))

            def forward_clocked(self, d_x, ldx, n, d_y, ldy, d_st, prec, flags):
                fake.launches.append(("clocked", prec, n))

        self.Context, self.Stack = Context, Stack


def _run_main(monkeypatch, argv):
    bench = _bench()
    native = _FakeNative()
    monkeypatch.setitem(sys.modules, "21cmvae_amd._native", native)
    monkeypatch.setitem(sys.modules, "torch", None)          # single rank: no process group, no torch device sync
    monkeypatch.setenv("WORLD_SIZE", "1")
    for k in ("RANK", "LOCAL_RANK", "V21_BENCH_REHEARSAL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(bench, "_reduce_clock_stamps", lambda st, ms: {"stamped_launches": int(st.shape[0])})
    line = io.StringIO()
    monkeypatch.setattr(bench, "_claim_stdout", lambda: line)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    return json.loads(line.getvalue()), native.launches


AUXILIARY_KEYS = ("other_precisions_1gpu", "predict_two_streams", "predict_generic_S1", "predict_table_driven_S1", "predict_jit_S1",
                  "predict_custom", "predict_hidden_352", "host_roundtrip_signals_per_s", "sweep", "sweep_scaling", "sweep_f32",
                  "train", "dp_compute_only", "train_custom_b16384", "train_ref_batch256_f32", "train_b16384", "train_b32768",
                  "train_variational", "fit_reference_recipe", "fit_n30000", "accuracy_on_trained_stack",
                  "class_surface_predict", "single_call_latency", "cpu_baseline")


def test_plain_run_launches_only_the_warm_up_and_timed_steps(monkeypatch, tmp_path):
    """Without --full the run is set-up, W warm-up and K timed launches of the headline kernel, the dump and the line: no
    repeat of the K launches, no other precision, route or leg."""
    out, launches = _run_main(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3", "--settle", "0", "--batch", "300",
                                            "--dump-outputs", str(tmp_path / "d")])
    assert launches == [("forward", "f16", 300)] * (3 + 7)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["metric"] == "emulated signals/sec (batched predict)" and out["unit"] == "signals/s" and out["higher_is_better"] is True
    assert out["steps"] == 7 and out["warmup"] == 3 and out["full"] is False
    assert not [k for k in AUXILIARY_KEYS if k in out]
    assert out["roofline"]["kernel_ms_median"] is None and out["roofline"]["clock_in_kernel"] is None
    assert np.load(tmp_path / "d" / "signals.npy").shape == (300, 451)


def test_full_run_repeats_the_timed_launches(monkeypatch):
    """--full (here without the legs) adds the per-launch-event repeat of the K launches and the clock-stamped one (settle,
    W warm-up, K stamped) after the timed steps, which stay first and unchanged."""
    out, launches = _run_main(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3", "--settle", "0", "--batch", "300",
                                            "--full", "--no-extras", "--no-train", "--no-cpu-baseline"])
    assert launches == [("forward", "f16", 300)] * (3 + 7 + 7) + [("clocked", "f16", 300)] * (3 + 7)
    assert out["full"] is True and out["roofline"]["kernel_ms_median"] == 0.05
    assert out["roofline"]["clock_in_kernel"] == {"stamped_launches": 7}
