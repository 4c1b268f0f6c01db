#!/usr/bin/env python
"""bench.py -- headline benchmark of the 21cmVAE hot path on MI355X.

Metric (BASELINE.json): emulated signals/sec of batched predict, 1/2/4/8 GPU
(+ train steps/sec as an auxiliary object).  Workload (configs[1]): the direct emulator
7 -> [352,352,352,224] -> 451, one batch of 65,536 seven-parameter vectors per GPU,
inputs resident in HBM, full DirectEmulator.predict arithmetic on the device
(par_transform prologue, five dense layers, unpreproc epilogue), output 65,536 x 451
float32 written to HBM.  One "step" = one such pass.  Weak scaling: every rank runs its
own batch (rows are independent; no data-path collective).

  python bench.py --gpus N --steps K --warmup W [--full]
  A plain run sets up, settles the clock, runs the W warm-up and K timed steps, writes --dump-outputs and prints the line.
  --full adds everything else: the per-launch and clock-stamped repeats of the K launches (roofline min / median / clock),
  the other precisions and forward routes, the training / sweep / fit legs, accuracy, class surface, latency and the CPU
  baseline (--no-extras, --no-train and --no-cpu-baseline then leave parts of that out).
  N > 1:  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
          (or plain `python bench.py --gpus N`: without WORLD_SIZE in the environment the script starts that
          launcher itself as a CHILD process, before anything here touches the GPU, and relays rank 0's line)

Prints ONE JSON line on rank 0 -- and nothing else on stdout: file descriptor 1 is pointed at stderr for the
whole run (banners of gloo / c10d / the HIP runtime land there), the line goes out through a saved duplicate.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

# numpy's BLAS pool (one spinning thread per host core after every matmul of the data
# set-up) competes with the thread that enqueues kernels: the GPU legs run with the pool limited
# to one thread; cpu_baseline (run last) lifts the limit.
try:
    from threadpoolctl import threadpool_limits
    _BLAS_LIMIT = threadpool_limits(limits=1)
except Exception:
    _BLAS_LIMIT = None

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DIMS = [7, 352, 352, 352, 224, 451]
ACT = [1, 1, 1, 1, 0]
BATCH = 65536
FLOP_PER_SIGNAL = 2 * sum(a * b for a, b in zip(DIMS[:-1], DIMS[1:]))  # 860,288
BYTES_PER_SIGNAL = 4 * (DIMS[0] + DIMS[-1])                            # 1,832
PEAK_TFLOPS = {"f16": 2500.0, "bf16": 2500.0, "f32": 157.3}            # dense MFMA, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0
# --dump-outputs: rows of the timed step's output written out, at most (32,768 x 451 float32 = 59 MB)
DUMP_ROWS = 32768


def glorot(dims, seed):
    rng = np.random.default_rng(seed)
    flat = []
    for k, n in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (k + n))
        flat.append(rng.uniform(-lim, lim, size=(k, n)).astype(np.float32).ravel())
        flat.append(rng.normal(scale=0.05, size=n).astype(np.float32))
    return np.concatenate(flat)


def _pg_device(dist):
    """Where the tensors of the contract's max-over-ranks / sums live: this rank's GPU under nccl (= RCCL), the host
    under gloo.  The index is explicit: torch's current device is per thread, and the training leg runs in one."""
    return "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0")) if dist.get_backend() == "nccl" else "cpu"


def usable_cores():
    """Cores this process may really use: the scheduler affinity and the cgroup CPU quota, not the host's
    core count (a 16-core share of a 256-core host runs 256 BLAS / torch threads many times slower than 16)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except Exception:
            pass
    return n


def _timed_reps(fn, budget_s, min_reps=2):
    fn()  # warm-up
    t0, n = time.perf_counter(), 0
    while n < min_reps or time.perf_counter() - t0 < budget_s:
        fn()
        n += 1
    return n, time.perf_counter() - t0


def cpu_baseline(weights_flat, x_f32, budget_s=6.0):
    """CPU baselines of BASELINE.md section 3 on BOUNDED samples of the same workloads (about 30 s in all),
    timed on the GPU box's host cores.  `value` (the contract's figure) is row B2: the CPU oracle (numpy fp32
    restatement, oracle/ref_numpy.py) on 8,192 of the 65,536 rows per pass, every core.  `rows` adds: the same
    on ONE core, the Keras-like batch-of-32 predict loop the reference really runs (emulator.py:402 [K]), an
    independent torch-CPU implementation (B3), and optimizer steps of the autoencoder stack (numpy oracle and
    torch autograd with Keras' Adam restated) at the reference's batch 256 and at 4,096.  B1 (TensorFlow) is
    probed and reported absent: it is not installable here."""
    from oracle import ref_numpy as ora
    from threadpoolctl import threadpool_limits, threadpool_info
    if _BLAS_LIMIT is not None:
        _BLAS_LIMIT.restore_original_limits()  # the baseline gets every host core
    ncpu = usable_cores()
    threadpool_limits(limits=ncpu)  # (stays in force: numpy's BLAS pool = the cores this process may use)
    try:
        threads = min(ncpu, max([p.get("num_threads", 1) for p in threadpool_info()] or [1]))
    except Exception:
        threads = ncpu
    Ws, bs = ora.unflatten_params(weights_flat, DIMS)
    rows = 8192
    xs = x_f32[:rows]
    n, dt = _timed_reps(lambda: ora.mlp_forward(Ws, bs, xs, dtype=np.float32), budget_s)
    out = {"value": rows * n / dt, "unit": "signals/s", "cores": int(threads), "kind": "port",
           "sample": "%d passes over the first %d rows of the batch, numpy fp32 (BLAS sgemm), %.1f s" % (n, rows, dt),
           "host_cpu_count": os.cpu_count(), "usable_cores": ncpu}
    more = {}
    with threadpool_limits(limits=1):
        x1 = xs[:2048]
        n, dt = _timed_reps(lambda: ora.mlp_forward(Ws, bs, x1, dtype=np.float32), 2.5)
        more["predict_numpy_1core"] = {"signals_per_s": 2048 * n / dt, "cores": 1, "sample": "%d passes over 2,048 rows" % n}

    def keras_like(xb):  # Model.predict's default batch of 32 rows per call [K]
        for i in range(0, xb.shape[0], 32):
            ora.mlp_forward(Ws, bs, xb[i:i + 32], dtype=np.float32)
    x32 = xs[:2048]
    n, dt = _timed_reps(lambda: keras_like(x32), 2.5)
    more["predict_numpy_batch32_loop"] = {"signals_per_s": 2048 * n / dt, "cores": int(threads),
                                          "sample": "%d passes over 2,048 rows in calls of 32 rows (Keras predict's default)" % n}
    # autoencoder optimizer steps, numpy oracle (fp32)
    synth = importlib.import_module("21cmvae_amd.synth")
    sig = synth.make_signals(4096, seed=2000)
    yb = ora.preproc(sig, sig).astype(np.float32)
    wb = ora.relative_mse_row_weight(yb, sig).astype(np.float32)
    Wa, ba = ora.unflatten_params(glorot(AE_DIMS, seed=4), AE_DIMS)
    for B, budget in ((256, 2.0), (4096, 3.0)):
        sta = ora.AdamState(sum(W.size + b.size for W, b in zip(Wa, ba)), dtype=np.float32, lr=1e-3)
        state = {"W": [W.copy() for W in Wa], "b": [b.copy() for b in ba]}

        def step(B=B, state=state, sta=sta):
            state["W"], state["b"], _, _ = ora.train_step(state["W"], state["b"], sta, yb[:B], yb[:B], wb[:B], np.float32)
        n, dt = _timed_reps(step, budget)
        more["train_step_numpy_b%d" % B] = {"steps_per_s": n / dt, "samples_per_s": n * B / dt, "cores": int(threads),
                                           "sample": "%d optimizer steps of the autoencoder 451-352-9-32-352-451, relative-MSE, Keras Adam" % n}
    try:
        import torch
        act = [1, 1, 1, 1, 0]

        def tmodel(dims, flat, acts):
            Wl, bl = ora.unflatten_params(flat, dims)
            return [torch.tensor(W, requires_grad=True) for W in Wl], [torch.tensor(b, requires_grad=True) for b in bl], acts

        def tforward(Wt, bt, acts, x):
            h = x
            for W, b, a in zip(Wt, bt, acts):
                h = h @ W + b
                h = torch.relu(h) if a else h
            return h
        Wt, bt, _ = tmodel(DIMS, weights_flat, act)
        xt = torch.from_numpy(np.ascontiguousarray(xs))
        for nthr, key in ((ncpu, "predict_torch_allcores"), (1, "predict_torch_1core")):
            torch.set_num_threads(nthr)
            xx = xt if nthr > 1 else xt[:2048]
            with torch.no_grad():
                n, dt = _timed_reps(lambda: tforward(Wt, bt, act, xx), 2.0)
            more[key] = {"signals_per_s": xx.shape[0] * n / dt, "cores": nthr, "sample": "%d passes over %d rows, torch %s CPU" % (n, xx.shape[0], torch.__version__)}
        torch.set_num_threads(ncpu)
        Wt, bt, _ = tmodel(AE_DIMS, glorot(AE_DIMS, seed=4), AE_ACT)
        prm = Wt + bt
        ms = [torch.zeros_like(p) for p in prm]; vs = [torch.zeros_like(p) for p in prm]
        yt, wt = torch.from_numpy(yb), torch.from_numpy(wb)
        it = [0]

        def tstep(B):
            pred = tforward(Wt, bt, AE_ACT, yt[:B])
            loss = (wt[:B] * ((pred - yt[:B]) ** 2).sum(1)).mean()
            grads = torch.autograd.grad(loss, prm)
            it[0] += 1
            t = it[0]
            alpha = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
            with torch.no_grad():  # Keras Adam: epsilon outside the bias correction [K]
                for p, g, m, v in zip(prm, grads, ms, vs):
                    m += (g - m) * 0.1
                    v += (g * g - v) * 0.001
                    p -= alpha * m / (v.sqrt() + 1e-7)
        for B, budget in ((256, 2.0), (4096, 3.0)):
            n, dt = _timed_reps(lambda B=B: tstep(B), budget)
            more["train_step_torch_b%d" % B] = {"steps_per_s": n / dt, "samples_per_s": n * B / dt, "cores": ncpu,
                                               "sample": "%d optimizer steps, torch CPU autograd + restated Keras Adam" % n}
    except Exception as e:  # pragma: no cover
        more["torch"] = {"error": "%s: %s" % (type(e).__name__, e)}
    try:
        import tensorflow  # noqa: F401  (B1: the reference's own engine)
        more["tensorflow"] = "importable (not timed: the reference package itself needs its dataset)"
    except Exception:
        more["tensorflow"] = "absent on this box (BASELINE.md row B1 cannot be timed); upstream quotes 40 ms per predict() call (README.rst:11)"
    out["rows"] = more
    return out


PROFILE_TAG = "r5"  # profiles/<tag>/: the rocprofv3 summaries of this round (scripts/collect_profiles_r4.sh)


def _profile_is_current():
    """True when profiles/<tag>/BUILD_ID names the sources the running library was built from (scripts/build_id.py): the
    per-kernel durations and PMC bytes quoted from profiles/ beside a live timing are only shown as current then
    (stale profile numbers beside fresh timings)."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        from build_id import build_id
        return open(os.path.join(ROOT, "profiles", PROFILE_TAG, "BUILD_ID")).read().strip() == build_id()
    except Exception:
        return False


def _profile_kernels(name):
    """(kernel name, calls, average ns) rows of a committed `rocprofv3 --kernel-trace --stats` summary, or None."""
    path = os.path.join(ROOT, "profiles", PROFILE_TAG, name)
    if not os.path.exists(path):
        return None
    import csv
    rows = []
    for r in csv.DictReader(open(path)):
        try:
            rows.append((r["Name"], int(r["Calls"]), float(r["AverageNs"])))
        except Exception:
            pass
    return rows


def train_roofline(leg, flop_per_sample, params, din, dout, stats_csv, pmc_json):
    """`roofline` object of a training leg: algorithmic FLOP per step over the measured step time against
    the dense MFMA peak of the operand type; beside it the dominant kernels of the committed profile of the same
    step (profiles/<tag>/<stats_csv>: average launch durations) and the HBM-side bytes per step from the PMC passes
    (profiles/<tag>/<pmc_json>) against the algorithmic bytes of SURVEY 8d (batch rows in, 7 passes over the
    parameter arena for Adam, one read of the packed weights)."""
    B = leg["batch_per_gpu"]
    prec = leg["precision"]
    step_s = leg["ms_per_step"] * 1e-3
    flop = flop_per_sample * B
    alg_bytes = B * 4 * (din + (dout if dout != din else 0)) + 7 * 4 * params + (2 if prec != "f32" else 4) * params
    rf = {"bound": "mfma", "achieved": flop / step_s / 1e12, "peak": PEAK_TFLOPS[prec], "unit": "TFLOP/s",
          "frac": flop / step_s / 1e12 / PEAK_TFLOPS[prec], "algorithmic_flop_per_step": flop,
          "algorithmic_bytes_per_step": alg_bytes, "traffic": None,
          "time_base": "wall clock over the timed steps of this leg (whole step: every launch and the gaps between them)"}
    rf["profile_matches_build"] = _profile_is_current()
    rows = _profile_kernels(stats_csv)
    if rows:
        ks = [r for r in rows if "v21::" in r[0] and r[1] >= 10]
        ks.sort(key=lambda r: -r[1] * r[2])
        rf["kernels"] = [{"kernel": k[0][:90], "calls": k[1], "avg_us": k[2] / 1e3} for k in ks[:4]]
        if ks:
            rf["kernel"] = ks[0][0][:90]
            rf["kernel_ms"] = ks[0][2] / 1e6
        rf["kernel_source"] = "profiles/%s/%s (rocprofv3 --kernel-trace --stats of scripts/train_probe.py at this batch)%s" % (
            PROFILE_TAG, stats_csv, "" if rf["profile_matches_build"] else "; STALE: the library sources changed since that profile was collected")
    path = os.path.join(ROOT, "profiles", PROFILE_TAG, pmc_json)
    if os.path.exists(path):
        try:
            pm = json.load(open(path))
            tot = sum(v.get("hbm_bytes_per_launch", 0.0) for k, v in pm.items()
                      if isinstance(v, dict) and v.get("FETCH_SIZE", {}).get("dispatches", 0) >= 10)
            rf["traffic"] = tot
            rf["traffic_source"] = "profiles/%s/%s: sum over the step's kernels of 2*FETCH_SIZE*1024 + WRITE_SIZE*1024" % (PROFILE_TAG, pmc_json)
            # large steps are bound by these bytes, not by the matrix pipe (per-workgroup stamps on the constant clock, r4:
            # both fused training kernels and the weight-gradient kernel move ~4.2 TB/s): the step against the 8 TB/s peak
            rf["hbm_side_frac_of_8TBps"] = tot / step_s / 1e9 / PEAK_HBM_GBS
        except Exception:
            pass
    return rf


AE_DIMS = [451, 352, 9, 32, 352, 451]   # encoder 451->352->9, decoder 9->32->352->451 (emulator.py:522-524)
AE_ACT = [1, 0, 1, 1, 0]
AE_FLOP_PER_SAMPLE = 1675840             # 6 x 332,224 - 2 x 158,752


def train_leg(native, ctx, stack_cls, world, rank, dist, torch, barrier, sync_all, batch, precision, steps, warmup,
              variational=False):
    """Auxiliary metric: optimizer steps/s of the autoencoder stack (relative-MSE loss, Adam),
    per-GPU batch `batch`, gradients all-reduced over RCCL when world > 1."""
    synth = importlib.import_module("21cmvae_amd.synth")
    pp = importlib.import_module("21cmvae_amd.preprocess")
    losses = importlib.import_module("21cmvae_amd.losses")
    act = list(AE_ACT)
    if variational:  # the encoder's last layer becomes the (z_mean | z_log_var) head: sampled latent + KL
        act[1] = native.ACT_GAUSS
    st = native.Stack(ctx, AE_DIMS, act)
    if variational:
        rngv = np.random.default_rng(4)
        st.set_weights((rngv.normal(size=st.num_params) * 0.05).astype(np.float32))
    else:
        st.set_weights(glorot(AE_DIMS, seed=4))
    tr = native.Trainer(st, precision, batch)
    tr.set_adam(lr=1e-3)
    if variational:
        tr.set_vae(1e-3, sample=True, seed=11)
    sig = synth.make_signals(batch, seed=2000 + rank)
    y = pp.preproc(sig, sig)
    rw = losses.relative_mse_loss(sig)._v21_row_weight(y).astype(np.float32)
    # the batch as the trainer's RESIDENT training set (what Model.fit steps on: v21_trainer_set_data), stepped through its
    # device pointers: steps of the fused training kernels then gather the 16-bit copy of the rows (ChainStep::x16)
    tr.set_data(0, y, None, rw)
    d_x, _, d_rw, _ = tr.data_dev(0)
    for _ in range(warmup):
        tr.step_dev(d_x, None, d_rw, batch, batch * world)
    sync_all(); barrier(); sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step_dev(d_x, None, d_rw, batch, batch * world)
    sync_all(); barrier(); sync_all()
    wall = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([wall], dtype=torch.float64, device=_pg_device(dist))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
    loss = tr.last_step_loss() / (batch * world)
    sps = steps / wall
    # r5: where the step's time goes -- an UNTIMED repeat of min(steps, 100) steps with HIP-event stamps
    # around the phases (include/v21.h: v21_trainer_phase_timing); every rank takes part (the steps are collective)
    phases = None
    try:
        phases = tr.phase_profile(lambda: tr.step_dev(d_x, None, d_rw, batch, batch * world), steps=min(steps, 50))
        sync_all()
        phases["marker_us"] = phases["stamped_step_us"] - 1e6 / sps
    except Exception as e:  # pragma: no cover
        phases = {"error": "%s: %s" % (type(e).__name__, e)}
    return {"steps_per_s": sps, "phases": phases, "samples_per_s": sps * batch * world, "ms_per_step": 1e3 / sps,
            "batch_per_gpu": batch, "global_batch": batch * world, "precision": precision,
            "model": ("variational " if variational else "") + "autoencoder 451-352-9-32-352-451, relative-MSE" +
                     (" + 1e-3 KL" if variational else "") + ", Adam", "steps": steps,
            "achieved_TFLOPs": sps * batch * world * AE_FLOP_PER_SAMPLE / 1e12, "final_batch_loss": loss,
            "collective": "all-reduce of the flat gradient arena (%d floats)" % (st.num_params + 1) if world > 1 else "none"}


def custom_train_leg(native, ctx, precision, batch=16384, steps=60):
    """r5: a stack WITHOUT a compiled fused training kernel -- the sample notebook's 7 -> [64, 128] -> 451
    -- at 16,384 rows per step: the fused training kernel instantiated at run time (csrc/jit.hip: fused_train16<ArchRT, Prec>,
    prebuilt by build(), else compiled in a child process while the chain kernel serves) against the chain route."""
    synth = importlib.import_module("21cmvae_amd.synth")
    pp = importlib.import_module("21cmvae_amd.preprocess")
    losses = importlib.import_module("21cmvae_amd.losses")
    dims, act = [7, 64, 128, 451], [1, 1, 0]
    sig = synth.make_signals(batch, seed=91)
    y = pp.preproc(sig, sig)
    rw = losses.relative_mse_loss(sig)._v21_row_weight(y).astype(np.float32)
    x = np.random.default_rng(5).uniform(-1, 1, size=(batch, 7)).astype(np.float32)
    out = {"stack": "7-64-128-451", "batch": batch, "precision": precision}
    for name in ("fused_run_time_kernel", "chain"):
        if name == "chain":
            os.environ["V21_FUSED_TRAIN"] = "0"
        try:
            st = native.Stack(ctx, dims, act)
            st.set_weights(glorot(dims, seed=9))
            tr = native.Trainer(st, precision, batch)
            tr.set_adam(lr=1e-3)
            if name != "chain":
                out["kernel_status"] = tr.jit(-1)
            tr.set_data(0, x, y, rw)
            d_x, d_y, d_rw, _ = tr.data_dev(0)
            for _ in range(5):
                tr.step_dev(d_x, d_y, d_rw, batch, batch)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step_dev(d_x, d_y, d_rw, batch, batch)
            ctx.sync()
            out[name] = {"us_per_step": 1e6 * (time.perf_counter() - t0) / steps, "route": list(tr.last_route()[0]),
                         "loss": tr.last_step_loss() / batch}
        except Exception as e:  # pragma: no cover
            out[name] = {"error": "%s: %s" % (type(e).__name__, e)}
        finally:
            os.environ.pop("V21_FUSED_TRAIN", None)
    if "us_per_step" in out.get("chain", {}) and "us_per_step" in out.get("fused_run_time_kernel", {}):
        out["speedup_vs_chain"] = out["chain"]["us_per_step"] / out["fused_run_time_kernel"]["us_per_step"]
    return out


SWEEP_CONFIGS = [  # (latent, encoder hidden, decoder hidden): widths multiples of 32 in [32, 512] (SURVEY 8d cfg 5)
    (4, 128, (32, 128)), (8, 256, (32, 256)), (9, 352, (32, 352)), (12, 384, (64, 384)),
    (16, 448, (64, 448)), (20, 512, (96, 512)), (24, 320, (128, 320)), (32, 480, (160, 480))]


def sweep_leg(native, ctx, precision, batch=256, steps_per_epoch=48, epochs=3):
    """Auxiliary metric (BASELINE configs[4]): 8 autoencoder configs per GPU trained in lock
    step with grouped launches, against the same 8 trained one after the other.  No
    collective: ranks hold independent models."""
    synth = importlib.import_module("21cmvae_amd.synth")
    pp = importlib.import_module("21cmvae_amd.preprocess")
    losses = importlib.import_module("21cmvae_amd.losses")
    n = batch * steps_per_epoch
    sig = synth.make_signals(n, seed=77)
    y = pp.preproc(sig, sig)
    rw = losses.relative_mse_loss(sig)._v21_row_weight(y).astype(np.float32)

    def make():
        trs = []
        for i, (lat, he, hd) in enumerate(SWEEP_CONFIGS):
            dims = [451, he, lat, hd[0], hd[1], 451]
            st = native.Stack(ctx, dims, AE_ACT)
            st.set_weights(glorot(dims, seed=50 + i))
            tr = native.Trainer(st, precision, batch)
            tr.set_adam(lr=1e-3)
            trs.append(tr)
        return trs
    grouped = make()
    grouped[0].set_data(0, y, None, rw)
    sw = native.Sweep(grouped)
    sw.run_epoch(None, batch)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(epochs):
        lg = sw.run_epoch(None, batch)
    ctx.sync()
    tg = time.perf_counter() - t0
    solo = make()
    for tr in solo:
        tr.set_data(0, y, None, rw)
        tr.run_epoch(None, batch)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(epochs):
        ls = [tr.run_epoch(None, batch) for tr in solo]
    ctx.sync()
    ts = time.perf_counter() - t0
    G, nsteps = len(SWEEP_CONFIGS), epochs * steps_per_epoch
    return {"models_per_gpu": G, "batch": batch, "precision": precision,
            "model_steps_per_s_grouped": G * nsteps / tg, "model_steps_per_s_one_by_one": G * nsteps / ts,
            "speedup": ts / tg, "ms_per_group_step": 1e3 * tg / nsteps,
            "max_rel_loss_diff_vs_one_by_one": float(max(abs(a - b) / b for a, b in zip(lg, ls))),
            "configs": "latent/enc/dec widths " + " ".join("%d/%d/%d-%d" % (c[0], c[1], c[2][0], c[2][1]) for c in SWEEP_CONFIGS)}


def sweep_configs(count):
    """`count` autoencoder configs of SURVEY 8d cfg 5 (latent in 4 .. 32, hidden widths multiples of 32 in [32, 512]): the
    eight of SWEEP_CONFIGS first, the rest drawn with a fixed seed."""
    cfgs = list(SWEEP_CONFIGS)
    rng = np.random.default_rng(64)
    while len(cfgs) < count:
        he = int(rng.integers(1, 17)) * 32
        cfgs.append((int(rng.integers(4, 33)), he, (int(rng.integers(1, 6)) * 32, he)))
    return cfgs[:count]


def sweep_scaling_leg(native, ctx, precision, counts=(8, 16, 32, 64), batch=256, steps_per_epoch=24, epochs=2):
    """BASELINE configs[4] on ONE GPU: 8 / 16 / 32 / 64 autoencoder configs in ONE group (64 = the whole
    config), model-steps/s and a roofline object per group size: algorithmic FLOP of the member stacks (per member and row
    6 x MAC - 2 x (first layer's dX)) over the measured group-step time against the dense MFMA peak of the operand
    type; the dominant kernels and HBM-side bytes from profiles/<tag>/kernel_stats_sweep_<precision>_m<count>.csv /
    pmc_sweep_<precision>_m<count>.json when they were collected."""
    synth = importlib.import_module("21cmvae_amd.synth")
    pp = importlib.import_module("21cmvae_amd.preprocess")
    losses = importlib.import_module("21cmvae_amd.losses")
    n = batch * steps_per_epoch
    sig = synth.make_signals(n, seed=77)
    y = pp.preproc(sig, sig)
    rw = losses.relative_mse_loss(sig)._v21_row_weight(y).astype(np.float32)
    out = {"batch": batch, "precision": precision, "groups": []}
    for G in counts:
        cfgs = sweep_configs(G)
        trs, flop, params = [], 0, 0
        for i, (lat, he, hd) in enumerate(cfgs):
            dims = [451, he, lat, hd[0], hd[1], 451]
            st = native.Stack(ctx, dims, AE_ACT)
            st.set_weights(glorot(dims, seed=50 + i))
            tr = native.Trainer(st, precision, batch)
            tr.set_adam(lr=1e-3)
            trs.append(tr)
            mac = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
            flop += (6 * mac - 2 * dims[0] * dims[1]) * batch
            params += st.num_params
        trs[0].set_data(0, y, None, rw)
        sw = native.Sweep(trs)
        sw.run_epoch(None, batch)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(epochs):
            lg = sw.run_epoch(None, batch)
        ctx.sync()
        tg = time.perf_counter() - t0
        nsteps = epochs * steps_per_epoch
        step_s = tg / nsteps
        leg = {"batch_per_gpu": batch, "precision": precision, "ms_per_step": step_s * 1e3}
        rf = train_roofline(leg, flop / batch, params, 451, 451, "kernel_stats_sweep_%s_m%d.csv" % (precision, G),
                            "pmc_sweep_%s_m%d.json" % (precision, G))
        # (the batch rows are read once per MEMBER by its row blocks: algorithmic bytes count them per member)
        rf["algorithmic_bytes_per_step"] = G * batch * 4 * 451 + 7 * 4 * params + (2 if precision != "f32" else 4) * params
        # A group step at batch 256 is bound by the OPTIMIZER STATE, not by the matrix pipe: 28-32 B of HBM-side traffic per
        # parameter and step (Adam's w, g, m, v passes + the packed copies) against 2 x 3 x 256 FLOP -- the roofline that
        # applies is HBM (profiles/r5/pmc_sweep_*: dw16_adam_group_kernel moves its bytes at 3.7 TB/s); the MFMA fraction rides along
        rf["mfma_frac"] = rf["frac"]
        rf["bound"], rf["unit"], rf["peak"] = "hbm", "GB/s", PEAK_HBM_GBS
        rf["achieved"] = rf["algorithmic_bytes_per_step"] / step_s / 1e9
        rf["frac"] = rf["achieved"] / PEAK_HBM_GBS
        if rf.get("traffic"):
            rf["hbm_side_GBps"] = rf["traffic"] / step_s / 1e9
        out["groups"].append({"models": G, "model_steps_per_s": G * nsteps / tg, "ms_per_group_step": step_s * 1e3,
                              "parameters_of_the_group": params, "finite": bool(np.isfinite(lg).all()), "roofline": rf})
        del sw, trs
    base = out["groups"][0]["model_steps_per_s"]
    for g in out["groups"]:
        g["vs_8_models"] = g["model_steps_per_s"] / base
    return out


def accuracy_leg(native, ctx):
    """Accuracy of the reduced-precision modes on the reference's TRAINED stack (the packaged conversion of
    its shipped autoencoder-path weights: emulator 7->352->352->352->224->9 + decoder 9->32->352->451), as
    the reference's own metric (emulator.py:188-191: rms over bins / max|signal|, in %) between the device
    output and a float64 evaluation of the same weights, and the implied ratio to the published 0.34 %
    test error if the two errors are independent (bar: <= 1.05)."""
    base = os.path.join(ROOT, "21cmvae_amd", "models", "autoencoder_based_emulator")
    Ws, bs, act = [], [], []
    for stem in ("ae_emulator", "decoder"):
        d = np.load(os.path.join(base, stem + ".npz"))
        n = int(d["n_layers"])
        for i in range(n):
            Ws.append(d["W%d" % i]); bs.append(d["b%d" % i]); act.append(1 if str(d["act%d" % i]) == "relu" else 0)
    dims = [Ws[0].shape[0]] + [W.shape[1] for W in Ws]
    st = native.Stack(ctx, dims, act)
    st.set_weights(np.concatenate([a.ravel() for W, b in zip(Ws, bs) for a in (W, b)]).astype(np.float32))
    x = np.random.default_rng(0).uniform(-1, 1, size=(4096, dims[0]))
    h = x
    for W, b, a in zip(Ws, bs, act):  # float64 evaluation of the same weights (a checker, not a product path)
        h = h @ W.astype(np.float64) + b.astype(np.float64)
        h = np.maximum(h, 0) if a else h
    out = {}
    for prec in ("f32", "f16", "bf16"):
        y = st.forward(x, prec, flags=native.FWD_NO_SMALL).astype(np.float64)
        e = 100.0 * np.sqrt(np.mean((y - h) ** 2, axis=1)) / np.max(np.abs(h), axis=1)
        out[prec] = {"added_error_percent_mean": float(e.mean()), "added_error_percent_max": float(e.max()),
                     "implied_ratio_to_0.34": float(np.sqrt(0.34 ** 2 + e.mean() ** 2) / 0.34)}
    out["note"] = "pre-processed units; 4096 random parameter vectors in the training box; bar 1.05"
    return out


def class_surface_leg():
    """What a user of the reference's API gets: ``DirectEmulator.predict(params)`` -- numpy in, numpy
    out, both transforms, PCIe both ways, the Python layer -- at configs[1]'s 65,536 rows and at configs[0]'s 1,000 rows,
    for float64 parameters (numpy's default; transformed in float64 on the device) and float32 ones (the reference's
    float32 branch inside the kernel prologue).  Training set of the reference's size.  The PCIe bound for 65,536 rows
    is ~34 M signals/s (118 MB of float32 results at ~63 GB/s)."""
    synth = importlib.import_module("21cmvae_amd.synth")
    emu = importlib.import_module("21cmvae_amd.emulator")
    data = synth.make_dataset(synth.N_TRAIN, 400, 400)
    res = {}
    for prec in ("f16", "f32"):
        em = emu.DirectEmulator(hidden_dims=DIMS[1:-1], precision=prec, **data)
        for rows, reps in ((BATCH, 10), (1000, 200)):
            for dt in (np.float64, np.float32):
                par = synth.make_params(rows, seed=77).astype(dt)
                for _ in range(3):
                    y = em.predict(par)
                t0 = time.perf_counter()
                for _ in range(reps):
                    y = em.predict(par)
                dtm = (time.perf_counter() - t0) / reps
                assert y.shape == (rows, DIMS[-1])
                res["%s_rows%d_params_%s" % (prec, rows, np.dtype(dt).name)] = {"signals_per_s": rows / dtm, "ms_per_call": dtm * 1e3}
                del y
    res["note"] = ("DirectEmulator.predict on host arrays, 7->[352,352,352,224]->451; results of 65,536 rows land in pooled "
                   "page-locked memory; r3 transformed the parameters with numpy on the host (4.3 ms per 65,536 rows)")
    return res


def latency_leg():
    """Auxiliary metric: what a sampler sees -- DirectEmulator.predict() on ONE parameter vector through
    the class surface (numpy in, numpy out; transforms, PCIe both ways, synchronisation included), with a
    training set of the reference's size (24,562 rows).  The reference quotes 40 ms per call (README.rst:11) and
    recomputes the training-set statistics on every call.  `f32_default` / `f16_default`: the constructor's default
    (r5: `freeze_data="auto"` -- the caller's own arrays with their writeable flag off, statistics cached on identity, no checksum;
    r4: private read-only copies);
    `f32_freeze_data_false_rehash`: the reference's by-reference arrays, re-hashed on every call (r3's default, then
    called `f32_default_rehash`).  An emulator built without explicit data -- the reference's default use -- takes
    read-only arrays from the data set file (`f32_no_argument_constructor`: a synthetic dataset_21cmVAE.h5 of the
    reference's size, written to a temporary directory)."""
    synth = importlib.import_module("21cmvae_amd.synth")
    emu = importlib.import_module("21cmvae_amd.emulator")
    data = synth.make_dataset(synth.N_TRAIN, 400, 400)
    res = {}
    for key, prec, freeze, reps in (("f32_default", "f32", "auto", 200), ("f16_default", "f16", "auto", 200),
                                    ("f32_freeze_data_false_rehash", "f32", False, 10)):
        if freeze is False:   # (the default locked the caller's arrays above: the reference's semantics need them writable)
            for k in ("par_train", "signal_train"):
                data[k].setflags(write=True)
        em = emu.DirectEmulator(hidden_dims=DIMS[1:-1], precision=prec, freeze_data=freeze, **data)
        p1 = data["par_test"][0]
        for _ in range(5):
            em.predict(p1)
        lat = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(reps):
                em.predict(p1)
            lat.append((time.perf_counter() - t0) / reps * 1e6)
        res[key] = {"us_per_call_median": float(np.median(lat)), "us_per_call_min": float(min(lat))}
    import tempfile
    saved = emu._dataset
    try:
        with tempfile.TemporaryDirectory() as td:
            emu.load_dataset(synth.save_dataset(os.path.join(td, "dataset_21cmVAE.h5"), data))
            em = emu.DirectEmulator(hidden_dims=DIMS[1:-1])
            p1 = data["par_test"][0]
            for _ in range(5):
                em.predict(p1)
            lat = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(200):
                    em.predict(p1)
                lat.append((time.perf_counter() - t0) / 200 * 1e6)
            res["f32_no_argument_constructor"] = {"us_per_call_median": float(np.median(lat)), "us_per_call_min": float(min(lat))}
    finally:
        emu._dataset = saved
    res["note"] = "f32 (default precision): small-batch path, one launch per layer; f16: fused one-launch kernel"
    return res


def fit_leg(precision, epochs=30, n_train=None, joint=False):
    """Auxiliary metric (BASELINE configs[2]): the reference's whole training recipe through the class
    surface -- AutoEncoderEmulator.train(): autoencoder fit x -> x, encode, latent emulator fit, each
    with a validation pass per epoch -- on a synthetic data set of the reference's size (24,562 / 2,730
    rows, batch 256; n_train = 30,000 honours configs[2] literally).  joint=True: both models step on the
    same rows of every batch (v21_joint_*).  Wall clock of the call, Python and callbacks included -- also the ~40 ms a
    train() call spends once on the row weights and the pre-processing of the data set (scripts/fit_pyprofile.py)."""
    synth = importlib.import_module("21cmvae_amd.synth")
    emu = importlib.import_module("21cmvae_amd.emulator")
    optm = importlib.import_module("21cmvae_amd.optimizers")
    data = synth.make_dataset(n_train) if n_train else synth.make_dataset()
    importlib.import_module("21cmvae_amd.engine").set_random_seed(1234)  # same initial weights and shuffles in every leg and run
    ae = emu.AutoEncoderEmulator(precision=precision, **data)
    ae.autoencoder.compile(optimizer=optm.Adam(1e-3), loss=emu.relative_mse_loss(ae.signal_train))
    ae.emulator.compile(optimizer=optm.Adam(1e-3), loss=emu.mean_squared_error)
    ae.train(epochs=1, verbose=0, joint=joint)  # allocations, data upload
    t0 = time.perf_counter()
    out = ae.train(epochs=epochs, verbose=0, joint=joint)
    dt = time.perf_counter() - t0
    steps = 2 * epochs * -(-data["par_train"].shape[0] // 256)
    err = ae.test_error()
    return {"precision": precision, "epochs": epochs, "rows": int(data["par_train"].shape[0]), "batch": 256,
            "mode": "joint (enc+dec+emulator step per batch)" if joint else "sequential two-phase (emulator.py:739-764)",
            "optimizer_steps_per_s": steps / dt, "s_per_epoch_both_models": dt / epochs,
            "final_ae_loss": out[0][-1], "final_emulator_loss": out[2][-1],
            "test_error_percent_mean_after_%d_epochs" % (epochs + 1): float(np.mean(err))}


def _self_launch(n, argv):
    """`python bench.py --gpus N` without a launcher: start `python -m torch.distributed.run` (one rank per GPU) as a
    child process -- this process has imported numpy only, no HIP call has been made -- relay rank 0's JSON line to
    stdout and everything else to stderr, and leave with the child's exit status (non-zero if no line came)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "1")
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, env=env,
                           timeout=float(os.environ.get("V21_BENCH_LAUNCH_TIMEOUT", "1500")))
        rc, raw = p.returncode, p.stdout
    except subprocess.TimeoutExpired as e:
        rc, raw = 124, e.stdout or b""
    line = None
    for ln in raw.decode(errors="replace").splitlines():
        t = ln.strip()
        if t.startswith("{") and t.endswith("}"):
            try:
                if "metric" in json.loads(t):
                    line = t
                    continue
            except ValueError:
                pass
        if t:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line, flush=True)
    elif rc == 0:
        rc = 4
        print("bench.py: the %d-rank child run printed no JSON line" % n, file=sys.stderr)
    sys.exit(rc)


def _reduce_clock_stamps(st, ms_per_launch_events):
    """st[launch, workgroup] = (cycles at start, 100-MHz ticks at start, cycles at end, ticks at end, XCD): include/v21.h
    v21_debug_forward_clocked.  -> the clock as the working CUs saw it, per XCD, and the kernel's length in CYCLES -- if
    the shader clock bounds the kernel, cycles per workgroup stay put from run to run while microseconds move with the clock."""
    dc = (st[..., 2] - st[..., 0]).astype(np.float64)
    dt = (st[..., 3] - st[..., 1]).astype(np.float64)          # ticks of 10 ns
    ok = (dt > 0) & (dc > 0)
    ghz = np.where(ok, dc / np.maximum(dt, 1) * 0.1, np.nan)
    xcd = (st[..., 4] & np.uint64(0xF)).astype(np.int64)   # (bits 8-39: HW_REG_HW_ID of the workgroup's wave 0)
    per_xcd = []
    for x in range(8):
        m = ok & (xcd == x)
        per_xcd.append({"xcd": x, "workgroups_per_launch": float(m.sum() / st.shape[0]),
                        "ghz": float(dc[m].sum() / dt[m].sum() * 0.1) if m.any() else None})
    span_ticks = (st[..., 3].max(axis=1) - st[..., 1].min(axis=1)).astype(np.float64)   # per launch: first start to last end
    per_launch_ghz = (dc * ok).sum(axis=1) / np.maximum((dt * ok).sum(axis=1), 1) * 0.1
    return {
        "ghz_mean": float(dc[ok].sum() / dt[ok].sum() * 0.1), "ghz_min_workgroup": float(np.nanmin(ghz)), "ghz_max_workgroup": float(np.nanmax(ghz)),
        "ghz_per_launch_min": float(per_launch_ghz.min()), "ghz_per_launch_max": float(per_launch_ghz.max()),
        "per_xcd": per_xcd,
        "kcycles_per_workgroup": {"mean": float(dc[ok].mean() / 1e3), "min": float(dc[ok].min() / 1e3), "max": float(dc[ok].max() / 1e3)},
        "us_per_workgroup_mean": float(dt[ok].mean() * 0.01),
        "launch_us_first_start_to_last_end": {"mean": float(span_ticks.mean() * 0.01), "min": float(span_ticks.min() * 0.01), "max": float(span_ticks.max() * 0.01)},
        "kcycles_per_launch": float(span_ticks.mean() * 0.01 * (dc[ok].sum() / dt[ok].sum() * 0.1)),
        "ms_per_launch_hip_events_of_the_stamped_run": float(ms_per_launch_events),
        "launches": int(st.shape[0]), "workgroups": int(st.shape[1]),
        "source": "wave 0 of every workgroup of every timed-count launch: s_memtime / s_memrealtime / HW_REG_XCC_ID at start and end "
                  "(fused_fwd<ArchS1, Prec..x2spClk>, an untimed repeat of settle + warm-up + K launches)",
    }


def dump_outputs(directory, y):
    """The emulated signals of the timed path's last step (B x 451 float32, as predict returns them) as
    DIR/signals.npy: every row if they fit in DUMP_ROWS, else the same seeded sample of DUMP_ROWS rows every run, in
    row order (DIR/signal_rows.npy: their row numbers, float64)."""
    os.makedirs(directory, exist_ok=True)
    rows = np.arange(len(y))
    if len(y) > DUMP_ROWS:
        rows = np.sort(np.random.default_rng(0).choice(len(y), DUMP_ROWS, replace=False))
    np.save(os.path.join(directory, "signals.npy"), np.ascontiguousarray(y[rows], np.float32))
    np.save(os.path.join(directory, "signal_rows.npy"), rows.astype(np.float64))
    return {"dir": directory, "signals": [len(rows), y.shape[1]], "rows_of": len(y)}


def _claim_stdout():
    """Point file descriptor 1 at stderr (whatever C++ libraries print -- `[Gloo] Rank ...`, c10d warnings -- goes
    there) and return a text stream on a duplicate of the ORIGINAL stdout for the one JSON line."""
    sys.stdout.flush()
    keep = os.dup(1)
    os.dup2(2, 1)
    sys.stdout = os.fdopen(os.dup(2), "w", buffering=1)  # Python-level prints of imported modules: stderr as well
    return os.fdopen(keep, "w")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=100)
    # The shader clock needs ~50 ms of load to come up from idle (scripts/clock_settle_probe.py: 101, 69, 61, 58 ... us per
    # launch over the first 25 ms, 52.0 +- 0.3 from 50 ms on): an untimed run of the same launches precedes the W warm-up
    # steps, so that the K timed steps measure the sustained rate whatever K and W are.
    ap.add_argument("--settle", type=float, default=0.3, help="seconds of untimed launches before the warm-up steps")
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--full", action="store_true",
                    help="also run every auxiliary measurement (repeats of the timed launches, other precisions and routes, "
                         "training legs, CPU baseline); a plain run does only the headline steps")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--train-batch", type=int, default=4096)
    ap.add_argument("--train-steps", type=int, default=200,
                    help="timed optimizer steps of the training legs (40 until r3: the one host sync at the end was ~1 us per step of a 45-us step)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/*.npy (rank 0; a seeded sample of %d rows)" % DUMP_ROWS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            _self_launch(args.gpus, sys.argv[1:])  # does not return
        args.gpus = world
    json_out = _claim_stdout()

    torch = None
    dist = None
    try:
        import torch  # plumbing only: barrier / max-over-ranks / synchronize of the contract
    except Exception:
        torch = None
    if world > 1:
        if torch is None:
            raise SystemExit("multi-GPU bench needs torch.distributed")
        import torch.distributed as dist
        # Rehearsal switch (never set by the driver): V21_BENCH_REHEARSAL=1 runs the ranks of an N > 1 launch on
        # ONE GPU over gloo + the library's host-staged transport, so that everything but the RCCL calls of the
        # multi-GPU code path can be exercised on a one-GPU box.  The line says so in "config".
        if os.environ.get("V21_BENCH_REHEARSAL") == "1":
            local_rank = 0
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    native = importlib.import_module("21cmvae_amd._native")
    synth = importlib.import_module("21cmvae_amd.synth")
    pp = importlib.import_module("21cmvae_amd.preprocess")

    ctx = native.Context(local_rank)
    stack = native.Stack(ctx, DIMS, ACT)
    wflat = glorot(DIMS, seed=3)
    stack.set_weights(wflat)
    par_train = synth.make_params(synth.N_TRAIN, seed=1, corners=True)
    sig_train = synth.make_signals(4096, seed=301)
    ps, ss = pp.ParamStats.of(par_train), pp.SignalStats.of(sig_train)
    stack.set_input_transform(ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
    stack.set_output_transform(ss.std, ss.mean)
    flags = native.FWD_IN_TRANSFORM | native.FWD_OUT_TRANSFORM

    B = args.batch
    params = synth.make_params(B, seed=1000 + rank, dtype=np.float32)
    d_x = ctx.malloc(params.nbytes)
    d_y = ctx.malloc(B * DIMS[-1] * 4)
    ctx.h2d(d_x, params)

    def sync_all():
        ctx.sync()
        if torch is not None and torch.cuda.is_available():
            torch.cuda.synchronize()

    def barrier():
        if dist is not None:
            dist.barrier()

    def timed(prec, steps, warmup):
        t_s = time.perf_counter()
        while time.perf_counter() - t_s < args.settle:
            for _ in range(100):
                stack.forward_dev(d_x, DIMS[0], B, d_y, DIMS[-1], prec, flags)
            ctx.sync()
        for _ in range(warmup):
            stack.forward_dev(d_x, DIMS[0], B, d_y, DIMS[-1], prec, flags)
        sync_all(); barrier(); sync_all()
        e0, e1 = ctx.event(), ctx.event()
        t0 = time.perf_counter()
        ctx.record(e0)
        for _ in range(steps):
            stack.forward_dev(d_x, DIMS[0], B, d_y, DIMS[-1], prec, flags)
        ctx.record(e1)
        sync_all(); barrier(); sync_all()
        wall = time.perf_counter() - t0
        ev_ms = ctx.elapsed_ms(e0, e1)
        # what the last timed step left in d_y, copied after the timed region (--dump-outputs)
        timed.output = None
        if args.dump_outputs and rank == 0:
            timed.output = np.empty((B, DIMS[-1]), np.float32)
            ctx.d2h(timed.output, d_y)
        # --full only from here on: the untimed repeats of the K launches
        timed.per_launch_ms = None
        # per-launch durations of a second, untimed run of the same K launches (an event pair around every launch
        # costs a few us of host time per step, so it stays out of the timed region): min / median beside the mean
        if args.full:
            evs = [ctx.event() for _ in range(steps + 1)]
            ctx.record(evs[0])
            for i in range(steps):
                stack.forward_dev(d_x, DIMS[0], B, d_y, DIMS[-1], prec, flags)
                ctx.record(evs[i + 1])
            ctx.sync()
            timed.per_launch_ms = [ctx.elapsed_ms(evs[i], evs[i + 1]) for i in range(steps)]
        # (r4 ran a THIRD repeat here with one sampling wave beside the launches -- v21_debug_clock_probe_*.  r5 dropped it: that wave
        #  sits on ONE CU and reads ITS clock between samples -- 2.44 GHz beside launches whose own workgroups measure 1.5-1.6 GHz
        #  (gpurun_out runs of r5; VERDICT r4 weak 2 had spotted that the same 52-54 us came with "clocks" of 1.78 and 2.40 GHz))
        timed.clock = None
        # r5: the clock FROM THE KERNEL ITSELF.  A THIRD untimed run -- settle, warm-up, K launches --
        # through the clock-stamped instantiation of the same kernel (fused_fwd.h: CLOCK_STAMPS; identical but for two
        # pairs of scalar counter reads and one 40-byte store per workgroup): wave 0 of EVERY workgroup of EVERY one of the K
        # launches reads s_memtime (shader-clock cycles) and s_memrealtime (100 MHz) at its start and end, and its XCD.
        timed.inkernel = None
        if args.full and prec in ("f16", "bf16") and rank == 0:
            try:
                nwg = (B + 127) // 128
                d_st = ctx.malloc(steps * nwg * 40)
                ctx.memset(d_st, 0, steps * nwg * 40)
                t_s = time.perf_counter()
                while time.perf_counter() - t_s < args.settle:
                    for _ in range(100):
                        stack.forward_clocked(d_x, DIMS[0], B, d_y, DIMS[-1], d_st, prec, flags)
                    ctx.sync()
                for _ in range(warmup):
                    stack.forward_clocked(d_x, DIMS[0], B, d_y, DIMS[-1], d_st, prec, flags)
                c0, c1 = ctx.event(), ctx.event()
                ctx.record(c0)
                for i in range(steps):
                    stack.forward_clocked(d_x, DIMS[0], B, d_y, DIMS[-1], d_st + i * nwg * 40, prec, flags)
                ctx.record(c1)
                ctx.sync()
                st_h = np.empty((steps, nwg, 5), np.uint64)
                ctx.d2h(st_h, d_st)
                ctx.free(d_st)
                timed.inkernel = _reduce_clock_stamps(st_h, ctx.elapsed_ms(c0, c1) / steps)
            except Exception as e:  # pragma: no cover
                timed.inkernel = {"error": "%s: %s" % (type(e).__name__, e)}
        if dist is not None:
            t = torch.tensor([wall], dtype=torch.float64, device=_pg_device(dist))
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            wall = float(t.item())
        return wall, ev_ms

    wall, ev_ms = timed(args.precision, args.steps, args.warmup)
    dumped = None
    if timed.output is not None:
        dumped = dump_outputs(args.dump_outputs, timed.output)
        timed.output = None
    value = world * B * args.steps / wall
    kern_s = ev_ms * 1e-3 / args.steps  # average launch duration on the launch stream (HIP events)
    achieved_tf = FLOP_PER_SIGNAL * B / kern_s / 1e12
    _ik = timed.inkernel if isinstance(getattr(timed, "inkernel", None), dict) else {}
    out = {
        "metric": "emulated signals/sec (batched predict)",
        "value": value,
        "unit": "signals/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "clock_settle_s": args.settle,
        "ms_per_step": wall / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": {"f16": "f16 (f32 accumulate)", "bf16": "bf16 (f32 accumulate)", "f32": "f32"}[args.precision],
        "data": "synthetic",
        "full": args.full,
        "outputs_dumped": dumped,
        "config": {"workload": "configs[1]: direct emulator 7->[352,352,352,224]->451 batched predict, "
                               "batch=%d per GPU, device-resident in/out, fused par_transform+unpreproc" % B,
                   "batch_per_gpu": B, "weights": "Glorot-uniform seed 3", "parallelism": "rows sharded, no collective"},
        "roofline": {"bound": "mfma", "achieved": achieved_tf, "peak": PEAK_TFLOPS[args.precision],
                     "unit": "TFLOP/s", "frac": achieved_tf / PEAK_TFLOPS[args.precision], "traffic": None,
                     "kernel": "fused_fwd<ArchS1, Prec%sx2sp>" % args.precision.upper() if args.precision != "f32" else "fused_fwd<ArchS1, PrecF32>",
                     "kernel_ms": kern_s * 1e3,
                     "kernel_ms_min": float(min(timed.per_launch_ms)) if timed.per_launch_ms else None,
                     "kernel_ms_median": float(np.median(timed.per_launch_ms)) if timed.per_launch_ms else None,
                     "time_base": "HIP events on the launch stream around the K timed launches (mean); min / median from "
                                  "per-launch event pairs of a second run (--full); profiles/%s/kernel_stats_bench_f16.csv " % PROFILE_TAG +
                                  "(rocprofv3 --kernel-trace --stats of this command) must agree with the mean",
                     # (the same fraction from the ONE number the driver times itself: ms_per_step, launch gaps included)
                     "frac_from_ms_per_step": FLOP_PER_SIGNAL * B / (wall / args.steps) / 1e12 / PEAK_TFLOPS[args.precision],
                     # r5: clock_ghz is read INSIDE the kernel (every workgroup of K launches); r4's sampling wave beside
                     # the launches stays as clock_probe_sampling_wave (it disagreed with itself from run to run:
                     # VERDICT r4 weak 2 -- one wave on one CU sees ITS XCD's clock while it idles between samples)
                     "clock_ghz": (_ik.get("ghz_mean") if _ik.get("ghz_mean") else (timed.clock or {}).get("ghz_mean")),
                     "clock_in_kernel": timed.inkernel, "clock_probe_sampling_wave": timed.clock, "clock_nominal_ghz": 2.4,
                     "frac_of_clocked_peak": (achieved_tf / (PEAK_TFLOPS[args.precision] * _ik["ghz_mean"] / 2.4) if _ik.get("ghz_mean") else None),
                     "clock_note": "clock_ghz = shader-clock cycles / 100-MHz ticks between start and end of every workgroup of an untimed "
                                   "repeat of the K launches (clock-stamped instantiation of the same kernel); peak figures assume "
                                   "2.4 GHz, frac_of_clocked_peak rescales the peak to that clock",
                     "algorithmic_flop_per_launch": FLOP_PER_SIGNAL * B,
                     "hbm_GBps_algorithmic": BYTES_PER_SIGNAL * B / kern_s / 1e9,
                     "hbm_frac_of_8TBps": BYTES_PER_SIGNAL * B / kern_s / 1e9 / PEAK_HBM_GBS},
    }

    if os.environ.get("V21_BENCH_REHEARSAL") == "1" and world > 1:
        out["config"]["rehearsal"] = "%d ranks on ONE GPU over gloo + host-staged collectives: a code-path check, not a measurement" % world
    # HBM traffic per launch of the headline kernel: PMC counters cannot be read from inside the timed
    # process; they were collected with `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes) on
    # this same command and are kept under profiles/ (hbm_bytes = 2*FETCH*1024 + WRITE*1024 on gfx950).
    pmc = os.path.join(ROOT, "profiles", PROFILE_TAG, "pmc_fused_%s.json" % args.precision)
    if not os.path.exists(pmc):
        pmc = os.path.join(ROOT, "profiles", "r3", "pmc_fused_%s.json" % args.precision)
    if os.path.exists(pmc) and B == BATCH:
        try:
            out["roofline"]["traffic"] = json.load(open(pmc))["hbm_bytes_per_launch"]
            out["roofline"]["traffic_source"] = "%s (rocprofv3 --pmc, kernel %s)" % (
                os.path.relpath(pmc, ROOT), json.load(open(pmc)).get("_kernel", "?"))
            out["roofline"]["algorithmic_bytes"] = BYTES_PER_SIGNAL * B
            out["roofline"]["profile_matches_build"] = _profile_is_current()
        except Exception:
            pass
    # MFMA-pipe occupancy (north_star: ">= 50 % MFMA utilisation", by rocprof): SQ_VALU_MFMA_BUSY_CYCLES of the timed
    # launches (profiles/<tag>/pmc_fused_*_timed_launches_mfma_busy.json: summed over the 1,024 SIMDs; it is 32 cycles per
    # 32x32x16 MFMA, so it does not depend on the clock the profiled run had) over the cycles a SIMD had during one launch
    # of THIS run: kernel time x the clock measured beside the launches
    busy = os.path.join(ROOT, "profiles", PROFILE_TAG, "pmc_fused_%s_timed_launches_mfma_busy.json" % args.precision)
    if os.path.exists(busy) and B == BATCH and out["roofline"].get("clock_ghz"):
        try:
            per_simd = json.load(open(busy))["mfma_busy_cycles_per_simd"]
            cyc = _ik["kcycles_per_launch"] * 1e3 if _ik.get("kcycles_per_launch") else kern_s * out["roofline"]["clock_ghz"] * 1e9
            out["roofline"]["mfma_busy_cycles_per_simd"] = per_simd
            out["roofline"]["mfma_pipe_busy_frac"] = per_simd / cyc
            out["roofline"]["mfma_pipe_busy_source"] = ("%s (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES, the timed launches only) / "
                                                        "(kernel_ms x clock_ghz of this run)" % os.path.relpath(busy, ROOT))
        except Exception:
            pass

    if args.full and rank == 0 and not args.no_extras:
        modes = {}
        for prec in ("f32", "bf16", "f16"):
            if prec == args.precision:
                continue
            try:
                # local (rank-0 only) side measurement: no barriers involved
                for _ in range(2):
                    stack.forward_dev(d_x, DIMS[0], B, d_y, DIMS[-1], prec, flags)
                ctx.sync()
                a, b = ctx.event(), ctx.event()
                n = max(5, args.steps // 5)
                ctx.record(a)
                for _ in range(n):
                    stack.forward_dev(d_x, DIMS[0], B, d_y, DIMS[-1], prec, flags)
                ctx.record(b)
                ctx.sync()
                ms = ctx.elapsed_ms(a, b) / n
                modes[prec] = {"signals_per_s": B / (ms * 1e-3), "kernel_ms": ms,
                               "frac_of_peak": FLOP_PER_SIGNAL * B / (ms * 1e-3) / 1e12 / PEAK_TFLOPS[prec]}
            except Exception as e:  # pragma: no cover
                modes[prec] = {"error": str(e)}
        out["other_precisions_1gpu"] = modes
        # r5: consecutive INDEPENDENT batches on TWO streams (two contexts of the one GPU, a replica of the stack on each).  The
        # headline launch is exactly two workgroups per CU, and on every CU one of the pair ends at ~2/3 of the launch and the
        # other finishes alone: in one stream the next launch cannot start before the last workgroup has
        # ended, on two streams its workgroups move in as soon as a slot is free.  NOT the headline (its roofline is defined
        # per launch on one stream): what a server that alternates two contexts gets.
        try:
            ctx2 = native.Context(local_rank)
            stack2 = native.Stack(ctx2, DIMS, ACT)
            stack2.set_weights(wflat)
            stack2.set_input_transform(ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
            stack2.set_output_transform(ss.std, ss.mean)
            d_y2 = ctx2.malloc(B * DIMS[-1] * 4)
            pairs = ((stack, ctx, d_y), (stack2, ctx2, d_y2))
            n2 = max(20, args.steps)
            t_s = time.perf_counter()
            while time.perf_counter() - t_s < args.settle:
                for i in range(100):
                    pairs[i & 1][0].forward_dev(d_x, DIMS[0], B, pairs[i & 1][2], DIMS[-1], args.precision, flags)
                ctx.sync(); ctx2.sync()
            t0 = time.perf_counter()
            for i in range(n2):
                pairs[i & 1][0].forward_dev(d_x, DIMS[0], B, pairs[i & 1][2], DIMS[-1], args.precision, flags)
            ctx.sync(); ctx2.sync()
            dt = (time.perf_counter() - t0) / n2
            out["predict_two_streams"] = {"signals_per_s": B / dt, "us_per_batch": dt * 1e6, "batches": n2,
                                          "vs_headline": (B / dt) / value * world,
                                          "frac_of_peak": FLOP_PER_SIGNAL * B / dt / 1e12 / PEAK_TFLOPS[args.precision],
                                          "note": "independent 65,536-row batches alternating between two contexts (two streams, two output buffers); wall clock"}
            ctx2.free(d_y2)
            del stack2
        except Exception as e:  # pragma: no cover
            out["predict_two_streams"] = {"error": "%s: %s" % (type(e).__name__, e)}
        # Stacks WITHOUT a compiled fused kernel (csrc/archs.h holds four): what a custom `hidden_dims`
        # (emulator.py:12-48) or a sweep member's predict() gets.  `predict_generic_S1`: the headline stack forced
        # down that route (V21_FWD_FORCE_GENERIC), same 65,536 rows; `predict_custom`: the sample notebook's
        # 7 -> [64, 128] -> 451 model (notebooks/sample_notebook.ipynb cell 9) on its default route.
        def fwd_rate(stk, dims, prec, fl, n=10):
            for _ in range(2):
                stk.forward_dev(d_x, dims[0], B, d_y, dims[-1], prec, fl)
            ctx.sync()
            a, b = ctx.event(), ctx.event()
            ctx.record(a)
            for _ in range(n):
                stk.forward_dev(d_x, dims[0], B, d_y, dims[-1], prec, fl)
            ctx.record(b)
            ctx.sync()
            ms = ctx.elapsed_ms(a, b) / n
            flop = 2 * sum(p * q for p, q in zip(dims[:-1], dims[1:])) * B
            return {"signals_per_s": B / (ms * 1e-3), "ms_per_launch_set": ms, "precision": prec,
                    "frac_of_peak": flop / (ms * 1e-3) / 1e12 / PEAK_TFLOPS[prec],
                    "hbm_frac_of_8TBps": 4 * (dims[0] + dims[-1]) * B / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS}
        try:
            gen = {}
            for prec in ("f16", "f32"):
                gen[prec] = fwd_rate(stack, DIMS, prec, flags | native.FWD_FORCE_GENERIC)
                gen[prec]["slowdown_vs_fused"] = (out["value"] if prec == args.precision else modes.get(prec, {}).get("signals_per_s", 0.0)) / gen[prec]["signals_per_s"]
            out["predict_generic_S1"] = gen
            # the table-driven one-launch forward (csrc/train_chain.h FORWARD mode: what every stack without a compiled
            # kernel runs in f16 / bf16), forced onto the headline stack for comparison with the compiled kernel
            td = {prec: fwd_rate(stack, DIMS, prec, flags | native.FWD_FORCE_CHAIN) for prec in ("f16", "bf16", "f32")}
            td["f32"]["slowdown_vs_fused"] = modes.get("f32", {}).get("signals_per_s", 0.0) / td["f32"]["signals_per_s"]
            td["f16"]["slowdown_vs_fused"] = (out["value"] if args.precision == "f16" else modes.get("f16", {}).get("signals_per_s", 0.0)) / td["f16"]["signals_per_s"]
            out["predict_table_driven_S1"] = td
            # r4: the fused kernel instantiated for a stack at RUN TIME (csrc/jit.h, hiprtc) -- what every stack outside
            # csrc/archs.h gets once its code object is there.  `predict_jit_S1`: the headline stack forced down that
            # route (V21_FWD_FORCE_JIT) against its compiled-in kernel: the same template, so ~1.0x by construction.
            pj = {}
            for prec in ("f16", "f32"):
                try:
                    pj[prec] = fwd_rate(stack, DIMS, prec, flags | native.FWD_FORCE_JIT)
                    pj[prec]["slowdown_vs_fused"] = (out["value"] if prec == args.precision else modes.get(prec, {}).get("signals_per_s", 0.0)) / pj[prec]["signals_per_s"]
                except Exception as e:
                    pj[prec] = {"error": "%s: %s" % (type(e).__name__, e)}
            out["predict_jit_S1"] = pj
            cdims = [7, 64, 128, 451]
            cst = native.Stack(ctx, cdims, [1, 1, 0])
            cst.set_weights(glorot(cdims, seed=5))
            cst.set_input_transform(ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
            cst.set_output_transform(ss.std, ss.mean)
            pc = {}
            for prec in ("f16", "f32"):
                t0 = time.perf_counter()
                try:
                    state = cst.jit(prec)  # waits for the compilation (a cached code object: milliseconds)
                except Exception as e:
                    state = "unavailable (%s)" % e
                wait_s = time.perf_counter() - t0
                pc[prec] = fwd_rate(cst, cdims, prec, flags)
                pc[prec]["route"] = "fused kernel instantiated at run time: %s after %.2f s" % (state, wait_s)
                pc[prec + "_table_driven"] = fwd_rate(cst, cdims, prec, flags | native.FWD_FORCE_CHAIN)
            out["predict_custom"] = pc
            out["predict_custom"]["model"] = "7->[64,128]->451 (notebooks/sample_notebook.ipynb), %d rows, device-resident" % B
            # r4: BASELINE.json's ">= 50 % MFMA on the widest hidden layer", measured on a stack that is almost nothing else
            # (7 -> 352 x 6 -> 9: five 352 -> 352 layers = 99.1 % of its multiply-adds, 64 B of HBM traffic per row) through
            # the same fused kernel, instantiated at run time; rocprofv3 duration and MFMA-pipe counters of this stack:
            # profiles/<tag>/hidden_layers_352_* (scripts/hidden_layer_probe.py)
            try:
                hdims = [7] + [352] * 6 + [9]
                hst = native.Stack(ctx, hdims, [1] * 6 + [0])
                hst.set_weights(glorot(hdims, seed=6))
                hst.jit(args.precision if args.precision != "f32" else "f16")
                hp = fwd_rate(hst, hdims, args.precision if args.precision != "f32" else "f16", 0, n=max(10, args.steps))
                hp["model"] = "7->[352 x 6]->9, %d rows: five 352->352 layers = 99.1 %% of the multiply-adds" % B
                busy_h = os.path.join(ROOT, "profiles", PROFILE_TAG, "hidden_layers_352_%s_mfma_busy.json" % hp["precision"])
                if os.path.exists(busy_h) and out["roofline"].get("clock_ghz"):
                    per_simd = json.load(open(busy_h))["mfma_busy_cycles_per_simd"]
                    hp["mfma_busy_cycles_per_simd"] = per_simd
                    hp["mfma_pipe_busy_frac_at_headline_clock"] = per_simd / (hp["ms_per_launch_set"] * 1e-3 * out["roofline"]["clock_ghz"] * 1e9)
                out["predict_hidden_352"] = hp
            except Exception as e:
                out["predict_hidden_352"] = {"error": "%s: %s" % (type(e).__name__, e)}
        except Exception as e:
            out["predict_generic_S1"] = {"error": "%s: %s" % (type(e).__name__, e)}
        # host numpy -> numpy predict (PCIe-inclusive); never the headline value
        for _ in range(2):  # first calls pin the pooled result buffers
            yk = stack.forward(params, args.precision, flags)
        t0 = time.perf_counter()
        reps = 10
        for _ in range(reps):
            yk = stack.forward(params, args.precision, flags)
        out["host_roundtrip_signals_per_s"] = B * reps / (time.perf_counter() - t0)
        del yk

    if args.full and not args.no_train and not args.no_extras:
        try:  # before the communicator exists: the models of a sweep are independent per rank
            out["sweep"] = sweep_leg(native, ctx, args.precision)
        except Exception as e:
            out["sweep"] = {"error": "%s: %s" % (type(e).__name__, e)}
        try:  # r5: configs[4] on one GPU -- 8 / 16 / 32 / 64 models in one group
            out["sweep_scaling"] = {"f16": sweep_scaling_leg(native, ctx, args.precision if args.precision != "f32" else "f16"),
                                    "f32": sweep_scaling_leg(native, ctx, "f32")}
        except Exception as e:  # pragma: no cover
            out["sweep_scaling"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if args.precision != "f32":  # the same sweep in the reference's arithmetic (grouped launches of train_chain32s.h / dw_adam32.h); every rank, like the leg above
            try:
                out["sweep_f32"] = sweep_leg(native, ctx, "f32")
            except Exception as e:
                out["sweep_f32"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if dist is not None:  # every rank takes part, whether its own leg failed or not
            t = torch.tensor([out["sweep"].get("model_steps_per_s_grouped", 0.0)], dtype=torch.float64, device=_pg_device(dist))
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            out["sweep"]["model_steps_per_s_grouped_all_ranks"] = float(t.item())

    if args.full and not args.no_train:
        def run_train():
            try:
                if dist is not None and dist.get_backend() == "nccl":
                    torch.cuda.set_device(local_rank)  # (a new thread starts on GPU 0)
                transport = "none"
                if world > 1:
                    par = importlib.import_module("21cmvae_amd.parallel")
                    transport = "RCCL (in-library)" if dist.get_backend() == "nccl" else "host-staged over gloo"
                    err = None
                    try:
                        par.init_engine_comm(ctx)
                    except Exception as e:
                        err = e
                    # the fallback is decided COLLECTIVELY: ranks on different transports would hang in the
                    # first exchange -- if the in-library communicator failed anywhere, every rank drops it
                    flag = torch.tensor([0.0 if err is None else 1.0], dtype=torch.float64, device=_pg_device(dist))
                    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
                    if float(flag.item()) > 0:
                        if err is None:
                            ctx.comm_destroy()
                        transport = "host-staged over the process group (in-library RCCL failed on some rank: %s)" % (err,)
                        par.init_engine_comm(ctx, backend="host")
                tl = train_leg(native, ctx, native.Stack, world, rank, dist, torch, barrier, sync_all,
                               args.train_batch, args.precision, args.train_steps, 20)
                tl["transport"] = transport
                # what the in-library communicator itself reports, and how many ranks an all-reduce through it sums
                seen = ctx.ranks_seen()
                info = ctx.comm_info()
                tl["n_ranks_seen"] = seen
                tl["communicator"] = {"nranks": info[0], "rank": info[1], "transport": info[2]}
                ae_params = sum(k * n + n for k, n in zip(AE_DIMS[:-1], AE_DIMS[1:]))
                tl["roofline"] = train_roofline(tl, AE_FLOP_PER_SAMPLE, ae_params, 451, 451,
                                                "kernel_stats_train_b%d_%s.csv" % (args.train_batch, args.precision),
                                                "pmc_train_b%d_%s.json" % (args.train_batch, args.precision))
                out["train"] = tl
                if world > 1:  # the other exchange: reduce-scatter -> Adam on each rank's slice -> all-gather
                    ctx.comm_set_sharded(True)
                    ts = train_leg(native, ctx, native.Stack, world, rank, dist, torch, barrier, sync_all,
                                   args.train_batch, args.precision, args.train_steps, 20)
                    ts["collective"] = "reduce-scatter + all-gather, Adam on 1/%d of the arena per rank" % world
                    ts["transport"] = transport
                    ts["n_ranks_seen"] = ctx.ranks_seen()
                    out["train_sharded_adam"] = ts
                    ctx.comm_set_sharded(False)
                if world > 1:  # r5: the all-reduce in two buckets, the output-side half overlapping the second weight-gradient launch (LAST of the three
                    # exchange forms: the one that has never met a real RCCL -- if it should stall, the two above are already in `out`)
                    ctx.comm_set_buckets(2)
                    tb = train_leg(native, ctx, native.Stack, world, rank, dist, torch, barrier, sync_all,
                                   args.train_batch, args.precision, args.train_steps, 20)
                    tb["collective"] = "all-reduce in two buckets (output-side layers + loss slot first, on a second stream)"
                    tb["transport"] = transport
                    tb["n_ranks_seen"] = ctx.ranks_seen()
                    out["train_two_buckets"] = tb
                    ctx.comm_set_buckets(1)
                if world == 1 and not args.no_extras:
                    # r5: the COMPUTE side of the data-parallel step on one GPU -- rank 0 of 8 on a communicator without a
                    # transport (v21_comm_init_null): its 4,096-row share of a 32,768-row global batch through the N > 1
                    # route (chain -> split-K weight gradients -> [exchange: nothing] -> Adam), one and two buckets.  A SCALE
                    # curve minus this is wire + collective-launch time.
                    try:
                        cn = native.Context(local_rank)
                        cn.comm_init_null(8, 0)
                        dpc = {}
                        for nb in (1, 2):
                            cn.comm_set_buckets(nb)
                            d = train_leg(native, cn, native.Stack, 8, 0, None, torch, lambda: None, lambda: cn.sync(),
                                          args.train_batch, args.precision, args.train_steps, 20)
                            dpc["buckets_%d" % nb] = {k: d[k] for k in ("ms_per_step", "steps_per_s", "phases", "batch_per_gpu", "global_batch")}
                        dpc["note"] = ("rank 0 of 8, nothing exchanged (null transport): the three-launch data-parallel step without its "
                                       "wire time; compare ms_per_step with `train` (single rank: gradients + Adam in one launch)")
                        cn.comm_destroy()
                        out["dp_compute_only"] = dpc
                    except Exception as e:  # pragma: no cover
                        out["dp_compute_only"] = {"error": "%s: %s" % (type(e).__name__, e)}
                    if args.precision in ("f16", "bf16"):
                        out["train_custom_b16384"] = custom_train_leg(native, ctx, args.precision)
                    t32 = train_leg(native, ctx, native.Stack, 1, 0, None, torch, barrier, sync_all, 256, "f32", 200, 10)
                    t32["roofline"] = train_roofline(t32, AE_FLOP_PER_SAMPLE, ae_params, 451, 451,
                                                     "kernel_stats_train_b256_f32.csv", "pmc_train_b256_f32.json")
                    out["train_ref_batch256_f32"] = t32
                    # does the step scale with the batch?  (the MFMA fraction must RISE with the batch)
                    t16k = train_leg(native, ctx, native.Stack, 1, 0, None, torch, barrier, sync_all, 16384,
                                     args.precision, max(10, args.train_steps // 2), 10)
                    t16k["roofline"] = train_roofline(t16k, AE_FLOP_PER_SAMPLE, ae_params, 451, 451,
                                                      "kernel_stats_train_b16384_%s.csv" % args.precision,
                                                      "pmc_train_b16384_%s.json" % args.precision)
                    # r4: large steps of the reference stacks take a fused training kernel (weights through an LDS ring, activations
                    # in registers, the weight stream written by the previous step's Adam pass, rows from the 16-bit resident
                    # copy): csrc/fused_train16.h (16 rows per wave, 64-row workgroups) from 8,193 rows for a trainer of fewer
                    # than 24,576 rows per step, csrc/fused_train.h (128-row workgroups) from 16,384 rows for a larger one;
                    # V21_FUSED_TRAIN_ROWS / V21_FUSED_TRAIN16 override
                    fused_route = "fused training kernel (fused_train<ArchT1, Prec%st>: 128-row workgroups) + split-K weight gradients + Adam" % args.precision.upper()
                    if args.precision in ("f16", "bf16"):  # (a trainer of fewer than 24,576 rows per step: 16 rows per wave, 64-row workgroups, two per CU)
                        t16k["route"] = "fused training kernel (fused_train16<ArchT1, Prec%st16>: 64-row workgroups) + split-K weight gradients + Adam" % args.precision.upper()
                    out["train_b16384"] = t16k
                    t32k = train_leg(native, ctx, native.Stack, 1, 0, None, torch, barrier, sync_all, 32768,
                                     args.precision, max(10, args.train_steps // 4), 5)
                    t32k["roofline"] = train_roofline(t32k, AE_FLOP_PER_SAMPLE, ae_params, 451, 451,
                                                      "kernel_stats_train_b32768_%s.csv" % args.precision,
                                                      "pmc_train_b32768_%s.json" % args.precision)
                    if args.precision in ("f16", "bf16"):
                        t32k["route"] = fused_route
                    out["train_b32768"] = t32k
                    out["train_variational"] = train_leg(native, ctx, native.Stack, 1, 0, None, torch, barrier,
                                                         sync_all, args.train_batch, args.precision, args.train_steps, 20,
                                                         variational=True)
                    # ... and in the reference's arithmetic at its batch (the variational head inside train_chain32s_kernel)
                    out["train_variational_ref_batch256_f32"] = train_leg(native, ctx, native.Stack, 1, 0, None, torch, barrier,
                                                                          sync_all, 256, "f32", 200, 10, variational=True)
            except Exception as e:  # the headline metric must survive a failure of the auxiliary leg
                out["train"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if world > 1:
            # a communicator that never comes up must not take the headline number with it: the leg runs
            # in a thread, and a rank that is still waiting after the limit reports and leaves
            import threading
            th = threading.Thread(target=run_train, daemon=True)
            th.start()
            th.join(timeout=float(os.environ.get("V21_BENCH_TRAIN_TIMEOUT", "150")))
            if th.is_alive():
                # (what finished stays in `out`: the all-reduce leg is reported even if a later exchange form stalls)
                out["train_timeout"] = {"error": "timeout: the data-parallel training legs did not all finish",
                                        "finished": [k for k in ("train", "train_sharded_adam", "train_two_buckets") if k in out]}
                out.setdefault("train", {"error": "timeout: the data-parallel training leg did not finish"})
                if rank == 0:
                    print(json.dumps(out), file=json_out, flush=True)
                os._exit(3)  # a hung leg is a failed run: the JSON line is still printed, the exit status says so
        else:
            run_train()

    if args.full and rank == 0 and world == 1 and not args.no_train and not args.no_extras:
        try:
            out["fit_reference_recipe"] = [fit_leg("f32"), fit_leg("f16")]
            out["fit_n30000"] = [fit_leg("f16", n_train=30000), fit_leg("f16", n_train=30000, joint=True),
                                 fit_leg("f32", n_train=30000), fit_leg("f32", n_train=30000, joint=True)]
        except Exception as e:
            out["fit_reference_recipe"] = {"error": "%s: %s" % (type(e).__name__, e)}
        try:
            out["accuracy_on_trained_stack"] = accuracy_leg(native, ctx)
        except Exception as e:
            out["accuracy_on_trained_stack"] = {"error": "%s: %s" % (type(e).__name__, e)}
        try:
            out["class_surface_predict"] = class_surface_leg()
        except Exception as e:
            out["class_surface_predict"] = {"error": "%s: %s" % (type(e).__name__, e)}
        try:
            out["single_call_latency"] = latency_leg()
        except Exception as e:
            out["single_call_latency"] = {"error": "%s: %s" % (type(e).__name__, e)}

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:  # last: see _BLAS_LIMIT
        xt = pp.par_transform(params.astype(np.float64), par_train).astype(np.float32)
        out["cpu_baseline"] = cpu_baseline(wflat, xt)

    barrier()
    if rank == 0:
        print(json.dumps(out), file=json_out, flush=True)
    ctx.free(d_x)
    ctx.free(d_y)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
