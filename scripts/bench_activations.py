"""Device time of the smooth activations (include/v21.h: V21_ACT_TANH .. V21_ACT_SOFTPLUS) beside ReLU, all versions of one
comparison alternated inside one process:

  forward   65,536 device-resident rows of the headline dims 7-352-352-352-224-451, f16 and f32, per activation: the fused
            forward kernel instantiated at run time (V21_FWD_FORCE_JIT), the same dims with ReLU down the same route, and
            the smooth stack forced onto the generic per-layer route (V21_FWD_FORCE_GENERIC).  HIP events around each call;
  train     one optimizer step on the per-layer route (V21_TRAIN_CHAIN=0 for the ReLU stack; smooth stacks take it anyway)
            at 256 and 4,096 rows, f32 and f16: tanh against ReLU.  Host clock around epochs of 16 steps (an epoch ends in a
            device synchronise);
  surface   wall time of one DirectEmulator.predict and one 64-chain sample_posterior on 7-64-128-451 tanh weights.

Before anything is timed the device runs the workload untimed for --settle seconds (clocks ramp up from idle), then every
version is warmed up; a figure is the median of --repeat rounds, each round visiting every version once.

  --prebuild        compile the run-time kernels this script uses into the library's kernel_cache/ (hiprtc, no GPU) and exit
  --only-relu-train print the ReLU per-layer step times only (one JSON line) -- with --lib PATH from another build of the
                    library: the driver below starts such children to compare two builds
  --against PATH    ReLU per-layer steps of this build (N) against the library at PATH (P), child processes in the order
                    N P P N P P ...: N against P, and P against P as the spread of the same call

    python scripts/bench_activations.py [--quick] [--against /path/to/other/libv21.so]
One JSON line per measurement.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HEADLINE = [7, 352, 352, 352, 224, 451]
T3 = [7, 64, 128, 451]
NAMES = {1: "relu", 3: "tanh", 4: "sigmoid", 5: "elu", 6: "softplus"}


def pkg(sub):
    return importlib.import_module("21cmvae_amd." + sub)


def codes(dims, code):
    return [code] * (len(dims) - 2) + [0]


def weights(dims, seed):
    from oracle import ref_numpy as ora
    Ws, bs = ora.init_mlp(dims, seed=seed)
    bs = [np.random.default_rng(seed + 1).normal(scale=0.05, size=b.shape).astype(np.float32) for b in bs]
    return ora.flatten_params(Ws, bs)


def settle(ctx, call, seconds):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            call()
        ctx.sync()


def alternated_ms(ctx, calls, repeat, warm=3):
    """{name: median ms} of HIP-event timings, every round visiting every version once"""
    for c in calls.values():
        for _ in range(warm):
            c()
    ctx.sync()
    a, b = ctx.event(), ctx.event()
    t = {k: [] for k in calls}
    for _ in range(repeat):
        for k, c in calls.items():
            ctx.record(a)
            c()
            ctx.record(b)
            ctx.sync()
            t[k].append(ctx.elapsed_ms(a, b))
    return {k: float(np.median(v)) for k, v in t.items()}


def bench_forward(ctx, args):
    nat = pkg("_native")
    n, din, dout = 65536, HEADLINE[0], HEADLINE[-1]
    x = np.random.default_rng(9).uniform(-1, 1, size=(n, din)).astype(np.float32)
    dx, dy = ctx.malloc(x.nbytes), ctx.malloc(n * dout * 4)
    ctx.h2d(dx, x)
    flat = weights(HEADLINE, 3)
    relu = nat.Stack(ctx, HEADLINE, codes(HEADLINE, 1))
    relu.set_weights(flat)
    for prec in ("f16", "f32"):
        assert relu.jit(prec) == "ready"
        settle(ctx, lambda: relu.forward_dev(dx, din, n, dy, dout, prec, nat.FWD_FORCE_JIT), args.settle)
        for code in (3, 4, 5, 6):
            st = nat.Stack(ctx, HEADLINE, codes(HEADLINE, code))
            st.set_weights(flat)
            row = {"what": "forward", "dims": HEADLINE, "rows": n, "precision": prec, "activation": NAMES[code], "repeats": args.repeat}
            calls = {"relu_fused_rt_ms": lambda: relu.forward_dev(dx, din, n, dy, dout, prec, nat.FWD_FORCE_JIT),
                     "generic_ms": lambda: st.forward_dev(dx, din, n, dy, dout, prec, nat.FWD_FORCE_GENERIC)}
            try:
                ready = st.jit(prec) == "ready"
                st.forward_dev(dx, din, n, dy, dout, prec, nat.FWD_FORCE_JIT)   # (loads the code object: refused if it needs scratch)
                ctx.sync()
            except nat.EngineError as e:
                ready, row["fused_rt_error"] = False, str(e)[:200]
            if ready:
                calls["fused_rt_ms"] = lambda: st.forward_dev(dx, din, n, dy, dout, prec, nat.FWD_FORCE_JIT)
            row.update(alternated_ms(ctx, calls, args.repeat))
            if ready:
                row["fused_rt_over_relu"] = row["fused_rt_ms"] / row["relu_fused_rt_ms"]
                row["generic_over_fused_rt"] = row["generic_ms"] / row["fused_rt_ms"]
                st.forward_dev(dx, din, n, dy, dout, prec, nat.FWD_NO_SMALL)
                row["default_route"] = st.last_route()[0]
            print(json.dumps(row), flush=True)
    ctx.free(dx)
    ctx.free(dy)


STEPS = 16   # optimizer steps per timed epoch


def step_timers(ctx, code, prec, rows):
    """-> a callable that runs one epoch of STEPS per-layer steps of the headline dims with activation `code`"""
    nat = pkg("_native")
    from train_support import new_trainer
    rng = np.random.default_rng(rows)
    x = rng.uniform(-1, 1, size=(STEPS * rows, HEADLINE[0])).astype(np.float32)
    y = rng.normal(size=(STEPS * rows, HEADLINE[-1])).astype(np.float32)
    w = np.full(STEPS * rows, 1.0 / HEADLINE[-1], np.float32)
    st, tr = new_trainer(ctx, HEADLINE, codes(HEADLINE, code), weights(HEADLINE, 3), prec, rows, lr=1e-4, env={"V21_TRAIN_CHAIN": "0"})
    tr.set_data(0, x, y, w)

    def epoch():
        tr.run_epoch(None, rows)
    epoch()
    assert tr.last_route()[0] == ("per_layer", "per_layer"), tr.last_route()[0]
    epoch.keep = (st, tr)
    return epoch


def alternated_us_per_step(calls, repeat):
    for c in calls.values():
        c()
    t = {k: [] for k in calls}
    for _ in range(repeat):
        for k, c in calls.items():
            t0 = time.perf_counter()
            c()
            t[k].append((time.perf_counter() - t0) * 1e6 / STEPS)
    return {k: float(np.median(v)) for k, v in t.items()}


def bench_train(ctx, args, only_relu=False):
    out = {}
    for prec in ("f32", "f16"):
        for rows in (256, 4096):
            calls = {"relu_us_per_step": step_timers(ctx, 1, prec, rows)}
            if not only_relu:
                calls["tanh_us_per_step"] = step_timers(ctx, 3, prec, rows)
            settle(ctx, calls["relu_us_per_step"], args.settle)
            r = alternated_us_per_step(calls, args.repeat)
            if only_relu:
                out["%s_%d" % (prec, rows)] = r["relu_us_per_step"]
                continue
            row = {"what": "train_step_per_layer", "dims": HEADLINE, "rows": rows, "precision": prec, "repeats": args.repeat}
            row.update(r)
            row["tanh_over_relu"] = r["tanh_us_per_step"] / r["relu_us_per_step"]
            print(json.dumps(row), flush=True)
    if only_relu:
        print(json.dumps({"what": "relu_per_layer_us_per_step", "lib": pkg("_native").LIB_PATH, **out}), flush=True)


def bench_surface(args):
    emulator, synth, eng, pp = pkg("emulator"), pkg("synth"), pkg("engine"), pkg("preprocess")
    ds = synth.make_dataset(n_train=3000, n_val=50, n_test=4096, seed=11)
    eng.set_random_seed(11)
    em = emulator.DirectEmulator(hidden_dims=T3[1:-1], activation_func="tanh", **ds)
    em.predict(em.par_test)
    t0 = time.perf_counter()
    em.predict(em.par_test)
    t_pred = time.perf_counter() - t0
    truth = pp.par_untransform(np.random.default_rng(4).uniform(-0.5, 0.5, size=(1, 7)), em.par_train)
    spec = np.asarray(em.predict(truth), np.float32).reshape(-1)
    n_steps = 200 if args.quick else 1000
    run = lambda: em.sample_posterior(spec, 1.0, n_chains=64, n_steps=n_steps, n_warmup=200, p0=truth[0])
    run()
    t0 = time.perf_counter()
    r = run()
    t_s = time.perf_counter() - t0
    print(json.dumps({"what": "surface_wall_time", "dims": T3, "activation": "tanh", "predict_rows": 4096, "predict_wall_s": t_pred,
                      "sample_posterior_chains": 64, "transitions": 200 + n_steps, "sample_posterior_wall_s": t_s,
                      "accept_rate": float(np.mean(r.accept_rate))}), flush=True)


def prebuild():
    jobs = [(HEADLINE, codes(HEADLINE, c), p) for c in (1, 3, 4, 5, 6) for p in ("f16", "f32")]
    child = ("import importlib, sys, json; sys.path.insert(0, %r); n = importlib.import_module('21cmvae_amd._native'); "
             "d, a, p = json.loads(sys.argv[1]); n.jit_prebuild(d, a, p)" % ROOT)
    procs = [subprocess.Popen([sys.executable, "-c", child, json.dumps(j)]) for j in jobs]
    bad = [j for j, p in zip(jobs, procs) if p.wait() != 0]
    print("prebuilt %d kernels, %d failed %s" % (len(jobs) - len(bad), len(bad), bad))
    return 1 if bad else 0


def against(args):
    """children N P P N P P ...: this build against the other one, and the other one against itself"""
    res = {"N": [], "P1": [], "P2": []}
    base = [sys.executable, os.path.abspath(__file__), "--only-relu-train", "--repeat", str(args.repeat), "--settle", str(args.settle)]
    for _ in range(args.rounds):
        for tag in ("N", "P1", "P2"):
            cmd = base + ([] if tag == "N" else ["--lib", args.against])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("child failed: %s" % out.stderr[-500:])
            res[tag].append(json.loads(out.stdout.strip().splitlines()[-1]))
    keys = [k for k in res["N"][0] if k not in ("what", "lib")]
    for k in keys:
        med = {t: float(np.median([r[k] for r in res[t]])) for t in res}
        allp = [r[k] for t in ("P1", "P2") for r in res[t]]
        print(json.dumps({"what": "relu_per_layer_new_vs_other", "case": k, "rounds": args.rounds, "new_us": med["N"], "other_us": med["P1"],
                          "other_again_us": med["P2"], "new_over_other": med["N"] / med["P1"], "other_over_other": med["P2"] / med["P1"],
                          "other_min_us": min(allp), "other_max_us": max(allp), "new_all_us": [r[k] for r in res["N"]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repeats, a shorter sampler run")
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prebuild", action="store_true")
    ap.add_argument("--only-relu-train", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--against", default=None)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: forward, train, surface")
    args = ap.parse_args()
    args.repeat = args.repeat or (5 if args.quick else 20)
    if args.prebuild:
        raise SystemExit(prebuild())
    nat = pkg("_native")
    if args.lib:
        nat.LIB_PATH = args.lib
    if args.only_relu_train:
        bench_train(nat.Context.default(), args, only_relu=True)
        return
    skip = set(args.skip.split(","))
    ctx = nat.Context.default()
    if "forward" not in skip:
        bench_forward(ctx, args)
    if "train" not in skip:
        bench_train(ctx, args)
    if "surface" not in skip:
        bench_surface(args)
    if args.against:
        against(args)


if __name__ == "__main__":
    main()
