"""Device time of forward-only ln L (v21_mlp_loglike_fwd_dev) on the run-time instantiated fused kernel ("fused_rt":
Stack.jit_loglike, include/v21.h: v21_mlp_jit_loglike) against the two-launch route a handle that never
asked takes -- the run-time forward into the workspace, then lnl_reduce_kernel -- the routes alternated inside one
process on the SAME weights and record: 65,536 and 1,024 device-resident rows, f32 and f16, of

  7-64-128-451 ReLU and tanh, 7-32-128-256-451 ReLU      the notebooks' stacks
  7-352-352-352-224-451 tanh                             the headline dims as a stack csrc/archs.h does not hold

A SECOND handle on the two-launch route is timed in the same rounds: the ratio of the two is the spread of two-launch
against itself, which the comparison has to exceed to mean anything.  The forward kernel of every two-launch handle is
loaded before anything is timed (Stack.jit).  A kernel that is refused when loaded (scratch memory) is reported as such.

Bytes a call implies: the rows (4 in_dim per row) and 4 bytes of ln L per row on both routes, the record (d, w) once per
128-row workgroup on route 3 and once per row of the reduction on two-launch (cached: not counted), and on two-launch
the out_dim floats per row written by the forward and read back by the reduction.

HIP events around each call.  Before anything is timed the device runs the workload untimed for --settle seconds (clocks
ramp up from idle), then every version is warmed up; a figure is the median of --repeat rounds, each round visiting every
version once.

  --prebuild   compile the run-time kernels this script uses into the library's kernel_cache/ (hiprtc, no GPU) and exit

    python scripts/bench_loglike_rt.py [--quick]
One JSON line per measurement.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from scripts.bench_activations import alternated_ms, settle, weights  # noqa: E402  (one timing loop for these scripts)
from scripts.bench_jacobian_rt import STACKS  # noqa: E402  (the same four stacks)

ROWS = (65536, 1024)


def pkg(sub):
    return importlib.import_module("21cmvae_amd." + sub)


def new_stack(ctx, dims, act):
    st = pkg("_native").Stack(ctx, dims, act)
    st.set_weights(weights(dims, 3))
    k = np.arange(dims[-1])
    st.set_likelihood(np.sin(0.05 * k).astype(np.float32), np.where(k % 6 == 0, 0.0, 25.0).astype(np.float32))
    return st


def bench(ctx, args):
    nat = pkg("_native")
    din, dout = 7, 451
    x = np.random.default_rng(9).uniform(-1, 1, size=(max(ROWS), din)).astype(np.float32)
    dx, dl = ctx.malloc(x.nbytes), ctx.malloc(max(ROWS) * 4)
    ctx.h2d(dx, x)
    for name, dims, act in STACKS:
        for prec in ("f32", "f16"):
            a, b, c = (new_stack(ctx, dims, act) for _ in range(3))   # a asks for its ln L kernel; b and c never do
            for s in (a, b, c):
                assert s.jit(prec, -1) == "ready"   # the forward inside two-launch is the run-time kernel from the first call on
            err = None
            try:
                assert a.jit_loglike(prec, -1) == "ready"
                a.loglike_fwd_dev(dx, din, 1024, dl, None, 0, prec, 0)   # (loads the code object: refused if it needs scratch)
                ctx.sync()
                if a.last_lnl_route()[0] != "fused_rt":
                    err = "the code object was refused when loaded (scratch memory): the handle stays on two_launch"
            except nat.EngineError as e:
                err = str(e)[:200]
            for n in ROWS:
                row = {"what": "loglike_fwd", "stack": name, "rows": n, "precision": prec, "repeats": args.repeat}
                call = lambda s: (lambda: s.loglike_fwd_dev(dx, din, n, dl, None, 0, prec, 0))
                settle(ctx, call(b), args.settle)
                calls = {"two_launch_ms": call(b), "two_launch_again_ms": call(c)}
                if err is None:
                    calls["fused_rt_ms"] = call(a)
                else:
                    row["fused_rt_error"] = err
                row.update(alternated_ms(ctx, calls, args.repeat))
                assert b.last_lnl_route()[0] == c.last_lnl_route()[0] == "two_launch", (b.last_lnl_route(), c.last_lnl_route())
                # (the forward inside two-launch: the run-time kernel, or -- f32, up to V21_SMALL_BATCH_ROWS rows -- the few-row route)
                row["two_launch_forward"] = b.last_route()[0]
                row["two_launch_self_ratio"] = row["two_launch_ms"] / row["two_launch_again_ms"]
                base = n * (4 * din + 4)
                row["two_launch_GBps"] = (base + 2 * 4 * dout * n) / row["two_launch_ms"] * 1e-6
                if err is None:
                    assert a.last_lnl_route()[0] == "fused_rt"
                    row["two_launch_over_fused_rt"] = row["two_launch_ms"] / row["fused_rt_ms"]
                    row["fused_rt_GBps"] = base / row["fused_rt_ms"] * 1e-6
                print(json.dumps(row), flush=True)
    ctx.free(dx)
    ctx.free(dl)


def prebuild():
    jobs = [(d, a, p, k) for _, d, a in STACKS for p in ("f16", "f32") for k in ("jit_prebuild", "jit_prebuild_loglike")]
    child = ("import importlib, sys, json; sys.path.insert(0, %r); n = importlib.import_module('21cmvae_amd._native'); "
             "d, a, p, k = json.loads(sys.argv[1]); getattr(n, k)(d, a, p)" % ROOT)
    procs = [subprocess.Popen([sys.executable, "-c", child, json.dumps(j)]) for j in jobs]
    bad = [j for j, p in zip(jobs, procs) if p.wait() != 0]
    print("prebuilt %d kernels, %d failed %s" % (len(jobs) - len(bad), len(bad), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repeats")
    ap.add_argument("--repeat", type=int, default=0)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--prebuild", action="store_true")
    args = ap.parse_args()
    args.repeat = args.repeat or (5 if args.quick else 20)
    if args.prebuild:
        raise SystemExit(prebuild())
    bench(pkg("_native").Context.default(), args)


if __name__ == "__main__":
    main()
