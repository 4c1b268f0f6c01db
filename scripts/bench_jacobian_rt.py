"""Device time of the Jacobian-side calls on the run-time instantiated fused kernel ("fused_rt": Stack.jit_jacobian,
include/v21.h: v21_mlp_jit_jacobian) against the generic kernel, the two routes alternated inside one process on the SAME
weights: 65,536 device-resident rows, f32 and f16, of

  7-64-128-451 ReLU and tanh, 7-32-128-256-451 ReLU      the notebooks' stacks
  7-352-352-352-224-451 tanh                             the headline dims as a stack csrc/archs.h does not hold

for the Jacobian (v21_mlp_jacobian_dev), ln L + gradient (v21_mlp_loglike_dev) and the Fisher matrix with ln L and gradient
(v21_mlp_fisher_dev); and the headline ReLU stack (S1) on its run-time kernel (V21_FWD_FORCE_JIT) against its compiled one
-- the same template, ~1.0x by construction.  A kernel that is refused when loaded (scratch memory) is reported as such.

HIP events around each call.  Before anything is timed the device runs the workload untimed for --settle seconds (clocks
ramp up from idle), then every version is warmed up; a figure is the median of --repeat rounds, each round visiting every
version once.

  --prebuild   compile the run-time kernels this script uses into the library's kernel_cache/ (hiprtc, no GPU) and exit

    python scripts/bench_jacobian_rt.py [--quick]
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

from scripts.bench_activations import alternated_ms, settle, weights  # noqa: E402  (one timing loop for both scripts)

HEADLINE = [7, 352, 352, 352, 224, 451]
STACKS = [
    ("7-64-128-451 relu", [7, 64, 128, 451], [1, 1, 0]),
    ("7-64-128-451 tanh", [7, 64, 128, 451], [3, 3, 0]),
    ("7-32-128-256-451 relu", [7, 32, 128, 256, 451], [1, 1, 1, 0]),
    ("headline tanh", HEADLINE, [3, 3, 3, 3, 0]),
]
S1 = ("S1 relu (archs.h)", HEADLINE, [1, 1, 1, 1, 0])
ROWS = 65536


def pkg(sub):
    return importlib.import_module("21cmvae_amd." + sub)


def new_stack(ctx, dims, act):
    nat = pkg("_native")
    st = nat.Stack(ctx, dims, act)
    st.set_weights(weights(dims, 3))
    k = np.arange(dims[-1])
    st.set_likelihood(np.sin(0.05 * k).astype(np.float32), np.where(k % 6 == 0, 0.0, 25.0).astype(np.float32))
    return st


def bench(ctx, args):
    nat = pkg("_native")
    n, din, dout = ROWS, 7, 451
    x = np.random.default_rng(9).uniform(-1, 1, size=(n, din)).astype(np.float32)
    dx = ctx.malloc(x.nbytes)
    ctx.h2d(dx, x)
    dy, dj = ctx.malloc(n * dout * 4), ctx.malloc(n * din * dout * 4)
    dl, dg, dF = ctx.malloc(n * 4), ctx.malloc(n * din * 4), ctx.malloc(n * din * din * 4)

    def calls_of(st, prec, flags):
        return {"jacobian": lambda: st.jacobian_dev(dx, din, n, dy, dout, dj, prec, flags),
                "loglike_grad": lambda: st.loglike_dev(dx, din, n, dl, dg, prec, flags),
                "fisher": lambda: st.fisher_dev(dx, din, n, dF, dl, dg, prec, flags)}

    for name, dims, act in STACKS + [S1]:
        compiled = name == S1[0]
        for prec in ("f32", "f16"):
            a, b = new_stack(ctx, dims, act), new_stack(ctx, dims, act)   # a asks for its kernel, b never does
            row = {"what": "jacobian_side", "stack": name, "rows": n, "precision": prec, "repeats": args.repeat,
                   "other_route": "fused" if compiled else "generic"}
            fa = nat.FWD_FORCE_JIT if compiled else 0
            try:
                if not compiled:
                    assert a.jit_jacobian(prec, -1) == "ready"
                a.jacobian_dev(dx, din, n, dy, dout, dj, prec, fa)   # (loads the code object: refused if it needs scratch)
                ctx.sync()
                ready = a.last_jac_route()[0] == "fused_rt"
                if not ready:
                    row["fused_rt_error"] = "the code object was refused when loaded (scratch memory): the handle stays on generic"
            except nat.EngineError as e:
                ready, row["fused_rt_error"] = False, str(e)[:200]
            other = calls_of(b, prec, 0)
            settle(ctx, other["loglike_grad"], args.settle)
            calls = {k + "_other_ms": c for k, c in other.items()}
            if ready:
                calls.update({k + "_fused_rt_ms": c for k, c in calls_of(a, prec, fa).items()})
            row.update(alternated_ms(ctx, calls, args.repeat))
            assert b.last_jac_route()[0] == row["other_route"], b.last_jac_route()
            if ready:
                assert a.last_jac_route()[0] == "fused_rt"
                for k in ("jacobian", "loglike_grad", "fisher"):
                    row[k + "_other_over_fused_rt"] = row[k + "_other_ms"] / row[k + "_fused_rt_ms"]
            print(json.dumps(row), flush=True)
    for p in (dx, dy, dj, dl, dg, dF):
        ctx.free(p)


def prebuild():
    jobs = [(d, a, p) for _, d, a in STACKS + [S1] for p in ("f16", "f32")]
    child = ("import importlib, sys, json; sys.path.insert(0, %r); n = importlib.import_module('21cmvae_amd._native'); "
             "d, a, p = json.loads(sys.argv[1]); n.jit_prebuild_jacobian(d, a, p)" % ROOT)
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
