"""Cost of the MAP fit (include/v21.h: v21_mlp_fit_map) on the headline stack S1 = 7-352-352-352-224-451 with the seeded
weights, transforms and spectrum of scripts/bench_sample.py: 65,536 start rows, f16 and f32, in ONE process on resident
buffers (the _dev entries, event-timed, 2 untimed calls, then the median of `--repeat`).  A call runs `--iters` LM
iterations (max_iter, with check_every above it: the host never reads the running-row count), so that
time / (max_iter + 1) is the time of one iteration: one Fisher evaluation and one fit_lm_kernel launch.  Reported per
precision: microseconds per LM iteration of v21_mlp_fit_dev, of v21_mlp_fit_map_dev without a prior and holds (the same
arithmetic through fit_lm_kernel<true>) and of v21_mlp_fit_map_dev with a two-column record and two held columns, and
the ratios over v21_mlp_fit_dev.

With `--parent-lib PATH` v21_mlp_fit_dev of another build of the library (the parent commit's libv21.so) is measured in
the same session, in a child process that loads it through V21_LIB, and the ratio this build / that build is reported
beside the process-to-process spread of DESIGN K11 (1.2 to 2.2 % in f16).  One JSON line per measurement.

    python scripts/bench_map.py [--quick] [--repeat 5] [--iters 8] [--parent-lib /path/to/parent/libv21.so]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from bench_sample import pkg, setup, starts  # noqa: E402
from bench_temper import timed_dev  # noqa: E402

N = 65536
PRIOR = (np.array([1, 0, 0, 1, 0, 0, 0], np.int32), np.array([-1.4, 0, 0, 0.2, 0, 0, 0.0]), np.array([0.2, 1, 1, 0.1, 1, 1, 1.0]))
HOLD = [0, 0, 1, 0, 0, 1, 0]
NEW_SYMBOLS = ("v21_mlp_fit_map", "v21_mlp_fit_map_dev")


def measure(ctx, st, nat, u_true, tin, repeat, iters, with_map):
    """-> {precision: {entry: microseconds per LM iteration}}"""
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    _, x0 = starts(u_true, N, tin)
    x32 = np.ascontiguousarray(x0.astype(np.float32))
    bufs = {"x": ctx.malloc(x32.nbytes), "xh": ctx.malloc(x32.nbytes), "lnl": ctx.malloc(N * 4), "lap": ctx.malloc(N * 8)}
    ctx.h2d(bufs["x"], x32)
    opts = dict(max_iter=iters, check_every=iters + 1)
    out = {}
    try:
        for prec in ("f16", "f32"):
            runs = {"fit_dev": (lambda: st.fit_dev(bufs["x"], 7, N, None, 0, bufs["xh"], bufs["lnl"], None, None, None, prec, flags, **opts), None)}
            if with_map:
                runs["fit_map_dev_plain"] = (lambda: st.fit_map_dev(bufs["x"], 7, N, None, 0, bufs["xh"], bufs["lnl"], precision=prec, flags=flags,
                                                                    **opts), None)
                runs["fit_map_dev_prior_2_held"] = (lambda: st.fit_map_dev(bufs["x"], 7, N, None, 0, bufs["xh"], bufs["lnl"], out={"laplace": bufs["lap"]},
                                                                           use_prior=True, hold=HOLD, precision=prec, flags=flags, **opts), PRIOR)
            out[prec] = {}
            for name, (run, rec) in runs.items():
                if rec is not None:
                    st.set_prior(*rec)
                try:
                    ms = float(np.median(timed_dev(ctx, run, 2, repeat)))
                finally:
                    if rec is not None:
                        st.set_prior(None)
                out[prec][name] = ms * 1e3 / (iters + 1)
    finally:
        for p in bufs.values():
            ctx.free(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8, help="LM iterations per call (max_iter)")
    ap.add_argument("--parent-lib", default=None, help="another build of libv21.so to measure v21_mlp_fit_dev of")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    nat = pkg("_native")
    if args.child:
        for name in NEW_SYMBOLS:  # (the other build need not export them)
            nat.SIGNATURES.pop(name, None)
    ctx = nat.Context.default()
    st, (_, _, _, tin, _, _, _), u_true = setup(ctx)
    repeat = 3 if args.quick else args.repeat
    res = measure(ctx, st, nat, u_true, tin, repeat, args.iters, not args.child)
    if args.child:
        print(json.dumps({p: v["fit_dev"] for p, v in res.items()}), flush=True)
        return
    parent = {}
    if args.parent_lib:
        env = dict(os.environ, V21_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(args.repeat), "--iters", str(args.iters)]
        done = subprocess.run(cmd + (["--quick"] if args.quick else []), env=env, capture_output=True, text=True)
        if done.returncode != 0:
            raise SystemExit("the run on %s failed:\n%s" % (args.parent_lib, done.stderr[-2000:]))
        parent = json.loads(done.stdout.strip().splitlines()[-1])
    for prec, v in res.items():
        rec = {"what": "map_fit_cost", "stack": "S1", "precision": prec, "rows": N, "lm_iterations": args.iters + 1, "unit": "us_per_lm_iteration",
               "repeats": repeat}
        rec.update(v)
        rec["map_plain_over_fit"] = v["fit_map_dev_plain"] / v["fit_dev"]
        rec["map_prior_2_held_over_fit"] = v["fit_map_dev_prior_2_held"] / v["fit_dev"]
        if prec in parent:
            rec["parent_fit_dev"] = parent[prec]
            rec["this_over_parent_time"] = v["fit_dev"] / parent[prec]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
