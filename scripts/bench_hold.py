"""Cost of the samplers' hold record (include/v21.h: v21_mlp_set_hold) on the headline stack S1 = 7-352-352-352-224-451
with the seeded weights, transforms and spectrum of scripts/bench_sample.py: the four on-device samplers at 65,536 rows,
f16 and f32, WITHOUT a record and WITH two columns held (the tau-like column 3 and column 0, at their starts' centre), in
ONE process on resident buffers (the _dev entries, event-timed, 2 untimed calls, then the median of `--repeat`).  The
sizes and units are scripts/bench_prior.py's: transitions/s (MALA: 65,536 chains; tempered: 8,192 ladders of 8 rungs, a
swap event every 5; ensemble: 1,024 ensembles of 64 walkers, walker-moves/s) and microseconds per move step (nested: 128
runs of 512 live points, 21 move steps), and the ratio with / without.

With `--parent-lib PATH` the no-record figures of another build of the library (the parent commit's libv21.so) are
measured in the same session, in a child process that loads it through V21_LIB, and the ratio this build / that build is
reported beside the process-to-process spread of DESIGN K11 (1.2 to 2.2 % in f16); `outside_spread` says when it is not
inside the wider of the two.  One JSON line per measurement.

    python scripts/bench_hold.py [--quick] [--repeat 5] [--parent-lib /path/to/parent/libv21.so]
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
HELD = (0, 3)
SPREAD = 0.022  # the process-to-process spread of DESIGN K11, its upper figure


def measure(ctx, st, nat, u_true, tin, repeat, quick, with_hold):
    """-> {(sampler, precision): (unit, value without a record, value with one or None)}"""
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    u0, x0 = starts(u_true, N, tin)
    x32 = np.ascontiguousarray(x0.astype(np.float32))
    us = np.ascontiguousarray(np.clip(u_true + 0.05 * np.random.default_rng(1).normal(size=(N, 7)), -0.999, 0.999).astype(np.float32))
    mask = np.zeros(7, np.int32)
    mask[list(HELD)] = 1
    hold = (mask, np.where(mask, np.asarray(u_true, np.float64).reshape(-1)[:7], 0.0))
    bufs = {"x": ctx.malloc(x32.nbytes), "u": ctx.malloc(us.nbytes), "out": ctx.malloc(x32.nbytes), "acc": ctx.malloc(N // 2 * 8)}
    ctx.h2d(bufs["x"], x32)
    ctx.h2d(bufs["u"], us)
    steps = 10 if quick else 20
    betas = pkg("emulator").default_betas(8)
    out = {}
    try:
        for prec in ("f16", "f32"):
            runs = {
                "mala": (lambda: st.sample_dev(bufs["x"], 7, N, None, 0, {"x_last": bufs["out"]}, None, prec, flags, n_steps=steps // 2,
                                               n_warmup=steps // 2, thin=0, seed=1), "transitions_per_s", N * steps),
                "tempered": (lambda: st.sample_tempered_dev(bufs["x"], 7, N, None, 0, {"x_last": bufs["out"]}, None, 8, betas, 5, None, prec, flags,
                                                            n_steps=steps // 2, n_warmup=steps // 2, thin=0, seed=1), "transitions_per_s", N * steps),
                "ensemble": (lambda: st.sample_ensemble_dev(bufs["x"], 7, N, None, 0, {"x_last": bufs["out"]}, 64, prec, flags, n_steps=steps // 2,
                                                            n_warmup=steps // 2, thin=0, seed=1), "walker_moves_per_s", N * steps),
                "nested": (lambda: st.sample_nested_dev(bufs["u"], 7, N, None, 0, {"live_u": bufs["out"], "accept_rate": bufs["acc"]}, 512, prec,
                                                        nat.FWD_OUT_TRANSFORM, n_iter=1, n_repeats=21, seed=1), "us_per_move_step", 21),
            }
            for name, (run, unit, work) in runs.items():
                vals = []
                for rec in ((None, hold) if with_hold else (None,)):
                    if rec is not None:
                        st.set_hold(*rec)
                    try:
                        ms = float(np.median(timed_dev(ctx, run, 2, repeat)))
                    finally:
                        if rec is not None:
                            st.set_hold(None)
                    vals.append(ms * 1e3 / work if unit.startswith("us") else work / (ms * 1e-3))
                out[(name, prec)] = (unit, vals[0], vals[1] if with_hold else None)
    finally:
        for p in bufs.values():
            ctx.free(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer transitions and repeats")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="another build of libv21.so to measure the no-record figures of")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    nat = pkg("_native")
    if args.child:
        nat.SIGNATURES.pop("v21_mlp_set_hold", None)  # (the other build need not export it)
    ctx = nat.Context.default()
    st, (Ws, bs, act, tin, tout, data, w), u_true = setup(ctx)
    repeat = 3 if args.quick else args.repeat
    res = measure(ctx, st, nat, u_true, tin, repeat, args.quick, not args.child)
    if args.child:
        print(json.dumps({"%s %s" % k: v[1] for k, v in res.items()}), flush=True)
        return
    parent = {}
    if args.parent_lib:
        env = dict(os.environ, V21_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(args.repeat)] + (["--quick"] if args.quick else [])
        done = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if done.returncode != 0:
            raise SystemExit("the run on %s failed:\n%s" % (args.parent_lib, done.stderr[-2000:]))
        parent = json.loads(done.stdout.strip().splitlines()[-1])
    for (name, prec), (unit, plain, held) in res.items():
        better = (lambda a, b: b / a) if unit.startswith("us") else (lambda a, b: a / b)  # (above 1: the first is faster)
        rec = {"what": "hold_cost", "stack": "S1", "sampler": name, "precision": prec, "rows": N, "held_columns": list(HELD), "unit": unit,
               "no_record": plain, "with_record": held, "with_over_without": 1.0 / better(held, plain), "repeats": repeat}
        key = "%s %s" % (name, prec)
        if key in parent:
            rec["parent_no_record"] = parent[key]
            rec["this_over_parent_speed"] = better(plain, parent[key])
            rec["outside_spread"] = bool(abs(rec["this_over_parent_speed"] - 1.0) > SPREAD)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
