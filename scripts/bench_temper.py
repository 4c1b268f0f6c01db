"""Throughput of the parallel-tempered sampler (include/v21.h: v21_mlp_sample_tempered_dev) beside the plain sampler
(v21_mlp_sample_dev) at the same number of rows, on the headline stack S1 = 7-352-352-352-224-451 with the seeded weights,
transforms and spectrum of scripts/bench_sample.py.

  plain      65,536 independent chains;
  tempered   8,192 ladders of 8 rungs (emulator.default_betas(8)) = 65,536 rows, swap_every 1 and 5.

Device entries on resident buffers, event timing, warm-up launches before every timed run, `--repeat` timed runs per
configuration: reported are the median transitions/s (rows x transitions / time), the spread of the repeats ((max - min) /
median) and the ratio to the plain sampler of the same precision.  Then the wall time of the class surface at its
defaults, AutoEncoderEmulator.sample_tempered (16 ladders x 8 rungs x (200 + 1,000) transitions) beside
sample_posterior (64 chains).  One JSON line per measurement.

    python scripts/bench_temper.py [--quick] [--repeat 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from bench_sample import pkg, setup, starts  # noqa: E402


def timed_dev(ctx, run, warmup, repeat):
    """event-timed milliseconds of `repeat` calls of run() on the context's stream, after `warmup` untimed ones"""
    for _ in range(warmup):
        run()
    ctx.sync()
    out = []
    e0, e1 = ctx.event(), ctx.event()
    try:
        for _ in range(repeat):
            ctx.record(e0)
            run()
            ctx.record(e1)
            ctx.sync()
            out.append(ctx.elapsed_ms(e0, e1))
    finally:
        ctx.lib.v21_event_destroy(ctx.h, e0)
        ctx.lib.v21_event_destroy(ctx.h, e1)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer transitions and repeats")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-class", action="store_true", help="skip the class-surface wall times")
    args = ap.parse_args()
    nat, em = pkg("_native"), pkg("emulator")
    ctx = nat.Context.default()
    st, (Ws, bs, act, tin, tout, data, w), u_true = setup(ctx)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    T, ladders = 8, 8192
    n = T * ladders
    betas = em.default_betas(T)
    steps = 20 if args.quick else 40
    repeat = 3 if args.quick else args.repeat
    opts = dict(n_steps=steps // 2, n_warmup=steps // 2, thin=0, seed=1)
    # every rung of a ladder from its ladder's start, as the class surface does
    _, x_lad = starts(u_true, ladders, tin)
    x0 = np.ascontiguousarray(np.repeat(x_lad, T, axis=0).astype(np.float32))
    bufs = {"x": ctx.malloc(x0.nbytes), "x_last": ctx.malloc(x0.nbytes), "mean_lnl": ctx.malloc(n * 8), "swap_accept": ctx.malloc(n * 8)}
    ctx.h2d(bufs["x"], x0)
    try:
        for prec in ("f16", "f32"):
            plain = lambda: st.sample_dev(bufs["x"], 7, n, None, 0, {"x_last": bufs["x_last"]}, None, prec, flags, **opts)
            ms = timed_dev(ctx, plain, 2, repeat)
            base = n * steps / (np.median(ms) * 1e-3)
            print(json.dumps({"what": "transitions_per_s", "sampler": "plain", "stack": "S1", "precision": prec, "rows": n, "transitions": steps,
                              "per_s": base, "ms_median": float(np.median(ms)), "spread": float((ms.max() - ms.min()) / np.median(ms)),
                              "repeats": repeat}), flush=True)
            for swap_every in (1, 5):
                run = lambda: st.sample_tempered_dev(bufs["x"], 7, n, None, 0, {"x_last": bufs["x_last"]},
                                                     {"mean_lnl": bufs["mean_lnl"], "swap_accept": bufs["swap_accept"]}, T, betas, swap_every,
                                                     None, prec, flags, **opts)
                ms = timed_dev(ctx, run, 2, repeat)
                sw = np.empty(n)
                ctx.d2h(sw, bufs["swap_accept"])
                rate = n * steps / (np.median(ms) * 1e-3)
                print(json.dumps({"what": "transitions_per_s", "sampler": "tempered", "stack": "S1", "precision": prec, "rows": n, "ladders": ladders,
                                  "rungs": T, "swap_every": swap_every, "transitions": steps, "per_s": rate, "ms_median": float(np.median(ms)),
                                  "spread": float((ms.max() - ms.min()) / np.median(ms)), "repeats": repeat, "over_plain": rate / base,
                                  "swap_rate": [float(v) for v in sw.reshape(ladders, T).mean(axis=0)[:T - 1].round(3)]}), flush=True)
    finally:
        for p in bufs.values():
            ctx.free(p)
    if args.no_class:
        return
    # the class surface at its defaults, beside sample_posterior's
    synth, pp = pkg("synth"), pkg("preprocess")
    ds = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = em.AutoEncoderEmulator(**ds)
    ae.load_model()
    truth = pp.par_untransform(np.random.default_rng(4).uniform(-0.6, 0.6, size=(1, 7)), ae.par_train)
    spec = np.asarray(ae.predict(truth), np.float32).reshape(-1)

    def wall(fn):
        fn()
        best = np.inf
        for _ in range(2):
            t = time.perf_counter()
            r = fn()
            best = min(best, time.perf_counter() - t)
        return best, r

    tp, rp = wall(lambda: ae.sample_posterior(spec, 1.0, p0=truth[0]))
    tt, rt = wall(lambda: ae.sample_tempered(spec, 1.0, p0=truth[0]))
    print(json.dumps({"what": "class_surface_wall_s", "sample_posterior": tp, "sample_posterior_chains": 64, "sample_tempered": tt,
                      "sample_tempered_rows": 16 * 8, "transitions": 1200, "log_evidence": float(rt.log_evidence),
                      "log_evidence_err": float(rt.log_evidence_err), "swap_rate": [float(v) for v in rt.swap_rate.round(3)],
                      "r_hat_max_tempered": float(np.max(rt.r_hat)), "r_hat_max_posterior": float(np.max(rp.r_hat))}), flush=True)


if __name__ == "__main__":
    main()
