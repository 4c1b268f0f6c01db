"""Throughput of the on-device ensemble sampler (include/v21.h: v21_mlp_sample_ensemble_dev) on the headline stack S1 =
7-352-352-352-224-451 with the seeded weights, transforms and spectrum of scripts/bench_sample.py, measured in ONE process
beside

  (b) the Fisher-preconditioned MALA sampler (v21_mlp_sample_dev) on as many rows, and
  (c) a host-driven numpy stretch move over Stack.loglike_fwd: one host round trip per half-move.

Rows: 65,536 walkers = 256 ensembles x 256, and 1,024 = 64 x 16 for the small end.  (a) and (b): device entries on resident
buffers, event-timed, 2 untimed calls, then the median of `--repeat` (5).  (c): wall clock of a few sweeps.  Reported:
walker-updates/s (rows x sweeps / time; for (b) transitions/s) and microseconds per sweep, f16 and f32.  The gate: at
65,536 rows in f16 the ensemble sampler makes at least 4 x the MALA sampler's updates/s.  Per-update cost is not per-sample
efficiency: the last line runs the class surface, sample_ensemble beside sample_posterior on the shipped model, at equal
wall time and reports both r_hat.  One JSON line per measurement.

    python scripts/bench_ensemble.py [--quick] [--repeat 5] [--no-class]

A kernel trace that splits a sweep into evaluation and step kernel is a run of its own (no counters in it):

    rocprofv3 --kernel-trace --stats -d profiles/ensemble -- python scripts/bench_ensemble.py --quick --no-class
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from bench_sample import pkg, setup  # noqa: E402
from bench_temper import timed_dev  # noqa: E402

GATE = 4.0


def host_stretch(st, nat, u0, W, prec, sweeps, a=2.0, seed=1):
    """a plain numpy stretch move driven from the host: Stack.loglike_fwd once per half-move -> seconds per sweep"""
    rng = np.random.default_rng(seed)
    n, d = u0.shape
    H = W // 2
    u = u0.astype(np.float32)
    rows = np.arange(n)
    e, h = rows // W, (rows % W) // H
    sets = [np.flatnonzero(h == hh) for hh in (0, 1)]
    lnl_of = lambda v: st.loglike_fwd(np.ascontiguousarray(v), prec, nat.FWD_OUT_TRANSFORM).astype(np.float64)
    lnl = lnl_of(u)
    t0 = time.perf_counter()
    for _ in range(sweeps):
        for hh, idx in enumerate(sets):
            m = idx.size
            z = ((a - 1.0) * rng.uniform(size=m) + 1.0) ** 2 / a
            pr = e[idx] * W + (1 - hh) * H + rng.integers(0, H, size=m)
            y = (u[pr] + z[:, None] * (u[idx].astype(np.float64) - u[pr])).astype(np.float32)
            inside = np.all(np.abs(y) <= 1.0, axis=1)
            ly = lnl_of(y)
            ok = inside & (np.log(rng.uniform(size=m)) < (d - 1) * np.log(z) + ly - lnl[idx])
            u[idx] = np.where(ok[:, None], y, u[idx])
            lnl[idx] = np.where(ok, ly, lnl[idx])
    return (time.perf_counter() - t0) / sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer sweeps and repeats")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-class", action="store_true", help="skip the class surface at equal wall time")
    args = ap.parse_args()
    nat, em = pkg("_native"), pkg("emulator")
    import fit_ref as fr
    ctx = nat.Context.default()
    st, (Ws, bs, act, tin, tout, data, w), u_true = setup(ctx)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    sweeps = 20 if args.quick else 40
    repeat = 3 if args.quick else args.repeat
    opts = dict(n_steps=sweeps // 2, n_warmup=sweeps // 2, thin=0, seed=1)
    verdict = None
    for n, W in ((65536, 256), (1024, 16)):
        u0 = np.clip(u_true + 0.05 * np.random.default_rng(1).normal(size=(n, 7)), -0.999, 0.999)
        x0 = np.ascontiguousarray(fr.untransform(u0, tin[0], tin[2], tin[3]).astype(np.float32))
        bufs = {"x": ctx.malloc(x0.nbytes), "x_last": ctx.malloc(x0.nbytes), "accept_rate": ctx.malloc(n * 8)}
        ctx.h2d(bufs["x"], x0)
        try:
            for prec in ("f16", "f32"):
                ens = lambda: st.sample_ensemble_dev(bufs["x"], 7, n, None, 0, {"x_last": bufs["x_last"], "accept_rate": bufs["accept_rate"]},
                                                     W, prec, flags, **opts)
                ms = timed_dev(ctx, ens, 2, repeat)
                acc = np.empty(n)
                ctx.d2h(acc, bufs["accept_rate"])
                rate = n * sweeps / (np.median(ms) * 1e-3)
                route = st.last_lnl_route()[0]
                mala = lambda: st.sample_dev(bufs["x"], 7, n, None, 0, {"x_last": bufs["x_last"]}, None, prec, flags, **opts)
                ms8 = timed_dev(ctx, mala, 2, repeat)
                rate8 = n * sweeps / (np.median(ms8) * 1e-3)
                per_sweep = host_stretch(st, nat, u0, W, prec, 2 if args.quick else 4)
                rec = {"what": "walker_updates_per_s", "stack": "S1", "precision": prec, "rows": n, "n_walkers": W, "sweeps": sweeps, "route": route,
                       "ensemble_per_s": rate, "ensemble_us_per_sweep": float(np.median(ms)) * 1e3 / sweeps,
                       "ensemble_spread": float((ms.max() - ms.min()) / np.median(ms)), "accept_rate": float(acc.mean()),
                       "mala_per_s": rate8, "mala_us_per_transition": float(np.median(ms8)) * 1e3 / sweeps, "over_mala": rate / rate8,
                       "host_loop_per_s": n / per_sweep, "host_loop_us_per_sweep": per_sweep * 1e6, "over_host_loop": rate * per_sweep / n,
                       "repeats": repeat}
                print(json.dumps(rec), flush=True)
                if n == 65536 and prec == "f16":
                    verdict = {"what": "gate", "rule": "ensemble updates/s >= %g x MALA transitions/s at 65,536 rows, f16" % GATE,
                               "ratio": rate / rate8, "met": bool(rate >= GATE * rate8)}
        finally:
            for p in bufs.values():
                ctx.free(p)
    print(json.dumps(verdict), flush=True)
    if args.no_class:
        return
    # the class surface on the shipped model at equal wall time: r_hat of both samplers (a finding, not a gate)
    synth, pp = pkg("synth"), pkg("preprocess")
    ds = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = em.AutoEncoderEmulator(**ds)
    ae.load_model()
    truth = pp.par_untransform(np.random.default_rng(4).uniform(-0.6, 0.6, size=(2, 7)), ae.par_train)[1]
    spec = np.asarray(ae.predict(truth[None]), np.float32).reshape(-1)

    def wall(fn):
        fn()
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    for sigma in (1.0, 0.05):
        tp, rp = wall(lambda: ae.sample_posterior(spec, sigma, p0=truth, thin=0))
        probe, _ = wall(lambda: ae.sample_ensemble(spec, sigma, n_steps=200, n_warmup=200, p0=truth, thin=0))
        total = max(4, int(400 * tp / probe))
        te, re_ = wall(lambda: ae.sample_ensemble(spec, sigma, n_steps=total - total // 3, n_warmup=total // 3, p0=truth, thin=0))
        print(json.dumps({"what": "class_surface_equal_wall", "sigma_mK": sigma, "sample_posterior_s": tp, "sample_posterior_chains": 64,
                          "sample_posterior_transitions": 1200, "r_hat_max_posterior": float(np.max(rp.r_hat)),
                          "sample_ensemble_s": te, "sample_ensemble_walkers": "4 x 64", "sample_ensemble_sweeps": total,
                          "r_hat_max_ensemble": float(np.max(re_.r_hat)), "accept_ensemble": float(re_.accept_rate.mean()),
                          "accept_posterior": float(rp.accept_rate.mean())}), flush=True)


if __name__ == "__main__":
    main()
