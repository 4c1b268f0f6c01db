"""Throughput of the on-device nested sampler (include/v21.h: v21_mlp_sample_nested_dev) on the headline stack S1 =
7-352-352-352-224-451 with the seeded weights, transforms and spectrum of scripts/bench_sample.py, measured in ONE process
beside the same algorithm driven from numpy over Stack.loglike_fwd: one host round trip per move step.

Rows: 65,536 = 128 runs x 512 live points, and 1,024 = 4 x 256 for the small end.  A call of T iterations at the default
n_repeats = 21 makes 21 T move steps (one evaluation of the n / 2 proposals and one step-kernel launch each) and the two
opening evaluations; the time of the whole call is divided by 21 T.  Device entries on resident buffers, event-timed, 2
untimed calls, then the median of `--repeat` (5); the numpy loop: wall clock of one iteration.  Reported: microseconds
per move step and point-moves/s (n / 2 proposals per step), f16 and f32.  The gate: at 65,536 rows in f16 the device form
is not slower than the numpy-driven loop.  The last line runs the class surface on the shipped model: nested_sample at its
defaults beside sample_tempered at its defaults, both ln Z with their errors.  One JSON line per measurement.

    python scripts/bench_nested.py [--quick] [--repeat 5] [--no-class]

A kernel trace that splits a move step into evaluation and step kernel is a run of its own (no counters in it):

    rocprofv3 --kernel-trace --stats -d profiles/nested -- python scripts/bench_nested.py --quick --no-class
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


def host_nested(st, nat, u0, N, prec, iters, repeats, seed=1):
    """the iteration of csrc/nested_kernels.h in plain numpy, Stack.loglike_fwd once per move step -> seconds per move step"""
    rng = np.random.default_rng(seed)
    n, d = u0.shape
    runs, k = n // N, N // 2
    g = np.float32(2.38 / np.sqrt(2.0 * d))
    lnl_of = lambda v: st.loglike_fwd(np.ascontiguousarray(v.reshape(-1, d)), prec, nat.FWD_OUT_TRANSFORM)
    u = u0.astype(np.float32).reshape(runs, N, d)
    lnl = lnl_of(u).reshape(runs, N)
    e = np.arange(runs)[:, None]
    t0 = time.perf_counter()
    for _ in range(iters):
        order = np.argsort(lnl, axis=1, kind="stable")
        u, lnl = np.take_along_axis(u, order[:, :, None], axis=1), np.take_along_axis(lnl, order, axis=1)
        lstar = lnl[:, k - 1:k].copy()
        c = rng.integers(0, k, size=(runs, k))
        u[:, :k], lnl[:, :k] = u[e, k + c], lnl[e, k + c]
        for _ in range(repeats):
            a = rng.integers(0, k, size=(runs, k))
            b = (a + 1 + rng.integers(0, k - 1, size=(runs, k))) % k
            y = u[:, :k] + g * (u[e, k + a] - u[e, k + b])
            ly = lnl_of(y).reshape(runs, k)
            ok = np.all(np.abs(y) <= 1.0, axis=2) & (ly > lstar)
            u[:, :k] = np.where(ok[:, :, None], y, u[:, :k])
            lnl[:, :k] = np.where(ok, ly, lnl[:, :k])
    return (time.perf_counter() - t0) / (iters * repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and repeats")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-class", action="store_true", help="skip the class surface")
    args = ap.parse_args()
    nat, em = pkg("_native"), pkg("emulator")
    ctx = nat.Context.default()
    st, (Ws, bs, act, tin, tout, data, w), u_true = setup(ctx)
    flags = nat.FWD_OUT_TRANSFORM
    iters, reps = (1 if args.quick else 2), 21
    repeat = 3 if args.quick else args.repeat
    verdict = None
    for n, N in ((65536, 512), (1024, 256)):
        u0 = np.clip(u_true + 0.05 * np.random.default_rng(1).normal(size=(n, 7)), -0.999, 0.999)
        x0 = np.ascontiguousarray(u0.astype(np.float32))
        bufs = {"x": ctx.malloc(x0.nbytes), "live_u": ctx.malloc(x0.nbytes), "accept_rate": ctx.malloc(n // 2 * 8)}
        ctx.h2d(bufs["x"], x0)
        try:
            for prec in ("f16", "f32"):
                run = lambda: st.sample_nested_dev(bufs["x"], 7, n, None, 0, {"live_u": bufs["live_u"], "accept_rate": bufs["accept_rate"]},
                                                   N, prec, flags, n_iter=iters, n_repeats=reps, seed=1)
                ms = timed_dev(ctx, run, 2, repeat)
                acc = np.empty(n // 2)
                ctx.d2h(acc, bufs["accept_rate"])
                steps = iters * reps
                per_step = float(np.median(ms)) * 1e-3 / steps
                host_step = host_nested(st, nat, u0, N, prec, 1, 2 if args.quick else 4)
                rec = {"what": "point_moves_per_s", "stack": "S1", "precision": prec, "rows": n, "n_live": N, "move_steps": steps,
                       "route": st.last_lnl_route()[0], "nested_us_per_step": per_step * 1e6, "nested_per_s": n / 2 / per_step,
                       "nested_spread": float((ms.max() - ms.min()) / np.median(ms)), "accept_rate": float(acc.mean()),
                       "host_loop_us_per_step": host_step * 1e6, "host_loop_per_s": n / 2 / host_step, "over_host_loop": host_step / per_step,
                       "repeats": repeat}
                print(json.dumps(rec), flush=True)
                if n == 65536 and prec == "f16":
                    verdict = {"what": "gate", "rule": "the device form is not slower than the numpy-driven loop at 65,536 rows, f16",
                               "ratio": host_step / per_step, "met": bool(host_step >= per_step)}
        finally:
            for p in bufs.values():
                ctx.free(p)
    print(json.dumps(verdict), flush=True)
    if args.no_class:
        return
    # the class surface on the shipped model: both evidences with their errors
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
        tn, rn = wall(lambda: ae.nested_sample(spec, sigma))
        tt, rt = wall(lambda: ae.sample_tempered(spec, sigma, thin=0))
        print(json.dumps({"what": "class_surface_evidence", "sigma_mK": sigma, "nested_sample_s": tn, "nested_log_evidence": float(rn.log_evidence),
                          "nested_log_evidence_err": float(rn.log_evidence_err), "nested_information": float(rn.information),
                          "nested_iterations": int(rn.n_iter), "nested_evals": int(rn.n_evals), "nested_stopped": rn.stopped,
                          "nested_accept": float(np.mean(rn.accept_rate)), "sample_tempered_s": tt,
                          "tempered_log_evidence": float(rt.log_evidence), "tempered_log_evidence_err": float(rt.log_evidence_err)}), flush=True)


if __name__ == "__main__":
    main()
