"""Fisher-matrix and fit throughput (csrc/fit_kernels.h, csrc/api_fit.hip): one JSON line.

The headline stack S1 (7 -> [352, 352, 352, 224] -> 451, seeded initial weights and N(0, 0.05) biases -- with zero
biases the 16-bit network is flat at the box centre, every row started there reports status 3 -- both transforms) at 65,536 rows, f32
and f16, device-resident rows and results, the context's stream, HIP events:
  * Fisher matrices / s: v21_mlp_fisher_dev, F only and F + ln L + gradient (median of 20 launches after 3 of warm-up);
  * fits / s: v21_mlp_fit_dev of 65,536 (spectrum, start) rows -- 8,192 noisy spectra of truths drawn in the training
    box x 8 starts (box centre + 7 uniform points) -- with the default options (max_iter 50, check_every 8), the Fisher
    matrix at x_hat included (median of 3 calls after 1 of warm-up);
  * iterations: proposals evaluated per row before it stopped (the first max_iter whose status is not 0, by a sweep of
    max_iter over 0 .. 50 on the first 8,192 rows; 50 for rows that never stop), mean and the status counts at 50.
--cpu: scipy.optimize.least_squares (trf, bounds = the box, analytic float64 Jacobian) on the same rows, 16 fits."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
nat = importlib.import_module("21cmvae_amd._native")
synth = importlib.import_module("21cmvae_amd.synth")
pp = importlib.import_module("21cmvae_amd.preprocess")
from oracle import ref_numpy as ora  # noqa: E402

N, STARTS, WARM, TIMED = 65536, 8, 3, 20
DIMS, ACT = [7, 352, 352, 352, 224, 451], [1, 1, 1, 1, 0]


def forward64(Ws, bs, u):
    h = u
    for l, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ W + b
        if ACT[l]:
            h = np.maximum(h, 0)
    return h


def main():
    ctx = nat.Context.default()
    Ws, bs = ora.init_mlp(DIMS, seed=0)
    brng = np.random.default_rng(1000)
    bs = [brng.normal(scale=0.05, size=b.shape).astype(np.float32) for b in bs]
    st = nat.Stack(ctx, DIMS, ACT)
    st.set_weights(ora.flatten_params(Ws, bs))
    par_train = synth.make_params(5000, seed=1, corners=True)
    ps = pp.ParamStats(par_train)
    st.set_input_transform(ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
    sig = synth.make_signals(2000, seed=2)
    std, mean = float(np.std(sig)), np.mean(sig, axis=0).astype(np.float32)
    st.set_output_transform(std, mean)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    rng = np.random.default_rng(3)
    m = N // STARTS
    u_true = rng.uniform(-0.9, 0.9, size=(m, 7))
    sigma = 0.01 * std
    W64 = [np.asarray(W, np.float64) for W in Ws]
    b64 = [np.asarray(b, np.float64) for b in bs]
    data = (forward64(W64, b64, u_true) * std + mean + rng.normal(size=(m, 451)) * sigma).astype(np.float32)
    w = np.full(451, 1.0 / sigma ** 2, np.float32)
    st.set_likelihood(data[0], w)
    u0 = np.vstack([np.zeros((1, 7)), rng.uniform(-1, 1, size=(STARTS - 1, 7))])
    x0 = np.tile(pp.par_untransform(u0, par_train), (m, 1)).astype(np.float32)
    x = synth.make_params(N, seed=4).astype(np.float32)
    dx, dx0, dd = ctx.malloc(x.nbytes), ctx.malloc(x0.nbytes), ctx.malloc(data.nbytes)
    dF, dl, dg = ctx.malloc(N * 49 * 4), ctx.malloc(N * 4), ctx.malloc(N * 7 * 4)
    dxh, dl0, ds = ctx.malloc(x0.nbytes), ctx.malloc(N * 4), ctx.malloc(N * 4)
    ctx.h2d(dx, x)
    ctx.h2d(dx0, x0)
    ctx.h2d(dd, data)
    out = {"rows": N, "stack": "S1", "starts_per_spectrum": STARTS, "sigma_over_std": 0.01}
    e0, e1 = ctx.event(), ctx.event()

    def timed(launch, warm, reps):
        for _ in range(warm):
            launch()
        ctx.sync()
        ts = []
        for _ in range(reps):
            ctx.record(e0)
            launch()
            ctx.record(e1)
            ctx.sync()
            ts.append(ctx.elapsed_ms(e0, e1) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    for prec in ("f32", "f16"):
        for mode in ("F", "F_lnl_grad"):
            like = mode != "F"
            us, mn = timed(lambda: st.fisher_dev(dx, 7, N, dF, dl if like else None, dg if like else None, prec, flags), WARM, TIMED)
            out["fisher_%s_%s_us" % (mode, prec)] = round(us, 1)
            out["fisher_%s_%s_per_s" % (mode, prec)] = float("%.3g" % (N / (us * 1e-6)))
        out["fisher_%s_route" % prec] = st.last_jac_route()[0]
        us, mn = timed(lambda: st.fit_dev(dx0, 7, N, dd, m, dxh, dl, dl0, dF, ds, prec, flags), 1, 3)
        out["fit_%s_ms" % prec] = round(us * 1e-3, 2)
        out["fit_%s_per_s" % prec] = float("%.3g" % (N / (us * 1e-6)))
        status = np.empty(N, np.int32)
        ctx.d2h(status, ds)
        out["fit_%s_status_counts" % prec] = {str(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))}
        lnl, l0 = np.empty(N, np.float32), np.empty(N, np.float32)
        ctx.d2h(lnl, dl)
        ctx.d2h(l0, dl0)
        best = lnl.reshape(m, STARTS).max(axis=1)
        out["fit_%s_best_chi2_per_bin_median" % prec] = round(float(np.median(-2 * best / 451)), 3)
        # iterations per row on the first 8,192 rows: sweep max_iter
        ns = 8192
        iters = np.full(ns, 50)
        done = np.zeros(ns, bool)
        for k in range(51):
            st.fit_dev(dx0, 7, ns, dd, ns // STARTS, dxh, dl, None, None, ds, prec, flags, max_iter=k)
            s = np.empty(ns, np.int32)
            ctx.sync()
            ctx.d2h(s, ds)
            new = (s != 0) & ~done
            iters[new] = k
            done |= s != 0
        out["fit_%s_mean_iterations" % prec] = round(float(iters.mean()), 2)
    if "--cpu" in sys.argv:
        from scipy.optimize import least_squares
        nfit = 16
        u0c = pp.par_transform(x0[:nfit].astype(np.float64), par_train)

        def jac_of(u):
            h, T = u[None, :], np.eye(7)
            for l, (W, b) in enumerate(zip(W64, b64)):
                z = h @ W + b
                T = T @ W
                if ACT[l]:
                    msk = z > 0
                    h, T = np.where(msk, z, 0), T * msk
                else:
                    h = z
            return h[0], T
        t0 = time.perf_counter()
        for i in range(nfit):
            d = data[i // STARTS].astype(np.float64)
            least_squares(lambda u: (jac_of(u)[0] * std + mean - d) / sigma, u0c[i], jac=lambda u: jac_of(u)[1].T * std / sigma,
                          bounds=(-1.0, 1.0), method="trf")
        out["cpu_scipy_fits_per_s"] = float("%.3g" % (nfit / (time.perf_counter() - t0)))
    for p in (dx, dx0, dd, dF, dl, dg, dxh, dl0, ds):
        ctx.free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
