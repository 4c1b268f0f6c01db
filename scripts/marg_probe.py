"""Cost of marginalising K linear foreground modes (csrc/nuisance_kernels.h, csrc/api_nuisance.hip): one JSON line.

The set-up of scripts/fit_probe.py (the headline stack S1, seeded weights, both transforms, 65,536 device-resident rows,
the context's stream, HIP events); with K > 0 the data carry a 5-term LinLog foreground of ~2e6 at 75 MHz:
  * Fisher + ln L + gradient (v21_mlp_fisher_dev), f32 and f16, K = 0 (no nuisance record), 5 and 8: median and minimum of
    20 launches after 3 of warm-up;
  * a 50-iteration fit (v21_mlp_fit_dev, max_iter 50, 8,192 spectra x 8 starts, data matrix projected once per call) and
    one transition of 65,536 chains (v21_mlp_sample_dev, n_steps 1), K = 0 and 5: median of 3 calls after 1 of warm-up.
A library without the nuisance entry points (an earlier build, V21_LIB=...) reports its K = 0 figures only: run the
script on both builds on the same machine to compare.  --fisher-only: the Fisher evaluations alone, 5 launches each (short
enough to run under `rocprofv3 --kernel-trace --stats`, which splits them into the Jacobian kernel and the reduction)."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
nat = importlib.import_module("21cmvae_amd._native")
synth = importlib.import_module("21cmvae_amd.synth")
pp = importlib.import_module("21cmvae_amd.preprocess")
fg = importlib.import_module("21cmvae_amd.foregrounds")
from oracle import ref_numpy as ora  # noqa: E402

N, STARTS, WARM, TIMED = 65536, 8, 3, 20
DIMS, ACT = [7, 352, 352, 352, 224, 451], [1, 1, 1, 1, 0]
NU = np.linspace(50.0, 200.0, 451)


def main():
    import ctypes as C
    has_nuisance = hasattr(C.CDLL(nat.LIB_PATH), "v21_mlp_set_nuisance")
    if not has_nuisance:  # an earlier build: bind what it exports
        for k in [k for k in nat.SIGNATURES if "nuisance" in k]:
            del nat.SIGNATURES[k]
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
    sigma = 0.01 * std
    truths = pp.par_untransform(rng.uniform(-0.9, 0.9, size=(m, 7)), par_train)
    A5 = fg.linlog_basis(NU, 5)
    a = np.array([2e6 * (75.0 / np.sqrt(NU[0] * NU[-1])) ** 2.5, 1e5, -3e4, 1e4, 2e3])
    clean = st.forward(truths, "f32", flags).astype(np.float64) + rng.normal(size=(m, 451)) * sigma
    plain, data = clean.astype(np.float32), (clean + a @ A5).astype(np.float32)  # K = 0 fits the spectra without the foreground
    w = np.full(451, 1.0 / sigma ** 2, np.float32)
    u0 = np.vstack([np.zeros((1, 7)), rng.uniform(-1, 1, size=(STARTS - 1, 7))])
    x0 = np.tile(pp.par_untransform(u0, par_train), (m, 1)).astype(np.float32)
    x = synth.make_params(N, seed=4).astype(np.float32)
    dx, dx0, dd, dp = ctx.malloc(x.nbytes), ctx.malloc(x0.nbytes), ctx.malloc(data.nbytes), ctx.malloc(plain.nbytes)
    dF, dl, dg = ctx.malloc(N * 49 * 4), ctx.malloc(N * 4), ctx.malloc(N * 7 * 4)
    dxh, dl0, ds = ctx.malloc(x0.nbytes), ctx.malloc(N * 4), ctx.malloc(N * 4)
    ctx.h2d(dx, x)
    ctx.h2d(dx0, x0)
    ctx.h2d(dd, data)
    ctx.h2d(dp, plain)
    out = {"rows": N, "stack": "S1", "nuisance_entry_points": has_nuisance}
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
        return round(float(np.median(ts)), 1), round(float(np.min(ts)), 1)

    quick = "--fisher-only" in sys.argv
    for K in ((0, 5, 8) if has_nuisance else (0,)):
        st.set_likelihood(data[0] if K else plain[0], w)
        dk = dd if K else dp
        if K:
            st.set_nuisance(fg.linlog_basis(NU, K))
        for prec in ("f32", "f16"):
            out["fisher_lnl_grad_K%d_%s_us" % (K, prec)] = timed(lambda: st.fisher_dev(dx, 7, N, dF, dl, dg, prec, flags), WARM, 5 if quick else TIMED)
            if K in (0, 5) and not quick:
                out["fit50_K%d_%s_us" % (K, prec)] = timed(lambda: st.fit_dev(dx0, 7, N, dk, m, dxh, dl, dl0, None, ds, prec, flags, max_iter=50), 1, 3)
                so = {"x_last": dxh, "lnl_last": dl}
                out["transition_K%d_%s_us" % (K, prec)] = timed(lambda: st.sample_dev(dx0, 7, N, dk, m, so, None, prec, flags, n_steps=1, n_warmup=0), 1, 3)
    st.set_likelihood(None, None)
    for p in (dx, dx0, dd, dp, dF, dl, dg, dxh, dl0, ds):
        ctx.free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
