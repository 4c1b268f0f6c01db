"""Parameter Jacobian / log-likelihood throughput (csrc/fused_jac.h): one JSON line.

Kernel time by events (20 timed launches after 3 of warm-up, device-resident rows and results, the context's stream) of
the headline stack S1 (7 -> [352, 352, 352, 224] -> 451) at 65,536 rows, f32 and f16, in Jacobian mode
(v21_mlp_jacobian_dev: y + 7 x 451 floats per row) and in likelihood mode (v21_mlp_loglike_dev: 8 floats per row), with
both transforms; Jacobians / s and the fraction of the MFMA peak (the kernel runs 8 virtual rows per parameter row:
8 x 860 kFLOP; dense peaks of the MI355X: 2.5 PFLOP/s f16, 157 TFLOP/s f32); and the host surface for ONE parameter
vector (Stack.jacobian / Stack.loglike: median of 200 calls; --no-host leaves that out, for profiler runs)."""
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

N, WARM, TIMED = 65536, 3, 20
DIMS, ACT = [7, 352, 352, 352, 224, 451], [1, 1, 1, 1, 0]
FLOP_ROW = 2 * sum(a * b for a, b in zip(DIMS[:-1], DIMS[1:]))
PEAK = {"f16": 2.5e15, "f32": 1.57e14}


def main():
    ctx = nat.Context.default()
    Ws, bs = ora.init_mlp(DIMS, seed=0)
    st = nat.Stack(ctx, DIMS, ACT)
    st.set_weights(ora.flatten_params(Ws, bs))
    par_train = synth.make_params(5000, seed=1, corners=True)
    ps = pp.ParamStats(par_train)
    st.set_input_transform(ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
    sig = synth.make_signals(2000, seed=2)
    st.set_output_transform(float(np.std(sig)), np.mean(sig, axis=0).astype(np.float32))
    st.set_likelihood(sig[0].astype(np.float32), np.full(451, 1e2, np.float32))
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    x = synth.make_params(N, seed=3).astype(np.float32)
    dx, dy = ctx.malloc(x.nbytes), ctx.malloc(N * 451 * 4)
    dj, dl, dg = ctx.malloc(N * 7 * 451 * 4), ctx.malloc(N * 4), ctx.malloc(N * 7 * 4)
    ctx.h2d(dx, x)
    out = {"rows": N, "stack": "S1", "flop_per_jacobian": 8 * FLOP_ROW}
    e0, e1 = ctx.event(), ctx.event()
    for prec in ("f32", "f16"):
        for mode in ("jac", "lnl"):
            def launch():
                if mode == "jac":
                    st.jacobian_dev(dx, 7, N, dy, 451, dj, prec, flags)
                else:
                    st.loglike_dev(dx, 7, N, dl, dg, prec, flags)
            for _ in range(WARM):
                launch()
            ctx.sync()
            ts = []
            for _ in range(TIMED):
                ctx.record(e0)
                launch()
                ctx.record(e1)
                ctx.sync()
                ts.append(ctx.elapsed_ms(e0, e1) * 1e3)
            us = float(np.median(ts))
            rate = N / (us * 1e-6)
            key = "%s_%s" % (mode, prec)
            out[key + "_us"] = round(us, 1)
            out[key + "_us_min"] = round(float(np.min(ts)), 1)
            out[key + "_per_s"] = float("%.3g" % rate)
            out[key + "_peak_frac"] = round(rate * 8 * FLOP_ROW / PEAK[prec], 4)
            out[key + "_route"] = st.last_jac_route()[0]
    x1 = x[:1].astype(np.float64)
    for prec in (() if "--no-host" in sys.argv else ("f32", "f16")):
        for mode in ("jac", "lnl"):
            f = (lambda: st.jacobian(x1, prec, flags)) if mode == "jac" else (lambda: st.loglike(x1, prec, flags))
            for _ in range(10):
                f()
            ts = []
            for _ in range(200):
                t0 = time.perf_counter()
                f()
                ts.append((time.perf_counter() - t0) * 1e6)
            out["host_one_vector_%s_%s_us" % (mode, prec)] = round(float(np.median(ts)), 1)
    for p in (dx, dy, dj, dl, dg):
        ctx.free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
