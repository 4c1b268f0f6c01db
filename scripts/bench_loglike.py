"""Device time of the forward-only log-likelihood (include/v21.h: v21_mlp_loglike_fwd_dev) beside what it replaces and
what bounds it, all in one process on the headline stack S1 = 7-352-352-352-224-451 with seeded weights, both transforms
and device-resident rows:

  lnl_fused       v21_mlp_loglike_fwd_dev on its fused route: chi-square reduced in the fused forward kernel's epilogue;
  lnl_two_launch  the same call on the two-launch route (the fused forward into the likelihood workspace, then the row
                  reduction), taken here because the rows come with a data matrix of 64 rows per spectrum -- every
                  spectrum a copy of the record, so the numbers are the same;
  lnl_old         v21_mlp_loglike_dev with d_grad = NULL: the Jacobian's route (8x the MFMA work, y and J through the
                  236 MB workspace), unchanged in the same library;
  forward         v21_mlp_forward_dev with V21_FWD_NO_SMALL: the fused forward of the same rows, 1,804 bytes per row out.

HIP events around each call, median of 20 after 3 untimed calls; 65,536 and 1,024 rows, f32 and f16.  One JSON line per
(rows, precision) with the two ratios DESIGN.md section 3 K12 quotes: old / fused (gate: >= 4 at 65,536 rows) and
fused / forward (expectation: <= 1.10).

    python scripts/bench_loglike.py [--quick]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

S1 = ([7, 352, 352, 352, 224, 451], [1, 1, 1, 1, 0])
RECORD = []  # the record's data row (setup)


def pkg(sub):
    return importlib.import_module("21cmvae_amd." + sub)


def setup(ctx):
    """the headline stack with seeded weights, the transforms of a synthetic training set, one noisy spectrum as the record"""
    import jacobian_ref as jr
    from helpers import init_weights
    from infer_cases import transforms
    nat = pkg("_native")
    dims, act = S1
    Ws, bs, _ = init_weights(dims, 3)
    tin, tout, _ = transforms(5)
    st = nat.Stack(ctx, dims, act)
    st.set_weights(jr.ora.flatten_params(Ws, bs))
    st.set_input_transform(*tin)
    st.set_output_transform(tout[0], tout[1].astype(np.float32))
    truth = pkg("synth").make_params(1, seed=3, zero_fx_frac=0)
    sig = 0.05 * tout[0]
    data = (jr.jacobian(Ws, bs, act, truth, tin, tout)[0][0] + np.random.default_rng(3).normal(size=dims[-1]) * sig).astype(np.float32)
    RECORD[:] = [data]
    st.set_likelihood(data, np.full(dims[-1], 1.0 / sig ** 2, np.float32))
    return st


def median_ms(ctx, call, repeat=20, warm=3):
    for _ in range(warm):
        call()
    ctx.sync()
    a, b = ctx.event(), ctx.event()
    t = []
    for _ in range(repeat):
        ctx.record(a)
        call()
        ctx.record(b)
        ctx.sync()
        t.append(ctx.elapsed_ms(a, b))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="5 repeats instead of 20")
    args = ap.parse_args()
    rep = 5 if args.quick else 20
    nat = pkg("_native")
    ctx = nat.Context.default()
    st = setup(ctx)
    din, dout = S1[0][0], S1[0][-1]
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    for n in (65536, 1024):
        x = pkg("synth").make_params(n, seed=9).astype(np.float32)
        nd = n // 64
        spectra = np.ascontiguousarray(np.tile(RECORD[0], (nd, 1)))
        dx, dy, dl, dd = ctx.malloc(x.nbytes), ctx.malloc(n * dout * 4), ctx.malloc(n * 4), ctx.malloc(spectra.nbytes)
        ctx.h2d(dx, x)
        ctx.h2d(dd, spectra)
        for prec in ("f32", "f16"):
            row = {"what": "loglike_fwd", "stack": "S1", "rows": n, "precision": prec, "repeats": rep}
            row["forward_ms"] = median_ms(ctx, lambda: st.forward_dev(dx, din, n, dy, dout, prec, flags | nat.FWD_NO_SMALL), rep)
            row["lnl_fused_ms"] = median_ms(ctx, lambda: st.loglike_fwd_dev(dx, din, n, dl, None, 0, prec, flags), rep)
            assert st.last_lnl_route()[0] == "fused"
            fused = np.empty(n, np.float32)
            ctx.d2h(fused, dl)
            row["lnl_old_ms"] = median_ms(ctx, lambda: st.loglike_dev(dx, din, n, dl, None, prec, flags), rep)
            old = np.empty(n, np.float32)
            ctx.d2h(old, dl)
            row["lnl_two_launch_ms"] = median_ms(ctx, lambda: st.loglike_fwd_dev(dx, din, n, dl, dd, nd, prec, flags), rep)
            assert st.last_lnl_route()[0] == "two_launch"
            two = np.empty(n, np.float32)
            ctx.d2h(two, dl)
            row["old_over_fused"] = row["lnl_old_ms"] / row["lnl_fused_ms"]
            row["fused_over_forward"] = row["lnl_fused_ms"] / row["forward_ms"]
            row["old_over_two_launch"] = row["lnl_old_ms"] / row["lnl_two_launch_ms"]
            row["max_rel_diff_fused_vs_old"] = float(np.max(np.abs(fused.astype(np.float64) - old) / np.abs(old)))
            row["two_launch_equals_old_bits"] = bool(np.array_equal(two, old))
            print(json.dumps(row), flush=True)
        for p in (dx, dy, dl, dd):
            ctx.free(p)


if __name__ == "__main__":
    main()
