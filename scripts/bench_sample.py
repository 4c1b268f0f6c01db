"""Throughput of the on-device posterior sampler (include/v21.h: v21_mlp_sample) beside two baselines:

  device    Stack.sample: the chain state stays on the device, the host only launches;
  python    the same algorithm (tests/sample_ref.py) driven from Python over the public Stack.fisher, one host call and one
            round trip of (ln L, gradient, Fisher matrix) per transition -- what a user had before the sampler existed;
  cpu       tests/sample_ref.py on its own float64 numpy evaluator.

Reported: transitions/s (chains x transitions / wall time, warm-up included, after one untimed call) on the headline stack
S1 = 7-352-352-352-224-451 per chain count and precision, and the wall time of the single-spectrum case a user runs,
64 chains x (200 + 1,000) transitions through AutoEncoderEmulator.sample_posterior.  One JSON line per measurement.

    python scripts/bench_sample.py [--quick]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

S1 = ([7, 352, 352, 352, 224, 451], [1, 1, 1, 1, 0])


def pkg(sub):
    return importlib.import_module("21cmvae_amd." + sub)


def setup(ctx):
    """the headline stack with seeded weights, the transforms of a synthetic training set, one noisy spectrum as data"""
    import sample_ref as sr
    from helpers import init_weights
    from infer_cases import transforms
    nat = pkg("_native")
    dims, act = S1
    Ws, bs, _ = init_weights(dims, 3)
    tin, tout, _ = transforms(5)
    st = nat.Stack(ctx, dims, act)
    st.set_weights(sr.jr.ora.flatten_params(Ws, bs))
    st.set_input_transform(*tin)
    st.set_output_transform(tout[0], tout[1].astype(np.float32))
    truth = pkg("synth").make_params(1, seed=3, zero_fx_frac=0)
    sig = 0.02 * tout[0]
    data = (sr.jr.jacobian(Ws, bs, act, truth, tin, tout)[0][0] + np.random.default_rng(3).normal(size=dims[-1]) * sig).astype(np.float32)
    w = np.full(dims[-1], 1.0 / sig ** 2, np.float32)
    st.set_likelihood(data, w)
    u_true = sr.jr.transform(truth, *tin)[0]
    return st, (Ws, bs, act, tin, tout, data, w), u_true


def starts(u_true, n, tin):
    import fit_ref as fr
    u = np.clip(u_true + 0.01 * np.random.default_rng(1).normal(size=(n, 7)), -0.999, 0.999)
    return u, fr.untransform(u, tin[0], tin[2], tin[3])


def timed(fn, repeat=3):
    fn()
    best = np.inf
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer transitions and chain counts")
    args = ap.parse_args()
    import sample_ref as sr
    nat = pkg("_native")
    ctx = nat.Context.default()
    st, (Ws, bs, act, tin, tout, data, w), u_true = setup(ctx)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    counts = (64, 65536) if args.quick else (64, 1024, 8192, 65536)
    for prec in ("f32", "f16"):
        for n in counts:
            steps = 40 if n >= 8192 else 200
            u0, x0 = starts(u_true, n, tin)
            opts = dict(n_steps=steps // 2, n_warmup=steps // 2, thin=0, seed=1)
            t_dev = timed(lambda: st.sample(x0, prec, flags, **opts))
            row = {"what": "transitions_per_s", "stack": "S1", "precision": prec, "chains": n, "transitions": steps,
                   "device": n * steps / t_dev, "device_us_per_transition": 1e6 * t_dev / steps}
            # the Python-driven loop over Stack.fisher: the same draws and arithmetic, one host call per transition
            def ev(u):
                F, l, g = st.fisher(np.ascontiguousarray(u, np.float32), prec, nat.FWD_OUT_TRANSFORM, lnl=True, grad=True)
                return l.astype(np.float64), g.astype(np.float64), F.astype(np.float64)
            psteps = steps if n < 8192 else 10
            popts = dict(n_steps=psteps // 2, n_warmup=psteps // 2, thin=0, seed=1)
            t_py = timed(lambda: sr.sample_ref(ev, u0, **popts), repeat=1)
            row["python_loop"] = n * psteps / t_py
            row["python_loop_us_per_transition"] = 1e6 * t_py / psteps
            row["device_over_python"] = row["device"] / row["python_loop"]
            print(json.dumps(row), flush=True)
    # the CPU reference
    n, csteps = 64, 20
    u0, _ = starts(u_true, n, tin)
    ev64 = sr.evaluator_batch(Ws, bs, act, data, w, tout)
    t_cpu = timed(lambda: sr.sample_ref(ev64, u0, n_steps=csteps // 2, n_warmup=csteps // 2, thin=0, seed=1), repeat=1)
    print(json.dumps({"what": "transitions_per_s", "stack": "S1", "precision": "float64 numpy", "chains": n, "transitions": csteps,
                      "cpu_reference": n * csteps / t_cpu}), flush=True)
    # the single-spectrum case through the class surface: 64 chains x (200 + 1000) transitions
    emulator, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    ds = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**ds)
    ae.load_model()
    truth = pp.par_untransform(np.random.default_rng(4).uniform(-0.6, 0.6, size=(1, 7)), ae.par_train)
    spec = np.asarray(ae.predict(truth), np.float32).reshape(-1)
    run = lambda: ae.sample_posterior(spec, 1.0, n_chains=64, n_steps=200 if args.quick else 1000, n_warmup=200, p0=truth[0])
    t = timed(run, repeat=2)
    r = run()
    total = 200 + (200 if args.quick else 1000)
    print(json.dumps({"what": "sample_posterior", "chains": 64, "transitions": total, "wall_s": t, "us_per_transition": 1e6 * t / total,
                      "accept_rate": float(np.mean(r.accept_rate)), "r_hat_max": float(np.max(r.r_hat))}), flush=True)


if __name__ == "__main__":
    main()
