"""Diagnostics (r4; r5: importable -- tests/test_fuzz_gpu.py runs a seeded slice under `pytest -m gpu`): the class surface
with random shapes -- DirectEmulator / AutoEncoderEmulator of random hidden layers
(1 to 600 wide, 0 to 5 layers), training sets of 40 to 3,000 rows, batch sizes 1 to 1,024, precisions, sequential and
joint recipes: train two epochs (losses finite, the optimizer counted every step), predict one row / a few / thousands
in float32 and float64 and compare with the float64 oracle evaluated on the weights the object reports
(get_weights), save -> load -> identical predictions, test_error finite.   python surface_fuzz.py [cases] [seed]"""
import importlib, os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HID = [1, 8, 16, 17, 32, 33, 64, 100, 128, 224, 288, 352, 400, 512, 600]


def dense_forward(weights, x, acts):
    h = x.astype(np.float64)
    for (W, b), a in zip(zip(weights[0::2], weights[1::2]), acts):
        h = h @ W.astype(np.float64) + b.astype(np.float64)
        h = np.maximum(h, 0) if a else h
    return h


def gen_cases(cases, seed):
    rng = np.random.default_rng(seed)
    for c in range(cases):
        kind = ["direct", "ae", "ae_joint"][int(rng.integers(0, 3))]
        prec = ["f32", "f16", "bf16"][int(rng.integers(0, 3))]
        n_train = int(rng.choice([40, 256, 300, 1000, 3000])); n_val = int(rng.choice([1, 17, 100])); n_test = int(rng.choice([1, 33, 200]))
        batch = int(rng.choice([1, 32, 100, 256, 257, 1024])) if n_train <= 1000 else int(rng.choice([100, 256, 1024]))
        hid = [int(rng.choice(HID)) for _ in range(int(rng.integers(0, 6)))]
        lat = int(rng.choice([1, 4, 9, 16, 32]))
        enc = [int(rng.choice(HID[1:])) for _ in range(int(rng.integers(0, 3)))]
        dec = [int(rng.choice(HID[1:])) for _ in range(int(rng.integers(0, 3)))]
        yield dict(c=c, kind=kind, prec=prec, n_train=n_train, n_val=n_val, n_test=n_test, batch=batch, hid=hid, lat=lat, enc=enc, dec=dec,
                   n_pred=int(rng.choice([1, 5, 4097])))


def tag_of(k):
    return "case %3d %-8s %-4s train %-4d val %-3d test %-3d batch %-4d hidden %-26s %s" % (
        k["c"], k["kind"], k["prec"], k["n_train"], k["n_val"], k["n_test"], k["batch"], k["hid"],
        "" if k["kind"] == "direct" else "latent %d enc %s dec %s" % (k["lat"], k["enc"], k["dec"]))


def settle_jit(em, kind, prec):
    """Wait for the run-time instantiated kernel of the stack `em.predict` runs on (a stack outside csrc/archs.h): it is
    compiled in the background from the first call on, and predict takes it once it is ready -- a bitwise comparison of two
    predictions must not straddle that switch of route (the f16 kernels round differently from the fallback's)."""
    nat = importlib.import_module("21cmvae_amd._native")
    model = em.emulator if kind == "direct" else em._predict_chain()
    try:
        model._ensure_stack().jit(prec)
    except nat.EngineError:
        pass  # no run-time kernel for this stack: its route does not change


def run_case(k):
    """-> ("OK" | "BAD" | "refused", message)"""
    emu = importlib.import_module("21cmvae_amd.emulator")
    synth = importlib.import_module("21cmvae_amd.synth")
    pp = importlib.import_module("21cmvae_amd.preprocess")
    eng = importlib.import_module("21cmvae_amd.engine")
    optm = importlib.import_module("21cmvae_amd.optimizers")
    c, kind, prec, n_train, batch, hid, lat, enc, dec, n_pred = (k[n] for n in ("c", "kind", "prec", "n_train", "batch", "hid", "lat", "enc", "dec", "n_pred"))
    par = [synth.make_params(n, seed=10 * c + i, corners=(i == 0)) for i, n in enumerate((n_train, k["n_val"], k["n_test"]))]
    sig = [synth.make_signals(n, seed=10 * c + 5 + i) for i, n in enumerate((n_train, k["n_val"], k["n_test"]))]
    q32 = synth.make_params(n_pred, seed=999 + c, dtype=np.float32)
    eng.set_random_seed(c)
    why = []
    try:
        if kind == "direct":
            em = emu.DirectEmulator(par[0], par[1], par[2], sig[0], sig[1], sig[2], hidden_dims=hid, precision=prec)
            em.emulator.compile(optimizer=optm.Adam(1e-3), loss=emu.relative_mse_loss(em.signal_train))
            loss, val = em.train(2, verbose=0, batch_size=batch)
            steps = em.emulator.optimizer.iterations
            models = [(em.emulator, [1] * len(hid) + [0])]
        else:
            em = emu.AutoEncoderEmulator(par[0], par[1], par[2], sig[0], sig[1], sig[2], latent_dim=lat, enc_hidden_dims=enc,
                                         dec_hidden_dims=dec, em_hidden_dims=hid, precision=prec)
            em.autoencoder.compile(optimizer=optm.Adam(1e-3), loss=emu.relative_mse_loss(em.signal_train))
            em.emulator.compile(optimizer=optm.Adam(1e-3), loss=emu.mean_squared_error)
            out = em.train(2, verbose=0, joint=(kind == "ae_joint"), batch_size=batch)
            loss, val = out[2], out[3]
            why += ["autoencoder loss not finite"] if not np.isfinite(out[0] + out[1]).all() else []
            steps = em.emulator.optimizer.iterations
        exp_steps = 2 * -(-n_train // batch)
        if steps != exp_steps:
            why.append("optimizer counted %d steps, expected %d" % (steps, exp_steps))
        if not (np.isfinite(loss).all() and np.isfinite(val).all()):
            why.append("loss not finite")
        # predictions against the float64 oracle on the weights the object reports
        settle_jit(em, kind, prec)
        p32 = np.atleast_2d(em.predict(q32)); p64 = np.atleast_2d(em.predict(q32.astype(np.float64)))
        if kind == "direct":
            chain = [(em.emulator.get_weights(), [1] * len(hid) + [0])]
        else:
            chain = [(em.emulator.get_weights(), [1] * len(hid) + [0]),
                     (em.autoencoder.decoder.get_weights(), [1] * len(dec) + [0])]
        for q, got, nm in ((q32, p32, "float32"), (q32.astype(np.float64), p64, "float64")):
            h = pp.par_transform(q, par[0])
            for wts, acts in chain:
                h = dense_forward(wts, h, acts)
            ref = pp.unpreproc(h, sig[0])
            scale = max(1.0, float(np.abs(ref).max()))
            tol = {"f32": 1e-4, "f16": 2e-2, "bf16": 1.5e-1}[prec] * scale
            err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else np.inf
            if err > tol:
                why.append("predict(%s, %d rows): max err %.3g > %.3g" % (nm, n_pred, err, tol))
        te = em.test_error()
        if not np.isfinite(te).all():
            why.append("test_error not finite")
        # save -> load -> the same predictions
        with tempfile.TemporaryDirectory() as d:
            if kind == "direct":
                em.emulator.save(os.path.join(d, "m.h5"))
                em2 = emu.DirectEmulator(par[0], par[1], par[2], sig[0], sig[1], sig[2], hidden_dims=[3], precision=prec)
                em2.load_model(os.path.join(d, "m.h5"))
            else:
                em.emulator.save(os.path.join(d, "e.h5")); em.autoencoder.encoder.save(os.path.join(d, "enc.h5")); em.autoencoder.decoder.save(os.path.join(d, "dec.h5"))
                em2 = emu.AutoEncoderEmulator(par[0], par[1], par[2], sig[0], sig[1], sig[2], precision=prec)
                em2.load_model(os.path.join(d, "e.h5"), os.path.join(d, "enc.h5"), os.path.join(d, "dec.h5"))
            settle_jit(em2, kind, prec)
            again = np.atleast_2d(em2.predict(q32))
            if not np.array_equal(again, p32):
                why.append("predictions after save -> load differ by %.3g" % float(np.abs(again - p32).max()))
    except Exception as e:
        if kind == "ae_joint" and "the joint step runs on the chain kernels" in str(e) and max(hid + enc + dec + [0]) > 512:
            # (joint=True is this package's extension; layers wider than 512 have no chain kernel: refused with that message.
            #  The reference's sequential recipe -- joint=False -- trains them, cases of kind "ae")
            return "refused", "joint step, a layer wider than 512"
        why.append("%s: %s" % (type(e).__name__, str(e)[:160]))
    return ("OK" if not why else "BAD"), "; ".join(why)


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    DRY = os.environ.get("FUZZ_DRY") == "1"
    bad = 0
    for k in gen_cases(cases, seed):
        if os.environ.get("FUZZ_ONLY") and int(os.environ["FUZZ_ONLY"]) != k["c"]:
            continue
        print(tag_of(k), "...", flush=True)
        if DRY:
            continue
        status, msg = run_case(k)
        bad += status == "BAD"
        print(tag_of(k), status, msg, flush=True)
    print("cases %d, BAD %d" % (cases, bad))
