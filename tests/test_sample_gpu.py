"""Posterior sampling on the GPU (include/v21.h: v21_mlp_sample[_dev]): one transition rebuilt in float64 from the device's
own evaluations and the same Philox draws, reproducibility and independence of chunking / splitting, statistics against
the float64 reference sampler (tests/sample_ref.py), the uniform target, edge cases and errors, the emulator classes'
surface."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as fr
import sample_ref as sr
from conftest import pkg
from infer_cases import N_SE
from infer_support import alpha_bound, alpha_of, between_chain, device_eval, fit_setup, flags_of, run_dev, same, starts_near, u_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "S3", "NB"])
def test_one_transition_against_reference(ctx, name, prec):
    """n_steps = 1 from given starts; the transition rebuilt in float64 from the device's own evaluations (st.fisher in
    the same precision: the arithmetic after the evaluation does not depend on it) and the same draws.
    last_prop_u: the float32 store of a float64 result -- one float32 ulp of the value, plus 1e-12 for the float64
    rounding (2e-16) through triangular solves of condition up to a few thousand.  last_log_alpha: the first-order
    effect of one float32 ulp of every input (alpha_bound), no slack factor.  The accept decisions agree wherever
    |log uniform - log alpha| exceeds that bound; at most 0.5 % of the chains may be excused."""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, name)
    n, seed, chain0, step0, eps0, ridge = 4096, 1234, 7, 40, 0.7, 1.0
    x0 = starts_near(truths[0], tin, n, 5)
    u0 = st.sample(x0, prec, flags_of(nat, True), n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
    assert np.max(np.abs(u0 - u_of(x0, tin))) <= 2.0 ** -23  # the start as the device holds it: float32 of the float64 transform
    r = st.sample(x0, prec, flags_of(nat, True), n_steps=1, n_warmup=0, eps0=eps0, ridge=ridge, seed=seed, chain0=chain0, step0=step0,
                  diagnostics=True)
    e0 = device_eval(st, nat, u0, prec)
    chains, eps = chain0 + np.arange(n), np.full(n, eps0)
    prop_ref, _, inside = sr.propose(u0, e0[1], e0[2], eps, sr.normals(seed, chains, step0, 7), ridge)
    prop = r["last_prop_u"].astype(np.float64)
    err = np.abs(prop - prop_ref)
    tol = np.spacing(np.abs(prop_ref).astype(np.float32)) + 1e-12
    print("%s %s: proposal max err / tol %.3f, inside %.3f" % (name, prec, np.max(err / tol), inside.mean()))
    assert np.all(err <= tol), (name, prec, np.max(err / tol))
    e1 = device_eval(st, nat, prop, prec)
    la = alpha_of(u0, e0, prop, e1, eps, ridge)
    bound = alpha_bound(u0, e0, prop, e1, eps, ridge, la)
    la_dev = r["last_log_alpha"]
    fin = np.isfinite(la)
    assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), (name, prec)
    ratio = np.abs(la_dev[fin] - la[fin]) / bound[fin]
    print("%s %s: log alpha max |diff| %.3e, max diff / bound %.3f, median bound %.2e" % (name, prec, np.max(np.abs(la_dev[fin] - la[fin])),
                                                                                     ratio.max(), np.median(bound[fin])))
    assert np.all(ratio <= 1.0), (name, prec, ratio.max())
    logu = np.log(sr.accept_uniform(seed, chains, step0))
    acc_ref, acc_dev = logu < la, r["accept_rate"] > 0.5
    excused = np.abs(logu - la) <= bound
    print("%s %s: accepted %.3f, excused %d of %d" % (name, prec, acc_dev.mean(), excused.sum(), n))
    assert excused.mean() <= 0.005
    assert np.array_equal(acc_ref[~excused], acc_dev[~excused])
    # the state after the transition: the proposal where accepted, the start elsewhere
    u1 = np.where(acc_dev[:, None], prop, u0)
    np.testing.assert_allclose(r["x_last"], fr.untransform(u1, tin[0], tin[2], tin[3]), rtol=1e-12)
    st.set_likelihood(None, None)


def dev_sample(ctx, st, x0, data_rows, prec, flags, keys=("x_last", "lnl_last", "samples", "mean_u"), guard=0, **opts):
    """v21_mlp_sample_dev on float32 starts -> dict of host arrays"""
    n, din = x0.shape
    o = st.sample_opts(**opts)
    keep = o.n_steps // o.thin if o.thin else 0
    shapes = {"x_last": ((n, din), np.float32), "lnl_last": ((n,), np.float32), "samples": ((n, keep, din), np.float32),
              "samples_lnl": ((n, keep), np.float32), "mean_u": ((n, din), np.float64), "cov_u": ((n, din, din), np.float64),
              "eps_last": ((n,), np.float64), "accept_rate": ((n,), np.float64)}
    call = lambda dx, dd, out: st.sample_dev(dx, din, n, dd, data_rows.shape[0], out, None, prec, flags, **opts)
    return run_dev(ctx, shapes, keys, call, x0, data_rows, guard)


def test_reproducible_and_chunk_independent(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    opts = dict(n_steps=6, n_warmup=4, thin=2, seed=99, eps0=0.8)
    keys = ("x_last", "lnl_last", "eps_last", "accept_rate", "mean_u", "cov_u", "samples", "samples_lnl")
    x12 = starts_near(truths[0], tin, 12, 21)
    a = st.sample(x12, "f16", flags, data=data, **opts)
    b = st.sample(x12, "f16", flags, data=data, **opts)
    for k in keys:
        assert same(a[k], b[k]), k
    c = st.sample(x12, "f16", flags, data=data, **dict(opts, seed=100))
    assert not same(a["samples"], c["samples"])
    # chains alone, with the matching chain0 and their own spectrum
    for k3 in range(3):
        part = st.sample(x12[4 * k3:4 * k3 + 4], "f16", flags, data=data[k3:k3 + 1], chain0=4 * k3, **opts)
        for k in keys:
            assert same(part[k], a[k][4 * k3:4 * k3 + 4]), (k3, k)
    # the device entry across the 16,384-row slice boundary: its first and last chains equal the same chains run alone
    n = 16392
    xb = np.ascontiguousarray(np.tile(x12, (n // 12 + 1, 1))[:n].astype(np.float32))
    d1 = np.ascontiguousarray(data[:1])
    whole = dev_sample(ctx, st, xb, d1, "f16", flags, **opts)
    for lo, hi in ((0, 12), (n - 12, n)):
        alone = dev_sample(ctx, st, np.ascontiguousarray(xb[lo:hi]), d1, "f16", flags, chain0=lo, **opts)
        for k in whole:
            assert same(alone[k], whole[k][lo:hi]), (lo, k)
    # a host call over two host chunks (8,192 + 8): the chains on both sides of the chunk boundary
    nh = 8200
    xh = np.ascontiguousarray(xb[:nh].astype(np.float64))
    big = st.sample(xh, "f16", flags, data=d1, **opts)
    for lo, hi in ((0, 8), (8188, 8200)):
        alone = st.sample(xh[lo:hi], "f16", flags, data=d1, chain0=lo, **opts)
        for k in keys:
            assert same(alone[k], big[k][lo:hi]), (lo, k)
    # 2k steps = k steps, then k more from x_last (float64: the float32 state survives the round trip), eps_last, step0 = k
    k = 5
    two = st.sample(x12, "f32", flags, data=data, n_steps=2 * k, n_warmup=0, seed=3, eps0=0.8)
    first = st.sample(x12, "f32", flags, data=data, n_steps=k, n_warmup=0, seed=3, eps0=0.8)
    second = st.sample(first["x_last"], "f32", flags, data=data, n_steps=k, n_warmup=0, seed=3, step0=k, eps_start=first["eps_last"])
    assert same(two["samples"], np.concatenate([first["samples"], second["samples"]], axis=1))
    assert same(two["x_last"], second["x_last"]) and same(two["samples_lnl"][:, k:], second["samples_lnl"])
    st.set_likelihood(None, None)


def test_statistics_against_reference_sampler(ctx):
    """NB, f32, the likelihood of fit_setup (sigma = 0.02 std: on the CPU the reference's two half-ensembles of 512 chains
    agree within 1.1 standard errors in the mean and 3.4 in the worst of the 49 covariance entries, and it accepts 0.578
    after the warm-up).  4,096 device chains against 1,024 reference chains, 100 + 200 transitions each."""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, "NB")
    opts = dict(n_steps=200, n_warmup=100, seed=11)
    x0 = starts_near(truths[0], tin, 4096, 1, scale=0.01)
    r = st.sample(x0, "f32", flags_of(nat, True), thin=0, **opts)
    assert "samples" not in r and np.all(np.isfinite(r["mean_u"])) and np.all(np.isfinite(r["cov_u"]))
    ev = sr.evaluator_batch(Ws, bs, act, data[0], w, tout)
    ref = sr.sample_ref(ev, u_of(x0[:1024], tin), thin=0, **opts)
    acc_ref = ref["accept_rate"].mean()
    print("reference acceptance after the warm-up %.3f (device %.3f); step size %.3f (device %.3f)"
          % (acc_ref, r["accept_rate"].mean(), np.median(ref["eps"]), np.median(r["eps_last"])))
    assert abs(acc_ref - 0.574) <= 0.15
    worst = {}
    for key, dev_c, ref_c in (("mean", r["mean_u"], ref["mean_u"]), ("cov", r["cov_u"], ref["cov_u"]),
                              ("accept", r["accept_rate"], ref["accept_rate"])):
        (md, vd), (mr, vr) = between_chain(dev_c), between_chain(ref_c)
        z = np.abs(md - mr) / np.sqrt(vd + vr)
        worst[key] = float(np.max(z))
        assert np.all(z < N_SE), (key, z)
    print("device vs reference, worst z: %s" % worst)
    st.set_likelihood(None, None)


def test_uniform_target_on_the_device(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    st.set_likelihood(data[0], np.zeros(dims[-1], np.float32))
    n = 4096
    u0 = np.random.default_rng(4).uniform(-1, 1, size=(n, 7))
    x0 = fr.untransform(u0, tin[0], tin[2], tin[3])
    opts = dict(n_steps=600, n_warmup=150, seed=5)
    r = st.sample(x0, "f32", flags_of(nat, True), thin=3, **opts)
    assert all(np.all(np.isfinite(r[k])) for k in r)
    acc = r["accept_rate"].mean()
    assert 0 < acc < 1 and np.all(r["lnl_last"] == 0)
    m2 = np.diagonal(r["cov_u"], axis1=1, axis2=2) + r["mean_u"] ** 2
    zm, zv = sr.pooled_check(r["mean_u"], 0.0)[1], sr.pooled_check(m2, 1.0 / 3.0)[1]
    print("uniform target on the device: accept %.3f, z mean %s var %s" % (acc, zm.round(2), zv.round(2)))
    assert np.all(zm < N_SE) and np.all(zv < N_SE), (zm, zv)
    us = u_of(r["samples"].reshape(-1, 7), tin).reshape(n, 200, 7)
    assert np.all(np.abs(us) <= 1 + 1e-12)
    # the moments of every transition (thin = 1, float64 samples) recomputed from the stored samples
    n1 = 64
    r1 = st.sample(x0[:n1], "f32", flags_of(nat, True), thin=1, **opts)
    u1 = u_of(r1["samples"].reshape(-1, 7), tin).reshape(n1, 600, 7)
    np.testing.assert_allclose(r1["mean_u"], u1.mean(axis=1), atol=1e-13)
    np.testing.assert_allclose(r1["cov_u"], np.einsum("nki,nkj->nij", u1, u1) / 600 - np.einsum("ni,nj->nij", u1.mean(axis=1), u1.mean(axis=1)),
                               atol=1e-13)
    # thin does not change the chain: the same moments with thin = 3 and with no sample buffer at all
    r0 = st.sample(x0[:n1], "f32", flags_of(nat, True), thin=0, **opts)
    assert "samples" not in r0
    for k in ("mean_u", "cov_u", "accept_rate", "x_last", "eps_last"):
        assert same(r0[k], r1[k]) and same(r0[k], r[k][:n1]), k
    assert same(r["samples"][:n1], r1["samples"][:, 2::3])
    st.set_likelihood(None, None)


def test_edge_cases(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    x0 = pkg("synth").make_params(4, seed=30, zero_fx_frac=0)
    # n = 1
    r = st.sample(x0[:1], "f32", flags, data=data[:1], n_steps=5, n_warmup=5)
    assert r["samples"].shape == (1, 5, 7) and np.all(np.isfinite(r["samples"])) and r["mean_u"].shape == (1, 7)
    # a start outside the box (clamped), fx = 0 (its floor is the box's lower bound); n_steps = 0 returns the clamped start
    xo = x0[1:2].copy(); xo[0, 3] = 1e6
    xz = x0[2:3].copy(); xz[0, 2] = 0.0
    xs = np.vstack([x0[:1], xo, xz])
    r0 = st.sample(xs, "f32", flags, data=data[:1], n_steps=0, n_warmup=0, diagnostics=True)
    uc = np.clip(u_of(xs, tin), -1, 1)
    assert uc[1, 3] == 1.0 and uc[2, 2] == -1.0
    np.testing.assert_allclose(r0["x_last"], fr.untransform(uc, tin[0], tin[2], tin[3]), rtol=1e-6)
    np.testing.assert_array_equal(r0["last_prop_u"], uc.astype(np.float32))
    assert "samples" not in r0 and np.all(r0["last_log_alpha"] == 0) and np.all(r0["accept_rate"] == 0)
    np.testing.assert_array_equal(r0["mean_u"], uc.astype(np.float32).astype(np.float64))
    st.set_likelihood(data[0], w)
    np.testing.assert_allclose(r0["lnl_last"], st.loglike(r0["x_last"], "f32", flags, grad=False), rtol=1e-5)
    r = st.sample(xs, "f32", flags, data=data[:1], n_steps=20, n_warmup=20)
    assert np.all(np.isfinite(r["samples"])) and np.all(np.abs(u_of(r["samples"].reshape(-1, 7), tin)) <= 1 + 1e-12)
    # thin that does not divide n_steps: n_steps // thin samples -- the states after kept transitions thin, 2 thin, ...
    full = st.sample(xs, "f32", flags, data=data[:1], n_steps=10, n_warmup=3, seed=2)
    part = st.sample(xs, "f32", flags, data=data[:1], n_steps=10, n_warmup=3, seed=2, thin=4)
    assert part["samples"].shape == (3, 2, 7) and same(part["samples"], full["samples"][:, [3, 7]])
    assert same(part["mean_u"], full["mean_u"]) and same(part["x_last"], full["x_last"])
    big = st.sample(xs, "f32", flags, data=data[:1], n_steps=3, n_warmup=0, thin=5)
    assert "samples" not in big
    st.set_likelihood(None, None)
    with pytest.raises(nat.EngineError):  # no record
        st.sample(x0, "f32", flags, n_steps=1, n_warmup=0)


def test_argument_errors_and_routes_counted(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    lib, F, P = st.lib, C.POINTER(C.c_float), C.c_void_p
    n = 6
    x0 = np.ascontiguousarray(pkg("synth").make_params(n, seed=40, zero_fx_frac=0).astype(np.float32))
    xl = np.empty_like(x0)
    d = np.ascontiguousarray(data[:1])
    out = nat.SampleOut(x_last=xl.ctypes.data)

    def opts(**kw):
        o = dict(nat.SAMPLE_DEFAULTS, n_steps=2, n_warmup=1)
        o.update(kw)
        return nat.SampleOpts(*[o[k] for k, _ in nat.SampleOpts._fields_])

    bad_opts = [opts(ridge=0.0), opts(ridge=-1.0), opts(eps0=0.0), opts(eps0=-0.5), opts(n_steps=-1), opts(n_warmup=-1), opts(thin=-1),
                opts(chain0=-1), opts(step0=-1), opts(target_accept=0.0), opts(target_accept=1.5)]
    host = lambda nd, o: lib.v21_mlp_sample(st.h, x0.ctypes.data_as(P), 0, n, d.ctypes.data_as(F), nd, C.byref(o) if o else None, None,
                                            C.byref(out), 0, flags)
    for nd in (0, -1, 4):
        assert host(nd, None) == -1, nd
    for o in bad_opts:
        assert host(1, o) == -1
    assert host(1, opts()) == 0
    bufs = [ctx.malloc(x0.nbytes), ctx.malloc(d.nbytes), ctx.malloc(x0.nbytes)]
    try:
        dout = nat.SampleOut(x_last=bufs[2])
        dev = lambda nd, o: lib.v21_mlp_sample_dev(st.h, P(bufs[0]), 7, n, P(bufs[1]), nd, C.byref(o) if o else None, None, C.byref(dout), 0, flags)
        for nd in (0, -1, 4):
            assert dev(nd, None) == -1, nd
        for o in bad_opts:
            assert dev(1, o) == -1
        ctx.h2d(bufs[0], x0)
        ctx.h2d(bufs[1], d)
        assert dev(1, opts()) == 0
        ctx.sync()
        ctx.d2h(xl, bufs[2])
        assert np.all(np.isfinite(xl))
    finally:
        for p in bufs:
            ctx.free(p)
    # one count per call on the Jacobian's route, whatever its transitions and chunks
    counts = lambda: sum(st.last_jac_route()[1].values())
    c0 = counts()
    st.sample(x0, "f16", flags, data=d, n_steps=3, n_warmup=2)
    assert counts() - c0 == 1 and st.last_jac_route()[0] == "fused"
    big = np.ascontiguousarray(np.tile(x0, (8193 // n + 1, 1))[:8193])  # two host chunks
    c0 = counts()
    st.sample(big, "f16", flags, n_steps=2, n_warmup=1, thin=0)
    assert counts() - c0 == 1
    st.set_likelihood(None, None)


def test_class_surface(shipped):
    emulator, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    u_true = np.random.default_rng(4).uniform(-0.6, 0.6, size=(2, 7))
    truths = pp.par_untransform(u_true, ae.par_train)
    spectra = np.asarray(ae.predict(truths), np.float32)  # noiseless
    lo, hi = pp.par_untransform(-np.ones(7), ae.par_train)[0], pp.par_untransform(np.ones(7), ae.par_train)[0]
    # One spectrum, started at the truth: shapes, the box, convergence, the truth within 5 posterior standard deviations.
    # The second truth at sigma = 0.05 mK is the well-conditioned case (posterior sd 0.002 .. 0.08 in u, inside the box;
    # the first truth leaves alpha and Rmfp prior-limited, sd 0.2 .. 0.4).  Length: on the MI355X 32 chains reach
    # r_hat = 2.35 after 400 kept transitions, 1.51 after 1,500 and 1.08 after 30,000: r_hat^2 - 1 = 4.5, 1.3, 0.16, falling
    # roughly as 1 / n; after the 60,000 run here it is 1.04.
    r = ae.sample_posterior(spectra[1], 0.05, n_chains=32, n_steps=60000, n_warmup=500, thin=200, p0=truths[1], return_lnl=True)
    assert r.params.shape == (32, 300, 7) and r.lnl.shape == (32, 300) and r.accept_rate.shape == (32,) and r.step_size.shape == (32,)
    assert r.r_hat.shape == (7,) and r.mean_u.shape == (7,) and r.cov_u.shape == (7, 7)
    assert np.all(r.params >= lo * (1 - 1e-12)) and np.all(r.params <= hi * (1 + 1e-12))
    print("r_hat %s, accept %.3f" % (r.r_hat.round(3), r.accept_rate.mean()))
    assert np.all(np.isfinite(r.r_hat)) and np.all(r.r_hat < 1.1), r.r_hat
    sd = np.sqrt(np.diag(r.cov_u))
    assert np.all(np.abs(r.mean_u - u_true[1]) <= 5 * sd), (r.mean_u, u_true[1], sd)
    # several spectra, default starts (the best fit per spectrum), no stored samples
    r2 = ae.sample_posterior(spectra, 1.0, n_chains=8, n_steps=50, n_warmup=50, thin=0)
    assert r2.params is None and r2.lnl is None and r2.accept_rate.shape == (2, 8) and r2.r_hat.shape == (2, 7) and r2.cov_u.shape == (2, 7, 7)
    r3 = ae.sample_posterior(spectra, 1.0, n_chains=8, n_steps=50, n_warmup=50)
    assert r3.params.shape == (2, 8, 50, 7) and r3.lnl is None
    de = emulator.DirectEmulator(**data)
    assert hasattr(de, "sample_posterior")
    with pytest.raises(ValueError):
        ae.sample_posterior(np.zeros(450), 1.0)
    with pytest.raises(ValueError):
        ae.sample_posterior(spectra[0], 1.0, n_steps=-1)
