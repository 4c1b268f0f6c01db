"""Fisher matrices and batched maximum-likelihood fits on the GPU (include/v21.h: v21_mlp_fisher[_dev], v21_mlp_fit[_dev]):
F against the float64 J^T W J of the device's own Jacobian and of tests/jacobian_ref.py, the fit's invariants (monotone,
inside the box, rows independent of each other and of chunking), recovery of truths on the shipped weights, agreement
with the float64 LM reference (tests/fit_ref.py), edge cases and the emulator classes' surface."""
import numpy as np
import pytest

import fit_ref as fr
import jacobian_ref as jr
from conftest import pkg
from infer_support import FUSED, GENERIC, check_rows, fit_setup, flags_of, pick, rows_for, setup, u_of

pytestmark = pytest.mark.gpu

# (p99, max) of F's relative Frobenius error against the 16-bit primal's masks, at most 4x the worst MI355X values (p99:
# f16 1.6e-3, bf16 1.2e-2; max: bf16 1.4e-2, f16 2.4e-2 outside the <= 0.5 % of rows with a unit at its kink)
F16_BOUND = {"f16": (6e-3, 6e-2), "bf16": (5e-2, 6e-2)}


def test_fisher_against_own_jacobian(ctx):
    nat = pkg("_native")
    cases = [(nm, p, n) for nm in FUSED + GENERIC for p in ("f32", "f16", "bf16") for n in (1, 5)]
    cases += [(nm, p, 16385) for nm, p in (("D1", "f32"), ("S3", "bf16"), ("S4", "f16"), ("NB", "f32"), ("W6", "f16"))]
    cases += [("D1", "f16", 65536)]
    for name, prec, n in cases:
        st, dims, act, Ws, bs, tin, tout, data, w = setup(ctx, name)
        flags = flags_of(nat, dims[0] == 7)
        x = rows_for(dims, n, 31 + n, np.float32)
        tag = "%s %s n=%d" % (name, prec, n)
        F, lnl, g = st.fisher(x, prec, flags, lnl=True, grad=True)
        assert st.last_jac_route()[0] == ("fused" if name in FUSED else "generic"), tag
        assert F.shape == (n, dims[0], dims[0]) and np.all(np.isfinite(F)), tag
        assert np.array_equal(F.view(np.uint32), F.transpose(0, 2, 1).view(np.uint32)), tag  # exactly symmetric
        idx = pick(n)
        jac = st.jacobian(x[idx], prec, flags)
        Fo = fr.fisher_ref(jac, w)
        err = jr.rel_frobenius(F[idx], Fo)
        assert err.max() <= 1e-5, (tag, err.max())
        l_ll, g_ll = st.loglike(x[idx], prec, flags)
        np.testing.assert_allclose(lnl[idx], l_ll, rtol=1e-6, atol=0, err_msg=tag)
        # (a sum with cancellation: relative to the sum of its terms' magnitudes)
        y = st.jacobian(x[idx], prec, flags, return_outputs=True)[0]
        scale = np.einsum("nk,njk->nj", np.abs(w * (data - y.astype(np.float64))), np.abs(jac.astype(np.float64)))
        assert np.all(np.abs(g[idx] - g_ll) <= 1e-6 * scale), (tag, np.max(np.abs(g[idx] - g_ll) / scale))
    st.set_likelihood(None, None)


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
def test_fisher_against_float64(ctx, prec):
    nat = pkg("_native")
    worst = {}
    for name in ("D1", "S3", "S4", "NB"):
        if name == "NB" and prec != "f32":
            continue
        st, dims, act, Ws, bs, tin, tout, data, w = setup(ctx, name)
        flags = flags_of(nat, dims[0] == 7)
        tin_on = dims[0] == 7
        x = rows_for(dims, 600, 77, np.float64)
        F = st.fisher(x, prec, flags)
        if prec == "f32":
            jac = st.jacobian(x, prec, flags)
            _, Jr = jr.jacobian(Ws, bs, act, x, tin if tin_on else None, tout)
            xt = jr.transform(x, *tin)[0] if tin_on else x.astype(np.float64)
            check_rows(name, "f32", jac, Jr, Ws, bs, act, xt, tin_on, x, tin, tout)  # J as the Jacobian tests accept it
            err = jr.rel_frobenius(F, fr.fisher_ref(Jr, w))
            bad = np.flatnonzero(err > 2e-5)
            assert bad.size <= max(1, int(0.005 * err.size)), (name, bad.size, err.max())
            for i in bad:  # a row beyond the bound: explained by ReLU units at their kink, as for the Jacobian
                kinks = jr.near_kinks(Ws, bs, act, xt[i:i + 1])
                _, Jf = jr.jacobian(Ws, bs, act, x[i:i + 1], tin if tin_on else None, tout, kinks)
                assert jr.rel_frobenius(F[i:i + 1], fr.fisher_ref(Jf, w))[0] <= 2e-5, (name, i, err[i])
            worst[name] = float(np.median(err))
        else:
            _, Jm = jr.jacobian(Ws, bs, act, x, tin if tin_on else None, tout, mask_prec=prec)
            err = jr.rel_frobenius(F, fr.fisher_ref(Jm, w))
            p99, mx = F16_BOUND[prec]
            worst[name] = (float(np.percentile(err, 99)), float(err.max()))
            assert np.percentile(err, 99) <= p99, (name, worst[name])
            assert np.sum(err > mx) <= max(1, int(0.005 * err.size)), (name, worst[name])
        st.set_likelihood(None, None)
    print("Fisher vs float64 %s: %s" % (prec, worst))


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
def test_fit_monotone_and_in_box(ctx, prec):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    x0 = pkg("synth").make_params(3 * 16, seed=8, zero_fx_frac=0).astype(np.float32)
    r = st.fit(x0, prec, flags, data=data, max_iter=30)
    assert np.all(r["lnl"] >= r["lnl_start"]), prec
    assert np.all(np.isfinite(r["lnl"])) and np.all(np.isfinite(r["x_hat"]))
    assert set(np.unique(r["status"])) <= {0, 1, 2}
    assert (r["lnl"] > r["lnl_start"]).mean() > 0.9
    u = u_of(r["x_hat"].astype(np.float64), tin)
    assert np.all(u >= -1 - 1e-6) and np.all(u <= 1 + 1e-6), (u.min(), u.max())
    if prec == "f32":
        # ln L at the start is log_likelihood(p0), per row's own spectrum
        for k in range(3):
            st.set_likelihood(data[k], w)
            l0 = st.loglike(x0[16 * k:16 * (k + 1)], prec, flags, grad=False)
            np.testing.assert_allclose(r["lnl_start"][16 * k:16 * (k + 1)], l0, rtol=1e-6, atol=0)
        st.set_likelihood(data[0], w)
    st.set_likelihood(None, None)


def test_fit_recovers_truths_on_trained_weights(shipped):
    emulator, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    rng = np.random.default_rng(4)
    u_true = rng.uniform(-0.8, 0.8, size=(4, 7))
    truths = pp.par_untransform(u_true, ae.par_train)
    spectra = np.asarray(ae.predict(truths), np.float32)  # noiseless
    sigma = 1.0
    res = ae.fit_parameters(spectra, sigma, n_starts=8, max_iter=100, return_all=True)
    best = np.argmax(res.lnl, axis=1)
    lnl_best = res.lnl[np.arange(4), best]
    print("recovery: best lnL %s, status %s" % (lnl_best, res.status[np.arange(4), best]))
    # (sigma = 1 mK: lnL >= -0.5 is an rms residual under 0.05 mK on signals of tens of mK; on MI355X three truths reach
    #  -3e-8 and one, whose 8 starts all end in a neighbouring optimum, -0.31)
    assert np.all(lnl_best >= -0.5), lnl_best
    # the best start's gradient at x_hat (u coordinates): small inside the box, pointing out of it at a bound
    model, st, flags, _ = ae._diff_stack(truths)
    nat = pkg("_native")
    for k in range(4):
        xh = res.params[k, best[k]]
        u = pp.par_transform(xh, ae.par_train)[0]
        st.use_likelihood(spectra[k], np.ones(451, np.float32))
        _, g = st.loglike(u[None, :].astype(np.float32), "f32", nat.FWD_OUT_TRANSFORM)
        F = st.fisher(u[None, :].astype(np.float32), "f32", nat.FWD_OUT_TRANSFORM)[0]
        g, scale = g[0].astype(np.float64), np.sqrt(np.maximum(np.diag(F), 1e-30))
        lo, hi = u <= -1 + 1e-6, u >= 1 - 1e-6
        inner = ~(lo | hi)
        assert np.all(np.abs(g[inner]) <= 1e-2 * scale[inner] + 1e-3), (k, g, scale)
        assert np.all(g[lo] <= 1e-3 + 1e-2 * scale[lo]) and np.all(g[hi] >= -1e-3 - 1e-2 * scale[hi]), (k, g, u)


def test_fit_against_lm_ref(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, "NB", seed=5, m=2)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    x0 = pkg("synth").make_params(2 * 3, seed=12, zero_fx_frac=0)
    r = st.fit(x0, "f32", flags, data=data, max_iter=40)
    u0 = u_of(x0, tin).astype(np.float32).astype(np.float64)  # (float64 starts, transformed in float64, rounded to float32)
    ud = u_of(r["x_hat"], tin)
    for i in range(x0.shape[0]):
        ev = fr.evaluator(Ws, bs, act, data[i // 3], w, tout)
        ref = fr.lm_ref(ev, u0[i], max_iter=40)
        tol = 1e-4 * max(1.0, abs(ref["lnl"]))
        assert r["lnl"][i] >= ref["lnl"] - tol, (i, r["lnl"][i], ref["lnl"], r["status"][i], ref["status"])
        if ref["status"] == 1 and np.all(np.abs(ref["u"]) < 1 - 1e-3) and np.linalg.cond(ev(ref["u"])[2]) < 1e6:
            np.testing.assert_allclose(ud[i], ref["u"], atol=1e-4, err_msg=str(i))
    st.set_likelihood(None, None)


def test_fit_rows_independent(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    x0 = pkg("synth").make_params(12, seed=21, zero_fx_frac=0).astype(np.float32)
    whole = st.fit(x0, "f16", flags, data=data, max_iter=12, fisher=True)
    for k in range(3):
        part = st.fit(x0[4 * k:4 * k + 4], "f16", flags, data=data[k:k + 1], max_iter=12, fisher=True)
        for key in ("x_hat", "lnl", "lnl_start", "status", "fisher"):
            assert np.array_equal(part[key].view(np.uint8), whole[key][4 * k:4 * k + 4].view(np.uint8)), (k, key)
    # the fit's Fisher matrix is v21_mlp_fisher at x_hat
    assert np.array_equal(whole["fisher"], st.fisher(whole["x_hat"], "f16", flags))
    # the device entry, and rows on both sides of a 16,384-row slice boundary
    n = 16392
    xb = np.tile(x0, (n // 12 + 1, 1))[:n]
    xb[16380:16392] = x0
    bufs = []
    try:
        dx, dd = ctx.malloc(xb.nbytes), ctx.malloc(data.nbytes)
        bufs += [dx, dd]
        dxh, dl, dl0, ds = ctx.malloc(xb.nbytes), ctx.malloc(n * 4), ctx.malloc(n * 4), ctx.malloc(n * 4)
        bufs += [dxh, dl, dl0, ds]
        ctx.h2d(dx, xb)
        ctx.h2d(dd, np.ascontiguousarray(data[:1]))
        st.fit_dev(dx, 7, n, dd, 1, dxh, dl, dl0, None, ds, "f16", flags, max_iter=12)
        ctx.sync()
        xh = np.empty_like(xb); ctx.d2h(xh, dxh)
        ll = np.empty(n, np.float32); ctx.d2h(ll, dl)
        ss = np.empty(n, np.int32); ctx.d2h(ss, ds)
    finally:
        for p in bufs:
            ctx.free(p)
    one = st.fit(x0, "f16", flags, data=data[:1], max_iter=12)
    assert np.array_equal(xh[16380:16392], one["x_hat"]) and np.array_equal(ll[16380:16392], one["lnl"])
    assert np.array_equal(ss[16380:16392], one["status"])
    assert np.array_equal(xh[:12], one["x_hat"]) and np.array_equal(ll[:12], one["lnl"])
    st.set_likelihood(None, None)


def test_fit_edge_cases(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    x0 = pkg("synth").make_params(4, seed=30, zero_fx_frac=0)
    # n = 1
    r = st.fit(x0[:1], "f32", flags, data=data[:1])
    assert r["x_hat"].shape == (1, 7) and r["lnl"][0] >= r["lnl_start"][0]
    # a start exactly on a bound and one outside the box (clamped), fx = 0 (its floor is the box's lower bound)
    u_b = np.array([[-1.0, 1.0, -1.0, 0.2, -0.3, 1.0, 0.0]])
    xb = fr.untransform(u_b, *[tin[0], tin[2], tin[3]])
    xo = x0[1:2].copy(); xo[0, 3] = 1e6
    xz = x0[2:3].copy(); xz[0, 2] = 0.0
    r = st.fit(np.vstack([xb, xo, xz]), "f32", flags, data=data[:1], max_iter=20)
    assert np.all(np.isfinite(r["x_hat"])) and np.all(r["lnl"] >= r["lnl_start"])
    u = u_of(r["x_hat"], tin)
    assert np.all(np.abs(u) <= 1 + 1e-6)
    # max_iter = 0: the clamped start comes back
    r0 = st.fit(x0, "f32", flags, data=data[:1], max_iter=0)
    np.testing.assert_allclose(r0["x_hat"], x0, rtol=1e-6)
    assert np.array_equal(r0["lnl"], r0["lnl_start"])
    # no information: every weight zero -> status 3, the clamped start, no NaN
    st.set_likelihood(data[0], np.zeros(dims[-1], np.float32))
    xs = np.vstack([x0[:2], xo])
    r3 = st.fit(xs, "f32", flags, fisher=True)
    assert np.all(r3["status"] == 3) and np.all(r3["lnl"] == 0) and np.all(np.isfinite(r3["x_hat"]))
    assert np.all(r3["fisher"] == 0)
    xc = fr.untransform(np.clip(u_of(xs, tin), -1, 1), tin[0], tin[2], tin[3])
    np.testing.assert_allclose(r3["x_hat"], xc, rtol=1e-6)
    st.set_likelihood(None, None)
    with pytest.raises(nat.EngineError):  # no record
        st.fit(x0, "f32", flags)


def test_fit_data_count_checked_and_routes_counted(ctx):
    """a data matrix of n_data < 1 rows (or one that does not divide n) is an argument error of both C entries, never a
    division by zero; a fit counts once for its iterations and once for the Fisher matrix at x_hat, whatever its chunks"""
    import ctypes as C
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    lib, F = st.lib, C.POINTER(C.c_float)
    n = 6
    x0 = np.ascontiguousarray(pkg("synth").make_params(n, seed=40, zero_fx_frac=0).astype(np.float32))
    xh, lnl = np.empty_like(x0), np.empty(n, np.float32)
    d = np.ascontiguousarray(data[:1])
    for nd in (0, -1, 4):
        assert lib.v21_mlp_fit(st.h, x0.ctypes.data_as(C.c_void_p), 0, n, d.ctypes.data_as(F), nd, None, xh.ctypes.data_as(C.c_void_p),
                               lnl.ctypes.data_as(F), None, None, None, 0, flags) == -1, nd
    bufs = [ctx.malloc(x0.nbytes), ctx.malloc(d.nbytes), ctx.malloc(x0.nbytes), ctx.malloc(n * 4)]
    try:
        for nd in (0, -1, 4):
            assert lib.v21_mlp_fit_dev(st.h, C.c_void_p(bufs[0]), 7, n, C.c_void_p(bufs[1]), nd, None, C.c_void_p(bufs[2]),
                                       C.c_void_p(bufs[3]), None, None, None, 0, flags) == -1, nd
    finally:
        for p in bufs:
            ctx.free(p)
    counts = lambda: sum(st.last_jac_route()[1].values())
    c0 = counts()
    st.fit(x0, "f16", flags, data=d, max_iter=3)
    assert counts() - c0 == 1
    big = np.ascontiguousarray(np.tile(x0, (8193 // n + 1, 1))[:8193])  # two host chunks of the record's data
    c0 = counts()
    r = st.fit(big, "f16", flags, max_iter=3, fisher=True)
    assert counts() - c0 == 2 and st.last_jac_route()[0] == "fused"
    assert np.array_equal(r["fisher"], st.fisher(r["x_hat"], "f16", flags))
    assert counts() - c0 == 3
    # so do the Jacobian and the log-likelihood: once per call, not once per host chunk
    for call in (st.jacobian, st.loglike):
        c0 = counts()
        call(big, "f16", flags)
        assert counts() - c0 == 1, call.__name__
    st.set_likelihood(None, None)


def test_class_surface(shipped):
    emulator, synth = pkg("emulator"), pkg("synth")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    de = emulator.DirectEmulator(**data)
    pars = data["par_test"][:5]
    F1 = de.fisher(pars[0], 0.05)
    assert F1.shape == (7, 7) and np.allclose(F1, F1.T)
    F = de.fisher(pars, np.full(451, 0.05), flow=60.0, fhigh=160.0)
    assert F.shape == (5, 7, 7)
    _, J = de.jacobian(pars, return_signal=True)
    nu = np.asarray(de.frequencies)
    w = np.where((nu >= 60) & (nu <= 160), 1 / 0.05 ** 2, 0.0)
    np.testing.assert_allclose(F, np.einsum("nki,k,nkj->nij", J.astype(np.float64), w, J.astype(np.float64)), rtol=1e-4,
                               atol=1e-6 * np.abs(F).max())
    spec = de.predict(pars[:2])
    r = de.fit_parameters(spec[0], 0.05, n_starts=3, max_iter=5)
    assert r.params.shape == (7,) and np.ndim(r.lnl) == 0 and np.ndim(r.status) == 0 and r.fisher is None
    r = de.fit_parameters(spec, 0.05, n_starts=3, max_iter=5, return_fisher=True)
    assert r.params.shape == (2, 7) and r.lnl.shape == (2,) and r.fisher.shape == (2, 7, 7)
    ra = de.fit_parameters(spec, 0.05, n_starts=3, max_iter=5, return_all=True, return_fisher=True)
    assert ra.params.shape == (2, 3, 7) and ra.lnl.shape == (2, 3) and ra.status.shape == (2, 3) and ra.fisher.shape == (2, 3, 7, 7)
    best = np.argmax(ra.lnl, axis=1)
    assert np.array_equal(r.params, ra.params[np.arange(2), best]) and np.array_equal(r.lnl, ra.lnl[np.arange(2), best])
    rp = de.fit_parameters(spec[0], 0.05, p0=pars[:2], max_iter=5, return_all=True)
    assert rp.params.shape == (2, 7)
    with pytest.raises(ValueError):
        de.fit_parameters(np.zeros(450), 0.05)
