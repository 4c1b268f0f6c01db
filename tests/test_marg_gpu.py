"""Linear foreground modes marginalised on the GPU (include/v21.h: v21_mlp_set_nuisance): the reductions of fisher /
loglike / nuisance_coef against the float64 reference (tests/marg_ref.py) fed the device's own y and J, the same at
foreground scale (float32 data carrying 10^6 times the signal), fits and sampler transitions against the references of
tests/fit_ref.py / tests/sample_ref.py on the marginalised evaluator, and the emulator classes' ``foreground=``.

Bounds of the reductions (the 1e-5 convention of test_fisher_against_own_jacobian), every scale taken from the PROJECTED
residual r~ = d~ - y, d~ = d - Q^T (Q W d) in float64 -- never larger than the raw one:
    F:     ||F - F_ref||_F <= 1e-5 ||J W J^T||_F
    lnl:   |lnl - ref|     <= 1e-5 (r~^T W r~ + |b~|^2)
    grad:  |g - ref|       <= 1e-5 (sum_k |w r~ J| + |B^T| |b~|)
    coef:  |a - ref|       <= |R^-1| (1e-5 sum_k |Q w r~|) + 1e-12 |R^-1| |Q W d|   (a = R^-1 (b~ + Q W d): the float32 sum b~
                              within 1e-5 of its terms' magnitudes, carried through the float64 back-substitution; the
                              second term is float64 rounding of the raw data's 10^6-fold larger share)"""
import numpy as np
import pytest

import fit_ref as fr
import jacobian_ref as jr
import marg_ref as mr
import sample_ref as sr
from conftest import pkg
from infer_support import (FUSED, GENERIC, NU, alpha_bound, alpha_of, basis, check_reduction, device_eval, fit_setup, flags_of, pick, reference,
                           rows_for, same, setup, starts_near, u_of)

pytestmark = pytest.mark.gpu


def foreground(amp75=2e6, K=5, seed=0):
    """a K-term LinLog foreground of ~amp75 at 75 MHz, float64 (451,)"""
    A = basis(K)
    a = np.zeros(K)
    a[0] = amp75 * (75.0 / np.sqrt(NU[0] * NU[-1])) ** 2.5
    a[1:] = a[0] * 0.1 * np.random.default_rng(seed).normal(size=K - 1) / (1 + np.arange(K - 1))
    return a @ A


def test_reductions_against_own_jacobian(ctx):
    """measured worst on the MI355X, as fractions of the scales: F 1.5e-7, lnl 5.0e-8, grad 4.3e-8 (the bounds stay at 1e-5),
    the amplitudes at 0.0085 of their bound"""
    nat = pkg("_native")
    cases = [(nm, p, n) for nm in FUSED + GENERIC for p in ("f32", "f16", "bf16") for n in (1, 5)]
    cases += [(nm, p, 16385) for nm, p in (("D1", "f32"), ("S3", "bf16"), ("S4", "f16"), ("NB", "f32"), ("W6", "f16"))]
    worst = {"F": 0.0, "lnl": 0.0, "grad": 0.0, "coef": 0.0}
    for c, (name, prec, n) in enumerate(cases):
        st, dims, act, Ws, bs, tin, tout, data, w = setup(ctx, name)
        flags = flags_of(nat, dims[0] == 7)
        K = (3, 5, 8, 1, 4)[c % 5]
        A = basis(K)
        x = rows_for(dims, n, 31 + n, np.float32)
        tag = "%s %s n=%d K=%d" % (name, prec, n, K)
        before = st.fisher(x, prec, flags, lnl=True, grad=True) + st.loglike(x, prec, flags)
        st.set_nuisance(A)
        assert st.nuisance_modes() == K
        F, lnl, g = st.fisher(x, prec, flags, lnl=True, grad=True)
        assert st.last_jac_route()[0] == ("fused" if name in FUSED else "generic"), tag
        assert F.shape == (n, dims[0], dims[0]) and np.all(np.isfinite(F)), tag
        assert np.array_equal(F.view(np.uint32), F.transpose(0, 2, 1).view(np.uint32)), tag  # exactly symmetric
        assert np.array_equal(st.fisher(x, prec, flags), F), tag  # (F alone: the data are not read)
        idx = pick(n)
        y, jac = st.jacobian(x[idx], prec, flags, return_outputs=True)
        coef = st.nuisance_coef(x[idx], prec, flags)
        assert coef.shape == (idx.size, K) and coef.dtype == np.float64
        ref, ls, gs, ct = reference(y, jac, data, w, A)
        check_reduction(tag, F[idx], lnl[idx], g[idx], coef, ref, ls, gs, ct, worst)
        # loglike against fisher's lnl and grad: the bounds test_fisher_against_own_jacobian uses between the two
        l_ll, g_ll = st.loglike(x[idx], prec, flags)
        np.testing.assert_allclose(lnl[idx], l_ll, rtol=1e-6, atol=0, err_msg=tag)
        scale = np.einsum("nk,njk->nj", np.abs(w * (data - y.astype(np.float64))), np.abs(jac.astype(np.float64)))
        assert np.all(np.abs(g[idx] - g_ll) <= 1e-6 * scale), (tag, np.max(np.abs(g[idx] - g_ll) / scale))
        assert np.array_equal(st.loglike(x[idx], prec, flags, grad=False), l_ll), tag
        # cleared: bit for bit what it was before
        st.set_nuisance(None)
        assert st.nuisance_modes() == 0
        after = st.fisher(x, prec, flags, lnl=True, grad=True) + st.loglike(x, prec, flags)
        for a, b in zip(before, after):
            assert same(a, b), tag
    print("worst of the reductions, fractions of the bounds: %s" % {k: "%.3g" % v for k, v in worst.items()})
    st.set_likelihood(None, None)


def test_record_state(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, data, w = setup(ctx, "NB")
    flags = flags_of(nat, dims[0] == 7)
    x = rows_for(dims, 4, 3, np.float32)
    A = basis(5)
    st.set_likelihood(None, None)
    with pytest.raises(nat.EngineError):  # no likelihood record
        st.set_nuisance(A)
    st.set_likelihood(data, w)
    with pytest.raises(nat.EngineError):  # no nuisance record
        st.nuisance_coef(x, "f32", flags)
    with pytest.raises(nat.EngineError):  # rank-deficient: the handle keeps what it had (nothing)
        st.set_nuisance(np.vstack([A, A[:1]]))
    assert st.nuisance_modes() == 0
    with pytest.raises(ValueError):
        st.set_nuisance(A[:, :450])
    st.set_nuisance(A)
    l1 = st.loglike(x, "f32", flags, grad=False)
    # a later set_likelihood re-whitens with the new weights: as if both had been set in that order
    w2 = w.copy(); w2[200:260] = 0
    st.set_likelihood(data, w2)
    assert st.nuisance_modes() == 5
    l2 = st.loglike(x, "f32", flags, grad=False)
    st.set_nuisance(None); st.set_nuisance(A)
    assert same(st.loglike(x, "f32", flags, grad=False), l2) and not same(l1, l2)
    # weights that leave fewer bins than modes + 1: refused, nothing changed
    w3 = np.zeros_like(w); w3[100:105] = w.max()
    with pytest.raises(nat.EngineError):
        st.set_likelihood(data, w3)
    assert same(st.loglike(x, "f32", flags, grad=False), l2)
    # invariance: any combination of the modes added to the data changes nothing beyond float32 rounding of the data
    y, jac = st.jacobian(x, "f32", flags, return_outputs=True)
    # (two evaluations, each within 1e-5 of its scale, and half a float32 ulp of the shifted data in every bin)
    _, ls, _, _ = reference(y, jac, data, w2, A)
    dn = (data + np.array([30.0, -20.0, 10.0, 5.0, -2.0]) @ A).astype(np.float32)
    w64 = w2.astype(np.float64)
    rt = np.abs(mr.project(data, mr.whiten(A, w64)[0], w64) - y.astype(np.float64))
    st.set_likelihood(dn, w2)
    assert np.all(np.abs(st.loglike(x, "f32", flags, grad=False) - l2) <= 2e-5 * ls + (rt * w64) @ (0.5 * np.spacing(np.abs(dn)).astype(np.float64)))
    # use_nuisance caches by value; clearing the likelihood clears both records
    st.use_nuisance(A)
    st.use_nuisance(A.copy())
    assert st.nuisance_modes() == 5
    st.set_likelihood(None, None)
    assert st.nuisance_modes() == 0 and st.nu_record is None
    st.use_nuisance(None)


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_foreground_scale(ctx, prec):
    """data = y(theta*) + a 5-term LinLog foreground of ~2e6 at 75 MHz + noise, float32: the record's path (fisher) and a
    data matrix through fit (lnl_start) against marg_ref in float64 fed the same float32 data, bounds from the projected
    residual.  An implementation that does not project the data misses the lnl bound by orders of magnitude."""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, "D1", seed=7, m=2)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    A = basis(5)
    d32 = (data.astype(np.float64) + np.stack([foreground(2e6, 5, 1), foreground(-1.5e6, 5, 2)])).astype(np.float32)
    assert np.abs(d32).max() > 1e6
    worst = {"F": 0.0, "lnl": 0.0, "grad": 0.0, "coef": 0.0}
    x0 = starts_near(truths[0], tin, 64, 3)
    st.set_likelihood(d32[0], w)
    st.set_nuisance(A)
    F, lnl, g = st.fisher(x0, prec, flags, lnl=True, grad=True)
    y, jac = st.jacobian(x0, prec, flags, return_outputs=True)
    ref, ls, gs, ct = reference(y, jac, d32[0], w, A)
    assert np.all(ls < 1e-6 * np.sum(w * d32[0].astype(np.float64) ** 2))  # the raw sums are 10^6 times the result and more
    check_reduction("record " + prec, F, lnl, g, st.nuisance_coef(x0, prec, flags), ref, ls, gs, ct, worst)
    # a data matrix: two spectra, 32 starts each; the device's own u of the starts, evaluated without the input transform
    u0 = st.sample(x0, prec, flags, data=d32, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"]
    r = st.fit(x0, prec, flags, data=d32, max_iter=0)
    y, jac = st.jacobian(u0, prec, nat.FWD_OUT_TRANSFORM, return_outputs=True)
    drow = d32[np.arange(64) // 32]
    ref, ls, gs, _ = reference(y, jac, drow, w, A)
    el = np.abs(r["lnl_start"] - ref["lnl"]) / ls
    print("fit lnl_start %s: %.2e (of 1e-5)" % (prec, el.max()))
    assert el.max() <= 1e-5, el.max()
    assert same(r["lnl"], r["lnl_start"])
    # ... and the sampler's evaluation of its start is the same number
    s = st.sample(x0, prec, flags, data=d32, n_steps=0, n_warmup=0)
    assert same(s["lnl_last"], r["lnl_start"])
    st.set_likelihood(None, None)


def test_fit_against_lm_ref_and_invariants(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, "NB", seed=5, m=2)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    A = basis(5)
    d32 = (data.astype(np.float64) + np.stack([foreground(2e6, 5, 1), foreground(1e6, 5, 2)])).astype(np.float32)
    st.set_likelihood(d32[0], w)
    st.set_nuisance(A)
    x0 = pkg("synth").make_params(2 * 3, seed=12, zero_fx_frac=0)
    r = st.fit(x0, "f32", flags, data=d32, max_iter=40)
    u0 = u_of(x0, tin).astype(np.float32).astype(np.float64)
    ud = u_of(r["x_hat"], tin)
    for i in range(x0.shape[0]):
        ev = mr.evaluator(Ws, bs, act, d32[i // 3], w, A, tout)
        ref = fr.lm_ref(ev, u0[i], max_iter=40)
        tol = 1e-4 * max(1.0, abs(ref["lnl"]))
        assert r["lnl"][i] >= ref["lnl"] - tol, (i, r["lnl"][i], ref["lnl"], r["status"][i], ref["status"])
        if ref["status"] == 1 and np.all(np.abs(ref["u"]) < 1 - 1e-3) and np.linalg.cond(ev(ref["u"])[2]) < 1e6:
            np.testing.assert_allclose(ud[i], ref["u"], atol=1e-4, err_msg=str(i))
    # invariants, as test_fit_monotone_and_in_box / test_fit_rows_independent: monotone, inside the box, rows independent
    # of each other and of chunking
    for prec in ("f32", "f16", "bf16"):
        x12 = pkg("synth").make_params(12, seed=21, zero_fx_frac=0).astype(np.float32)
        d3 = np.vstack([d32, d32[:1]])
        whole = st.fit(x12, prec, flags, data=d3, max_iter=12, fisher=True)
        assert np.all(whole["lnl"] >= whole["lnl_start"]) and np.all(np.isfinite(whole["x_hat"])), prec
        assert set(np.unique(whole["status"])) <= {0, 1, 2}
        u = u_of(whole["x_hat"].astype(np.float64), tin)
        assert np.all(u >= -1 - 1e-6) and np.all(u <= 1 + 1e-6), (u.min(), u.max())
        for k in range(3):
            part = st.fit(x12[4 * k:4 * k + 4], prec, flags, data=d3[k:k + 1], max_iter=12, fisher=True)
            for key in ("x_hat", "lnl", "lnl_start", "status", "fisher"):
                assert same(part[key], whole[key][4 * k:4 * k + 4]), (prec, k, key)
        st.set_likelihood(d3[0], w)  # the fit's Fisher matrix is v21_mlp_fisher (marginalised) at x_hat
        assert np.array_equal(whole["fisher"], st.fisher(whole["x_hat"], prec, flags))
    # two host chunks, rows on both sides of the boundary; the record's data
    big = np.ascontiguousarray(np.tile(x12, (8200 // 12 + 1, 1))[:8200])
    rb = st.fit(big, "f16", flags, max_iter=6)
    one = st.fit(x12, "f16", flags, max_iter=6)
    assert same(rb["x_hat"][:12], one["x_hat"]) and same(rb["x_hat"][8196:8200], one["x_hat"][:4]) and same(rb["lnl"][8196:8200], one["lnl"][:4])
    st.set_likelihood(None, None)


@pytest.mark.parametrize("name,prec", [("D1", "f32"), ("NB", "f16"), ("S3", "bf16")])
def test_one_transition_against_reference(ctx, name, prec):
    """test_sample_gpu.test_one_transition_against_reference with the marginalised likelihood at foreground scale: the
    same comparisons and tolerances (bit-equal proposal up to the float32 store, log alpha within the first-order effect of
    one float32 ulp of its inputs, accept decisions agree outside that bound)"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, name)
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    d32 = (data[0].astype(np.float64) + foreground(2e6, 5, 1)).astype(np.float32)
    st.set_likelihood(d32, w)
    st.set_nuisance(basis(5))
    n, seed, chain0, step0, eps0, ridge = 2048, 1234, 7, 40, 0.7, 1.0
    x0 = starts_near(truths[0], tin, n, 5)
    u0 = st.sample(x0, prec, flags, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
    r = st.sample(x0, prec, flags, n_steps=1, n_warmup=0, eps0=eps0, ridge=ridge, seed=seed, chain0=chain0, step0=step0, diagnostics=True)
    e0 = device_eval(st, nat, u0, prec)
    chains, eps = chain0 + np.arange(n), np.full(n, eps0)
    prop_ref, _, inside = sr.propose(u0, e0[1], e0[2], eps, sr.normals(seed, chains, step0, 7), ridge)
    prop = r["last_prop_u"].astype(np.float64)
    err = np.abs(prop - prop_ref)
    tol = np.spacing(np.abs(prop_ref).astype(np.float32)) + 1e-12
    assert np.all(err <= tol), (name, prec, np.max(err / tol))
    e1 = device_eval(st, nat, prop, prec)
    la = alpha_of(u0, e0, prop, e1, eps, ridge)
    bound = alpha_bound(u0, e0, prop, e1, eps, ridge, la)
    la_dev = r["last_log_alpha"]
    fin = np.isfinite(la)
    assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), (name, prec)
    ratio = np.abs(la_dev[fin] - la[fin]) / bound[fin]
    print("%s %s: inside %.3f, log alpha max diff / bound %.3f" % (name, prec, inside.mean(), ratio.max()))
    assert np.all(ratio <= 1.0), (name, prec, ratio.max())
    logu = np.log(sr.accept_uniform(seed, chains, step0))
    acc_ref, acc_dev = logu < la, r["accept_rate"] > 0.5
    excused = np.abs(logu - la) <= bound
    assert excused.mean() <= 0.005
    assert np.array_equal(acc_ref[~excused], acc_dev[~excused])
    u1 = np.where(acc_dev[:, None], prop, u0)
    np.testing.assert_allclose(r["x_last"], fr.untransform(u1, tin[0], tin[2], tin[3]), rtol=1e-12)
    st.set_likelihood(None, None)


def test_class_surface(shipped):
    emulator, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    nu = np.asarray(ae.frequencies, np.float64)
    fgm = pkg("foregrounds")
    A = fgm.linlog_basis(nu, 5)
    rng = np.random.default_rng(6)
    truth = pp.par_untransform(rng.uniform(-0.6, 0.6, size=(1, 7)), ae.par_train)[0]
    sigma = 20.0
    y_true = np.asarray(ae.predict(truth), np.float64)
    a_inj = np.zeros(5)
    a_inj[0] = 2e6 * (75.0 / np.sqrt(nu.min() * nu.max())) ** 2.5
    a_inj[1:] = a_inj[0] * np.array([0.05, -0.02, 0.01, 0.003])
    fg_inj = a_inj @ A
    noise = rng.normal(size=nu.size) * sigma
    d32 = (y_true + fg_inj + noise).astype(np.float32)
    l_true = ae.log_likelihood(truth, d32, sigma, foreground=5)
    l_arr = ae.log_likelihood(truth, d32, sigma, foreground=A)
    assert l_true == l_arr  # an int is that many LinLog terms over the band
    # chi^2 of 451 bins less 5 amplitudes at the truth: -2 lnL within 5 standard deviations of its mean
    assert abs(-2.0 * l_true - 446) <= 5 * np.sqrt(2 * 446), l_true
    lnl, g = ae.log_likelihood(np.stack([truth, truth]), d32, sigma, foreground=5, grad=True)
    assert lnl.shape == (2,) and g.shape == (2, 7)
    F = ae.fisher(truth, sigma, foreground=5)
    F0 = ae.fisher(truth, sigma)
    assert F.shape == (7, 7) and np.array_equal(F, F.T) and np.all(np.diag(F) <= np.diag(F0) * (1 + 1e-5))
    # at the truth the amplitudes reproduce the injected foreground up to the noise's share in span(A)
    a_hat, fg_hat = ae.foreground_amplitudes(truth, d32, sigma, 5)
    assert a_hat.shape == (5,) and fg_hat.shape == (451,) and a_hat.dtype == np.float64
    assert np.sqrt(np.mean((fg_hat - fg_inj) ** 2)) <= sigma, np.sqrt(np.mean((fg_hat - fg_inj) ** 2))
    r = ae.fit_parameters(d32, sigma, n_starts=16, max_iter=100, foreground=5)
    print("lnL_m at the truth %.3f, at the fit %.3f (status %d)" % (l_true, r.lnl, r.status))
    assert r.lnl >= l_true, (r.lnl, l_true)
    # at the fit: the amplitudes reproduce the injected foreground to within the noise, and so does the whole model the data
    a_fit, fg_fit = ae.foreground_amplitudes(r.params, d32, sigma, 5)
    y_fit = np.asarray(ae.predict(r.params), np.float64)
    rms_fg, rms_all = np.sqrt(np.mean((fg_fit - fg_inj) ** 2)), np.sqrt(np.mean((d32 - y_fit - fg_fit) ** 2))
    print("at the fit: rms(foreground model - injected) %.3f sigma, rms(data - model) %.3f sigma, rms(y_fit - y_true) %.3f sigma"
          % (rms_fg / sigma, rms_all / sigma, np.sqrt(np.mean((y_fit - y_true) ** 2)) / sigma))
    assert rms_fg <= sigma, rms_fg / sigma
    assert rms_all <= sigma, rms_all / sigma
    # a band, the sampler, and back to no foreground
    rb = ae.fit_parameters(d32, sigma, n_starts=4, max_iter=20, flow=60.0, fhigh=150.0, foreground=4, return_fisher=True)
    assert rb.params.shape == (7,) and rb.fisher.shape == (7, 7)
    s = ae.sample_posterior(d32, sigma, n_chains=8, n_steps=40, n_warmup=40, foreground=5, p0=r.params)
    assert s.params.shape == (8, 40, 7) and np.all(np.isfinite(s.params)) and np.all(np.isfinite(s.accept_rate))
    l_plain = ae.log_likelihood(truth, (y_true + noise).astype(np.float32), sigma)
    assert abs(-2.0 * l_plain - 451) <= 5 * np.sqrt(2 * 451)
    model, st, _, _ = ae._diff_stack(truth)
    assert st.nuisance_modes() == 0
    with pytest.raises(ValueError):
        ae.log_likelihood(truth, d32, sigma, foreground=np.zeros((3, 450)))
    with pytest.raises(ValueError):
        ae.foreground_amplitudes(truth, d32, sigma, None)
