"""The samplers' prior without a GPU (include/v21.h: v21_mlp_set_prior): the Prior class of 21cmvae_amd/priors.py, the
float64 reference tests/prior_ref.py against closed forms, the statistical tests of tests/test_prior_gpu.py on the
reference at the seeds and sizes they use there, and the binding's argument checks that need no device.

The cases the GPU tests share are in tests/infer_cases.py: the mixed record of a d-column stack, the flat-likelihood runs,
and the two evidence problems (the tempering tests' quadrature problems under a Gaussian prior)."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.special import ndtr

import ensemble_ref as er
import nested_ref as nr
import prior_ref as pr
import sample_ref as sr
import shape_cases as sc
import temper_ref as tr
from conftest import pkg
from infer_cases import (BETAS, BETAS3, FLAT_ENSEMBLE, FLAT_MALA, FLAT_TEMPER, N_SE, RUNS, SPREAD, evidence_quadrature, flat_starts, ladder_lz, mixed_prior,
                         moment_z, near, nested_reference, problem, run_stats, second_moment, tempered_reference, z_of)
from infer_support import alpha_bound_prior, alpha_of, posterior_eval


def flat_ev(u):
    n, d = np.shape(u)
    return np.zeros(n), np.zeros((n, d)), np.zeros((n, d, d))


# ---- the Prior class
def par_train():
    return pkg("synth").make_params(2000, seed=1)


def test_prior_parsing_errors():
    P = pkg("priors").Prior
    for bad, word in (({"tauu": ("normal", 0.05, 0.01)}, "tauu"), ({"fstar": ("normal", 0.1, 0.01)}, "fstar"),
                      ({"tau": ("lognormal", -1.0, 0.1)}, "tau"), ({"alpha": ("normal", 1.0, 0.0)}, "alpha"),
                      ({"nu_min": ("cauchy", 1.0, 0.1)}, "nu_min"), ({"Vc": "flat"}, "Vc"), ({"Rmfp": ("normal", 1.0)}, "Rmfp"),
                      ({"fx": ("lognormal", float("nan"), 0.1)}, "fx")):
        with pytest.raises(ValueError, match=word):
            P(bad)
    p = P({"tau": "uniform"})
    assert p.spec == {} and np.all(p.to_u(par_train())[0] == 0)
    assert P.of(None) is None and P.of(p) is p and isinstance(P.of({"tau": ("normal", 0.06, 0.01)}), P)
    with pytest.raises(ValueError):
        P({"tau": ("normal", 0.06, 0.01)}).to_u()  # (no training parameters to take the box from)


def test_to_u_is_par_transform():
    P, pp = pkg("priors").Prior, pkg("preprocess")
    pt = par_train()
    mid = np.median(pt, axis=0)
    p = P({"tau": ("normal", 0.06, 0.01), "fx": ("lognormal", -1.5, 0.4)}, pt)
    kind, mu, sd = p.to_u()
    assert list(kind) == [0, 0, 1, 1, 0, 0, 0]
    rows = np.tile(mid, (3, 1))
    rows[:, 3] = [0.06, 0.07, 0.05]
    rows[:, 2] = 10.0 ** np.array([-1.5, -1.1, -1.9])
    u = pp.par_transform(rows, pt)
    for j in (2, 3):
        np.testing.assert_allclose([mu[j], mu[j] + sd[j], mu[j] - sd[j]], u[:, j], rtol=0, atol=1e-12)
    assert np.all(mu[kind == 0] == 0) and np.all(sd[kind == 0] == 1)


def test_ppf_inverts_the_cdf_and_density_integrates():
    P = pkg("priors").Prior
    pt = par_train()
    # one and two normal columns, one mode outside the box
    for spec in ({"tau": ("normal", 0.06, 0.01)}, {"tau": ("normal", 0.06, 0.01), "alpha": ("normal", float(pt[:, 4].max()) + 0.2 * float(np.ptp(pt[:, 4])), 0.1 * float(np.ptp(pt[:, 4])))}):
        p = P(spec, pt)
        kind, mu, sd = p.to_u()
        cols = np.flatnonzero(kind)
        c = np.random.default_rng(3).uniform(size=(4001, 7))
        c[0], c[1] = 2.0 ** -33, 1.0 - 2.0 ** -33
        u = p.ppf_u(c)
        assert np.all(np.abs(u) <= 1.0) and np.array_equal(u[:, kind == 0], (2.0 * c - 1.0)[:, kind == 0])
        for j in cols:
            a, b, z = (-1.0 - mu[j]) / sd[j], (1.0 - mu[j]) / sd[j], (u[:, j] - mu[j]) / sd[j]
            # (the CDF in the tail the quantile was taken in)
            cdf = (ndtr(-a) - ndtr(-z)) / (ndtr(-a) - ndtr(-b)) if a + b > 0 else (ndtr(z) - ndtr(a)) / (ndtr(b) - ndtr(a))
            assert np.max(np.abs(cdf - c[:, j])) < 1e-12, (j, np.max(np.abs(cdf - c[:, j])))
        np.testing.assert_allclose(u, pr.ppf(pr.as_prior(kind, mu, sd), c), rtol=0, atol=1e-15)
        # the density relative to the uniform prior integrates to 2^d over the box: Gauss-Legendre per normal column
        x, w = np.polynomial.legendre.leggauss(400)
        if len(cols) == 1:
            pts = np.zeros((400, 7))
            pts[:, cols[0]] = x
            total = np.sum(w * np.exp(p.log_density_u(pts)))
        else:
            X, Y = np.meshgrid(x, x, indexing="ij")
            pts = np.zeros((400 * 400, 7))
            pts[:, cols[0]], pts[:, cols[1]] = X.ravel(), Y.ravel()
            total = np.sum(np.outer(w, w).ravel() * np.exp(p.log_density_u(pts)))
        assert abs(total / 2.0 ** len(cols) - 1.0) < 1e-10, total
        # ... and equals the reference's unnormalised density minus its norm
        q = np.random.default_rng(4).uniform(-1, 1, size=(50, 7))
        ref = pr.log_prior((kind, mu, sd), q) - pr.log_norm((kind, mu, sd))
        np.testing.assert_allclose(p.log_density_u(q), ref, rtol=0, atol=1e-12)
    assert P({}, pt).log_density_u(np.zeros(7)) == 0.0 and np.array_equal(P({}, pt).ppf_u(np.full(7, 0.25)), np.full(7, -0.5))


# ---- prior_ref against closed forms
def test_reference_pieces():
    prior = mixed_prior(7)
    u = np.random.default_rng(1).uniform(-1, 1, size=(5, 7))
    h = 1e-6
    for j in range(7):
        du = np.zeros(7)
        du[j] = h
        fd = (pr.log_prior(prior, u + du) - pr.log_prior(prior, u - du)) / (2 * h)
        np.testing.assert_allclose(pr.grad_log_prior(prior, u)[:, j], fd, rtol=1e-6, atol=1e-8)
    assert np.array_equal(np.diag(pr.precision(prior)), [0, 1 / 0.25 ** 2, 0, 0, 1 / 0.2 ** 2, 0, 0])
    m, v = pr.moments(prior)
    x, w = np.polynomial.legendre.leggauss(400)
    for j in (1, 4):
        pts = np.zeros((400, 7))
        pts[:, j] = x
        pj = pr.as_prior(np.eye(7, dtype=int)[j], prior[1], prior[2])  # (column j alone)
        dens = np.exp(pr.log_prior(pj, pts))
        Z = np.sum(w * dens)
        assert abs(np.sum(w * dens * x) / Z - m[j]) < 1e-12 and abs(np.sum(w * dens * x * x) / Z - m[j] ** 2 - v[j]) < 1e-12
        assert abs(math.log(Z / 2.0) - pr.log_norm(pj)) < 1e-12
    ev = pr.with_prior(flat_ev, prior)
    l, g, F = ev(u)
    assert np.array_equal(l, pr.log_prior(prior, u)) and np.array_equal(g, pr.grad_log_prior(prior, u)) and np.array_equal(F[2], pr.precision(prior))
    # drawn starts: the uniform columns are nested_ref's, the normal ones ppf of the same words
    s = pr.start_draws(prior, 3, np.arange(40), 7)
    s0 = nr.start_draws(3, np.arange(40), 7)
    assert s.dtype == np.float32 and np.array_equal(s[:, prior[0] == 0], s0[:, prior[0] == 0]) and np.all(s[:, 4] < -0.5)


def test_beta_zero_rung_of_the_reference_samples_the_prior():
    """the tempered reference on a likelihood that is NOT flat (a Gaussian in u): the beta = 0 rung has the truncated
    normal's mean and variance per column, the beta = 1 rung does not"""
    d, L = 2, 128
    prior = mixed_prior(d)

    def ev(u):
        u = np.asarray(u, np.float64)
        return -0.5 * np.sum((u - 0.5) ** 2, axis=1) / 0.01, -(u - 0.5) / 0.01, np.repeat(np.eye(d)[None] / 0.01, len(u), axis=0)
    r = pr.temper_ref(ev, prior, np.repeat(flat_starts(d, L, 2), 3, axis=0), BETAS3, swap_every=3, n_steps=500, n_warmup=150, thin=0, seed=2)
    zm, zv = moment_z(r["mean_u"][2::3], second_moment(r)[2::3], prior)
    print("beta = 0 rung: z mean %s, second moment %s" % (zm.round(2), zv.round(2)))
    assert np.all(zm < N_SE) and np.all(zv < N_SE)
    zm1, _ = moment_z(r["mean_u"][0::3], second_moment(r)[0::3], prior)
    assert np.all(zm1 > 4 * N_SE)
    assert r["swaps"] > 0


def gauss_gauss_lnz(d, s_l, prior):
    """ln of the mean under the normalised prior of exp(-|u|^2 / (2 s_l^2)), u in [-1, 1]^d, column by column in closed form"""
    kind, mu, sd = prior
    out = 0.0
    for i in range(d):
        if not kind[i]:
            out += nr.gauss_lnz(1, s_l)
            continue
        s2 = 1.0 / (1.0 / s_l ** 2 + 1.0 / sd[i] ** 2)
        m, s = s2 * mu[i] / sd[i] ** 2, math.sqrt(s2)
        mass = lambda c, w: ndtr((1.0 - c) / w) - ndtr((-1.0 - c) / w)
        out += math.log(s / sd[i]) - 0.5 * mu[i] ** 2 / (s_l ** 2 + sd[i] ** 2) + math.log(mass(m, s) / mass(mu[i], sd[i]))
    return out


@pytest.mark.parametrize("d,N", [(1, 16), (2, 32)])
def test_nested_reference_on_gaussian_times_gaussian(d, N):
    """the nested reference from starts drawn from the prior: ln Z of a Gaussian likelihood (width 0.3 at the centre)
    under a normal prior (0.5, 0.05) on column 0 within 5 standard errors of the closed form over 64 runs; without the
    prior's acceptance (the starts kept) it misses by far more"""
    kind, mu, sd = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    kind[0], mu[0], sd[0] = 1, 0.5, 0.05
    prior = pr.as_prior(kind, mu, sd)
    runs, sigma = 64, 0.3
    truth = gauss_gauss_lnz(d, sigma, prior)
    T = int(math.ceil((d * math.log(1.0 / sigma) + 12.0) / np.sum(1.0 / (N - np.arange(N // 2)))))
    u0 = pr.start_draws(prior, 1, np.arange(runs * N), d)
    out = {}
    for use in (True, False):
        r = pr.nested_ref(nr.gauss_lnl(sigma), prior, u0, N, T, seed=1, use_prior=use)
        out[use] = z_of(run_stats(r, N, runs)[0], truth)
    print("d=%d N=%d: closed form %.4f, z %.2f; without the prior's acceptance z %.2f" % (d, N, truth, out[True], out[False]))
    assert abs(out[True]) < N_SE
    assert abs(out[False]) > N_SE


# ---- the statistical tests of test_prior_gpu.py on the reference, at their seeds and sizes
def test_flat_runs_on_the_reference():
    c = FLAT_MALA
    prior = mixed_prior(c["d"])
    r = sr.sample_ref(pr.with_prior(flat_ev, prior), flat_starts(c["d"], c["chains"], 4), **c["opts"])
    zm, zv = moment_z(r["mean_u"], second_moment(r), prior)
    print("MALA: accept %.3f, z mean %s second moment %s" % (r["accept_rate"].mean(), zm.round(2), zv.round(2)))
    assert np.all(zm < N_SE) and np.all(zv < N_SE)
    c = FLAT_TEMPER
    prior = mixed_prior(c["d"])
    r = pr.temper_ref(flat_ev, prior, np.repeat(flat_starts(c["d"], c["ladders"], 4), 3, axis=0), BETAS3, swap_every=c["swap_every"], **c["opts"])
    for k in range(3):
        zm, zv = moment_z(r["mean_u"][k::3], second_moment(r)[k::3], prior)
        print("tempered rung %d: z mean %s second moment %s" % (k, zm.round(2), zv.round(2)))
        assert np.all(zm < N_SE) and np.all(zv < N_SE)
    c = FLAT_ENSEMBLE
    prior = mixed_prior(c["d"])
    r = er.ensemble_ref(pr.with_prior(lambda u: np.zeros(len(u)), prior), flat_starts(c["d"], c["W"] * c["ensembles"], 4), c["W"], **c["opts"])
    zm, zv = moment_z(*er.ensemble_estimates(r["mean_u"], r["cov_u"], c["W"]), prior)
    print("ensemble: accept %.3f, z mean %s second moment %s" % (r["accept_rate"].mean(), zm.round(2), zv.round(2)))
    assert np.all(zm < N_SE) and np.all(zv < N_SE)


@pytest.mark.parametrize("name", ["i1", "i2"])
def test_evidence_on_the_reference(name):
    """both estimators' references on the evidence problems under the prior: within 5 standard errors of the quadrature of
    L p over the box, and more than 5 away from the uniform prior's evidence (a sampler that ignores the record fails)"""
    lz_q, lz_flat, E_q = evidence_quadrature(name)
    r = tempered_reference(name)
    lz, se = ladder_lz(r["mean_lnl"])
    bias = tr.trapezoid(BETAS, E_q) - lz_q
    print("%s tempered: ln Z %.4f +- %.4f, quadrature %.4f (z %+.2f), trapezoid of the quadrature %+.4f off it, uniform prior %.4f"
          % (name, lz, se, lz_q, (lz - lz_q) / se, bias, lz_flat))
    assert abs(lz - lz_q) < N_SE * se and abs(lz - lz_flat) > N_SE * se
    assert abs(lz - tr.trapezoid(BETAS, E_q)) < N_SE * se
    rn, lzn = nested_reference(name)
    se_n = lzn.std(ddof=1) / math.sqrt(RUNS)
    print("%s nested: ln Z %.4f +- %.4f (z %+.2f), accept %.2f" % (name, lzn.mean(), se_n, (lzn.mean() - lz_q) / se_n, rn["accept_rate"].mean()))
    assert abs(lzn.mean() - lz_q) < N_SE * se_n and abs(lzn.mean() - lz_flat) > N_SE * se_n


def test_transition_cases_excuse_none_on_the_reference():
    """the one-transition tests of test_prior_gpu.py on the small stacks, with the float64 oracle in the device's place, at
    their seeds and row counts: no decision lies within the bound of its uniform (0 excused), and the nested rebuild's
    smallest |ln U - (ln p(y) - ln p(x))| is far above float64 rounding.  (D1's evaluations exist only on the device: its
    cases assert the same cap there.)"""
    p = problem("i2")
    prior = mixed_prior(2)
    for n, betas in ((3, None), (257, None), (6, BETAS3), (258, BETAS3)):
        beta = np.ones(n) if betas is None else BETAS3[np.arange(n) % 3]
        u0 = near(p["truth_u"], n, 5, 0.03).astype(np.float32).astype(np.float64)
        chains, eps = sc.CHAIN0 + np.arange(n), np.full(n, sc.EPS0)
        e0 = p["ev"](u0)
        t0 = posterior_eval(e0, u0, beta, prior)
        prop, _, _ = sr.propose(u0, t0[1], t0[2], eps, sr.normals(sc.SEED, chains, sc.STEP0, 2), sc.RIDGE)
        e1 = p["ev"](prop)
        la = alpha_of(u0, t0, prop, posterior_eval(e1, prop, beta, prior), eps, sc.RIDGE)
        bound = alpha_bound_prior(u0, e0, prop, e1, eps, sc.RIDGE, la, beta, prior) + 1e-12
        logu = np.log(sr.accept_uniform(sc.SEED, chains, sc.STEP0))
        assert not np.any(np.abs(logu - la) <= bound), (n, betas is None)
    # the ensemble sweep: two ensembles of 16 walkers
    st = p["stack"]
    lnl_of = er.forward_evaluator(st["Ws"], st["bs"], st["act"], p["data"], p["w"], st["tout"])
    W, n = 16, 32
    u = near(p["truth_u"], n, W, SPREAD).astype(np.float32).astype(np.float64)
    r = er.ensemble_ref(pr.with_prior(lnl_of, prior), u, W, n_steps=1, n_warmup=0, seed=100 + W, chain0=11, step0=40)
    _, _, logu = er.draws(100 + W, 11 + np.arange(n), 40, 2.0, W // 2)
    fin = np.isfinite(r["last_log_alpha"])
    assert np.min(np.abs(logu - r["last_log_alpha"])[fin]) > 1e-3  # (a float32 ulp of ln L ~ 40 is 4e-6)
    # the nested rebuild on the 1-input stack
    p1 = problem("i1")
    s1 = p1["stack"]
    ev1 = er.forward_evaluator(s1["Ws"], s1["bs"], s1["act"], p1["data"], p1["w"], s1["tout"])
    for runs in (1, 5):
        ref = pr.nested_ref(ev1, mixed_prior(1), near(p1["truth_u"], 16 * runs, 16 + runs, SPREAD), 16, n_iter=2, n_repeats=2, seed=116,
                            chain0=176, iter0=40)
        assert ref["min_margin"] > 1e-9, (runs, ref["min_margin"])


# ---- the binding without a device
def test_abi_symbol_and_null_checks():
    nat = pkg("_native")
    assert "v21_mlp_set_prior" in nat.SIGNATURES
    lib = nat.load_library()
    assert hasattr(lib, "v21_mlp_set_prior")
    kind, one = (C.c_int32 * 1)(1), (C.c_double * 1)(0.5)
    assert lib.v21_mlp_set_prior(None, None, None, None, 0) == -1
    assert lib.v21_mlp_set_prior(None, kind, one, one, 1) == -1


def test_use_prior_caches_by_value():
    """Stack.use_prior sets the record only when it changed and clears it only when there is one (on a stack object
    without a device: the calls are counted)"""
    nat = pkg("_native")
    st = object.__new__(nat.Stack)
    calls = []
    st.prior_record = None
    st.set_prior = lambda *a: calls.append(a[0] is not None)
    rec = (np.array([0, 1], np.int32), np.array([0.0, 0.3]), np.array([1.0, 0.2]))
    st.use_prior(None)
    assert calls == []
    st.use_prior(rec)
    st.use_prior(tuple(a.copy() for a in rec))
    assert calls == [True] and all(np.array_equal(a, b) for a, b in zip(st.prior_record, rec))
    st.use_prior((rec[0], rec[1], np.array([1.0, 0.25])))
    assert calls == [True, True]
    st.use_prior(None)
    assert calls == [True, True, False]
    with pytest.raises(ValueError):
        nat.Stack.set_prior(st, [0, 1], [0.0], [1.0, 1.0])
