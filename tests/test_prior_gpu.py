"""The samplers' prior record on the GPU (include/v21.h: v21_mlp_set_prior): one transition of each of the four samplers
rebuilt in float64 with tests/prior_ref.py from the device's own evaluations and draws, the prior itself sampled on a flat
likelihood, both evidences against quadrature and the float64 references, bit-equality of everything without a record,
continuation and host chunks with a record, argument errors, and the emulator classes' ``prior=`` keyword.

The stacks: D1 (7 inputs, the fused routes; f32, f16, bf16) and the 1-, 2- and 4-input stacks of tests/shape_cases.py
(the padded columns of kFitMaxIn, one Philox block; generic routes, f32).  The cases, seeds and sizes shared with the
reference-only checks (tests/test_prior_cpu.py) live in tests/infer_cases.py.  Every test leaves its stack without a record: the
handles are shared with the other test files."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import ensemble_ref as er
import fit_ref as fr
import infer_cases as ic
import prior_ref as pr
import sample_ref as sr
import shape_cases as sc
import temper_ref as tr
from conftest import pkg
from infer_cases import BETAS3, N_SE, SPREAD, near
from infer_support import (alpha_bound_prior, alpha_of, dev_tempered, device_eval, device_stack, fit_setup, flags_of, posterior_eval, ready, same,
                           shape_setup, starts_in_box, u_of, ulp32)

pytestmark = pytest.mark.gpu


def same_results(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert same(a[k], b[k]), k


@contextlib.contextmanager
def prior_on(st, prior):
    """the record set for the block, and cleared after it whatever happens in it"""
    st.set_prior(*prior)
    try:
        yield
    finally:
        st.set_prior(None)


def small_setup(ctx, name):
    """the 1- or 2-input quadrature problem of infer_cases on the device -> (stack handle, problem, tin)"""
    p = ic.problem(name)
    st, rec = device_stack(ctx, p["dims"], p["act"])
    st.set_likelihood(p["data"], p["w"])
    return st, p, rec["tin"]


def untransform(u, tin):
    return fr.untransform(np.asarray(u, np.float64), tin[0], tin[2], tin[3])


def setup(ctx, which):
    """-> (stack, tin, truth in u (d,)) of D1 or of a small problem, its likelihood record set"""
    if which == "D1":
        st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
        return st, tin, u_of(truths[:1], tin)[0]
    st, p, tin = small_setup(ctx, which)
    return st, tin, p["truth_u"]


CASES = [("D1", "f32"), ("D1", "f16"), ("D1", "bf16"), ("i2", "f32")]


# ---- 1. one transition against the reference
def langevin_transition(st, nat, tin, x0, prec, prior, betas, tag):
    """one transition of sample (betas None) or sample_tempered under the record, rebuilt as
    test_temper_gpu.test_one_tempered_transition_against_reference rebuilds it: the proposal within one float32 ulp + 1e-12,
    log alpha within the first-order effect of one ulp of every evaluated input + 1e-12 (the prior's terms are float64 on
    both sides: that 1e-12, granted there for float64 rounding through the triangular solves, covers them too), the
    decisions equal outside that bound with at most 0.5 % excused.  -> share excused"""
    n, d = x0.shape
    T = 1 if betas is None else len(betas)
    beta = np.ones(n) if betas is None else np.asarray(betas)[np.arange(n) % T]
    flags = flags_of(nat, True)
    seed, chain0, step0, eps0, ridge = sc.SEED, sc.CHAIN0, sc.STEP0, sc.EPS0, sc.RIDGE
    u0 = st.sample(x0, prec, flags, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
    opts = dict(n_steps=1, n_warmup=0, eps0=eps0, ridge=ridge, seed=seed, chain0=chain0, step0=step0, diagnostics=True)
    with prior_on(st, prior):
        r = st.sample(x0, prec, flags, **opts) if betas is None else st.sample_tempered(x0, T, betas, 0, prec, flags, **opts)
    e0 = device_eval(st, nat, u0, prec)
    chains, eps = chain0 + np.arange(n), np.full(n, eps0)
    t0 = posterior_eval(e0, u0, beta, prior)
    prop_ref, _, inside = sr.propose(u0, t0[1], t0[2], eps, sr.normals(seed, chains, step0, d), ridge)
    prop = r["last_prop_u"].astype(np.float64)
    err, tol = np.abs(prop - prop_ref), np.spacing(np.abs(prop_ref).astype(np.float32)) + 1e-12
    print("%s: proposal max err / tol %.3f, inside %.3f" % (tag, np.max(err / tol), inside.mean()))
    assert np.all(err <= tol), (tag, np.max(err / tol))
    e1 = device_eval(st, nat, prop, prec)
    la = alpha_of(u0, t0, prop, posterior_eval(e1, prop, beta, prior), eps, ridge)
    bound = alpha_bound_prior(u0, e0, prop, e1, eps, ridge, la, beta, prior) + 1e-12
    la_dev = r["last_log_alpha"]
    fin = np.isfinite(la)
    assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), tag
    ratio = np.abs(la_dev[fin] - la[fin]) / bound[fin]
    # (the record is read: without the prior's terms log alpha is another number)
    la_flat = alpha_of(u0, [tr.tmul(beta, a) for a in e0], prop, [tr.tmul(beta, a) for a in e1], eps, ridge)
    print("%s: log alpha max |diff| %.3e, max diff / bound %.3f; the prior moves it by up to %.3g"
          % (tag, np.max(np.abs(la_dev[fin] - la[fin]), initial=0.0), ratio.max(initial=0.0), np.max(np.abs(la[fin] - la_flat[fin]), initial=0.0)))
    assert np.all(ratio <= 1.0), (tag, ratio.max())
    logu = np.log(sr.accept_uniform(seed, chains, step0))
    acc_ref, acc_dev = logu < la, r["accept_rate"] > 0.5
    excused = np.abs(logu - la) <= bound
    print("%s: accepted %.3f, excused %d of %d" % (tag, acc_dev.mean(), excused.sum(), n))
    assert excused.mean() <= 0.005, tag
    assert np.array_equal(acc_ref[~excused], acc_dev[~excused]), tag
    u1 = np.where(acc_dev[:, None], prop, u0)
    np.testing.assert_allclose(r["x_last"], untransform(u1, tin), rtol=1e-12)
    # the state keeps ln L alone
    np.testing.assert_allclose(r["lnl_last"], np.where(acc_dev, e1[0], e0[0]), rtol=1e-5)
    return excused.mean()


@pytest.mark.parametrize("which,prec", CASES)
def test_one_mala_transition_against_reference(ctx, which, prec):
    """3 rows (a partial workgroup) and 257 (a second one) under the mixed record"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    prior = ic.mixed_prior(len(truth))
    for n in (3, 257):
        langevin_transition(st, nat, tin, untransform(near(truth, n, 5, 0.03), tin), prec, prior, None, "MALA %s %s n=%d" % (which, prec, n))
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which,prec", CASES)
def test_one_tempered_transition_against_reference(ctx, which, prec):
    """the ladder (1, 0.3, 0), 2 ladders and 86 (85 per workgroup: a second workgroup) under the mixed record: the prior's
    terms enter unscaled, also at beta = 0"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    prior = ic.mixed_prior(len(truth))
    for ladders in (2, 86):
        x0 = untransform(near(truth, 3 * ladders, 5, 0.03), tin)
        langevin_transition(st, nat, tin, x0, prec, prior, BETAS3, "tempered %s %s ladders=%d" % (which, prec, ladders))
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which,prec", CASES)
def test_one_ensemble_sweep_against_reference(ctx, which, prec):
    """test_ensemble_gpu.test_one_sweep_against_reference under the mixed record, two ensembles of 16 walkers: partners and
    proposals bit-equal, log alpha = (d - 1) ln z + ln L(y) - ln L(x) + ln p(y) - ln p(x) within one float32 ulp of each of
    its two ln L (+ 1e-12 for the float64 rounding of the prior's terms), the decisions equal outside that bound, at most
    0.5 % (of 32: none) excused; lnl_last is loglike_fwd of the same u, bit for bit: ln L alone"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    ready(st, prec)
    d = len(truth)
    prior = ic.mixed_prior(d)
    a, W, E = 2.0, 16, 2
    n, H = W * E, W // 2
    seed, chain0, step0 = 100 + W, 11, 40
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, nat.FWD_OUT_TRANSFORM)
    x0 = untransform(near(truth, n, W, SPREAD), tin)
    u0 = st.sample_ensemble(x0, W, prec, flags_of(nat, True), n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
    with prior_on(st, prior):
        r = st.sample_ensemble(x0, W, prec, flags_of(nat, True), n_steps=1, n_warmup=0, a=a, seed=seed, chain0=chain0, step0=step0, diagnostics=True)
    e, h, _ = er.layout(n, W)
    z, k, logu = er.draws(seed, chain0 + np.arange(n), step0, a, H)
    acc_dev = r["accept_rate"] > 0.5
    u, lnl = u0.copy(), lnl_of(u0).astype(np.float64)
    excused_all, moved = 0, 0.0
    for hh in (0, 1):
        idx = np.flatnonzero(h == hh)
        prt = e[idx] * W + (1 - hh) * H + k[idx]
        tag = "%s %s set %d" % (which, prec, hh)
        assert np.array_equal(r["last_partner"][idx], prt - e[idx] * W), tag
        y = er.stretch(u[idx], u[prt], z[idx])
        assert same(y.astype(np.float32), r["last_prop_u"][idx]), tag
        inside = np.all(np.abs(y) <= 1.0, axis=1)
        lnl_y = lnl_of(y).astype(np.float64)
        dlp = pr.log_prior(prior, y) - pr.log_prior(prior, u[idx])
        la = np.where(inside, (d - 1) * np.log(z[idx]) + (lnl_y - lnl[idx]) + dlp, -np.inf)
        bound = ulp32(lnl[idx]) + ulp32(lnl_y) + 1e-12
        la_dev = r["last_log_alpha"][idx]
        assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), tag
        fin = np.isfinite(la)
        assert np.all(np.abs(la_dev[fin] - la[fin]) <= bound[fin]), (tag, float(np.max(np.abs(la_dev[fin] - la[fin]) / bound[fin])))
        moved = max(moved, float(np.max(np.abs(dlp[fin]) / bound[fin], initial=0.0)))
        excused = np.abs(logu[idx] - la) <= bound
        excused_all += int(excused.sum())
        assert np.array_equal((logu[idx] < la)[~excused], acc_dev[idx][~excused]), tag
        u[idx] = np.where(acc_dev[idx][:, None], y, u[idx])
        lnl[idx] = np.where(acc_dev[idx], lnl_y, lnl[idx])
    print("ENSEMBLE %s %s: accepted %.3f, excused %d of %d, the prior's term up to %.3g bounds" % (which, prec, acc_dev.mean(), excused_all, n, moved))
    assert excused_all <= 0.005 * n and moved > 10.0
    np.testing.assert_allclose(r["x_last"], untransform(u, tin), rtol=1e-12)
    assert same(r["lnl_last"], lnl_of(u)), (which, prec)
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which,prec,N", [("D1", "f32", 56), ("D1", "f16", 56), ("D1", "bf16", 56), ("i1", "f32", 16)])
def test_nested_iterations_against_rebuild(ctx, which, prec, N):
    """test_nested_gpu.test_iterations_against_rebuild under the mixed record, 1 run and 5: two iterations of two moves
    from given live points, every ln L taken from the device, the prior's acceptance ln U(block 4) < ln p(y) - ln p(x)
    rebuilt in float64 -- everything BIT-EQUAL, no decision excused: the reference reports the smallest
    |ln U - (ln p(y) - ln p(x))| it met, which is far above float64 rounding at these seeds"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    ready(st, prec)
    d = len(truth)
    prior = ic.mixed_prior(d)
    flags = nat.FWD_OUT_TRANSFORM
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, flags)
    taken = taken_plain = 0.0
    for runs in (1, 5):
        n, k = N * runs, N // 2
        opts = dict(n_iter=2, n_repeats=2, seed=100 + N, chain0=11 * N, iter0=40)
        u0 = near(truth, n, N + runs, SPREAD)
        r0 = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, n_iter=0)
        with prior_on(st, prior):
            r = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, diagnostics=True, **opts)
        plain = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, diagnostics=True, **opts)
        ref = pr.nested_ref(lnl_of, prior, u0, N, lnl0=r0["live_lnl"], **opts)
        tag = "%s %s N=%d runs=%d" % (which, prec, N, runs)
        print("NESTED %s: accepted %.3f (without the record %.3f), smallest margin %.3g" % (tag, r["accept_rate"].mean(), plain["accept_rate"].mean(),
                                                                                       ref["min_margin"]))
        assert ref["min_margin"] > 1e-9, tag
        assert same(r["dead_lnl"], ref["dead_lnl"].astype(np.float32)), tag
        assert same(r["dead_u"], ref["dead_u"].astype(np.float64)), tag
        assert same(r["lstar"], ref["lstar"].astype(np.float32)), tag
        assert np.array_equal(r["last_partner"], ref["last_partner"]), tag
        assert same(r["last_prop_u"], ref["last_prop_u"]), tag
        assert np.array_equal(r["accept_rate"], ref["accept_rate"]), tag
        assert same(r["live_u"], ref["live_u"].astype(np.float64)), tag
        assert same(r["live_lnl"], ref["live_lnl"].astype(np.float32)), tag
        taken, taken_plain = taken + r["accept_rate"].sum(), taken_plain + plain["accept_rate"].sum()
    # (the prior refused moves that ln L alone lets through)
    assert taken < taken_plain, (which, prec, taken, taken_plain)
    st.set_likelihood(None, None)


# ---- 2. the prior is really sampled
def test_flat_likelihood_mala(ctx):
    """all weights zero on D1: 256 chains under the mixed record have the truncated normal's mean and second moment in its
    two columns and 0, 1 / 3 in the uniform ones, within 5 standard errors over the chains"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    st.set_likelihood(data[0], np.zeros(dims[-1], np.float32))
    c = ic.FLAT_MALA
    prior = ic.mixed_prior(c["d"])
    with prior_on(st, prior):
        r = st.sample(untransform(ic.flat_starts(c["d"], c["chains"], 4), tin), "f32", flags_of(nat, True), **c["opts"])
    zm, zv = ic.moment_z(r["mean_u"], ic.second_moment(r), prior)
    print("MALA: accept %.3f, z mean %s second moment %s" % (r["accept_rate"].mean(), zm.round(2), zv.round(2)))
    assert np.all(r["lnl_last"] == 0) and np.all(zm < N_SE) and np.all(zv < N_SE), (zm, zv)
    st.set_likelihood(None, None)


def test_flat_likelihood_tempered(ctx):
    """all weights zero on the 2-input stack, ladder (1, 0.3, 0), 256 ladders: every rung -- the beta = 0 rung, which
    samples the prior whatever the likelihood, among them -- has the prior's moments; mean_lnl stays exactly 0"""
    nat = pkg("_native")
    st, p, tin = small_setup(ctx, "i2")
    st.set_likelihood(p["data"], np.zeros(p["dims"][-1], np.float32))
    c = ic.FLAT_TEMPER
    prior = ic.mixed_prior(c["d"])
    x0 = untransform(np.repeat(ic.flat_starts(c["d"], c["ladders"], 4), 3, axis=0), tin)
    with prior_on(st, prior):
        r = st.sample_tempered(x0, 3, BETAS3, c["swap_every"], "f32", flags_of(nat, True), **c["opts"])
    assert np.all(r["mean_lnl"] == 0) and np.all(r["lnl_last"] == 0)
    for k in range(3):
        zm, zv = ic.moment_z(r["mean_u"][k::3], ic.second_moment(r)[k::3], prior)
        print("tempered rung %d: accept %.3f, z mean %s second moment %s" % (k, r["accept_rate"][k::3].mean(), zm.round(2), zv.round(2)))
        assert np.all(zm < N_SE) and np.all(zv < N_SE), (k, zm, zv)
    st.set_likelihood(None, None)


def test_flat_likelihood_ensemble(ctx):
    """all weights zero on the 4-input stack: 64 ensembles of 16 walkers, per-ensemble estimates within 5 standard errors"""
    nat = pkg("_native")
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    st.set_likelihood(prob["data"][0], np.zeros(65, np.float32))
    c = ic.FLAT_ENSEMBLE
    prior = ic.mixed_prior(c["d"])
    x0 = untransform(ic.flat_starts(c["d"], c["W"] * c["ensembles"], 4), rec["tin"])
    with prior_on(st, prior):
        r = st.sample_ensemble(x0, c["W"], "f32", flags, **c["opts"])
    zm, zv = ic.moment_z(*er.ensemble_estimates(r["mean_u"], r["cov_u"], c["W"]), prior)
    print("ensemble: accept %.3f, z mean %s second moment %s" % (r["accept_rate"].mean(), zm.round(2), zv.round(2)))
    assert np.all(r["lnl_last"] == 0) and np.all(zm < N_SE) and np.all(zv < N_SE), (zm, zv)
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which,prec,N,runs", [("D1", "f16", 64, 8), ("i1", "f32", 16, 5)])
def test_flat_likelihood_nested(ctx, which, prec, N, runs):
    """test_nested_gpu.test_flat_target under the mixed record: ln Z is the constant ln L (0) to 1e-12, and -- ties
    everywhere, so iteration 0's dead points are the first half of the starts -- the drawn starts are prior_ref.ppf of
    the same Philox words to one float32 ulp; the uniform columns are exactly the draws made without a record"""
    nat, em = pkg("_native"), pkg("emulator")
    st, tin, truth = setup(ctx, which)
    d = len(truth)
    st.set_likelihood(np.zeros(st.dims[-1], np.float32), np.zeros(st.dims[-1], np.float32))
    prior = ic.mixed_prior(d)
    with prior_on(st, prior):
        r = st.sample_nested(None, N * runs, N, prec, nat.FWD_OUT_TRANSFORM, n_iter=3, seed=3, diagnostics=True)
    plain = st.sample_nested(None, N * runs, N, prec, nat.FWD_OUT_TRANSFORM, n_iter=3, seed=3)
    c = r["live_lnl"][0]
    assert np.all(r["live_lnl"] == c) and np.all(r["dead_lnl"] == c) and np.all(r["accept_rate"] == 0)
    lz = em.nested_evidence(r["dead_lnl"].transpose(1, 0, 2), r["live_lnl"].reshape(runs, N), N)[0]
    np.testing.assert_allclose(lz, 0.0, rtol=0, atol=1e-12)
    u0 = pr.start_draws(prior, 3, np.arange(N * runs), d).reshape(runs, N, d)[:, :N // 2].astype(np.float64)
    got = r["dead_u"][0]
    err = np.abs(got - u0) / ulp32(u0)
    print("NESTED %s: drawn starts max err %.2f ulp; column means %s" % (which, err.max(), got.reshape(-1, d).mean(axis=0).round(2)))
    assert np.all(err <= 1.0), err.max()
    uni = prior[0] == 0
    assert same(got[..., uni], plain["dead_u"][0][..., uni]) and not same(got[..., ~uni], plain["dead_u"][0][..., ~uni])
    st.set_likelihood(None, None)


# ---- 3. the evidence
@pytest.mark.parametrize("name", ["i1", "i2"])
def test_evidence_tempered(ctx, name):
    """test_temper_gpu.test_evidence_against_quadrature's problems, ladder and run under infer_cases.evidence_prior: ln Z
    within 5 standard errors (the scatter over the 64 ladders) of the quadrature of L p over the box and of the trapezoid
    of the quadrature's E_beta[ln L], within 5 (both errors) of prior_ref.temper_ref at the same seeds, and more than 5 away
    from the uniform prior's evidence"""
    nat = pkg("_native")
    st, p, tin = small_setup(ctx, name)
    lz_q, lz_flat, E_q = ic.evidence_quadrature(name)
    with prior_on(st, ic.evidence_prior(name)):
        r = st.sample_tempered(untransform(p["starts_u"], tin), ic.RUNGS, ic.BETAS, ic.SWAP_EVERY, "f32", flags_of(nat, True), **ic.RUN)
    lz, se = ic.ladder_lz(r["mean_lnl"])
    lz_r, se_r = ic.ladder_lz(ic.tempered_reference(name)["mean_lnl"])
    print("%s tempered: ln Z %.4f +- %.4f; quadrature %.4f (z %+.2f), its trapezoid z %+.2f; reference %.4f +- %.4f (z %+.2f); uniform prior %.4f"
          % (name, lz, se, lz_q, (lz - lz_q) / se, (lz - tr.trapezoid(ic.BETAS, E_q)) / se, lz_r, se_r, (lz - lz_r) / np.hypot(se, se_r), lz_flat))
    assert abs(lz - lz_q) < N_SE * se and abs(lz - tr.trapezoid(ic.BETAS, E_q)) < N_SE * se
    assert abs(lz - lz_r) < N_SE * np.hypot(se, se_r)
    assert abs(lz - lz_flat) > N_SE * se
    st.set_likelihood(None, None)


@pytest.mark.parametrize("name", ["i1", "i2"])
def test_evidence_nested(ctx, name):
    """test_nested_gpu.test_evidence_against_quadrature_and_reference's sizes under the same prior, starts drawn from it on
    the device: the same four bounds"""
    nat, em = pkg("_native"), pkg("emulator")
    st, p, tin = small_setup(ctx, name)
    N, T = ic.QUAD[name]
    lz_q, lz_flat, _ = ic.evidence_quadrature(name)
    with prior_on(st, ic.evidence_prior(name)):
        r = st.sample_nested(None, ic.RUNS * N, N, "f32", nat.FWD_OUT_TRANSFORM, n_iter=T, seed=ic.SEED)
    lz = em.nested_evidence(r["dead_lnl"].transpose(1, 0, 2), r["live_lnl"].reshape(ic.RUNS, N), N)[0]
    lz_ref = ic.nested_reference(name)[1]
    se, se_r = lz.std(ddof=1) / 8, lz_ref.std(ddof=1) / 8
    print("%s nested: ln Z %.4f +- %.4f; quadrature %.4f (z %+.2f); reference %.4f +- %.4f (z %+.2f); uniform prior %.4f; accept %.2f"
          % (name, lz.mean(), se, lz_q, (lz.mean() - lz_q) / se, lz_ref.mean(), se_r, (lz.mean() - lz_ref.mean()) / np.hypot(se, se_r), lz_flat,
             r["accept_rate"].mean()))
    assert abs(lz.mean() - lz_q) < N_SE * se
    assert abs(lz.mean() - lz_ref.mean()) < N_SE * np.hypot(se, se_r)
    assert abs(lz.mean() - lz_flat) > N_SE * se
    st.set_likelihood(None, None)


# ---- 4. nothing moves without a record
def sampler_calls(st, nat, x0, u0, prec, flags):
    """a seeded call of each sampler on the stack's record -> {sampler: results}"""
    n = x0.shape[0]
    return {"sample": st.sample(x0, prec, flags, n_steps=4, n_warmup=3, seed=9, diagnostics=True),
            "tempered": st.sample_tempered(x0[:n // 3 * 3], 3, BETAS3, 2, prec, flags, n_steps=4, n_warmup=3, seed=9, diagnostics=True),
            "ensemble": st.sample_ensemble(x0, 16, prec, flags, n_steps=3, n_warmup=2, seed=9, diagnostics=True),
            "nested": st.sample_nested(u0, n_live=16, precision=prec, flags=nat.FWD_OUT_TRANSFORM, n_iter=2, n_repeats=2, seed=9, diagnostics=True),
            "nested_drawn": st.sample_nested(None, n, 16, prec, nat.FWD_OUT_TRANSFORM, n_iter=2, n_repeats=2, seed=9, diagnostics=True)}


@pytest.mark.parametrize("which,prec", [("D1", "f16"), ("i2", "f32")])
def test_nothing_moves_without_a_record(ctx, which, prec):
    """every output of a seeded call of each sampler: with no record, with an all-uniform record and after set-then-clear
    the three are equal bit for bit, and a real record changes them; loglike, loglike_fwd, fisher and fit do not read it"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    d = len(truth)
    flags = flags_of(nat, True)
    u0 = near(truth, 48, 3, SPREAD)
    x0 = untransform(u0, tin)
    prior = ic.mixed_prior(d)
    none = sampler_calls(st, nat, x0, u0, prec, flags)
    others = lambda: {"loglike": st.loglike(x0, prec, flags), "loglike_fwd": st.loglike_fwd(x0, prec, flags),
                      "fisher": st.fisher(x0, prec, flags, lnl=True, grad=True), "fit": st.fit(x0, prec, flags, max_iter=5)}
    plain = others()
    try:
        st.set_prior(np.zeros(d, np.int32), np.full(d, 0.3), np.full(d, 0.1))
        uniform = sampler_calls(st, nat, x0, u0, prec, flags)
        st.set_prior(*prior)
        with_record = sampler_calls(st, nat, x0, u0, prec, flags)
        recorded = others()
        st.set_prior(None)
        cleared = sampler_calls(st, nat, x0, u0, prec, flags)
    finally:
        st.set_prior(None)
    for k in none:
        same_results(none[k], uniform[k])
        same_results(none[k], cleared[k])
        assert not same(none[k]["live_u" if k.startswith("nested") else "x_last"], with_record[k]["live_u" if k.startswith("nested") else "x_last"]), k
    for k, a in plain.items():
        b = recorded[k]
        if isinstance(a, dict):
            same_results(a, b)
        else:
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert same(x, y), k
    st.set_likelihood(None, None)


# ---- 5. continuation and chunking
def test_chunks_and_continuation(ctx):
    """test_temper_gpu.test_chunks_and_continuation under the mixed record (i4o65, T = 3, 8,220 rows: two host chunks of
    whole ladders): host form and _dev form agree bit for bit, one call of 6 transitions equals two of 3; and the split in
    two equals the whole for the plain, the ensemble and the nested sampler too"""
    nat = pkg("_native")
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    prior = ic.mixed_prior(4)
    T, n, betas = 3, 8220, [1.0, 0.3, 0.0]
    x64 = np.ascontiguousarray(np.tile(starts_in_box(rec, prob, 30, 12, 0.2), (n // 30, 1)))
    x32 = np.ascontiguousarray(x64.astype(np.float32))
    opts = dict(n_warmup=0, n_steps=6, thin=0, seed=5, eps0=0.6)
    half = dict(opts, n_steps=3)
    with prior_on(st, prior):
        host = st.sample_tempered(x32, T, betas, 2, "f32", flags, **opts)
        dev = dev_tempered(ctx, st, x32, "f32", flags, T, betas, 2, **opts)
        for k in dev:
            assert same(np.ascontiguousarray(host[k]), dev[k]), k
        whole = st.sample_tempered(x64, T, betas, 2, "f32", flags, **opts)
        first = st.sample_tempered(x64, T, betas, 2, "f32", flags, **half)
        second = st.sample_tempered(first["x_last"], T, betas, 2, "f32", flags, eps_start=first["eps_last"], **dict(half, step0=3))
        assert same(whole["x_last"], second["x_last"]) and same(whole["lnl_last"], second["lnl_last"]) and not same(whole["x_last"], first["x_last"])
        np.testing.assert_allclose(whole["mean_lnl"], (first["mean_lnl"] + second["mean_lnl"]) / 2, rtol=1e-12)
        x = x64[:96]
        whole = mala = st.sample(x, "f32", flags, **opts)
        first = st.sample(x, "f32", flags, **half)
        second = st.sample(first["x_last"], "f32", flags, eps_start=first["eps_last"], **dict(half, step0=3))
        assert same(whole["x_last"], second["x_last"]) and same(whole["lnl_last"], second["lnl_last"]) and not same(whole["x_last"], first["x_last"])
        eo = dict(n_warmup=0, n_steps=6, thin=0, seed=5)
        whole = st.sample_ensemble(x, 16, "f32", flags, **eo)
        first = st.sample_ensemble(x, 16, "f32", flags, **dict(eo, n_steps=3))
        second = st.sample_ensemble(first["x_last"], 16, "f32", flags, **dict(eo, n_steps=3, step0=3))
        assert same(whole["x_last"], second["x_last"]) and same(whole["lnl_last"], second["lnl_last"]) and not same(whole["x_last"], first["x_last"])
        no = dict(n_live=16, precision="f32", flags=nat.FWD_OUT_TRANSFORM, n_repeats=3, seed=5)
        whole = st.sample_nested(None, 96, n_iter=4, **no)
        first = st.sample_nested(None, 96, n_iter=2, **no)
        second = st.sample_nested(first["live_u"], n_iter=2, iter0=2, **no)
        assert same(whole["live_u"], second["live_u"]) and same(whole["live_lnl"], second["live_lnl"])
        assert same(whole["dead_u"], np.concatenate([first["dead_u"], second["dead_u"]])) and not same(whole["live_u"], first["live_u"])
    assert not same(st.sample(x, "f32", flags, **opts)["x_last"], mala["x_last"])  # (the record was read)
    st.set_likelihood(None, None)


# ---- 6. argument errors
def test_argument_errors_leave_the_handle_usable(ctx):
    """every refused case of include/v21.h returns V21_ERR_ARG and the record stays as it was: the sampler call after it
    returns the earlier result bit for bit; clearing by in_dim = 0 and by kind = NULL both give the no-record result"""
    nat = pkg("_native")
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    lib = st.lib
    x0 = starts_in_box(rec, prob, 32, 3, 0.05)
    run = lambda: st.sample_ensemble(x0, 16, "f32", flags, n_steps=3, n_warmup=2, seed=4, diagnostics=True)
    none = run()
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(kind, mu, sd, n=None):
        k, m, s = np.asarray(kind, np.int32), np.asarray(mu, np.float64), np.asarray(sd, np.float64)
        return lib.v21_mlp_set_prior(st.h, k.ctypes.data_as(I), m.ctypes.data_as(D), s.ctypes.data_as(D), len(k) if n is None else n)
    kind, mu, sd = ic.mixed_prior(4)
    try:
        assert call(kind, mu, sd) == 0
        before = run()
        assert not same(before["x_last"], none["x_last"])
        nan, inf = float("nan"), float("inf")
        bad = [(kind[:3], mu[:3], sd[:3], None), (np.r_[kind, 0], np.r_[mu, 0.0], np.r_[sd, 1.0], None), ([2, 0, 0, 0], mu, sd, None),
               ([-1, 0, 0, 1], mu, sd, None), (kind, mu, [0.25, 1, 1, 9e-4], None), (kind, mu, [nan, 1, 1, 0.2], None),
               (kind, mu, [0.25, 1, 1, inf], None), (kind, mu, [0.25, 1, 1, -0.2], None), (kind, [nan, 0, 0, -1.4], sd, None),
               (kind, [inf, 0, 0, -1.4], sd, None), (kind, [0.3, 0, 0, -2.01], sd, None), (kind, [2.26, 0, 0, -1.4], sd, None)]
        for k, m, s, n in bad:
            assert call(k, m, s, n) == -1, (list(k), list(m), list(s))
            same_results(run(), before)
        # (what is not read is not checked: mu and sd of a uniform column)
        assert call(kind, [0.3, nan, inf, -1.4], [0.25, -1.0, nan, 0.2]) == 0
        same_results(run(), before)
        assert call(kind, [0.3, 0, 0, -2.0], sd) == 0  # (5 sd outside: the last that is taken)
        assert lib.v21_mlp_set_prior(st.h, np.asarray(kind, np.int32).ctypes.data_as(I), None, None, 4) == -1
        assert call(kind, mu, sd, 0) == 0  # (in_dim = 0 clears)
        same_results(run(), none)
        assert call(kind, mu, sd) == 0
        assert lib.v21_mlp_set_prior(st.h, None, None, None, 4) == 0  # (kind = NULL clears)
        same_results(run(), none)
    finally:
        st.set_prior(None)
    st.set_likelihood(None, None)


# ---- 7. the class surface on the shipped model
def test_class_surface(shipped):
    emulator, synth, pp, priors = pkg("emulator"), pkg("synth"), pkg("preprocess"), pkg("priors")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    u_true = np.random.default_rng(4).uniform(-0.4, 0.4, size=(1, 7))
    truth = pp.par_untransform(u_true, ae.par_train)[0]
    spectrum = np.asarray(ae.predict(truth[None]), np.float32).reshape(-1)
    # a prior on tau inside its training range: the mean 0.15 in u above the truth's, the width 0.02 in u (at 50 mK the data
    # alone hold tau to about 0.08 in u: measured on the MI355X, variance 0.006)
    lo, hi = float(np.min(ae.par_train[:, 3])), float(np.max(ae.par_train[:, 3]))
    m_u, s_u = u_true[0, 3] + 0.15, 0.02
    spec = {"tau": ("normal", lo + (m_u + 1.0) * (hi - lo) / 2.0, s_u * (hi - lo) / 2.0)}
    kind, mu, sd = priors.Prior(spec).to_u(ae.par_train)
    assert list(kind) == [0, 0, 0, 1, 0, 0, 0] and abs(mu[3] - m_u) < 1e-9 and abs(sd[3] - s_u) < 1e-9
    sigma = 50.0  # mK
    tau_u = lambda params: pp.par_transform(params.reshape(-1, 7), ae.par_train)[:, 3].reshape(params.shape[:-1])
    checks = []
    for name, call, pool in (("sample_posterior", lambda **kw: ae.sample_posterior(spectrum, sigma, n_chains=64, n_steps=1000, n_warmup=300, p0=truth,
                                                                                 seed=2, **kw), lambda t: t),
                             ("sample_ensemble", lambda **kw: ae.sample_ensemble(spectrum, sigma, n_walkers=32, n_ensembles=16, n_steps=600,
                                                                               n_warmup=400, p0=truth, seed=2, **kw),
                              lambda t: t.reshape(t.shape[0], -1))):
        a, b = call(), call(prior=spec)
        again = call()
        assert same(a.params, again.params), name  # (the prior of the call before does not leak in)
        ta, tb = pool(tau_u(a.params)), pool(tau_u(b.params))  # (independent chains or ensembles, samples)
        va, vb = ta.var(axis=1), tb.var(axis=1)
        se = np.hypot(va.std(ddof=1), vb.std(ddof=1)) / np.sqrt(len(va))
        print("%s: tau in u without the prior %.3f (variance %.5f), with it %.3f (%.5f), prior mean %.3f; variance drop %.1f standard errors"
              % (name, a.mean_u[3], va.mean(), b.mean_u[3], vb.mean(), m_u, (va.mean() - vb.mean()) / se))
        checks.append((name, abs(b.mean_u[3] - m_u) < abs(a.mean_u[3] - m_u), va.mean() - vb.mean() > 5.0 * se))
    for name, toward, shrunk in checks:
        assert toward and shrunk, (name, toward, shrunk)
    r = ae.nested_sample(spectrum, sigma, n_live=64, n_runs=2, max_iter=64, prior=priors.Prior(spec))
    assert np.all(np.isfinite(r.log_evidence)) and np.isfinite(r.log_evidence_err)
    assert abs(np.sum(np.exp(r.log_weights)) - 1.0) < 1e-9
    assert abs(r.mean_u[3] - m_u) < abs(a.mean_u[3] - m_u)
    lp = ae.log_posterior(spectrum, sigma, prior=spec)
    theta = pp.par_untransform(np.random.default_rng(5).uniform(-0.9, 0.9, size=(9, 7)), ae.par_train)
    want = ae.log_likelihood(theta, spectrum, sigma, forward_only=True) + priors.Prior(spec, ae.par_train).log_density_u(pp.par_transform(theta, ae.par_train))
    np.testing.assert_allclose(lp(theta), want, rtol=1e-14, atol=0)
    assert np.array_equal(ae.log_posterior(spectrum, sigma)(theta), ae.log_likelihood(theta, spectrum, sigma, forward_only=True))
    cube = np.random.default_rng(6).uniform(size=(200, 7))
    draws = pp.par_transform(lp.prior_transform(cube), ae.par_train)
    assert abs(draws[:, 3].mean() - m_u) < 5 * s_u / np.sqrt(200) and np.allclose(np.delete(draws, 3, axis=1), np.delete(2 * cube - 1, 3, axis=1), atol=1e-9)
    with pytest.raises(ValueError, match="fstar"):
        ae.sample_posterior(spectrum, sigma, p0=truth, prior={"fstar": ("normal", 0.1, 0.01)})
