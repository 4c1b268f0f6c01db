"""CPU: the float64 references of the four samplers' transitions with a hold mask (tests/hold_ref.py) pinned to the
existing references on the reduced problem, the control that shows the ensemble's (d_free - 1) ln z is tested, the
conditional evidence of the i2 problem with a column held against a 1-D midpoint rule, and the surface of
v21_mlp_set_hold (no GPU needed).  The cases, sizes and seeds shared with the GPU file (tests/test_hold_gpu.py) live in
tests/hold_ref.py."""
import math
import os
import re

import numpy as np
import pytest

import ensemble_ref as er
import hold_ref as hr
import infer_cases as ic
import prior_ref as pr
import sample_ref as sr
import temper_ref as tr
from conftest import ROOT, pkg
from infer_cases import BETAS3, N_SE

_cache = {}


# ---- the shared cases
def gauss_evaluator(d, seed):
    """a correlated Gaussian ln L on d columns -> ev: u (n, d) -> (lnl, g, F), and the forward-only u -> lnl"""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(d, d))
    A = B @ B.T / d + 4.0 * np.eye(d)
    m = rng.uniform(-0.3, 0.3, size=d)

    def ev(u):
        r = np.asarray(u, np.float64) - m
        return -0.5 * np.einsum("ni,ij,nj->n", r, A, r), -r @ A, np.broadcast_to(A, (r.shape[0], d, d)).copy()
    return ev, lambda u: ev(u)[0]


def flat_ensemble_runs():
    """the flat-likelihood ensemble case of the GPU file on the reference: d = 4, column 3 held; the correct reference and
    the one with (d - 1) ln z -> z of the free columns' mean and second moment against 0 and 1 / 3; computed once"""
    if "flat" not in _cache:
        c = hr.FLAT_ENSEMBLE
        hold = hr.as_hold(*hr.FLAT_HOLD)
        u0 = ic.flat_starts(c["d"], c["W"] * c["ensembles"], 4)
        out = {}
        for wrong in (False, True):
            r = hr.ensemble_ref(lambda u: np.zeros(u.shape[0]), hold, u0, c["W"], count_held=wrong, **c["opts"])
            m, m2 = er.ensemble_estimates(r["mean_u"], r["cov_u"], c["W"])
            out[wrong] = (sr.pooled_check(m[:, :3], 0.0)[1], sr.pooled_check(m2[:, :3], 1.0 / 3.0)[1], r)
        _cache["flat"] = out
    return _cache["flat"]


def conditional_tempered_reference():
    """hold_ref.temper_ref on the conditional problem on hold_ref.HELD_BETAS, at the tempering tests' run and starts; computed once"""
    if "tref" not in _cache:
        p = ic.problem("i2")
        _cache["tref"] = hr.temper_ref(p["ev"], hr.uniform_prior(2), hr.held_hold(), hr.held_starts(), hr.HELD_BETAS, swap_every=ic.SWAP_EVERY, **ic.RUN)
    return _cache["tref"]


def conditional_nested_reference():
    """hold_ref.nested_ref on the conditional problem from drawn starts, at the nested tests' sizes; -> (result, ln Z per run)"""
    if "nref" not in _cache:
        p, (N, T) = ic.problem("i2"), ic.QUAD["i2"]
        st = p["stack"]
        ev = er.forward_evaluator(st["Ws"], st["bs"], st["act"], p["data"], p["w"], st["tout"])
        prior, hold = hr.uniform_prior(2), hr.held_hold()
        r = hr.nested_ref(ev, prior, hold, hr.start_draws(prior, hold, ic.SEED, np.arange(ic.RUNS * N), 2), N, T, seed=ic.SEED)
        _cache["nref"] = (r, ic.run_stats(r, N, ic.RUNS)[0])
    return _cache["nref"]


# ---- 1. the references with the last column held are the existing references on the reduced problem
def close(a, b, tag):
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12, err_msg=tag)


@pytest.mark.parametrize("case", ["gauss4", "i2"])
def test_references_equal_the_reduced_problem(case):
    if case == "gauss4":
        d = 4
        ev, lnl = gauss_evaluator(d, 2)
        prior = ic.mixed_prior(d)  # (normal columns 0 and 3: the held one carries a normal that must not be read)
    else:
        p, d = ic.problem("i2"), 2
        ev, lnl = p["ev"], (lambda u: p["ev"](u)[0])
        prior = ic.mixed_prior(d)
    assert prior[0][d - 1] == 1
    mask = np.zeros(d, int)
    mask[d - 1] = 1
    hold = hr.as_hold(mask, np.full(d, 0.3))
    red_prior = tuple(a[:d - 1] for a in prior)
    rev, rlnl = hr.reduced_evaluator(ev, hold), hr.reduced_evaluator(lnl, hold)
    u0 = ic.scattered_u(d, 96, 8) * 0.5
    hv = hold[1][d - 1]
    # MALA under the uniform prior: sample_ref
    opts = dict(n_steps=12, n_warmup=8, eps0=0.7, seed=5, chain0=3, step0=7)
    a, b = hr.temper_ref(ev, hr.uniform_prior(d), hold, u0, **opts), sr.sample_ref(rev, u0[:, :d - 1], **opts)
    for k in ("u", "mean_u", "last_prop_u", "samples_u"):
        close(a[k][..., :d - 1], b[k], "MALA " + k)
        assert np.all(a[k][..., d - 1] == hv), k
    for k in ("lnl", "eps", "accept_rate", "last_log_alpha", "samples_lnl"):
        close(a[k], b[k], "MALA " + k)
    close(a["cov_u"][:, :d - 1, :d - 1], b["cov_u"], "MALA cov_u")
    assert np.all(a["cov_u"][:, d - 1, :] == 0) and np.all(a["cov_u"][:, :, d - 1] == 0)
    assert 0.1 < a["accept_rate"].mean() < 0.95
    # tempered under the mixed prior, with swaps: prior_ref.temper_ref
    topts = dict(swap_every=2, **opts)
    a, b = hr.temper_ref(ev, prior, hold, u0, BETAS3, **topts), pr.temper_ref(rev, red_prior, u0[:, :d - 1], BETAS3, **topts)
    for k in ("u", "mean_u", "last_prop_u"):
        close(a[k][..., :d - 1], b[k], "tempered " + k)
    for k in ("lnl", "eps", "accept_rate", "last_log_alpha", "mean_lnl", "var_lnl", "swap_accept"):
        close(a[k], b[k], "tempered " + k)
    assert b["swaps"] > 0
    # ensemble: ensemble_ref on the evaluator of L p
    eopts = dict(a=2.0, n_steps=10, n_warmup=6, seed=5, chain0=3, step0=7)
    a, b = hr.ensemble_ref(lnl, hold, u0, 16, prior=prior, **eopts), er.ensemble_ref(pr.with_prior(rlnl, red_prior), u0[:, :d - 1], 16, **eopts)
    for k in ("u", "mean_u", "last_prop_u"):
        close(a[k][..., :d - 1], b[k], "ensemble " + k)
        assert np.all(a[k][..., d - 1] == hv), k
    close(a["lnl"], b["lnl"] - pr.log_prior(red_prior, b["u"]), "ensemble lnl")
    close(a["last_log_alpha"], b["last_log_alpha"], "ensemble log alpha")
    assert np.array_equal(a["last_partner"], b["last_partner"]) and np.array_equal(a["accept_rate"], b["accept_rate"])
    # nested: prior_ref.nested_ref, n_repeats and gamma spelt out (their defaults follow the column count)
    nopts = dict(n_repeats=3, gamma=0.8, seed=5, chain0=32, iter0=2)
    s0 = hr.start_draws(prior, hold, 5, np.arange(96), d)
    assert np.array_equal(s0[:, :d - 1], pr.start_draws(red_prior, 5, np.arange(96), d - 1)) and np.all(s0[:, d - 1] == np.float32(hv))
    a, b = hr.nested_ref(lnl, prior, hold, s0, 16, 4, **nopts), pr.nested_ref(rlnl, red_prior, s0[:, :d - 1], 16, 4, **nopts)
    for k in ("dead_u", "live_u", "last_prop_u"):
        assert np.array_equal(a[k][..., :d - 1], b[k]), k
    for k in ("dead_lnl", "lstar", "live_lnl", "accept_rate", "last_partner"):
        close(a[k], b[k], "nested " + k)
    assert 0.0 < a["accept_rate"].mean() < 1.0


# ---- 2. a control that must fail
def test_the_ensemble_control_fails_the_bound():
    """a flat likelihood, d = 4 with one column held, hold_ref.FLAT_ENSEMBLE: with (d_free - 1) ln z the free columns have
    the uniform's mean and second moment within N_SE standard errors; with (d - 1) ln z the second moment is missed by at
    least 4 N_SE"""
    runs = flat_ensemble_runs()
    zm, zv, r = runs[False]
    zm_w, zv_w, _ = runs[True]
    print("flat ensemble, column 3 held: z mean %s second moment %s; with (d - 1) ln z: mean %s second moment %s"
          % (zm.round(2), zv.round(2), zm_w.round(2), zv_w.round(2)))
    assert np.all(zm < N_SE) and np.all(zv < N_SE), (zm, zv)
    assert np.all(zv_w >= 4.0 * N_SE), zv_w
    assert np.all(r["mean_u"][:, 3] == np.float32(0.25)) and np.all(r["cov_u"][:, 3, :] == 0) and np.all(r["cov_u"][:, :, 3] == 0)


# ---- 3. the conditional evidence
def test_conditional_evidence_of_the_references():
    lz_q, lz_half, E_q = hr.conditional_quadrature()
    assert abs(lz_q - lz_half) <= 1e-6, (lz_q, lz_half)
    lz_t, se_t = hr.held_ladder_lz(conditional_tempered_reference()["mean_lnl"])
    lz_n = conditional_nested_reference()[1]
    se_n = lz_n.std(ddof=1) / math.sqrt(len(lz_n))
    print("i2, column 1 at %.1f: quadrature %.6f (half the cells %+.1e; its trapezoid %.4f); tempered reference %.4f +- %.4f (z %+.2f); "
          "nested reference %.4f +- %.4f (z %+.2f)" % (hr.HELD_U, lz_q, lz_half - lz_q, tr.trapezoid(hr.HELD_BETAS, E_q), lz_t, se_t, (lz_t - lz_q) / se_t,
                                                       lz_n.mean(), se_n, (lz_n.mean() - lz_q) / se_n))
    assert abs(lz_t - lz_q) < N_SE * se_t
    assert abs(lz_n.mean() - lz_q) < N_SE * se_n


# ---- 4. the surface
def test_abi_symbol_and_null_checks():
    nat = pkg("_native")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "v21.h")).read(), flags=re.S)
    assert re.search(r"\bv21_mlp_set_hold\s*\(", src)
    assert "v21_mlp_set_hold" in nat.SIGNATURES
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("library not built")
    lib = nat.load_library()
    assert hasattr(lib, "v21_mlp_set_hold")
    one = np.ones(1, np.int32)
    assert lib.v21_mlp_set_hold(None, None, None, 0) == -1
    assert lib.v21_mlp_set_hold(None, one.ctypes.data_as(nat.C.POINTER(nat.C.c_int32)), None, 1) == -1


def test_stack_set_hold_checks_its_arguments_and_use_hold_caches_by_value():
    nat = pkg("_native")
    st = object.__new__(nat.Stack)
    st.hold_record = None
    with pytest.raises(ValueError, match="one entry per input column"):
        nat.Stack.set_hold(st, [0, 1], [0.0])
    with pytest.raises(ValueError, match="needs its u"):
        nat.Stack.set_hold(st, [0, 1])
    calls = []
    st.set_hold = lambda *a: calls.append(a[0] is not None)
    st.use_hold(None)
    assert calls == []
    st.use_hold(([0, 1], [0.0, 0.4]))
    st.use_hold(([0, 1], [0.0, 0.4]))
    assert calls == [True]
    st.use_hold(([0, 1], [0.0, 0.5]))
    st.use_hold(None)
    st.use_hold(None)
    assert calls == [True, True, False]


def hostless_emulator():
    emu, synth = pkg("emulator"), pkg("synth")
    e = emu.Emulator.__new__(emu.Emulator)
    e.par_train = synth.make_params(500, seed=2, corners=True)
    e.par_labels = list(pkg("priors").PAR_LABELS)
    return e


def test_fixed_errors_come_before_any_device_work():
    """the four samplers validate ``fixed`` first: on an emulator object without a model nothing else could run"""
    e = hostless_emulator()
    pp = pkg("preprocess")
    hi = float(e.par_train[:, 3].max())
    spectrum = np.zeros(451, np.float32)
    for call in (e.sample_posterior, e.sample_ensemble, e.sample_tempered, e.nested_sample):
        with pytest.raises(ValueError, match="taus"):
            call(spectrum, 1.0, fixed={"taus": 0.05})
        with pytest.raises(ValueError, match="tau"):
            call(spectrum, 1.0, fixed={"tau": 2.0 * hi + 1.0})
        with pytest.raises(ValueError, match="every parameter"):
            call(spectrum, 1.0, fixed=dict(zip(e.par_labels, pp.par_untransform(np.zeros((1, 7)), e.par_train)[0])))
    hold, val, u = e._hold_u({"tau": hi})
    assert list(np.flatnonzero(hold)) == [3] and u[3] == pytest.approx(1.0, abs=1e-12) and np.all(u[~hold] == 0)
    # the pooled results of a call with a fixed column
    mean, cov, rh = e._held_results(hold, u, np.full(7, 0.1), np.full((7, 7), 0.2), np.full(7, 1.01))
    assert mean[3] == 1.0 and np.all(cov[3] == 0) and np.all(cov[:, 3] == 0) and np.isnan(rh[3]) and np.nanmax(rh) == 1.01
    assert cov[0, 1] == 0.2


def test_log_posterior_shapes_with_fixed():
    emu, pp = pkg("emulator"), pkg("preprocess")
    e = hostless_emulator()
    lo, hi = float(e.par_train[:, 3].min()), float(e.par_train[:, 3].max())
    lp = emu.LogPosterior.__new__(emu.LogPosterior)
    lp.em, lp.prior = e, None
    lp.hold, lp.held = e._fixed_columns({"tau": 0.5 * (lo + hi), "fx": 0.0})
    lp.ndim = int(np.count_nonzero(~lp.hold))
    assert lp.ndim == 5
    cube = np.random.default_rng(1).uniform(size=(9, 5))
    theta = lp.prior_transform(cube)
    assert theta.shape == (9, 5) and lp.prior_transform(cube[0]).shape == (5,)
    full = lp._full(theta)
    assert full.shape == (9, 7) and np.all(full[:, 3] == 0.5 * (lo + hi)) and np.all(full[:, 2] == 0.0)
    # the free columns in label order, uniform in u
    np.testing.assert_allclose(pp.par_transform(full, e.par_train)[:, ~lp.hold], 2.0 * cube - 1.0, atol=1e-9)
    assert np.all(lp.inside(theta)) and not lp.inside(theta[:1] * 0.0 - 1e9)[0]
    with pytest.raises(ValueError):
        lp.prior_transform(np.zeros((2, 7)))
    with pytest.raises(ValueError):
        lp(np.zeros((2, 7)))
