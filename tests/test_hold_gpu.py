"""The samplers' hold record on the GPU (include/v21.h: v21_mlp_set_hold): the record's refusals, bit-equality of everything
without a record and of everything that does not read it, one transition of each of the four samplers rebuilt in float64
from the device's own evaluations and draws ON THE REDUCED PROBLEM -- the free block of the evaluations through the
existing references and bounds of tests/test_prior_gpu.py, which know nothing of a hold --, the draws' independence of
what is held, split calls, the prior of the free columns sampled on a flat likelihood, the conditional evidence of the i2
problem against the quadrature of tests/hold_ref.py, and the emulator classes' ``fixed=`` keyword.

The stacks: D1 (7 inputs, the fused routes; f32, f16, bf16; columns 0 and 3 held), i8o64 (kFitMaxIn inputs, both Philox
blocks; column 0 held, and column 7) and the 2-input quadrature stack (column 1 held).  Every test leaves its stack without
a record: the handles are shared with the other test files."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import ensemble_ref as er
import fit_ref as fr
import hold_ref as hr
import infer_cases as ic
import prior_ref as pr
import sample_ref as sr
import shape_cases as sc
from conftest import pkg
from infer_cases import BETAS3, N_SE, SPREAD, near
from infer_support import (alpha_bound_prior, alpha_of, device_eval, device_stack, fit_setup, flags_of, posterior_eval, ready, same, shape_setup,
                           starts_in_box, u_of, ulp32)

pytestmark = pytest.mark.gpu


def same_results(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert same(a[k], b[k]), k


@contextlib.contextmanager
def records_on(st, hold, prior=None):
    """the hold record (and the prior record) set for the block, and cleared after it whatever happens in it"""
    st.set_hold(hold[0].astype(np.int32), hold[1])
    if prior is not None:
        st.set_prior(*prior)
    try:
        yield
    finally:
        st.set_hold(None)
        st.set_prior(None)


def untransform(u, tin):
    return fr.untransform(np.asarray(u, np.float64), tin[0], tin[2], tin[3])


def setup(ctx, which):
    """-> (stack, tin, truth in u (d,)) of D1, of a stack of shape_cases or of a quadrature problem, its likelihood record set"""
    if which == "D1":
        st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
        return st, tin, u_of(truths[:1], tin)[0]
    if which in sc.BY_NAME:
        st, rec, prob, _ = shape_setup(ctx, which)
        return st, rec["tin"], prob["truths_u"][0]
    p = ic.problem(which)
    st, rec = device_stack(ctx, p["dims"], p["act"])
    st.set_likelihood(p["data"], p["w"])
    return st, rec["tin"], p["truth_u"]


def case_records(d, held):
    """the hold of the columns `held` at scattered values, and the mixed record with a narrow normal on the first held column
    where it has none: a normal that must not be read (read, it would move every log alpha by thousands)"""
    mask = np.zeros(d, int)
    mask[list(held)] = 1
    hold = hr.as_hold(mask, np.linspace(-0.37, 0.41, d))
    kind, mu, sd = (a.copy() for a in ic.mixed_prior(d))
    j = held[0]
    if not kind[j]:
        kind[j], mu[j], sd[j] = 1, 0.9, 0.01
    assert kind[mask.astype(bool)].any() and kind[~mask.astype(bool)].any()
    return hold, pr.as_prior(kind, mu, sd)


def held_bits(a, hold, tag):
    """the held columns of float32 rows `a` are the record's float32, bit for bit"""
    m = hold[0]
    want = np.broadcast_to(hold[1][m].astype(np.float32), a[..., m].shape)
    assert same(np.ascontiguousarray(a[..., m], np.float32), np.ascontiguousarray(want)), tag


def held_raw(x, hold, tin, tag):
    """the held columns of raw rows `x` (float64) are box_to_raw of the record's float32"""
    m = hold[0]
    want = untransform(hold[1][None, :], tin)[0]
    np.testing.assert_allclose(x[..., m], np.broadcast_to(want[m], x[..., m].shape), rtol=1e-14, err_msg=tag)
    assert np.all(x[..., m] == x.reshape(-1, x.shape[-1])[0, m]), tag


# (stack, precision, held columns)
CASES = [("D1", "f32", (0, 3)), ("D1", "f16", (0, 3)), ("D1", "bf16", (0, 3)), ("i8o64", "f32", (0,)), ("i8o64", "f32", (7,)), ("i2", "f32", (1,))]


# ---- 1. the record
def test_refusals_leave_the_handle_and_the_record_as_they_were(ctx):
    nat = pkg("_native")
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    lib = st.lib
    x0 = starts_in_box(rec, prob, 32, 3, 0.05)
    run = lambda: st.sample_ensemble(x0, 16, "f32", flags, n_steps=3, n_warmup=2, seed=4, diagnostics=True)
    none = run()
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(mask, u, n=None, handle=None):
        m, v = np.asarray(mask, np.int32), np.asarray(u, np.float64)
        return lib.v21_mlp_set_hold(handle or st.h, m.ctypes.data_as(I), v.ctypes.data_as(D), len(m) if n is None else n)
    mask, u = [0, 1, 0, 1], [9.0, 0.3, float("nan"), -0.6]  # (what is not read is not checked: u of a free column)
    try:
        assert call(mask, u) == 0
        before = run()
        assert not same(before["x_last"], none["x_last"])
        held_bits(before["last_prop_u"], hr.as_hold(mask, np.where(mask, u, 0.0)), "ensemble proposals")
        nan, inf = float("nan"), float("inf")
        bad = [(mask[:3], u[:3]), (mask + [0], u + [0.0]), ([0, 2, 0, 1], u), ([0, -1, 0, 1], u), (mask, [0, nan, 0, -0.6]), (mask, [0, inf, 0, -0.6]),
               (mask, [0, 0.3, 0, -1.0000001]), (mask, [0, 1.0000001, 0, -0.6]), ([1, 1, 1, 1], [0.1, 0.2, 0.3, 0.4])]
        for m, v in bad:
            assert call(m, v) == -1, (m, v)
            same_results(run(), before)
        assert lib.v21_mlp_set_hold(st.h, np.asarray(mask, np.int32).ctypes.data_as(I), None, 4) == -1  # (a held column without u)
        same_results(run(), before)
        # more than kFitMaxIn inputs: refused
        case = sc.BY_NAME["i9o65"]
        wide, _ = device_stack(ctx, case.dims, case.act)
        assert call([1] + [0] * 8, [0.0] * 9, handle=wide.h) == -1
        assert call(mask, [0, 1.0, 0, -1.0]) == 0  # (the box's ends are inside)
        assert call(mask, u) == 0
        same_results(run(), before)
        assert call(mask, u, 0) == 0  # (in_dim = 0 clears)
        same_results(run(), none)
        assert call(mask, u) == 0
        assert lib.v21_mlp_set_hold(st.h, None, None, 4) == 0  # (hold = NULL clears)
        same_results(run(), none)
        assert call(mask, u) == 0
        assert call([0, 0, 0, 0], u) == 0  # (an all-zero mask clears)
        same_results(run(), none)
    finally:
        st.set_hold(None)
    st.set_likelihood(None, None)


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
    """every output of a seeded call of each sampler: with no record, with an all-zero mask and after set-then-clear the
    three are equal bit for bit, and a real record changes them; loglike, loglike_fwd, fisher, fit and fit_map (which keeps
    the hold mask of its own options) do not read it"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    d = len(truth)
    flags = flags_of(nat, True)
    u0 = near(truth, 48, 3, SPREAD)
    x0 = untransform(u0, tin)
    hold, prior = case_records(d, (d - 1,))
    own = np.zeros(d, np.int32)
    own[0] = 1
    none = sampler_calls(st, nat, x0, u0, prec, flags)
    others = lambda: {"loglike": st.loglike(x0, prec, flags), "loglike_fwd": st.loglike_fwd(x0, prec, flags),
                      "fisher": st.fisher(x0, prec, flags, lnl=True, grad=True), "fit": st.fit(x0, prec, flags, max_iter=5),
                      "fit_map": st.fit_map(x0, prec, flags, max_iter=5, hold=own), "fit_map_free": st.fit_map(x0, prec, flags, max_iter=5)}
    plain = others()
    try:
        st.set_hold(np.zeros(d, np.int32), np.full(d, 0.3))
        zero = sampler_calls(st, nat, x0, u0, prec, flags)
        st.set_hold(hold[0].astype(np.int32), hold[1])
        with_record = sampler_calls(st, nat, x0, u0, prec, flags)
        recorded = others()
        st.set_hold(None)
        cleared = sampler_calls(st, nat, x0, u0, prec, flags)
    finally:
        st.set_hold(None)
    for k in none:
        same_results(none[k], zero[k])
        same_results(none[k], cleared[k])
        last = "live_u" if k.startswith("nested") else "x_last"
        assert not same(none[k][last], with_record[k][last]), k
    for k, a in plain.items():
        b = recorded[k]
        if isinstance(a, dict):
            same_results(a, b)
        else:
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert same(x, y), k
    st.set_likelihood(None, None)


# ---- 2. one transition against the reference on the reduced problem
def langevin_transition(st, nat, tin, x0, prec, hold, prior, betas, tag):
    """one transition of sample (betas None) or sample_tempered under both records.  The rebuild is
    test_prior_gpu.langevin_transition's on the free block: the device's evaluations with the held rows and columns
    dropped, the prior's free columns, the normals of the free columns from the words they always had -- sample_ref.propose,
    infer_support.alpha_of and alpha_bound_prior then ARE the d_free-dimensional sampler.  The proposal's free columns
    within one float32 ulp + 1e-12, its held columns the record's float32, log alpha inside the bound of one ulp of every
    evaluated input + 1e-12, the decisions equal outside it with at most 0.5 % excused"""
    n, d = x0.shape
    free = ~hold[0]
    T = 1 if betas is None else len(betas)
    beta = np.ones(n) if betas is None else np.asarray(betas)[np.arange(n) % T]
    flags = flags_of(nat, True)
    seed, chain0, step0, eps0, ridge = sc.SEED, sc.CHAIN0, sc.STEP0, sc.EPS0, sc.RIDGE
    opts = dict(n_steps=1, n_warmup=0, eps0=eps0, ridge=ridge, seed=seed, chain0=chain0, step0=step0, diagnostics=True)
    with records_on(st, hold, prior):
        u0 = st.sample(x0, prec, flags, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"]
        r = st.sample(x0, prec, flags, **opts) if betas is None else st.sample_tempered(x0, T, betas, 0, prec, flags, **opts)
    held_bits(u0, hold, tag + " state")
    held_bits(r["last_prop_u"], hold, tag + " proposal")
    held_raw(r["x_last"], hold, tin, tag + " x_last")
    held_raw(r["samples"], hold, tin, tag + " samples")
    assert same(r["mean_u"][:, hold[0]], np.broadcast_to(hold[1][hold[0]], (n, int(hold[0].sum())))), tag
    assert np.all(r["cov_u"][:, hold[0], :] == 0) and np.all(r["cov_u"][:, :, hold[0]] == 0), tag
    u0 = u0.astype(np.float64)
    red = lambda e: (e[0], e[1][:, free], e[2][:, free][:, :, free])
    pf = tuple(a[free] for a in prior)
    e0 = device_eval(st, nat, u0, prec)
    chains, eps = chain0 + np.arange(n), np.full(n, eps0)
    t0 = posterior_eval(red(e0), u0[:, free], beta, pf)
    prop_ref, _, inside = sr.propose(u0[:, free], t0[1], t0[2], eps, sr.normals(seed, chains, step0, d)[:, free], ridge)
    prop = r["last_prop_u"].astype(np.float64)
    err, tol = np.abs(prop[:, free] - prop_ref), np.spacing(np.abs(prop_ref).astype(np.float32)) + 1e-12
    print("%s: proposal max err / tol %.3f, inside %.3f" % (tag, np.max(err / tol), inside.mean()))
    assert np.all(err <= tol), (tag, np.max(err / tol))
    e1 = device_eval(st, nat, prop, prec)
    la = alpha_of(u0[:, free], t0, prop[:, free], posterior_eval(red(e1), prop[:, free], beta, pf), eps, ridge)
    bound = alpha_bound_prior(u0[:, free], red(e0), prop[:, free], red(e1), eps, ridge, la, beta, pf) + 1e-12
    la_dev = r["last_log_alpha"]
    fin = np.isfinite(la)
    assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), tag
    ratio = np.abs(la_dev[fin] - la[fin]) / bound[fin]
    # (the hold is read: the d-dimensional log alpha under the whole record is another number)
    la_full = alpha_of(u0, posterior_eval(e0, u0, beta, prior), prop, posterior_eval(e1, prop, beta, prior), eps, ridge)
    both = fin & np.isfinite(la_full)
    print("%s: log alpha max |diff| %.3e, max diff / bound %.3f; without the hold it differs by up to %.3g"
          % (tag, np.max(np.abs(la_dev[fin] - la[fin]), initial=0.0), ratio.max(initial=0.0), np.max(np.abs(la[both] - la_full[both]), initial=0.0)))
    assert np.all(ratio <= 1.0), (tag, ratio.max())
    assert np.max(np.abs(la[both] - la_full[both]), initial=0.0) > 10.0 * np.max(bound[both], initial=0.0), tag
    logu = np.log(sr.accept_uniform(seed, chains, step0))
    acc_ref, acc_dev = logu < la, r["accept_rate"] > 0.5
    excused = np.abs(logu - la) <= bound
    print("%s: accepted %.3f, excused %d of %d" % (tag, acc_dev.mean(), excused.sum(), n))
    assert excused.mean() <= 0.005, tag
    assert np.array_equal(acc_ref[~excused], acc_dev[~excused]), tag
    u1 = np.where(acc_dev[:, None], prop, u0)
    np.testing.assert_allclose(r["x_last"], untransform(u1, tin), rtol=1e-12)
    np.testing.assert_allclose(r["lnl_last"], np.where(acc_dev, e1[0], e0[0]), rtol=1e-5)


@pytest.mark.parametrize("which,prec,held", CASES)
def test_one_mala_transition_against_reference(ctx, which, prec, held):
    """3 chains (a partial workgroup) and 257 (a second one)"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    hold, prior = case_records(len(truth), held)
    for n in (3, 257):
        x0 = untransform(near(truth, n, 5, 0.03), tin)
        langevin_transition(st, nat, tin, x0, prec, hold, prior, None, "MALA %s %s held %s n=%d" % (which, prec, held, n))
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which,prec,held", CASES)
def test_one_tempered_transition_against_reference(ctx, which, prec, held):
    """the ladder (1, 0.3, 0): 6 rows and 258 (255 per workgroup: a second workgroup)"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    hold, prior = case_records(len(truth), held)
    for n in (6, 258):
        x0 = untransform(near(truth, n, 5, 0.03), tin)
        langevin_transition(st, nat, tin, x0, prec, hold, prior, BETAS3, "tempered %s %s held %s n=%d" % (which, prec, held, n))
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which,prec,held", CASES)
def test_one_ensemble_sweep_against_reference(ctx, which, prec, held):
    """test_prior_gpu.test_one_ensemble_sweep_against_reference with the hold, 2 ensembles and 33 (a second workgroup) of
    16 walkers (18 on the 8-input stack, whose walker rule asks for 2 (8 + 1)): partners bit-equal, proposals bit-equal --
    in a held column the record's float32: the stretch returns it exactly --, log alpha = (d_free - 1) ln z + ln L(y) -
    ln L(x) + ln p(y) - ln p(x) over the free normal columns within one float32 ulp of each of its two ln L (+ 1e-12), the
    decisions equal outside that bound, at most 0.5 % excused; with (d - 1) ln z it is another number"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    ready(st, prec)
    d = len(truth)
    hold, prior = case_records(d, held)
    pf, d_free = hr.free_prior(prior, hold), int(np.sum(~hold[0]))
    a, W = 2.0, 16 if d < 8 else 18
    H = W // 2
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, nat.FWD_OUT_TRANSFORM)
    for E in (2, 33):
        n = W * E
        seed, chain0, step0 = 100 + W, 11, 40
        tag = "%s %s held %s E=%d" % (which, prec, held, E)
        x0 = untransform(near(truth, n, W, SPREAD), tin)
        with records_on(st, hold, prior):
            u0 = st.sample_ensemble(x0, W, prec, flags_of(nat, True), n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"]
            r = st.sample_ensemble(x0, W, prec, flags_of(nat, True), n_steps=1, n_warmup=0, a=a, seed=seed, chain0=chain0, step0=step0,
                                   diagnostics=True)
        held_bits(u0, hold, tag + " state")
        held_raw(r["x_last"], hold, tin, tag + " x_last")
        held_raw(r["samples"], hold, tin, tag + " samples")
        assert same(r["mean_u"][:, hold[0]], np.broadcast_to(hold[1][hold[0]], (n, d - d_free))), tag
        assert np.all(r["cov_u"][:, hold[0], :] == 0) and np.all(r["cov_u"][:, :, hold[0]] == 0), tag
        e, h, _ = er.layout(n, W)
        z, k, logu = er.draws(seed, chain0 + np.arange(n), step0, a, H)
        acc_dev = r["accept_rate"] > 0.5
        u, lnl = u0.astype(np.float64), lnl_of(u0).astype(np.float64)
        excused_all, moved = 0, 0.0
        for hh in (0, 1):
            idx = np.flatnonzero(h == hh)
            prt = e[idx] * W + (1 - hh) * H + k[idx]
            assert np.array_equal(r["last_partner"][idx], prt - e[idx] * W), tag
            y = er.stretch(u[idx], u[prt], z[idx])
            assert same(y.astype(np.float32), r["last_prop_u"][idx]), tag
            held_bits(r["last_prop_u"][idx], hold, tag + " proposal")
            inside = np.all(np.abs(y) <= 1.0, axis=1)
            lnl_y = lnl_of(y).astype(np.float64)
            la = np.where(inside, (d_free - 1) * np.log(z[idx]) + (lnl_y - lnl[idx]) + pr.log_prior(pf, y) - pr.log_prior(pf, u[idx]), -np.inf)
            bound = ulp32(lnl[idx]) + ulp32(lnl_y) + 1e-12
            la_dev = r["last_log_alpha"][idx]
            assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), tag
            fin = np.isfinite(la)
            assert np.all(np.abs(la_dev[fin] - la[fin]) <= bound[fin]), (tag, float(np.max(np.abs(la_dev[fin] - la[fin]) / bound[fin])))
            moved = max(moved, float(np.max(np.abs((d - d_free) * np.log(z[idx]))[fin] / bound[fin], initial=0.0)))
            excused = np.abs(logu[idx] - la) <= bound
            excused_all += int(excused.sum())
            assert np.array_equal((logu[idx] < la)[~excused], acc_dev[idx][~excused]), tag
            u[idx] = np.where(acc_dev[idx][:, None], y, u[idx])
            lnl[idx] = np.where(acc_dev[idx], lnl_y, lnl[idx])
        print("ENSEMBLE %s: accepted %.3f, excused %d of %d, the held columns' ln z up to %.3g bounds" % (tag, acc_dev.mean(), excused_all, n, moved))
        assert excused_all <= max(0.005 * n, 0) and moved > 10.0
        np.testing.assert_allclose(r["x_last"], untransform(u, tin), rtol=1e-12)
        assert same(r["lnl_last"], lnl_of(u)), tag
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which,prec,held", CASES)
def test_nested_iterations_against_rebuild(ctx, which, prec, held):
    """test_prior_gpu.test_nested_iterations_against_rebuild with the hold, N = 16, 1 run and 33 (16 per workgroup: a third
    workgroup): two iterations of two moves from given live points whose held columns the device overwrites, every ln L
    taken from the device -- everything BIT-EQUAL; dead_u, live_u and the proposals carry the record's float32.  Then
    drawn starts: the free columns keep their words (and their prior), a held column takes none"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, which)
    ready(st, prec)
    d = len(truth)
    hold, prior = case_records(d, held)
    flags, N = nat.FWD_OUT_TRANSFORM, 16
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, flags)
    for runs in (1, 33):
        n = N * runs
        opts = dict(n_iter=2, n_repeats=2, seed=100 + N, chain0=11 * N, iter0=40)
        u0 = near(truth, n, N + runs, SPREAD)
        tag = "%s %s held %s runs=%d" % (which, prec, held, runs)
        with records_on(st, hold, prior):
            r0 = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, n_iter=0)
            r = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, diagnostics=True, **opts)
            drawn = st.sample_nested(None, n, N, prec, flags, n_iter=0, seed=7, chain0=5)
        held_bits(r0["live_u"].astype(np.float32), hold, tag + " starts")
        assert same(r0["live_u"][:, ~hold[0]], u0.astype(np.float32).astype(np.float64)[:, ~hold[0]]), tag
        ref = hr.nested_ref(lnl_of, prior, hold, u0, N, lnl0=r0["live_lnl"], **opts)
        print("NESTED %s: accepted %.3f, smallest margin %.3g" % (tag, r["accept_rate"].mean(), ref["min_margin"]))
        assert ref["min_margin"] > 1e-9, tag
        assert same(r["dead_lnl"], ref["dead_lnl"].astype(np.float32)), tag
        assert same(r["dead_u"], ref["dead_u"].astype(np.float64)), tag
        assert same(r["lstar"], ref["lstar"].astype(np.float32)), tag
        assert np.array_equal(r["last_partner"], ref["last_partner"]), tag
        assert same(r["last_prop_u"], ref["last_prop_u"]), tag
        assert np.array_equal(r["accept_rate"], ref["accept_rate"]), tag
        assert same(r["live_u"], ref["live_u"].astype(np.float64)), tag
        assert same(r["live_lnl"], ref["live_lnl"].astype(np.float32)), tag
        for k in ("dead_u", "live_u", "last_prop_u"):
            held_bits(r[k].astype(np.float32), hold, tag + " " + k)
        want = hr.start_draws(prior, hold, 7, 5 + np.arange(n), d).astype(np.float64)
        err = np.abs(drawn["live_u"] - want) / ulp32(want)
        assert np.all(err <= 1.0), (tag, err.max())
        held_bits(drawn["live_u"].astype(np.float32), hold, tag + " drawn starts")
    st.set_likelihood(None, None)


# ---- 3. a free column's draw does not depend on what is held
def test_draws_do_not_depend_on_what_is_held(ctx):
    """a flat likelihood on D1 (all weights zero), column 3 held: the first proposal of every sampler equals the no-hold
    call's in the free columns, bit for bit: MALA's (F = 0: the step is eps xi / sqrt(ridge) from the same words), the
    stretch's and the drawn nested starts"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    st.set_likelihood(data[0], np.zeros(dims[-1], np.float32))
    flags = flags_of(nat, True)
    hold = hr.as_hold([0, 0, 0, 1, 0, 0, 0], np.full(7, -0.21))
    free = ~hold[0]
    x0 = untransform(ic.flat_starts(7, 257, 4) * 0.5, tin)
    calls = {"MALA": lambda: st.sample(x0, "f32", flags, n_steps=1, n_warmup=0, eps0=0.3, seed=3, diagnostics=True)["last_prop_u"],
             "ensemble": lambda: st.sample_ensemble(x0[:256], 16, "f32", flags, n_steps=1, n_warmup=0, seed=3, diagnostics=True)["last_prop_u"],
             "nested": lambda: st.sample_nested(None, 256, 16, "f32", nat.FWD_OUT_TRANSFORM, n_iter=0, seed=3)["live_u"]}
    plain = {k: f() for k, f in calls.items()}
    with records_on(st, hold):
        held = {k: f() for k, f in calls.items()}
    # (of the stretch the first half-move's proposals, those of set 0: the second's start from positions that the first
    # half-move's decisions left, and those take (d_free - 1) ln z)
    rows = {"MALA": np.arange(257), "ensemble": np.flatnonzero(er.layout(256, 16)[1] == 0), "nested": np.arange(256)}
    for k in calls:
        assert same(plain[k][rows[k]][:, free], held[k][rows[k]][:, free]), k
        held_bits(np.asarray(held[k], np.float32), hold, k)
        assert not same(plain[k][:, ~free], held[k][:, ~free]), k
    st.set_likelihood(None, None)


# ---- 4. split calls
def test_split_calls_equal_the_whole(ctx):
    """with both records set (i4o65, column 2 held): a call split by step0 (the second half continuing the first) and a call
    split by chain0 (the rows in two calls) equal the whole call byte for byte, for all four samplers"""
    nat = pkg("_native")
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    hold, prior = case_records(4, (2,))
    x = np.ascontiguousarray(starts_in_box(rec, prob, 96, 12, 0.2))
    opts = dict(n_warmup=0, n_steps=6, thin=0, seed=5, eps0=0.6)
    half = dict(opts, n_steps=3)
    with records_on(st, hold, prior):
        for name, run in (("MALA", lambda x, **o: st.sample(x, "f32", flags, **o)),
                          ("tempered", lambda x, **o: st.sample_tempered(x, 3, BETAS3, 2, "f32", flags, **o))):
            whole = run(x, **opts)
            first = run(x, **half)
            second = run(first["x_last"], eps_start=first["eps_last"], **dict(half, step0=3))
            assert same(whole["x_last"], second["x_last"]) and same(whole["lnl_last"], second["lnl_last"]) and not same(whole["x_last"], first["x_last"]), name
            a, b = run(x[:48], **opts), run(x[48:], **dict(opts, chain0=48))
            for k in ("x_last", "lnl_last", "mean_u", "cov_u", "accept_rate"):
                assert same(whole[k], np.concatenate([a[k], b[k]])), (name, k)
        eo = dict(n_warmup=0, n_steps=6, thin=0, seed=5)
        whole = st.sample_ensemble(x, 16, "f32", flags, **eo)
        first = st.sample_ensemble(x, 16, "f32", flags, **dict(eo, n_steps=3))
        second = st.sample_ensemble(first["x_last"], 16, "f32", flags, **dict(eo, n_steps=3, step0=3))
        assert same(whole["x_last"], second["x_last"]) and same(whole["lnl_last"], second["lnl_last"]) and not same(whole["x_last"], first["x_last"])
        a, b = st.sample_ensemble(x[:48], 16, "f32", flags, **eo), st.sample_ensemble(x[48:], 16, "f32", flags, **dict(eo, chain0=48))
        for k in ("x_last", "lnl_last", "mean_u", "cov_u"):
            assert same(whole[k], np.concatenate([a[k], b[k]])), ("ensemble", k)
        no = dict(n_live=16, precision="f32", flags=nat.FWD_OUT_TRANSFORM, n_repeats=3, seed=5)
        whole = st.sample_nested(None, 96, n_iter=4, **no)
        first = st.sample_nested(None, 96, n_iter=2, **no)
        second = st.sample_nested(first["live_u"], n_iter=2, iter0=2, **no)
        assert same(whole["live_u"], second["live_u"]) and same(whole["live_lnl"], second["live_lnl"])
        assert same(whole["dead_u"], np.concatenate([first["dead_u"], second["dead_u"]])) and not same(whole["live_u"], first["live_u"])
        a, b = st.sample_nested(None, 48, n_iter=4, **no), st.sample_nested(None, 48, n_iter=4, chain0=48, **no)
        assert same(whole["live_u"], np.concatenate([a["live_u"], b["live_u"]]))
        held_bits(whole["live_u"].astype(np.float32), hold, "nested live_u")
    st.set_likelihood(None, None)


# ---- 5. the free columns' prior is really sampled
def flat_check(tag, mean_c, m2_c, hold, prior, r):
    free = ~hold[0]
    pf = hr.free_prior(prior, hold)
    zm, zv = ic.moment_z(mean_c[:, free], m2_c[:, free], tuple(a[free] for a in pf))
    print("%s: accept %.3f, z mean %s second moment %s" % (tag, r["accept_rate"].mean(), zm.round(2), zv.round(2)))
    assert np.all(zm < N_SE) and np.all(zv < N_SE), (tag, zm, zv)
    n = r["mean_u"].shape[0]
    assert same(r["mean_u"][:, hold[0]], np.broadcast_to(hold[1][hold[0]], (n, int(hold[0].sum())))), tag
    assert np.all(r["cov_u"][:, hold[0], :] == 0) and np.all(r["cov_u"][:, :, hold[0]] == 0), tag


def test_flat_likelihood_mala(ctx):
    """all weights zero on D1, FLAT_MALA's chains under the mixed record with column 4 -- one of its normal columns -- held:
    the free columns have their prior's mean and second moment within N_SE standard errors, the held column is the value"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    st.set_likelihood(data[0], np.zeros(dims[-1], np.float32))
    c = ic.FLAT_MALA
    prior, hold = ic.mixed_prior(c["d"]), hr.as_hold([0, 0, 0, 0, 1, 0, 0], np.full(7, 0.25))
    with records_on(st, hold, prior):
        r = st.sample(untransform(ic.flat_starts(c["d"], c["chains"], 4), tin), "f32", flags_of(nat, True), **c["opts"])
    assert np.all(r["lnl_last"] == 0)
    flat_check("MALA", r["mean_u"], ic.second_moment(r), hold, prior, r)
    st.set_likelihood(None, None)


def test_flat_likelihood_tempered(ctx):
    """all weights zero on the 2-input stack, ladder (1, 0.3, 0), FLAT_TEMPER's ladders, column 1 held: every rung has the
    free column's prior"""
    nat = pkg("_native")
    st, tin, truth = setup(ctx, "i2")
    p = ic.problem("i2")
    st.set_likelihood(p["data"], np.zeros(p["dims"][-1], np.float32))
    c = ic.FLAT_TEMPER
    prior, hold = ic.mixed_prior(c["d"]), hr.as_hold([0, 1], [0.0, 0.25])
    x0 = untransform(np.repeat(ic.flat_starts(c["d"], c["ladders"], 4), 3, axis=0), tin)
    with records_on(st, hold, prior):
        r = st.sample_tempered(x0, 3, BETAS3, c["swap_every"], "f32", flags_of(nat, True), **c["opts"])
    assert np.all(r["mean_lnl"] == 0) and np.all(r["lnl_last"] == 0)
    for k in range(3):
        rk = {a: r[a][k::3] for a in ("mean_u", "cov_u", "accept_rate")}
        flat_check("tempered rung %d" % k, rk["mean_u"], ic.second_moment(rk), hold, prior, rk)
    st.set_likelihood(None, None)


def test_flat_likelihood_ensemble(ctx):
    """all weights zero on the 4-input stack, hold_ref.FLAT_ENSEMBLE (the case whose control, with (d - 1) ln z, misses by
    4 N_SE on the reference: tests/test_hold_cpu.py), column 3 held, uniform prior"""
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    st.set_likelihood(prob["data"][0], np.zeros(65, np.float32))
    c = hr.FLAT_ENSEMBLE
    hold = hr.as_hold(*hr.FLAT_HOLD)
    x0 = untransform(ic.flat_starts(c["d"], c["W"] * c["ensembles"], 4), rec["tin"])
    with records_on(st, hold):
        r = st.sample_ensemble(x0, c["W"], "f32", flags, **c["opts"])
    assert np.all(r["lnl_last"] == 0)
    m, m2 = er.ensemble_estimates(r["mean_u"], r["cov_u"], c["W"])
    flat_check("ensemble", m, m2, hold, hr.uniform_prior(4), r)
    st.set_likelihood(None, None)


# ---- 6. the conditional evidence
def test_conditional_evidence(ctx):
    """i2 with column 1 held at 0.4, the sizes and seeds of tests/test_hold_cpu.py's references: the tempered ln Z (the
    32-rung ladder of hold_ref) and the nested one (infer_cases.QUAD, RUNS runs from drawn starts) within N_SE of the 1-D
    midpoint rule by their own reported errors"""
    nat, em = pkg("_native"), pkg("emulator")
    st, tin, truth = setup(ctx, "i2")
    hold = hr.held_hold()
    lz_q = hr.conditional_quadrature()[0]
    N, T = ic.QUAD["i2"]
    with records_on(st, hold):
        rt = st.sample_tempered(untransform(hr.held_starts(), tin), hr.HELD_RUNGS, hr.HELD_BETAS, ic.SWAP_EVERY, "f32", flags_of(nat, True), **ic.RUN)
        rn = st.sample_nested(None, ic.RUNS * N, N, "f32", nat.FWD_OUT_TRANSFORM, n_iter=T, seed=ic.SEED)
    lz_t, se_t = hr.held_ladder_lz(rt["mean_lnl"])
    lz_n = em.nested_evidence(rn["dead_lnl"].transpose(1, 0, 2), rn["live_lnl"].reshape(ic.RUNS, N), N)[0]
    se_n = lz_n.std(ddof=1) / np.sqrt(ic.RUNS)
    print("i2, column 1 at %.1f: quadrature %.4f; tempered %.4f +- %.4f (z %+.2f); nested %.4f +- %.4f (z %+.2f), accept %.2f"
          % (hr.HELD_U, lz_q, lz_t, se_t, (lz_t - lz_q) / se_t, lz_n.mean(), se_n, (lz_n.mean() - lz_q) / se_n, rn["accept_rate"].mean()))
    held_bits(rn["live_u"].astype(np.float32), hold, "live_u")
    assert abs(lz_t - lz_q) < N_SE * se_t
    assert abs(lz_n.mean() - lz_q) < N_SE * se_n
    st.set_likelihood(None, None)


# ---- 7. the class surface on the shipped model
def test_class_surface(shipped):
    emulator, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    u_true = np.random.default_rng(4).uniform(-0.4, 0.4, size=(1, 7))
    truth = pp.par_untransform(u_true, ae.par_train)[0]
    spectrum = np.asarray(ae.predict(truth[None]), np.float32).reshape(-1)
    sigma = 50.0  # mK
    v = float(truth[3])
    fixed = {"tau": v}
    u_v = pp.par_transform(truth[None], ae.par_train)[0, 3]
    tau_u = lambda params: pp.par_transform(params.reshape(-1, 7), ae.par_train)[:, 3]
    call = lambda **kw: ae.sample_posterior(spectrum, sigma, n_chains=16, n_steps=60, n_warmup=40, p0=truth, seed=2, **kw)
    a = call()
    b = call(fixed=fixed)
    again = call()
    assert same(a.params, again.params) and same(a.cov_u, again.cov_u)  # (the record of the call before does not leak in)
    assert np.all(np.abs(tau_u(b.params) - u_v) <= np.spacing(np.float32(abs(u_v))))
    assert np.isnan(b.r_hat[3]) and np.all(np.isfinite(np.delete(b.r_hat, 3))) and np.isfinite(np.nanmax(b.r_hat))
    assert np.all(b.cov_u[3] == 0) and np.all(b.cov_u[:, 3] == 0) and b.mean_u[3] == np.float32(u_v) and np.all(np.diag(b.cov_u)[np.arange(7) != 3] > 0)
    e = ae.sample_ensemble(spectrum, sigma, n_walkers=16, n_ensembles=2, n_steps=30, n_warmup=20, p0=truth, seed=2, fixed=fixed)
    assert np.all(np.abs(tau_u(e.params) - u_v) <= np.spacing(np.float32(abs(u_v)))) and np.all(e.cov_u[3] == 0) and np.isnan(e.r_hat[3])
    t = ae.sample_tempered(spectrum, sigma, n_ladders=4, n_temps=4, n_steps=40, n_warmup=20, p0=truth, seed=2, fixed=fixed)
    assert np.isfinite(t.log_evidence) and np.all(np.abs(tau_u(t.params) - u_v) <= np.spacing(np.float32(abs(u_v))))
    r = ae.nested_sample(spectrum, sigma, n_live=64, n_runs=2, max_iter=32, fixed=fixed)
    assert np.all(np.isfinite(r.log_evidence)) and np.isfinite(r.log_evidence_err)
    assert np.all(np.abs(tau_u(r.params) - u_v) <= np.spacing(np.float32(abs(u_v))))
    assert r.mean_u[3] == np.float32(u_v) and np.all(r.cov_u[3] == 0) and np.all(r.cov_u[:, 3] == 0)
    assert r.n_evals == 2 * (64 + 32 * r.n_iter * 3 * 6)  # (the default n_repeats is 3 d_free)
    assert same(call().params, a.params)
    lp = ae.log_posterior(spectrum, sigma, fixed=fixed)
    assert lp.ndim == 6
    theta = pp.par_untransform(np.random.default_rng(5).uniform(-0.9, 0.9, size=(9, 7)), ae.par_train)
    theta[:, 3] = v
    np.testing.assert_allclose(lp(np.delete(theta, 3, axis=1)), ae.log_likelihood(theta, spectrum, sigma, forward_only=True), rtol=1e-14, atol=0)
    assert lp.prior_transform(np.full(6, 0.5)).shape == (6,)
    with pytest.raises(ValueError, match="taus"):
        ae.sample_posterior(spectrum, sigma, p0=truth, fixed={"taus": v})
