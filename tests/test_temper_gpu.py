"""Parallel tempering on the GPU (include/v21.h: v21_mlp_sample_tempered[_dev]): one rung and no swaps against the plain
sampler bit for bit, one tempered transition rebuilt in float64 from the device's own evaluations, the swap events as the
exact permutation tests/temper_ref.py states, independence of host chunks and of splitting a run over calls, the uniform
target, the evidence against grid quadrature and against the float64 reference sampler, argument errors and the emulator
classes' surface."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as fr
import infer_cases as ic
import sample_ref as sr
import shape_cases as sc
import temper_ref as tr
from conftest import pkg
from infer_cases import N_SE
from infer_support import (alpha_of, between_chain, dev_tempered, device_eval, device_stack, fit_setup, flags_of, same, shape_setup,
                           starts_in_box, starts_near, u_of, ulp32)

pytestmark = pytest.mark.gpu

SAMPLE_KEYS = ("x_last", "lnl_last", "eps_last", "accept_rate", "mean_u", "cov_u", "samples", "samples_lnl", "last_prop_u", "last_log_alpha")
LADDER4 = np.array([1.0, 0.5, 0.1, 0.0])


def plain_and_tempered_inputs(ctx, which, n):
    """(stack, precision, flags, n starts) of the generic-route case (i4o65, f32) or the fused-route case (D1, f16)"""
    if which == "i4o65":
        st, rec, prob, flags = shape_setup(ctx, "i4o65")
        return st, "f32", flags, starts_in_box(rec, prob, n, 7, 0.03), "generic"
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    return st, "f16", flags_of(pkg("_native"), True), starts_near(truths[0], tin, n, 5), "fused"


@pytest.mark.parametrize("swap_every", [0, 3])
@pytest.mark.parametrize("which", ["i4o65", "D1"])
def test_one_rung_is_the_plain_sampler(ctx, which, swap_every):
    """T = 1, beta = 1: every output of v21_sample_out equals v21_mlp_sample's bit for bit, whatever swap_every says (300
    chains: a partial second workgroup; 5 warm-up and 12 kept transitions)"""
    st, prec, flags, x0, route = plain_and_tempered_inputs(ctx, which, 300)
    opts = dict(n_warmup=5, n_steps=12, thin=2, seed=77, eps0=0.8, chain0=3, step0=9)
    a = st.sample(x0, prec, flags, diagnostics=True, **opts)
    b = st.sample_tempered(x0, 1, None, swap_every, prec, flags, diagnostics=True, **opts)
    assert st.last_jac_route()[0] == route
    for k in SAMPLE_KEYS:
        assert same(a[k], b[k]), k
    assert 0 < a["accept_rate"].mean() < 1
    assert np.all(b["swap_accept"] == 0)
    st.set_likelihood(None, None)


@pytest.mark.parametrize("which", ["i4o65", "D1"])
def test_without_swaps_the_cold_rows_are_plain_chains(ctx, which):
    """T = 3, swap_every = 0, 3 x 100 rows: the rung-0 rows equal the same rows of a plain call on all 300 starts bit for
    bit (their beta is 1 and nothing reaches them); the hotter rows do not"""
    st, prec, flags, x0, _ = plain_and_tempered_inputs(ctx, which, 300)
    opts = dict(n_warmup=5, n_steps=12, seed=78, eps0=0.8)
    a = st.sample(x0, prec, flags, diagnostics=True, **opts)
    b = st.sample_tempered(x0, 3, [1.0, 0.4, 0.05], 0, prec, flags, diagnostics=True, **opts)
    for k in SAMPLE_KEYS:
        assert same(a[k][0::3], b[k][0::3]), k
    assert not same(a["x_last"][1::3], b["x_last"][1::3])
    st.set_likelihood(None, None)


def tempered(e, beta):
    """an evaluation (lnl, g, F) as the transition at the rows' beta sees it"""
    return [tr.tmul(beta, a) for a in e]


def alpha_bound_tempered(u0, e0, prop, e1, eps, ridge, la, beta):
    """infer_support.alpha_bound with the beta-scaling inside the perturbed function: what one float32 ulp of every
    un-tempered input (ln L, each gradient component, each Fisher entry, at both points) moves the tempered log alpha by,
    to first order, summed in magnitude"""
    d = u0.shape[1]

    def moved(e):
        with np.errstate(invalid="ignore"):
            return np.abs(np.nan_to_num(alpha_of(u0, tempered(e[0], beta), prop, tempered(e[1], beta), eps, ridge) - la, nan=0.0, posinf=0.0,
                                        neginf=0.0))
    bound = tr.tmul(beta, ulp32(e0[0]) + ulp32(e1[0]))
    for side in (0, 1):
        for j in range(d):
            e = [[a.copy() for a in e0], [a.copy() for a in e1]]
            e[side][1][:, j] += ulp32(e[side][1][:, j])
            bound += moved(e)
            for k in range(j, d):
                e = [[a.copy() for a in e0], [a.copy() for a in e1]]
                h = ulp32(e[side][2][:, j, k])
                e[side][2][:, j, k] += h
                if k != j:
                    e[side][2][:, k, j] += h
                bound += moved(e)
    return bound


@pytest.mark.parametrize("which", ["i5o130", "D1"])
def test_one_tempered_transition_against_reference(ctx, which):
    """test_sample_gpu.test_one_transition_against_reference on the ladder (1, 0.5, 0.1, 0), 4 x 250 rows (64 ladders per
    workgroup, a partial last one), same recipe and tolerances: the proposal within one float32 ulp + 1e-12 of the float64
    rebuild from the device's own evaluations scaled by the row's beta, log alpha within the first-order effect of one ulp
    of every un-tempered input, the decisions equal outside that bound with at most 0.5 % of the rows excused.  At beta = 0
    no input reaches log alpha and that effect is exactly 0, while the two float64 evaluations (device and numpy: other
    log and sqrt, other summation order) still differ by rounding: about ten terms of magnitude up to 1e2 at 2e-16 each,
    through the same triangular solves the proposal's 1e-12 is granted for -- the bound carries that 1e-12 on every row
    (at beta > 0 it is three orders below one ulp of ln L; measured on the MI355X: 8.9e-15 at most).  i5o130: f32, two
    Philox blocks, generic route; D1: f16, fused route."""
    nat = pkg("_native")
    n, T = 1000, 4
    if which == "D1":
        st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
        prec, flags, x0 = "f16", flags_of(nat, True), starts_near(truths[0], tin, n, 5)
    else:
        st, rec, prob, flags = shape_setup(ctx, which)
        prec, tin, x0 = "f32", rec["tin"], starts_in_box(rec, prob, n, 7, 0.03)
    d = x0.shape[1]
    seed, chain0, step0, eps0, ridge = sc.SEED, sc.CHAIN0, sc.STEP0, sc.EPS0, sc.RIDGE
    beta = LADDER4[np.arange(n) % T]
    u0 = st.sample(x0, prec, flags, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
    r = st.sample_tempered(x0, T, LADDER4, 0, prec, flags, n_steps=1, n_warmup=0, eps0=eps0, ridge=ridge, seed=seed, chain0=chain0,
                           step0=step0, diagnostics=True)
    e0 = device_eval(st, nat, u0, prec)
    chains, eps = chain0 + np.arange(n), np.full(n, eps0)
    t0 = tempered(e0, beta)
    prop_ref, _, inside = sr.propose(u0, t0[1], t0[2], eps, sr.normals(seed, chains, step0, d), ridge)
    prop = r["last_prop_u"].astype(np.float64)
    err = np.abs(prop - prop_ref)
    tol = np.spacing(np.abs(prop_ref).astype(np.float32)) + 1e-12
    print("%s: proposal max err / tol %.3f, inside per rung %s" % (which, np.max(err / tol), inside.reshape(-1, T).mean(axis=0).round(3)))
    assert np.all(err <= tol), (which, np.max(err / tol))
    e1 = device_eval(st, nat, prop, prec)
    la = alpha_of(u0, t0, prop, tempered(e1, beta), eps, ridge)
    bound = alpha_bound_tempered(u0, e0, prop, e1, eps, ridge, la, beta) + 1e-12
    la_dev = r["last_log_alpha"]
    fin = np.isfinite(la)
    assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), which
    ratio = np.abs(la_dev[fin] - la[fin]) / bound[fin]
    print("%s: log alpha max |diff| %.3e, max diff / bound %.3f" % (which, np.max(np.abs(la_dev[fin] - la[fin])), ratio.max()))
    assert np.all(ratio <= 1.0), (which, ratio.max())
    logu = np.log(sr.accept_uniform(seed, chains, step0))
    acc_ref, acc_dev = logu < la, r["accept_rate"] > 0.5
    excused = np.abs(logu - la) <= bound
    print("%s: accepted per rung %s, excused %d of %d" % (which, acc_dev.reshape(-1, T).mean(axis=0).round(3), excused.sum(), n))
    assert excused.mean() <= 0.005
    assert np.array_equal(acc_ref[~excused], acc_dev[~excused])
    u1 = np.where(acc_dev[:, None], prop, u0)
    np.testing.assert_allclose(r["x_last"], fr.untransform(u1, tin[0], tin[2], tin[3]), rtol=1e-12)
    # the state keeps the un-tempered ln L
    np.testing.assert_allclose(r["lnl_last"], np.where(acc_dev, e1[0], e0[0]), rtol=1e-5)
    st.set_likelihood(None, None)


@pytest.mark.parametrize("T,ladders", ic.SWAP_CASES)
def test_swaps_are_the_stated_permutation(ctx, T, ladders):
    """One kept transition without swaps (run A) and with swap_every = 1 (run B), at step0 = 0 (event 0: the even pairs)
    and step0 = 1 (event 1: the odd pairs): B's x_last and lnl_last are A's rows, bit for bit, permuted by the decision
    temper_ref.swap_event forms from A's lnl_last and the Philox uniform.  A pair is excused only where |log U - rhs| <=
    1e-9 max(1, |rhs|) (at most 1 % of the pairs; tests/test_temper_cpu.py finds none on the reference).  The starts are
    scattered over the box, so that at least 10 % of the pairs swap and 10 % refuse.  The rows' sums see the state after
    the swap; swap_every = 2 at step0 = 0 has no event and equals A.  The last workgroup is partial at every T."""
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    n = T * ladders
    betas = ic.swap_betas(T)
    x0 = starts_in_box(rec, prob, n, ic.SWAP_SEED, None)
    opts = dict(n_warmup=0, n_steps=1, seed=sc.SEED, chain0=sc.CHAIN0, eps0=0.5)
    for step0 in (0, 1):
        A = st.sample_tempered(x0, T, betas, 0, "f32", flags, step0=step0, **opts)
        B = st.sample_tempered(x0, T, betas, 1, "f32", flags, step0=step0, **opts)
        perm, lower, swapped, logu, rhs = tr.swap_event(A["lnl_last"].astype(np.float64), betas, step0, sc.SEED, sc.CHAIN0, step0)
        assert np.array_equal(lower % T % 2, np.full(lower.size, step0 % 2)) and (lower.size == 0) == (T == 2 and step0 == 1)
        excused = np.abs(logu - rhs) <= 1e-9 * np.maximum(1.0, np.abs(rhs))
        print("T=%d step0=%d: %d pairs, %d swap, %d excused" % (T, step0, lower.size, swapped.sum(), excused.sum()))
        if lower.size:  # (T = 2 has no odd pair: event 1 proposes nothing there, and B is A)
            assert excused.mean() <= 0.01
            assert swapped.mean() >= 0.1 and (~swapped).mean() >= 0.1
        keep = np.ones(n, bool)
        keep[lower[excused]] = keep[lower[excused] + 1] = False
        assert same(B["x_last"][keep], A["x_last"][perm][keep]) and same(B["lnl_last"][keep], A["lnl_last"][perm][keep])
        assert same(B["eps_last"], A["eps_last"]) and same(B["accept_rate"], A["accept_rate"])  # (these stay with the row)
        dec = np.zeros(n)
        dec[lower] = swapped
        ok = np.ones(n, bool)
        ok[lower[excused]] = False
        assert np.array_equal(B["swap_accept"][ok], dec[ok])
        assert np.array_equal(B["mean_lnl"], B["lnl_last"].astype(np.float64)) and np.all(B["var_lnl"] == 0)
        assert same(B["samples"][:, 0], B["x_last"]) and same(B["samples_lnl"][:, 0], B["lnl_last"])
        assert np.all(A["swap_accept"] == 0) and np.array_equal(A["mean_lnl"], A["lnl_last"].astype(np.float64))
    A = st.sample_tempered(x0, T, betas, 0, "f32", flags, step0=0, **opts)
    B2 = st.sample_tempered(x0, T, betas, 2, "f32", flags, step0=0, **opts)
    for k in A:
        assert same(A[k], B2[k]), k
    st.set_likelihood(None, None)


def test_chunks_and_continuation(ctx):
    """i4o65, T = 3, 3 x 2,740 = 8,220 rows, 6 transitions, swap_every = 2.  8,192 is no multiple of 3: a fixed 8,192-row
    host chunk would split ladder 2,730, the host form works in chunks of 8,190.  On float32 starts the host form and the
    _dev form (one launch sequence over all rows) agree bit for bit; on float64 starts (another branch of the input
    transform, so other chains) one call of 6 transitions equals two calls of 3, the second continued from the float64
    x_last and eps_last with step0 advanced (swap events after S = 1, 3 and 5: one in the first call, two in the second)."""
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    T, n, betas = 3, 8220, [1.0, 0.3, 0.0]
    x64 = np.ascontiguousarray(np.tile(starts_in_box(rec, prob, 30, 12, 0.2), (n // 30, 1)))
    x32 = np.ascontiguousarray(x64.astype(np.float32))
    opts = dict(n_warmup=0, n_steps=6, thin=0, seed=5, eps0=0.6)
    host = st.sample_tempered(x32, T, betas, 2, "f32", flags, **opts)
    dev = dev_tempered(ctx, st, x32, "f32", flags, T, betas, 2, **opts)
    for k in dev:
        bad = np.flatnonzero(np.ascontiguousarray(host[k]).reshape(n, -1).view(np.uint8) != dev[k].reshape(n, -1).view(np.uint8))
        assert bad.size == 0, (k, bad[:6])
    assert host["swap_accept"].reshape(-1, T)[:, :2].mean() > 0.05  # (swaps happened)
    whole = st.sample_tempered(x64, T, betas, 2, "f32", flags, **opts)
    first = st.sample_tempered(x64, T, betas, 2, "f32", flags, **dict(opts, n_steps=3))
    second = st.sample_tempered(first["x_last"], T, betas, 2, "f32", flags, eps_start=first["eps_last"], **dict(opts, n_steps=3, step0=3))
    assert same(whole["x_last"], second["x_last"]) and same(whole["lnl_last"], second["lnl_last"])
    assert not same(whole["x_last"], first["x_last"])
    # the sums of the two halves are the whole's
    np.testing.assert_allclose(whole["mean_lnl"], (first["mean_lnl"] + second["mean_lnl"]) / 2, rtol=1e-12)
    st.set_likelihood(None, None)


def test_uniform_target(ctx):
    """all weights zero, T = 4: ln L = 0 everywhere, so every proposed swap is accepted, mean_lnl and the evidence are
    exactly 0, and every rung samples the uniform density on the box: per-rung mean and second moment of u within 5
    standard errors (over 256 ladders) of 0 and 1 / 3"""
    em = pkg("emulator")
    st, rec, prob, flags = shape_setup(ctx, "i4o65")
    st.set_likelihood(prob["data"][0], np.zeros(65, np.float32))
    T, L = 4, 256
    x0 = np.repeat(starts_in_box(rec, prob, L, 4, None), T, axis=0)
    r = st.sample_tempered(x0, T, LADDER4, 1, "f32", flags, n_steps=600, n_warmup=150, thin=0, seed=5)
    sw = r["swap_accept"].reshape(L, T)
    assert np.all(sw[:, :3] == 1.0) and np.all(sw[:, 3] == 0.0)
    assert np.all(r["mean_lnl"] == 0) and np.all(r["var_lnl"] == 0) and np.all(r["lnl_last"] == 0)
    assert np.all(em.log_evidence(LADDER4, r["mean_lnl"].reshape(L, T)) == 0)
    m2 = np.diagonal(r["cov_u"], axis1=1, axis2=2) + r["mean_u"] ** 2
    for k in range(T):
        zm, zv = sr.pooled_check(r["mean_u"][k::T], 0.0)[1], sr.pooled_check(m2[k::T], 1.0 / 3.0)[1]
        print("rung %d: accept %.3f, z mean %s second moment %s" % (k, r["accept_rate"][k::T].mean(), zm.round(2), zv.round(2)))
        assert np.all(zm < N_SE) and np.all(zv < N_SE), (k, zm, zv)
    st.set_likelihood(None, None)


@pytest.mark.parametrize("name", ["i1", "i2"])
def test_evidence_against_quadrature(ctx, name):
    """the two quadrature problems of tests/infer_cases.py with their constants, on the device in f32: every rung's mean
    ln L within 5 standard errors (the scatter over the 64 ladders) of the quadrature value, ln Z within 5 of its own"""
    nat, em = pkg("_native"), pkg("emulator")
    p = ic.problem(name)
    st, rec = device_stack(ctx, p["dims"], p["act"])
    st.set_likelihood(p["data"], p["w"])
    tin = rec["tin"]
    x0 = fr.untransform(p["starts_u"], tin[0], tin[2], tin[3])
    r = st.sample_tempered(x0, ic.RUNGS, ic.BETAS, ic.SWAP_EVERY, "f32", flags_of(nat, True), **ic.RUN)
    z, z_lz, se = ic.ladder_check(r["mean_lnl"], name)
    lz = em.log_evidence(ic.BETAS, r["mean_lnl"].reshape(ic.LADDERS, ic.RUNGS))
    print("%s: z per rung %s, ln Z %.4f +- %.4f (quadrature trapezoid %.4f, z %.2f), swap rates %s"
          % (name, z.round(2), lz.mean(), lz.std(ddof=1) / 8, tr.trapezoid(ic.BETAS, ic.quadrature(name)[0]), z_lz,
             r["swap_accept"].reshape(ic.LADDERS, ic.RUNGS).mean(axis=0).round(2)))
    assert np.all(np.abs(z) < N_SE), z
    assert abs(z_lz) < N_SE, z_lz
    st.set_likelihood(None, None)


_d1_ref = {}


def d1_reference(Ws, bs, act, data, w, tout, u0, betas, opts):
    if "r" not in _d1_ref:
        ev = sr.evaluator_batch(Ws, bs, act, data, w, tout)
        _d1_ref["r"] = tr.temper_ref(ev, u0, betas, **opts)
    return _d1_ref["r"]


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_mean_lnl_against_reference_sampler(ctx, prec):
    """D1 (7 inputs, the fused route), 16 ladders of 4 rungs against temper_ref on the float64 oracle from the same
    starts, 100 + 200 transitions as test_statistics_against_reference_sampler: per-rung mean ln L within 5 combined
    standard errors (the scatter over ladders, on both sides)"""
    nat, em = pkg("_native"), pkg("emulator")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    L, T = 16, 4
    betas = em.default_betas(T)
    opts = dict(n_steps=200, n_warmup=100, thin=0, seed=11, swap_every=4)
    x0 = np.repeat(starts_near(truths[0], tin, L, 1, scale=0.01), T, axis=0)
    kw = dict(opts)
    se = kw.pop("swap_every")
    r = st.sample_tempered(x0, T, betas, se, prec, flags_of(nat, True), **kw)
    assert st.last_jac_route()[0] == "fused"
    ref = d1_reference(Ws, bs, act, data[0], w, tout, u_of(x0, tin), betas, opts)
    (md, vd), (mr, vr) = between_chain(r["mean_lnl"].reshape(L, T)), between_chain(ref["mean_lnl"].reshape(L, T))
    z = np.abs(md - mr) / np.sqrt(vd + vr)
    print("%s: mean ln L per rung device %s reference %s, z %s; swap rates device %s reference %s"
          % (prec, md.round(1), mr.round(1), z.round(2), r["swap_accept"].reshape(L, T).mean(axis=0).round(2),
             ref["swap_accept"].reshape(L, T).mean(axis=0).round(2)))
    assert np.all(np.isfinite(r["mean_lnl"])) and np.all(z < N_SE), z
    st.set_likelihood(None, None)


def test_argument_errors_and_routes_counted(ctx):
    """every refused case of include/v21.h returns V21_ERR_ARG from both forms and the next valid call succeeds; a call
    counts once on the Jacobian's route whatever its transitions and chunks; n = 0 is a no-op"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    lib, F, P = st.lib, C.POINTER(C.c_float), C.c_void_p
    n = 6
    x0 = np.ascontiguousarray(pkg("synth").make_params(n, seed=40, zero_fx_frac=0).astype(np.float32))
    xl = np.full_like(x0, -7.0)
    d3 = np.ascontiguousarray(data[:3])
    out = nat.SampleOut(x_last=xl.ctypes.data)
    o = nat.Stack.sample_opts(n_steps=2, n_warmup=1)

    def ladder(T, betas, swap_every=1):
        return nat.TemperOpts(T, (C.c_double * 32)(*betas), swap_every)

    good = ladder(3, [1.0, 0.5, 0.0])
    bad = [ladder(0, []), ladder(33, [1.0] * 32), ladder(-1, []), ladder(3, [1.5, 0.5, 0.0]), ladder(3, [1.0, 0.5, -0.1]),
           ladder(3, [1.0, 0.5, 0.5]), ladder(3, [0.2, 0.5, 0.1]), ladder(3, [1.0, float("nan"), 0.0]), ladder(3, [1.0, 0.5, 0.0], -1),
           ladder(4, [1.0, 0.5, 0.2, 0.0])]  # (the last: 6 rows are no whole ladders of 4)
    host = lambda t, nd=0, rows=n: lib.v21_mlp_sample_tempered(st.h, x0.ctypes.data_as(P), 0, rows, d3.ctypes.data_as(F) if nd else None, nd,
                                                             C.byref(o), C.byref(t) if t else None, None, C.byref(out), None, 0, flags)
    for t in bad:
        assert host(t) == -1, (t.n_temps, list(t.betas)[:4], t.swap_every)
    assert host(good, nd=3) == -1  # two rows per spectrum: a ladder of 3 would straddle two spectra
    assert host(ladder(2, [1.0, 0.0]), nd=3) == 0
    assert host(good) == 0 and np.all(np.isfinite(xl))
    assert host(None) == 0  # (no ladder: one rung at beta = 1)
    xl[:] = -7.0
    assert host(good, rows=0) == 0 and np.all(xl == -7.0)
    bufs = [ctx.malloc(x0.nbytes), ctx.malloc(d3.nbytes), ctx.malloc(x0.nbytes)]
    try:
        dout = nat.SampleOut(x_last=bufs[2])
        ctx.h2d(bufs[0], x0)
        ctx.h2d(bufs[1], d3)
        dev = lambda t, nd=0, rows=n: lib.v21_mlp_sample_tempered_dev(st.h, P(bufs[0]), 7, rows, P(bufs[1]) if nd else None, nd, C.byref(o),
                                                                     C.byref(t), None, C.byref(dout), None, 0, flags)
        for t in bad:
            assert dev(t) == -1, (t.n_temps, list(t.betas)[:4], t.swap_every)
        assert dev(good, nd=3) == -1
        assert dev(good, rows=0) == 0
        assert dev(good) == 0
        ctx.sync()
        ctx.d2h(xl, bufs[2])
        assert np.all(np.isfinite(xl))
    finally:
        for p in bufs:
            ctx.free(p)
    counts = lambda: sum(st.last_jac_route()[1].values())
    c0 = counts()
    st.sample_tempered(x0, 3, [1.0, 0.5, 0.0], 1, "f16", flags, n_steps=3, n_warmup=2)
    assert counts() - c0 == 1 and st.last_jac_route()[0] == "fused"
    big = np.ascontiguousarray(np.tile(x0, (8196 // n, 1)))  # 8,196 rows: two host chunks of 8,190 + 6
    c0 = counts()
    st.sample_tempered(big, 3, [1.0, 0.5, 0.0], 1, "f16", flags, n_steps=2, n_warmup=1, thin=0)
    assert counts() - c0 == 1
    with pytest.raises(ValueError):
        st.sample_tempered(x0, 4, [1.0, 0.5, 0.2, 0.0], 1, "f16", flags, n_steps=1, n_warmup=0)
    st.set_likelihood(None, None)


def test_class_surface(shipped):
    emulator, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    u_true = np.random.default_rng(4).uniform(-0.6, 0.6, size=(2, 7))
    truths = pp.par_untransform(u_true, ae.par_train)
    spectra = np.asarray(ae.predict(truths), np.float32)
    r = ae.sample_tempered(spectra[1], 1.0, n_ladders=8, n_temps=4, n_steps=60, n_warmup=40, p0=truths[1], return_lnl=True)
    assert isinstance(r, emulator.TemperedSamples)
    assert r.params.shape == (8, 60, 7) and r.lnl.shape == (8, 60) and r.accept_rate.shape == (8,) and r.step_size.shape == (8,)
    assert r.r_hat.shape == (7,) and r.mean_u.shape == (7,) and r.cov_u.shape == (7, 7)
    assert np.array_equal(r.betas, emulator.default_betas(4)) and r.mean_lnl.shape == (8, 4) and r.swap_rate.shape == (3,)
    assert np.isfinite(r.log_evidence) and np.isfinite(r.log_evidence_err) and r.log_evidence_err > 0
    assert np.all((r.swap_rate >= 0) & (r.swap_rate <= 1)) and np.all(np.isfinite(r.mean_lnl))
    assert r.mean_lnl[:, 0].mean() > r.mean_lnl[:, -1].mean()  # (E_beta[ln L] falls with the temperature)
    print("ln Z %.3f +- %.3f, swap rates %s, mean ln L per rung %s" % (r.log_evidence, r.log_evidence_err, r.swap_rate.round(2),
                                                                      r.mean_lnl.mean(axis=0).round(1)))
    # several spectra
    r2 = ae.sample_tempered(spectra, 1.0, n_ladders=4, n_temps=3, n_steps=30, n_warmup=20, thin=0, p0=truths[0])
    assert r2.params is None and r2.mean_lnl.shape == (2, 4, 3) and r2.swap_rate.shape == (2, 2) and r2.log_evidence.shape == (2,)
    assert r2.log_evidence_err.shape == (2,) and r2.accept_rate.shape == (2, 4) and r2.cov_u.shape == (2, 7, 7)
    # one rung: sample_posterior's chains, bit for bit, and no evidence
    kw = dict(n_steps=50, n_warmup=30, thin=5, p0=truths[0], seed=3, return_lnl=True)
    a = ae.sample_posterior(spectra, 1.0, n_chains=8, **kw)
    b = ae.sample_tempered(spectra, 1.0, n_ladders=8, n_temps=1, **kw)
    for k in emulator.PosteriorSamples._fields:
        assert same(getattr(a, k), getattr(b, k)), k
    assert np.all(np.isnan(b.log_evidence)) and np.all(np.isnan(b.log_evidence_err)) and b.swap_rate.shape == (2, 0)
    with pytest.raises(ValueError):
        ae.sample_tempered(spectra[0], 1.0, n_temps=3, betas=[1.0, 0.5])
    with pytest.raises(ValueError):
        ae.sample_tempered(spectra[0], 1.0, swap_every=-1)
