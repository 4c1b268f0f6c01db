"""The Jacobian-side kernels over the shapes of tests/shape_cases.py: jac_generic_kernel (Jacobian and likelihood mode),
the jac_reduce_kernel<8 / 15, 0 / 4 / 8, with / without F> instantiations and nuis_project_kernel, fit_lm_kernel and the sample_*
kernels, each against its float64 reference (jacobian_ref, fit_ref, marg_ref, sample_ref) at in_dim 1 .. 17 and out_dim
1 .. 451, the 65,535-row launch split of the generic route and the documented refusals.  Every bound is the one the
project already uses for the same quantity (infer_support.check_rows, check_reduction and alpha_bound, imported; test_loglike,
test_fisher_against_own_jacobian and test_fit_against_lm_ref, quoted); every test prints the fraction of its bound it used."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as fr
import jacobian_ref as jr
import sample_ref as sr
import shape_cases as sc
from conftest import pkg
from infer_support import POISON, alpha_bound, alpha_of, check_reduction, check_rows, device_eval, device_stack, flags_of, reference, same

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE, ARG = -3, -4, -1


def status_of(call):
    """the status a call of the Python front end ends with: 0, or the code of its EngineError"""
    nat = pkg("_native")
    try:
        call()
    except nat.EngineError as e:
        return int(str(e).split("v21 error ")[1].split(":")[0])
    return 0


def c_fit(st, x0):
    """v21_mlp_fit itself (Stack.fit refuses more than 8 inputs before the library sees them) -> its status"""
    x = np.ascontiguousarray(x0, np.float32)
    n, din = x.shape
    xh, lnl = np.empty_like(x), np.empty(n, np.float32)
    return st.lib.v21_mlp_fit(st.h, x.ctypes.data_as(C.c_void_p), 0, n, None, 0, None, xh.ctypes.data_as(C.c_void_p),
                              lnl.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, 0, 0)


def c_sample(st, x0):
    nat = pkg("_native")
    x = np.ascontiguousarray(x0, np.float32)
    xl = np.empty_like(x)
    out = nat.SampleOut(x_last=xl.ctypes.data)
    return st.lib.v21_mlp_sample(st.h, x.ctypes.data_as(C.c_void_p), 0, x.shape[0], None, 0, None, None, C.byref(out), 0, 0)


def test_jacobian_and_primal(ctx):
    """every stack of the table, rows 1, 3, 4, 5, 9, with and without each transform, float64 and float32 rows: the route
    is generic, y against jacobian_ref and against the forward at test_generic_route_parity's bounds, the Jacobian through
    check_rows at 1e-5 per row.  Measured worst on the MI355X, as fractions of the bounds: y 0.0076, Jacobian rows 0.088 (no
    row needed a kink)."""
    nat = pkg("_native")
    worst = {"y": 0.0, "jac": 0.0}
    for case in sc.CASES:
        st, rec = device_stack(ctx, case.dims, case.act)
        Ws, bs, act, tin, tout = rec["Ws"], rec["bs"], rec["act"], rec["tin"], rec["tout"]
        assert nat.route_jacobian(case.dims, case.act, "f32", 9) == "generic", case.name
        for n, tin_on, tout_on, x in sc.jac_inputs(case):
            flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | (nat.FWD_OUT_TRANSFORM if tout_on else 0)
            tag = "%s n=%d %s flags=%d" % (case.name, n, x.dtype.name, flags)
            y, jac = st.jacobian(x, "f32", flags, return_outputs=True)
            assert st.last_jac_route()[0] == "generic", tag
            assert jac.shape == (n, case.dims[0], case.dims[-1]) and np.all(np.isfinite(jac)) and np.all(np.isfinite(y)), tag
            to = tout if tout_on else None
            yr, Jr = jr.jacobian(Ws, bs, act, x, tin if tin_on else None, to)
            atol = 2e-5 * (tout[0] if tout_on else 1.0)
            np.testing.assert_allclose(y, yr, rtol=1e-5, atol=atol, err_msg=tag)
            np.testing.assert_allclose(y, st.forward(x, "f32", flags), rtol=1e-5, atol=atol, err_msg=tag)
            xt = jr.transform(x, *tin)[0] if tin_on else x.astype(np.float64)
            check_rows(tag, "f32", jac, Jr, Ws, bs, act, xt, tin_on, x, tin, to)
            worst["y"] = max(worst["y"], float(np.max(np.abs(y - yr) / (atol + 1e-5 * np.abs(yr)))))
            worst["jac"] = max(worst["jac"], float(jr.rel_frobenius(jac, Jr).max()) / 1e-5)
            assert np.array_equal(st.jacobian(x, "f32", flags), jac), tag  # (without y: the same Jacobian)
        assert set(st.last_jac_route()[1]) == {"generic"}, case.name
    print("worst of the table, fractions of the bounds: y %.3g, Jacobian rows %.3g (of 1e-5)" % (worst["y"], worst["jac"]))


def test_input_transform_limit(ctx):
    """above 8 inputs: v21_mlp_set_input_transform refuses the columns (V21_ERR_ARG, the handle keeps none) and
    V21_FWD_IN_TRANSFORM without a transform is the documented state error of every entry"""
    nat = pkg("_native")
    for name in ("i9o65", "i16o3"):
        case = sc.BY_NAME[name]
        st, rec = device_stack(ctx, case.dims, case.act)
        t = nat.AffineIn()
        t.n = case.dims[0]
        for j in range(8):
            t.span[j] = 1.0
        assert st.lib.v21_mlp_set_input_transform(st.h, C.byref(t)) == ARG, name
        x = sc.rows(case.dims, 3, 1)
        assert status_of(lambda: st.jacobian(x, "f32", nat.FWD_IN_TRANSFORM)) == STATE, name
        st.set_likelihood(*likelihood(rec, 1)[:2])
        assert status_of(lambda: st.loglike(x, "f32", nat.FWD_IN_TRANSFORM)) == STATE, name
        st.set_likelihood(None, None)
        assert np.all(np.isfinite(st.jacobian(x, "f32", nat.FWD_OUT_TRANSFORM)))


def likelihood(rec, seed, K=0):
    """(data float32, weights float32, weights float64) of a stack of the table"""
    w = sc.weights(rec["dims"][-1], seed, K)
    return sc.data_for(rec, seed)[0], w, w.astype(np.float64)


def test_likelihood_mode_of_the_generic_kernel(ctx):
    """st.loglike (jac_generic_kernel's likelihood mode: one block reduction per tangent group, lnl from group 0 alone)
    against jacobian_ref.loglike of the device's own y and J at test_loglike's bounds: lnl within 1e-5 of its value (a sum
    of terms of one sign), the gradient within 1e-5 of the sum of its terms' magnitudes; data of 1e30 in the zero-weight
    bins change no bit.  Measured worst on the MI355X: lnl 0.013, grad 0.013 of 1e-5."""
    nat = pkg("_native")
    worst = {"lnl": 0.0, "grad": 0.0}
    for i, case in enumerate(sc.CASES):
        st, rec = device_stack(ctx, case.dims, case.act)
        flags = flags_of(nat, rec["tin"] is not None)
        data, w, w64 = likelihood(rec, 1)
        st.set_likelihood(data, w)
        for n in (5, sc.ROWS[i % len(sc.ROWS)]):
            x = sc.rows(case.dims, n, 20 + n)
            tag = "%s n=%d" % (case.name, n)
            lnl, g = st.loglike(x, "f32", flags)
            assert st.last_jac_route()[0] == "generic" and lnl.shape == (n,) and g.shape == (n, case.dims[0]), tag
            y, jac = st.jacobian(x, "f32", flags, return_outputs=True)
            l64, g64 = jr.loglike(y, jac, data, w64)
            np.testing.assert_allclose(lnl, l64, rtol=1e-5, atol=0, err_msg=tag)
            scale = np.einsum("nk,njk->nj", np.abs(w64 * (data - y.astype(np.float64))), np.abs(jac.astype(np.float64)))
            assert np.all(np.abs(g - g64) <= 1e-5 * scale), (tag, np.max(np.abs(g - g64) / scale))
            worst["lnl"] = max(worst["lnl"], float(np.max(np.abs(lnl - l64) / np.abs(l64))) / 1e-5)
            worst["grad"] = max(worst["grad"], float(np.max(np.abs(g - g64) / np.maximum(scale, 1e-300))) / 1e-5)
            assert np.array_equal(st.loglike(x, "f32", flags, grad=False), lnl), tag
            # against float64 throughout (test_loglike's f32 tolerance, here on every row)
            yr, Jr = jr.jacobian(rec["Ws"], rec["bs"], rec["act"], x, rec["tin"], rec["tout"])
            lr, gr = jr.loglike(yr, Jr, data, w64)
            assert np.median(np.abs(lnl - lr) / np.abs(lr)) <= 1e-4 and np.median(jr.rel_frobenius(g, gr)) <= 1e-4, tag
            if np.any(w == 0):
                d2 = data.copy()
                d2[w == 0] = 1e30
                st.set_likelihood(d2, w)
                l2, g2 = st.loglike(x, "f32", flags)
                assert same(l2, lnl) and same(g2, g), tag
                st.set_likelihood(data, w)
        st.set_likelihood(None, None)
    print("worst of the table, fractions of the bounds: lnl %.3g, grad %.3g (of 1e-5)" % (worst["lnl"], worst["grad"]))


def test_fisher_lnl_and_gradient(ctx):
    """jac_reduce_kernel<8, 0, true> (in_dim <= 8, unpadded at 8) and <15, 0, true> (9 .. 15, unpadded at 15) against fit_ref.fisher_ref of
    the device's own Jacobian at 1e-5 relative Frobenius, exactly symmetric; lnl and grad against loglike at the bounds of
    test_fisher_against_own_jacobian (1e-6 of the value / of the sum of the terms' magnitudes).  Measured worst on the
    MI355X: F 0.010 of 1e-5, lnl 0.099 and grad 0.12 of 1e-6."""
    nat = pkg("_native")
    worst = {"F": 0.0, "lnl": 0.0, "grad": 0.0}
    for i, case in enumerate(c for c in sc.CASES if c.dims[0] <= 15):
        st, rec = device_stack(ctx, case.dims, case.act)
        din = case.dims[0]
        flags = flags_of(nat, rec["tin"] is not None)
        data, w, w64 = likelihood(rec, 2)
        st.set_likelihood(data, w)
        for n in (5, sc.ROWS[i % len(sc.ROWS)]):
            x = sc.rows(case.dims, n, 30 + n).astype(np.float32)
            tag = "%s n=%d" % (case.name, n)
            F, lnl, g = st.fisher(x, "f32", flags, lnl=True, grad=True)
            assert st.last_jac_route()[0] == "generic" and F.shape == (n, din, din) and np.all(np.isfinite(F)), tag
            assert np.array_equal(F.view(np.uint32), F.transpose(0, 2, 1).view(np.uint32)), tag  # exactly symmetric
            assert np.array_equal(st.fisher(x, "f32", flags), F), tag
            y, jac = st.jacobian(x, "f32", flags, return_outputs=True)
            err = jr.rel_frobenius(F, fr.fisher_ref(jac, w64))
            assert err.max() <= 1e-5, (tag, err.max())
            l_ll, g_ll = st.loglike(x, "f32", flags)
            np.testing.assert_allclose(lnl, l_ll, rtol=1e-6, atol=0, err_msg=tag)
            scale = np.einsum("nk,njk->nj", np.abs(w64 * (data - y.astype(np.float64))), np.abs(jac.astype(np.float64)))
            assert np.all(np.abs(g - g_ll) <= 1e-6 * scale), (tag, np.max(np.abs(g - g_ll) / scale))
            worst["F"] = max(worst["F"], float(err.max()) / 1e-5)
            worst["lnl"] = max(worst["lnl"], float(np.max(np.abs(lnl - l_ll) / np.abs(l_ll))) / 1e-6)
            worst["grad"] = max(worst["grad"], float(np.max(np.abs(g - g_ll) / np.maximum(scale, 1e-300))) / 1e-6)
        st.set_likelihood(None, None)
    print("worst of the table, fractions of the bounds: F %.3g (of 1e-5), lnl %.3g, grad %.3g (of 1e-6)" % (worst["F"], worst["lnl"], worst["grad"]))


def test_in_dim_limits(ctx):
    """include/v21.h: fit and sample serve at most 8 inputs, fisher and the nuisance entries at most 15 -- V21_ERR_UNSUPPORTED
    beyond, whatever else is set, and the handle goes on serving what it can"""
    nat = pkg("_native")
    # 16 inputs: the Jacobian and loglike only
    case = sc.BY_NAME["i16o3"]
    st, rec = device_stack(ctx, case.dims, case.act)
    flags = flags_of(nat, rec["tin"] is not None)
    data, w, w64 = likelihood(rec, 1, 1)
    st.set_likelihood(data, w)
    x = sc.rows(case.dims, 5, 1)
    lnl, g = st.loglike(x, "f32", flags)
    assert status_of(lambda: st.fisher(x, "f32", flags)) == UNSUPPORTED
    assert c_fit(st, x) == UNSUPPORTED and c_sample(st, x) == UNSUPPORTED
    with pytest.raises(ValueError):
        st.fit(x, "f32", flags)
    with pytest.raises(ValueError):
        st.sample(x, "f32", flags, n_steps=1, n_warmup=0)
    st.set_nuisance(sc.basis(3, 1))  # (the record itself does not depend on in_dim)
    assert status_of(lambda: st.fisher(x, "f32", flags)) == UNSUPPORTED
    assert status_of(lambda: st.nuisance_coef(x, "f32", flags)) == UNSUPPORTED
    assert status_of(lambda: st.loglike(x, "f32", flags)) == UNSUPPORTED  # (marginalised: jac_reduce_kernel's limit)
    st.set_nuisance(None)
    l2, g2 = st.loglike(x, "f32", flags)
    assert same(l2, lnl) and same(g2, g)
    st.set_likelihood(None, None)
    # 9 inputs: fisher too
    case = sc.BY_NAME["i9o65"]
    st, rec = device_stack(ctx, case.dims, case.act)
    data, w, w64 = likelihood(rec, 1)
    st.set_likelihood(data, w)
    x = sc.rows(case.dims, 5, 1)
    assert c_fit(st, x) == UNSUPPORTED and c_sample(st, x) == UNSUPPORTED
    assert np.all(np.isfinite(st.fisher(x, "f32", flags_of(nat, rec["tin"] is not None))))
    st.set_likelihood(None, None)


def test_a_layer_too_wide_for_the_lds_is_refused(ctx):
    """[2, 10241, 1]: one tangent per workgroup still needs 16 bytes more than 160 KB -- V21_ERR_UNSUPPORTED from the Jacobian
    and from loglike, host and device entry, and the handle serves its forward before and after"""
    nat = pkg("_native")
    dims, act = sc.TOO_WIDE
    st, rec = device_stack(ctx, dims, act)
    flags = flags_of(nat, rec["tin"] is not None)
    x = sc.rows(dims, 3, 1)
    y0 = st.forward(x, "f32", flags)
    np.testing.assert_allclose(y0, jr.oracle_outputs(rec["Ws"], rec["bs"], act, x, rec["tin"], rec["tout"]), rtol=1e-5, atol=2e-5 * sc.OUT_STD)
    assert status_of(lambda: st.jacobian(x, "f32", flags)) == UNSUPPORTED
    st.set_likelihood(np.zeros(1, np.float32), np.ones(1, np.float32))
    assert status_of(lambda: st.loglike(x, "f32", flags)) == UNSUPPORTED
    assert status_of(lambda: st.fisher(x, "f32", flags)) == UNSUPPORTED
    dx, dj = ctx.malloc(x.size * 4), ctx.malloc(3 * 2 * 4)
    try:
        ctx.h2d(dx, x.astype(np.float32))
        assert status_of(lambda: st.jacobian_dev(dx, 2, 3, None, 1, dj, "f32", flags)) == UNSUPPORTED
    finally:
        ctx.free(dx)
        ctx.free(dj)
    st.set_likelihood(None, None)
    assert np.array_equal(st.forward(x, "f32", flags), y0)


def test_marginalised_reductions(ctx):
    """the eight jac_reduce_kernel<8 | 15, 4 | 8, with / without F> instantiations over the table's out_dim and K in {1, 4, 5,
    8}: fisher, loglike and nuisance_coef against marg_ref fed the device's own y and J, bounds and scales of
    infer_support.check_reduction; clearing the record restores the earlier bits; a basis on fewer than K + 1 live bins
    is refused and leaves the handle as it was.  Measured worst on the MI355X, as fractions of the scales: F 1.6e-7, lnl
    5.8e-8, grad 1.2e-7 (bounds 1e-5); the amplitudes at 0.012 of their bound."""
    nat = pkg("_native")
    worst = {"F": 0.0, "lnl": 0.0, "grad": 0.0, "coef": 0.0}
    for i, case in enumerate(c for c in sc.CASES if c.modes):
        st, rec = device_stack(ctx, case.dims, case.act)
        din, dout = case.dims[0], case.dims[-1]
        flags = flags_of(nat, rec["tin"] is not None)
        for K in case.modes:
            data, w, w64 = likelihood(rec, 3, K)
            st.set_likelihood(data, w)
            A = sc.basis(dout, K)
            n = sc.ROWS[(i + K) % len(sc.ROWS)]
            x = sc.rows(case.dims, n, 40 + n).astype(np.float32)
            tag = "%s K=%d n=%d" % (case.name, K, n)
            before = st.fisher(x, "f32", flags, lnl=True, grad=True) + st.loglike(x, "f32", flags)
            st.set_nuisance(A)
            assert st.nuisance_modes() == K
            F, lnl, g = st.fisher(x, "f32", flags, lnl=True, grad=True)
            assert st.last_jac_route()[0] == "generic" and F.shape == (n, din, din) and np.all(np.isfinite(F)), tag
            assert np.array_equal(F.view(np.uint32), F.transpose(0, 2, 1).view(np.uint32)), tag
            assert np.array_equal(st.fisher(x, "f32", flags), F), tag
            y, jac = st.jacobian(x, "f32", flags, return_outputs=True)
            coef = st.nuisance_coef(x, "f32", flags)
            assert coef.shape == (n, K) and coef.dtype == np.float64
            ref, ls, gs, ct = reference(y, jac, data, w, A)
            check_reduction(tag, F, lnl, g, coef, ref, ls, gs, ct, worst)
            l_ll, g_ll = st.loglike(x, "f32", flags)  # (jac_reduce_kernel without F)
            np.testing.assert_allclose(lnl, l_ll, rtol=1e-6, atol=0, err_msg=tag)
            scale = np.einsum("nk,njk->nj", np.abs(w64 * (data - y.astype(np.float64))), np.abs(jac.astype(np.float64)))
            assert np.all(np.abs(g - g_ll) <= 1e-6 * scale), (tag, np.max(np.abs(g - g_ll) / scale))
            assert np.array_equal(st.loglike(x, "f32", flags, grad=False), l_ll), tag
            st.set_nuisance(None)
            assert st.nuisance_modes() == 0
            after = st.fisher(x, "f32", flags, lnl=True, grad=True) + st.loglike(x, "f32", flags)
            for a, b in zip(before, after):
                assert same(a, b), tag
        st.set_likelihood(None, None)
    print("worst of the reductions, fractions of the bounds: %s" % {k: "%.3g" % v for k, v in worst.items()})
    # refused: out_dim = 1 (one live bin for one mode), and out_dim = 3 with two live bins for four modes
    for name, K in (("i1o1", 1), ("i2o1", 1), ("i4o3", 4)):
        case = sc.BY_NAME[name]
        st, rec = device_stack(ctx, case.dims, case.act)
        flags = flags_of(nat, rec["tin"] is not None)
        data, w, _ = likelihood(rec, 3)
        st.set_likelihood(data, w)
        x = sc.rows(case.dims, 4, 2)
        before = st.loglike(x, "f32", flags)
        assert status_of(lambda: st.set_nuisance(sc.basis(case.dims[-1], K))) == ARG, name
        assert st.nuisance_modes() == 0
        for a, b in zip(before, st.loglike(x, "f32", flags)):
            assert same(a, b), name
        st.set_likelihood(None, None)


def test_foreground_scale_at_a_lane_tail(ctx):
    """out_dim = 65, data = y(truth) + a 5-mode foreground of 1e6 OUT_STD + noise in float32: the record's path and a data
    matrix of 3 rows through fit(max_iter = 0) -- nuis_project_kernel with one bin past the first pass of the lanes and
    n_data no multiple of the 4 rows of a workgroup -- against marg_ref fed the same float32 data (test_foreground_scale).
    Measured on the MI355X: F 1.1e-7, lnl 5.7e-8, grad 4.9e-8 (record), lnl_start through fit 8.2e-8 (bounds 1e-5)."""
    nat = pkg("_native")
    case = sc.BY_NAME["i4o65"]
    st, rec = device_stack(ctx, case.dims, case.act)
    flags = flags_of(nat, rec["tin"] is not None)
    prob = sc.fit_problem(case)
    w, K = prob["w"], 5
    A = sc.basis(65, K)
    rng = np.random.default_rng(9)
    d3 = np.vstack([prob["data"], prob["data"][:1]]).astype(np.float64)
    d32 = (d3 + (1e6 * sc.OUT_STD * rng.normal(size=(3, K)) / (1 + np.arange(K))) @ A).astype(np.float32)
    assert np.abs(d32).max() > 1e6
    worst = {"F": 0.0, "lnl": 0.0, "grad": 0.0, "coef": 0.0}
    x0 = np.tile(prob["x0"], (2, 1))[:9]  # 9 starts, 3 per data row
    st.set_likelihood(d32[0], w)
    st.set_nuisance(A)
    F, lnl, g = st.fisher(x0, "f32", flags, lnl=True, grad=True)
    y, jac = st.jacobian(x0, "f32", flags, return_outputs=True)
    ref, ls, gs, ct = reference(y, jac, d32[0], w, A)
    assert np.all(ls < 1e-6 * np.sum(w * d32[0].astype(np.float64) ** 2))
    check_reduction("record", F, lnl, g, st.nuisance_coef(x0, "f32", flags), ref, ls, gs, ct, worst)
    u0 = st.sample(x0, "f32", flags, data=d32, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"]
    r = st.fit(x0, "f32", flags, data=d32, max_iter=0)
    y, jac = st.jacobian(u0, "f32", nat.FWD_OUT_TRANSFORM, return_outputs=True)
    ref, ls, gs, _ = reference(y, jac, d32[np.arange(9) // 3], w, A)
    el = np.abs(r["lnl_start"] - ref["lnl"]) / ls
    print("fit lnl_start: %.2e (of 1e-5)" % el.max())
    assert el.max() <= 1e-5, el.max()
    assert same(r["lnl"], r["lnl_start"])
    s = st.sample(x0, "f32", flags, data=d32, n_steps=0, n_warmup=0)
    assert same(s["lnl_last"], r["lnl_start"])
    st.set_likelihood(None, None)


FIT_CASES = [c for c in sc.CASES if c.fit]


@pytest.mark.parametrize("case", FIT_CASES, ids=[c.name for c in FIT_CASES])
def test_fits(ctx, case):
    """fit_lm_kernel at in_dim 1, 4, 5 and 8 against fit_ref.lm_ref as test_fit_against_lm_ref compares them (lnl >= ref -
    1e-4 max(1, |ref|); u within 1e-4 where the reference converged inside the box with cond(F) < 1e6 -- every start of
    the table, test_shapes_cpu), monotone, inside the box, rows independent of their neighbours; a start outside the box
    and one with a NaN are clamped.  Measured on the MI355X: every row converged (status 1), worst |u - ref| 0.074 of
    1e-4 (in_dim 1), 0.0074, 0.0024, 0.029 (in_dim 4, 5, 8)."""
    nat = pkg("_native")
    st, rec = device_stack(ctx, case.dims, case.act)
    tin, tout = rec["tin"], rec["tout"]
    flags = flags_of(nat, rec["tin"] is not None)
    prob = sc.fit_problem(case)
    data, w, x0 = prob["data"], prob["w"], prob["x0"]
    st.set_likelihood(data[0], w)
    r = st.fit(x0, "f32", flags, data=data, max_iter=40, fisher=True)
    assert st.last_jac_route()[0] == "generic"
    ud = jr.transform(r["x_hat"], *tin)[0]
    worst, compared = 0.0, 0
    for i in range(x0.shape[0]):
        ev = fr.evaluator(rec["Ws"], rec["bs"], rec["act"], data[i // sc.FIT_STARTS], w, tout)
        ref = fr.lm_ref(ev, prob["u0"][i], max_iter=40)
        tol = 1e-4 * max(1.0, abs(ref["lnl"]))
        assert r["lnl"][i] >= ref["lnl"] - tol, (i, r["lnl"][i], ref["lnl"], r["status"][i], ref["status"])
        if ref["status"] == 1 and np.all(np.abs(ref["u"]) < 1 - 1e-3) and np.linalg.cond(ev(ref["u"])[2]) < 1e6:
            np.testing.assert_allclose(ud[i], ref["u"], atol=1e-4, err_msg=str(i))
            worst, compared = max(worst, float(np.max(np.abs(ud[i] - ref["u"]))) / 1e-4), compared + 1
    assert compared == x0.shape[0]
    print("%s: worst |u - ref| %.3g (of 1e-4), status %s" % (case.name, worst, r["status"]))
    assert np.all(r["lnl"] >= r["lnl_start"]) and np.all(np.isfinite(r["lnl"])) and set(np.unique(r["status"])) <= {0, 1, 2}
    assert np.all(np.abs(ud) <= 1 + 1e-6)
    # ln L at the start and the Fisher matrix at x_hat are the entries' own
    for k in range(sc.FIT_TRUTHS):
        rows_k = slice(k * sc.FIT_STARTS, (k + 1) * sc.FIT_STARTS)
        st.set_likelihood(data[k], w)
        np.testing.assert_allclose(r["lnl_start"][rows_k], st.loglike(x0[rows_k], "f32", flags, grad=False), rtol=1e-6, atol=0)
        assert np.array_equal(r["fisher"][rows_k], st.fisher(r["x_hat"][rows_k], "f32", flags))
        # a row does not depend on its neighbours: the rows of one spectrum, and one row of them, refitted alone
        part = st.fit(x0[rows_k], "f32", flags, data=data[k:k + 1], max_iter=40, fisher=True)
        one = st.fit(x0[rows_k][1:2], "f32", flags, max_iter=40, fisher=True)
        for key in ("x_hat", "lnl", "lnl_start", "status", "fisher"):
            assert same(part[key], r[key][rows_k]), (k, key)
            assert same(one[key], r[key][rows_k][1:2]), (k, key)
    # the clamps: a coordinate far outside the box, a NaN, and the column with the zero floor at 0
    xo, xn, xz = x0[:1].copy(), x0[1:2].copy(), x0[2:3].copy()
    xo[0, -1] = 1e30
    xn[0, 0] = np.nan
    xz[0, 0] = 0.0
    xs = np.vstack([xo, xn, xz])
    r0 = st.fit(xs, "f32", flags, max_iter=0)
    uc = jr.transform(r0["x_hat"], *tin)[0]
    assert np.all(np.isfinite(r0["x_hat"])) and abs(uc[0, -1] - 1.0) <= 1e-6 and abs(uc[1, 0] + 1.0) <= 1e-6 and abs(uc[2, 0] + 1.0) <= 1e-6
    rc = st.fit(xs, "f32", flags, max_iter=20)
    assert np.all(np.isfinite(rc["x_hat"])) and np.all(rc["lnl"] >= rc["lnl_start"]) and same(rc["lnl_start"], r0["lnl"])
    assert np.all(np.abs(jr.transform(rc["x_hat"], *tin)[0]) <= 1 + 1e-6)
    st.set_likelihood(None, None)


@pytest.mark.parametrize("case", FIT_CASES, ids=[c.name for c in FIT_CASES])
def test_sampler_transition(ctx, case):
    """test_sample_gpu.test_one_transition_against_reference at in_dim 1, 4, 5 and 8 (one Philox block, one, two of which
    three normals are unused, two full): 384 chains, seed (both words), chain0 and step0 non-zero.  The proposal equals
    the float64 rebuild up to its float32 store, log alpha lies within its first-order bound, the accept decisions agree
    outside the excused share (<= 0.5 %); 20 transitions in two calls equal one call bit for bit.  Measured on the MI355X:
    proposal and log alpha below 0.001 of their bounds, 0 of 384 decisions excused at every in_dim."""
    nat = pkg("_native")
    st, rec = device_stack(ctx, case.dims, case.act)
    tin = rec["tin"]
    flags = flags_of(nat, rec["tin"] is not None)
    din = case.dims[0]
    prob = sc.fit_problem(case)
    st.set_likelihood(prob["data"][0], prob["w"])
    x0 = sc.chain_starts(case, prob)
    n = x0.shape[0]
    opts = dict(eps0=sc.EPS0, ridge=sc.RIDGE, seed=sc.SEED, chain0=sc.CHAIN0)
    u0 = st.sample(x0, "f32", flags, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
    assert np.max(np.abs(u0 - jr.transform(x0, *tin)[0])) <= 2.0 ** -23
    r = st.sample(x0, "f32", flags, n_steps=1, n_warmup=0, step0=sc.STEP0, diagnostics=True, **opts)
    assert st.last_jac_route()[0] == "generic"
    e0 = device_eval(st, nat, u0, "f32")
    chains, eps = sc.CHAIN0 + np.arange(n), np.full(n, sc.EPS0)
    prop_ref, _, inside = sr.propose(u0, e0[1], e0[2], eps, sr.normals(sc.SEED, chains, sc.STEP0, din), sc.RIDGE)
    prop = r["last_prop_u"].astype(np.float64)
    err = np.abs(prop - prop_ref)
    tol = np.spacing(np.abs(prop_ref).astype(np.float32)) + 1e-12
    assert np.all(err <= tol), (case.name, np.max(err / tol))
    e1 = device_eval(st, nat, prop, "f32")
    la = alpha_of(u0, e0, prop, e1, eps, sc.RIDGE)
    bound = alpha_bound(u0, e0, prop, e1, eps, sc.RIDGE, la)
    la_dev = r["last_log_alpha"]
    fin = np.isfinite(la)
    assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), case.name
    ratio = np.abs(la_dev[fin] - la[fin]) / bound[fin]
    assert np.all(ratio <= 1.0), (case.name, ratio.max())
    logu = np.log(sr.accept_uniform(sc.SEED, chains, sc.STEP0))
    acc_ref, acc_dev = logu < la, r["accept_rate"] > 0.5
    excused = np.abs(logu - la) <= bound
    print("%s: proposal max err / tol %.3f, inside %.3f, log alpha max diff / bound %.3f, accepted %.3f, excused %d of %d"
          % (case.name, np.max(err / tol), inside.mean(), ratio.max(), acc_dev.mean(), excused.sum(), n))
    assert excused.mean() <= 0.005
    assert np.array_equal(acc_ref[~excused], acc_dev[~excused])
    u1 = np.where(acc_dev[:, None], prop, u0)
    np.testing.assert_allclose(r["x_last"], fr.untransform(u1, tin[0], tin[2], tin[3]), rtol=1e-12)
    # 20 transitions = 10, then 10 more from x_last with step0 advanced
    keys = ("samples", "samples_lnl", "x_last", "lnl_last", "mean_u")
    k = 10
    xs = x0[:32]
    two = st.sample(xs, "f32", flags, n_steps=2 * k, n_warmup=0, step0=sc.STEP0, **opts)
    first = st.sample(xs, "f32", flags, n_steps=k, n_warmup=0, step0=sc.STEP0, **opts)
    second = st.sample(first["x_last"], "f32", flags, n_steps=k, n_warmup=0, step0=sc.STEP0 + k, eps_start=first["eps_last"],
                       **dict(opts, eps0=1.0))
    assert np.all(np.isfinite(two["samples"])) and 0 < two["accept_rate"].mean() < 1
    assert same(two["samples"], np.concatenate([first["samples"], second["samples"]], axis=1))
    assert same(two["x_last"], second["x_last"]) and same(two["samples_lnl"][:, k:], second["samples_lnl"])
    assert np.all(np.abs(jr.transform(two["samples"].reshape(-1, din), *tin)[0]) <= 1 + 1e-12)
    # the moments of the kept transitions, recomputed from the stored samples (the padding of su / suu below 8 inputs)
    us = jr.transform(two["samples"].reshape(-1, din), *tin)[0].reshape(xs.shape[0], 2 * k, din)
    np.testing.assert_allclose(two["mean_u"], us.mean(axis=1), atol=1e-13)
    np.testing.assert_allclose(two["cov_u"], np.einsum("nki,nkj->nij", us, us) / (2 * k) - np.einsum("ni,nj->nij", us.mean(axis=1), us.mean(axis=1)),
                               atol=1e-13)
    st.set_likelihood(None, None)


def test_launch_split_at_65535_rows(ctx):
    """[2, 4, 3] at 65,537 rows: jacobian_dev and loglike_dev cross the 65,535-row launch split of the generic route in one
    call (second launch: two rows, every pointer moved by the offset); the host forms (chunks of 8,192 rows) give the same
    bits, the rows on both sides of the split match float64, 64 guard rows behind every output stay as they were"""
    nat = pkg("_native")
    dims, act = sc.SPLIT
    st, rec = device_stack(ctx, dims, act)
    flags = flags_of(nat, rec["tin"] is not None)
    n, din, dout, g = sc.SPLIT_ROWS, 2, 3, 64
    data, w, w64 = likelihood(rec, 1)
    st.set_likelihood(data, w)
    x = sc.rows(dims, n, 5).astype(np.float32)
    xp = np.zeros((n, din + 1), np.float32)
    xp[:, :din] = x
    sizes = {"y": (n + g) * dout, "jac": (n + g) * din * dout, "lnl": n + g, "grad": (n + g) * din}
    d = {}
    try:
        d["x"] = ctx.malloc(xp.nbytes)
        for k, v in sizes.items():
            d[k] = ctx.malloc(v * 4)
            ctx.memset(d[k], 0x7F, v * 4)
        ctx.h2d(d["x"], xp)
        st.jacobian_dev(d["x"], din + 1, n, d["y"], dout, d["jac"], "f32", flags)
        st.loglike_dev(d["x"], din + 1, n, d["lnl"], d["grad"], "f32", flags)
        ctx.sync()
        out = {}
        for k, shape in (("y", (n + g, dout)), ("jac", (n + g, din, dout)), ("lnl", (n + g,)), ("grad", (n + g, din))):
            out[k] = np.empty(shape, np.float32)
            ctx.d2h(out[k], d[k])
    finally:
        for p in d.values():
            ctx.free(p)
    for k, a in out.items():
        assert np.all(a[n:].view(np.uint32) == POISON), k
        assert np.all(np.isfinite(a[:n])), k
    yh, jh = st.jacobian(x, "f32", flags, return_outputs=True)
    lh, gh = st.loglike(x, "f32", flags)
    for k, a in (("y", yh), ("jac", jh), ("lnl", lh), ("grad", gh)):
        bad = np.flatnonzero((a.reshape(n, -1).view(np.uint32) != out[k][:n].reshape(n, -1).view(np.uint32)).any(axis=1))
        assert bad.size == 0, (k, bad[:8])
    idx = np.unique(np.r_[0, 65534, 65535, 65536, np.random.default_rng(0).choice(n, 500, replace=False)])
    yr, Jr = jr.jacobian(rec["Ws"], rec["bs"], act, x[idx], rec["tin"], rec["tout"])
    np.testing.assert_allclose(out["y"][idx], yr, rtol=1e-5, atol=2e-5 * sc.OUT_STD)
    xt = jr.transform(x[idx], *rec["tin"])[0]
    check_rows("split", "f32", out["jac"][idx], Jr, rec["Ws"], rec["bs"], act, xt, True, x[idx], rec["tin"], rec["tout"])
    l64, g64 = jr.loglike(out["y"][idx], out["jac"][idx], data, w64)
    np.testing.assert_allclose(out["lnl"][idx], l64, rtol=1e-5, atol=0)
    scale = np.einsum("nk,njk->nj", np.abs(w64 * (data - out["y"][idx].astype(np.float64))), np.abs(out["jac"][idx].astype(np.float64)))
    assert np.all(np.abs(out["grad"][idx] - g64) <= 1e-5 * scale)
    st.set_likelihood(None, None)


def test_guard_rows_of_fisher_and_fit(ctx):
    """fisher_dev (in_dim 8 / out_dim 64 and in_dim 15 / out_dim 65) and fit_dev (in_dim 8) at n = 5: the bytes past row n
    of every output stay as they were, and the rows equal the host forms'"""
    nat = pkg("_native")
    n, g = 5, 64
    for name in ("i8o64", "i15o65"):
        case = sc.BY_NAME[name]
        st, rec = device_stack(ctx, case.dims, case.act)
        din = case.dims[0]
        flags = flags_of(nat, rec["tin"] is not None)
        data, w, _ = likelihood(rec, 2)
        st.set_likelihood(data, w)
        x = sc.rows(case.dims, n, 6).astype(np.float32)
        sizes = {"F": ((n + g, din, din), np.float32), "lnl": ((n + g,), np.float32), "grad": ((n + g, din), np.float32),
                 "xh": ((n + g, din), np.float32), "lnl0": ((n + g,), np.float32), "status": ((n + g,), np.int32)}
        d = {}

        def fetch(keys):
            res = {}
            for k in keys:
                res[k] = np.empty(*sizes[k])
                ctx.d2h(res[k], d[k])
                assert np.all(res[k][n:].view(np.uint32) == POISON), (name, k)
            return res

        try:
            d["x"] = ctx.malloc(x.nbytes)
            ctx.h2d(d["x"], x)
            for k, (shape, _) in sizes.items():
                d[k] = ctx.malloc(int(np.prod(shape)) * 4)
                ctx.memset(d[k], 0x7F, int(np.prod(shape)) * 4)
            st.fisher_dev(d["x"], din, n, d["F"], d["lnl"], d["grad"], "f32", flags)
            ctx.sync()
            o = fetch(("F", "lnl", "grad", "xh", "lnl0", "status"))
            Fh, lh, gh = st.fisher(x, "f32", flags, lnl=True, grad=True)
            assert same(Fh, o["F"][:n]) and same(lh, o["lnl"][:n]) and same(gh, o["grad"][:n]), name
            if din <= 8:
                for k in ("F", "lnl"):
                    ctx.memset(d[k], 0x7F, int(np.prod(sizes[k][0])) * 4)
                st.fit_dev(d["x"], din, n, None, 0, d["xh"], d["lnl"], d["lnl0"], d["F"], d["status"], "f32", flags, max_iter=5,
                           check_every=2)
                ctx.sync()
                o = fetch(("xh", "lnl", "lnl0", "F", "status", "grad"))
                r = st.fit(x, "f32", flags, max_iter=5, check_every=2, fisher=True)
                for key, a in (("x_hat", o["xh"]), ("lnl", o["lnl"]), ("lnl_start", o["lnl0"]), ("fisher", o["F"]), ("status", o["status"])):
                    assert same(r[key], a[:n]), (name, key)
        finally:
            for p in d.values():
                ctx.free(p)
        st.set_likelihood(None, None)
