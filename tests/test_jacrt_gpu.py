"""GPU: fused_jac<ArchRT, Prec> instantiated at run time (csrc/jit.hip: kJitJac) -- the "fused_rt" route of
the Jacobian-side calls, opt-in per handle (Stack.jit_jacobian) -- on the small stacks of tests/jacrt_cases.py: ReLU /
linear stacks and stacks with the smooth activations of csrc/act.h, both group sizes, partial tiles, every row count at a
wave's and a workgroup's edge.  Compilation is the module fixture's cost (build() leaves the code objects in
kernel_cache/).  No reference is recomputed: jacrt_cases caches stacks, the fixture caches the device's results."""
import numpy as np
import pytest

import act_ref as ar
import fit_ref as fr
import half_ref as hr
import jacobian_ref as jr
import jacrt_cases as jc
import shape_cases as sc
from conftest import pkg
from helpers import JAC16_TOL
from infer_support import check_reduction, flags_of, reference

pytestmark = pytest.mark.gpu

F32_BOUND = 1e-5   # per-row relative Frobenius error of an f32 Jacobian


def _handle(ctx, rec):
    st = pkg("_native").Stack(ctx, rec["dims"], rec["act"])
    st.set_weights(rec["flat"])
    if rec["tin"] is not None:
        st.set_input_transform(*rec["tin"])
    st.set_output_transform(rec["tout"][0], rec["tout"][1].astype(np.float32))
    return st


def _flags(nat, tin_on, tout_on):
    return (nat.FWD_IN_TRANSFORM if tin_on else 0) | (nat.FWD_OUT_TRANSFORM if tout_on else 0)


@pytest.fixture(scope="module")
def rt(ctx):
    """per case: the handle that asked (every precision, forward kernel too), a twin that never asks, and the device's
    (y, J) of every call of jacrt_cases.calls on the fused_rt route, computed once"""
    nat = pkg("_native")
    out = {}
    for name in jc.CASES:
        rec = jc.stack(name)
        st, twin = _handle(ctx, rec), _handle(ctx, rec)
        for prec in jc.PRECS:
            assert st.jit_jacobian(prec, -1) == "ready", (name, prec)
            assert st.jit(prec, -1) == "ready", (name, prec)
        out[name] = {"st": st, "twin": twin, "rec": rec, "got": {}}
    return out


def _run(rt, name, prec):
    """[(n, tin_on, tout_on, x, y, J)] of a case in a precision on the asked handle, cached"""
    nat = pkg("_native")
    e = rt[name]
    if prec not in e["got"]:
        st, res = e["st"], []
        for n, tin_on, tout_on, x in jc.calls(name):
            c0 = st.last_jac_route()[1].get("fused_rt", 0)
            y, J = st.jacobian(x, prec, _flags(nat, tin_on, tout_on), return_outputs=True)
            last, counts = st.last_jac_route()
            assert last == "fused_rt" and counts["fused_rt"] == c0 + 1, (name, prec, n, last, counts)
            res.append((n, tin_on, tout_on, x, y, J))
        e["got"][prec] = res
    return e["got"][prec]


# ---- 1. the primal is the forward's run-time route, bit for bit
@pytest.mark.parametrize("prec", jc.PRECS)
@pytest.mark.parametrize("name", list(jc.CASES))
def test_primal_is_bit_identical_to_the_forward(rt, name, prec):
    nat = pkg("_native")
    st, rec = rt[name]["st"], rt[name]["rec"]
    for n, tin_on, tout_on, x, y, J in _run(rt, name, prec):
        tag = (name, prec, n, tin_on, tout_on)
        assert y.shape == (n, rec["dims"][-1]) and J.shape == (n, rec["dims"][0], rec["dims"][-1]), tag
        yf = st.forward(x, prec, _flags(nat, tin_on, tout_on) | nat.FWD_FORCE_JIT)
        assert st.last_route()[0] == "fused_rt", tag
        assert np.array_equal(y.view(np.uint32), yf.view(np.uint32)), tag


# ---- 2. run time equals compiled (S4, f16): same template, same options, same stream
def test_runtime_kernel_equals_the_compiled_one(ctx):
    nat = pkg("_native")
    rec = jc.stack("S4")
    st = _handle(ctx, rec)
    assert st.jit_jacobian("f16", -1) == "ready"   # (compiled in: nothing is asked for)
    for n in (1, 9, 130):
        x = sc.rows_u(rec["dims"], n, 20 + n).astype(np.float32)
        y0, J0 = st.jacobian(x, "f16", nat.FWD_OUT_TRANSFORM, return_outputs=True)
        assert st.last_jac_route()[0] == "fused", n
        y1, J1 = st.jacobian(x, "f16", nat.FWD_OUT_TRANSFORM | nat.FWD_FORCE_JIT, return_outputs=True)
        assert st.last_jac_route()[0] == "fused_rt", n
        assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32)) and np.array_equal(J0.view(np.uint32), J1.view(np.uint32)), n
    st.jacobian(x, "f16", nat.FWD_OUT_TRANSFORM)
    assert st.last_jac_route()[0] == "fused"   # a compiled stack keeps its kernel when nothing forces the other


# ---- 3. f32 against float64, and against the generic route
@pytest.mark.parametrize("name", list(jc.CASES))
def test_f32_jacobian_against_float64_and_the_generic_route(rt, name):
    nat = pkg("_native")
    rec, twin = rt[name]["rec"], rt[name]["twin"]
    worst = worst_g = 0.0
    for n, tin_on, tout_on, x, y, J in _run(rt, name, "f32"):
        tag = (name, n, tin_on, tout_on)
        keep = ~jc.kink_rows(rec, jc.transformed(rec, x, tin_on))
        assert keep.any() and (keep.all() or name in jc.RELU_CASES), tag
        yr, Jr = jc.reference64(rec, x, tin_on, tout_on)
        e = jr.rel_frobenius(J, Jr)[keep]
        Jg = twin.jacobian(x, "f32", _flags(nat, tin_on, tout_on))
        assert twin.last_jac_route()[0] == "generic", tag
        eg = jr.rel_frobenius(J, Jg)[keep]
        worst, worst_g = max(worst, e.max()), max(worst_g, eg.max())
        assert np.isfinite(J).all() and e.max() <= F32_BOUND, (tag, e.max())
        assert eg.max() <= F32_BOUND, (tag, "against generic", eg.max())
        np.testing.assert_allclose(y, yr, rtol=1e-5, atol=2e-5 * (rec["tout"][0] if tout_on else 1.0), err_msg=str(tag))
    print("JACRT f32 %s: worst row against float64 %.3e, against the generic route %.3e (bound %.0e)" % (name, worst, worst_g, F32_BOUND))
    assert set(twin.last_jac_route()[1]) == {"generic"}


# ---- 4. 16 bits, ReLU / linear stacks: the rounding reference, JAC16_TOL as it stands
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(jc.RELU_CASES))
def test_16_bit_relu_jacobian_matches_rounding_reference(rt, name, prec):
    rec = rt[name]["rec"]
    worst = 0.0
    for n, tin_on, tout_on, x, y, J in _run(rt, name, prec):
        _, J16 = jc.jacobian16(rec, x, prec, tin_on, tout_on)
        stat = hr.jac_worst_cell_median(J, J16)
        worst = max(worst, stat)
        print("JACRT16 %s %s n=%d: worst-cell median %.3e (bound %.1e)" % (name, prec, n, stat, JAC16_TOL[prec]))
        assert stat <= JAC16_TOL[prec], (name, prec, n, stat)
    print("JACRT16 worst %s %s: %.3e" % (name, prec, worst))


# ---- 5. 16 bits, smooth stacks: the restatement of jacrt_cases, medians per (input, 32-bin tile) cell
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(jc.SMOOTH_CASES))
def test_16_bit_smooth_jacobian_matches_rounding_reference(rt, name, prec):
    rec = rt[name]["rec"]
    tol = jc.SMOOTH16_TOL[prec]
    worst, least = 0.0, {m: np.inf for m in jc.SMOOTH_MUTATIONS}
    for n, tin_on, tout_on, x, y, J in _run(rt, name, prec):
        _, J16 = jc.jacobian16(rec, x, prec, tin_on, tout_on)
        stat = hr.jac_worst_cell_median(J, J16)
        worst = max(worst, stat)
        print("JACRT16 %s %s n=%d: worst-cell median %.3e (bound %s)" % (name, prec, n, stat, tol))
        assert tol is not None and stat <= tol, (name, prec, n, stat)
        if n >= hr.JAC_POOL_BELOW:   # the catalogue on the device's own J: refused, and at least 4x beyond the bound
            for mut in jc.SMOOTH_MUTATIONS:
                Jm = np.asarray(J, np.float64) + (jc.jacobian16(rec, x, prec, tin_on, tout_on, mut=mut)[1] - J16)
                v = hr.jac_worst_cell_median(Jm, J16)
                least[mut] = min(least[mut], v)
                print("JACRT16 %s %s n=%d: %s worst-cell median %.3e" % (name, prec, n, mut, v))
                assert v >= 4 * tol, (name, prec, n, "the bound is more than 1/4 of what the mutation makes", mut, v)
    print("JACRT16 worst %s %s: %.3e; mutations least %s" % (name, prec, worst, {m: "%.3e" % v for m, v in least.items()}))


# ---- 6. saturation: units 1 and 2 of every hidden layer sit at bias +-90
def _reads_only(ctx, rec, layer, unit, prec):
    """a twin whose layer `layer` + 1 reads only `unit` of hidden layer `layer`: its J is the image of the tangents that
    pass through that one saturated unit"""
    nat = pkg("_native")
    Ws = [np.array(W, np.float32) for W in rec["Ws"]]
    keep = np.zeros(rec["dims"][layer + 1], bool)
    keep[unit] = True
    Ws[layer + 1][~keep, :] = 0.0
    st = nat.Stack(ctx, rec["dims"], rec["act"])
    st.set_weights(jr.ora.flatten_params(Ws, rec["bs"]))
    assert st.jit_jacobian(prec, -1) == "ready"
    x = sc.rows_u(rec["dims"], 9, 5).astype(np.float32)
    J = st.jacobian(x, prec, 0)
    assert st.last_jac_route()[0] == "fused_rt" and np.isfinite(J).all()
    return dict(rec, Ws=Ws), x, J


@pytest.mark.parametrize("prec", jc.PRECS)
@pytest.mark.parametrize("name", list(jc.SMOOTH_CASES))
def test_saturated_units_give_finite_jacobians(ctx, rt, name, prec):
    """J is finite everywhere; and the tangents THROUGH a saturated unit -- of every hidden layer, one unit at a time -- are
    what the formulas of csrc/act.h give at |z| ~ 90:
      tanh, either side: exactly 0 (exp(-180) underflows to 0);
      sigmoid either side, elu and softplus at -90: the factor is ~exp(-90) = 8e-40, below f32's normal range -- J is zero to
        that range, exactly 0 in f16 where the pack rounds it away (bf16 has f32's exponents and keeps a subnormal);
      elu and softplus at +90: the linear side, factor exactly 1 -- J is the reference's: float64 within the f32 bound, and in
        16 bits the rounding restatement (jacrt_cases.jvp16_smooth) within the bound of the smooth 16-bit check."""
    for _, _, _, _, y, J in _run(rt, name, prec):
        assert np.isfinite(J).all() and np.isfinite(y).all(), (name, prec)
    rec = rt[name]["rec"]
    tiny = 0.0 if prec == "f16" else 1e-37
    for layer, code in enumerate(rec["act"][:-1]):
        for unit, side in ((1, +1), (2, -1)):   # bias +90, bias -90
            rec1, x, J = _reads_only(ctx, rec, layer, unit, prec)
            tag = (name, prec, layer, ar.NAMES[code], side)
            if code == ar.TANH:
                assert np.all(J == 0), (tag, np.abs(J).max())
            elif code == ar.SIGMOID or side < 0:
                assert np.abs(J).max() <= tiny, (tag, np.abs(J).max())
            elif prec == "f32":
                Jr = jc.reference64(rec1, x, False, False)[1]
                e = jr.rel_frobenius(J, Jr).max()
                print("JACRT saturation %s: linear side against float64 %.3e" % (tag, e))
                assert np.abs(Jr).max() > 0 and e <= F32_BOUND, (tag, e)
            else:
                J16 = jc.jacobian16(rec1, x, prec, False, False)[1]
                stat = hr.jac_worst_cell_median(J, J16)
                print("JACRT saturation %s: linear side against the rounding reference %.3e" % (tag, stat))
                assert np.abs(J16).max() > 0 and stat <= jc.SMOOTH16_TOL[prec], (tag, stat)


# ---- 7. the consumers on the route
def _record(rec, seed=3, K=0):
    w = sc.weights(rec["dims"][-1], seed, K)
    assert (w == 0).any()
    return sc.data_for(rec, seed)[0] if not jc.smooth(rec["act"]) else _smooth_data(rec, seed), w


def _smooth_data(rec, seed):
    x1 = sc.rows(rec["dims"], 1, 90 + seed)
    y = jc.reference64(rec, x1, True, True)[0][0]
    return (y + np.random.default_rng(3000 + seed).normal(size=rec["dims"][-1]) * 0.05 * sc.OUT_STD).astype(np.float32)


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("name", ["R1", "T1"])
def test_loglike_and_fisher_on_the_route(rt, name, prec):
    """test_fit_gpu's identity: ln L, g and F against the float64 reductions of the device's OWN y and J, <= 1e-5 relative"""
    nat = pkg("_native")
    st, rec = rt[name]["st"], rt[name]["rec"]
    flags = flags_of(nat, True)
    data, w = _record(rec)
    st.set_likelihood(data, w)
    try:
        x = sc.rows(rec["dims"], 33, 61)
        c0 = st.last_jac_route()[1].get("fused_rt", 0)
        lnl, g = st.loglike(x, prec, flags)
        assert st.last_jac_route()[0] == "fused_rt"
        F, lnl_f, g_f = st.fisher(x, prec, flags, lnl=True, grad=True)
        assert st.last_jac_route()[0] == "fused_rt"
        y, J = st.jacobian(x, prec, flags, return_outputs=True)
        assert st.last_jac_route()[1]["fused_rt"] == c0 + 3
        w64, d64 = w.astype(np.float64), data.astype(np.float64)
        lr, gr = jr.loglike(y, J, d64, w64)
        gscale = np.einsum("nk,njk->nj", np.abs(w64 * (d64 - y)), np.abs(J.astype(np.float64)))
        for l_, g_ in ((lnl, g), (lnl_f, g_f)):
            assert np.all(np.abs(l_ - lr) <= 1e-5 * np.abs(lr)), (name, prec, np.max(np.abs(l_ - lr) / np.abs(lr)))
            assert np.all(np.abs(g_ - gr) <= 1e-5 * gscale), (name, prec, np.max(np.abs(g_ - gr) / gscale))
        assert jr.rel_frobenius(F, fr.fisher_ref(J, w64)).max() <= 1e-5, (name, prec)
    finally:
        st.set_likelihood(None, None)


def test_marginalised_reductions_on_the_route(rt):
    nat = pkg("_native")
    st, rec = rt["R1"]["st"], rt["R1"]["rec"]
    flags = flags_of(nat, True)
    data, w = _record(rec, K=4)
    st.set_likelihood(data, w)
    try:
        A = sc.basis(rec["dims"][-1], 4)
        st.set_nuisance(A)
        x = sc.rows(rec["dims"], 33, 62)
        for prec in ("f32", "f16"):
            F, lnl, g = st.fisher(x, prec, flags, lnl=True, grad=True)
            assert st.last_jac_route()[0] == "fused_rt"
            y, J = st.jacobian(x, prec, flags, return_outputs=True)
            ref, ls, gs, _ = reference(y, J, data, w, A)
            check_reduction("JACRT marginalised R1 %s" % prec, F, lnl, g, None, ref, ls, gs, None, {"F": 0.0, "lnl": 0.0, "grad": 0.0})
    finally:
        st.set_likelihood(None, None)


def _truth_and_starts(rec, n, seed, scale):
    tin = rec["tin"]
    rng = np.random.default_rng(seed)
    tu = rng.uniform(-0.5, 0.5, size=(1, rec["dims"][0]))
    us = np.clip(tu + scale * rng.normal(size=(n, rec["dims"][0])), -0.95, 0.95)
    return fr.untransform(tu, tin[0], tin[2], tin[3]), fr.untransform(us, tin[0], tin[2], tin[3])


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_fit_and_sampler_on_the_route(rt, prec):
    """a fit on T1 recovers a point the stack made itself (test_act_gpu's criterion: best ln L >= -0.5 at sigma = 1), on ONE
    route for all its iterations; one sample call of 64 chains x 20 transitions is finite and on the route.  (The
    transition is not rebuilt here: infer_support's helpers are written for 7 inputs.)"""
    nat = pkg("_native")
    st, rec = rt["T1"]["st"], rt["T1"]["rec"]
    flags = flags_of(nat, True)
    truth, starts = _truth_and_starts(rec, 8, 4, 0.1)
    spectrum = st.forward(truth, prec, flags | nat.FWD_FORCE_JIT)[0]
    w = np.where(sc.weights(rec["dims"][-1], 3) > 0, 1.0, 0.0).astype(np.float32)   # sigma = 1, zero-weight bins
    st.set_likelihood(spectrum, w)
    try:
        before = dict(st.last_jac_route()[1])
        res = st.fit(starts, prec, flags, max_iter=100, fisher=True)
        last, counts = st.last_jac_route()
        moved = {k: v - before.get(k, 0) for k, v in counts.items() if v != before.get(k, 0)}
        assert last == "fused_rt" and moved == {"fused_rt": 2}, moved   # the fit and its Fisher matrix: a single route
        print("JACRT fit T1 %s: ln L of the 8 starts %s" % (prec, res["lnl"]))
        assert np.isfinite(res["lnl"]).all() and res["lnl"].max() >= -0.5, res["lnl"]
        _, x0 = _truth_and_starts(rec, 64, 5, 0.03)
        s = st.sample(x0, prec, flags, n_steps=20, n_warmup=0)
        assert st.last_jac_route()[0] == "fused_rt"
        for k in ("x_last", "lnl_last", "accept_rate", "mean_u", "cov_u"):
            assert np.isfinite(s[k]).all(), k
        t = st.sample_tempered(x0, 2, [1.0, 0.5], 5, prec, flags, n_steps=20, n_warmup=0)
        assert st.last_jac_route()[0] == "fused_rt" and np.isfinite(t["lnl_last"]).all()
    finally:
        st.set_likelihood(None, None)


# ---- 8. latch and fallback
def test_opt_in_flags_and_refusals(ctx, rt):
    nat = pkg("_native")
    st, twin, rec = rt["R1"]["st"], rt["R1"]["twin"], rt["R1"]["rec"]
    flags = flags_of(nat, True)
    x = sc.rows(rec["dims"], 33, 63)
    data, w = _record(rec)
    for s in (st, twin):
        s.set_likelihood(data, w)
    try:
        for call in (lambda s, f: s.jacobian(x, "f32", f), lambda s, f: s.loglike(x, "f32", f), lambda s, f: s.fisher(x, "f32", f),
                     lambda s, f: s.fit(x[:8], "f32", f, max_iter=5)):
            call(twin, flags)
            assert twin.last_jac_route()[0] == "generic"            # never asked
            call(st, flags | nat.FWD_FORCE_GENERIC)
            assert st.last_jac_route()[0] == "generic"              # asked, forced away
            call(st, flags)
            assert st.last_jac_route()[0] == "fused_rt"
        assert set(twin.last_jac_route()[1]) == {"generic"}
    finally:
        for s in (st, twin):
            s.set_likelihood(None, None)
    # V21_FWD_FORCE_JIT on a stack that cannot have the kernel: V21_ERR_UNSUPPORTED, and the handle stays usable
    for key in ("i16o3", "i8relu"):
        dims, act, why = jc.REFUSALS[key]
        bad = _handle(ctx, sc.make_stack(dims, act))
        xb = sc.rows_u(dims, 5, 1).astype(np.float32)
        J0 = bad.jacobian(xb, "f32", 0)
        with pytest.raises(nat.EngineError, match=r"error -3.*V21_FWD_FORCE_JIT.*" + why):
            bad.jacobian(xb, "f32", nat.FWD_FORCE_JIT)
        with pytest.raises(nat.EngineError, match=why):
            bad.jit_jacobian("f32")
        J1 = bad.jacobian(xb, "f32", 0)
        assert bad.last_jac_route()[0] == "generic" and np.array_equal(J0, J1), key
    # a forced call asks: on a twin of its own, and from then on the handle has opted in
    t2 = _handle(ctx, rec)
    t2.jacobian(x, "f16", flags | nat.FWD_FORCE_JIT)
    assert t2.last_jac_route()[0] == "fused_rt"


def test_a_kernel_with_scratch_leaves_the_handle_on_generic(ctx):
    """9-500-512-33 in f16 compiles, spills, and is refused when its code object is loaded -- when the first call after
    jit_jacobian decides its route: that call and every later one record "generic" and compute what a handle that never
    asked computes, with no error; a forced call is refused; nothing is launched that needs scratch memory."""
    nat = pkg("_native")
    rec = sc.make_stack(*jc.SPILLS)
    st, twin = _handle(ctx, rec), _handle(ctx, rec)
    assert st.jit_jacobian("f16", -1) == "ready"   # compiled: the registers are counted when it is loaded
    x = sc.rows_u(rec["dims"], 33, 7).astype(np.float32)
    st.set_likelihood(*_record_of(rec))
    try:
        for _ in range(2):
            J = st.jacobian(x, "f16", nat.FWD_OUT_TRANSFORM)
            assert st.last_jac_route()[0] == "generic"
            F = st.fisher(x, "f16", nat.FWD_OUT_TRANSFORM)
            assert np.isfinite(F).all()
        assert set(st.last_jac_route()[1]) == {"generic"}, st.last_jac_route()
        assert np.array_equal(J, twin.jacobian(x, "f16", nat.FWD_OUT_TRANSFORM))
        with pytest.raises(nat.EngineError, match=r"error -3.*V21_FWD_FORCE_JIT.*register budget"):
            st.jacobian(x, "f16", nat.FWD_FORCE_JIT)
        with pytest.raises(nat.EngineError, match="register budget"):
            st.jit_jacobian("f16")
        assert np.array_equal(J, st.jacobian(x, "f16", nat.FWD_OUT_TRANSFORM)) and st.last_jac_route()[0] == "generic"
    finally:
        st.set_likelihood(None, None)
    # a forced call whose y pitch the kernel cannot address is refused, not sent to the generic kernel
    # (one row in real buffers: whatever the call did, it would stay inside them)
    ok = _handle(ctx, jc.stack("R1"))
    dx, dy, dj = ctx.malloc(5 * 4), ctx.malloc(37 * 4), ctx.malloc(5 * 37 * 4)
    try:
        ctx.h2d(dx, np.zeros((1, 5), np.float32))
        with pytest.raises(nat.EngineError, match=r"error -3.*V21_FWD_FORCE_JIT.*pitch"):
            ok.jacobian_dev(dx, 5, 1, dy, 1 << 21, dj, "f32", nat.FWD_FORCE_JIT)
        ctx.sync()
    finally:
        for p_ in (dx, dy, dj):
            ctx.free(p_)


def _record_of(rec, seed=3):
    return sc.data_for(rec, seed)[0], sc.weights(rec["dims"][-1], seed)


# ---- 9. the class surface
@pytest.fixture(scope="module")
def emulators():
    emulator, synth, eng = pkg("emulator"), pkg("synth"), pkg("engine")
    data = synth.make_dataset(n_train=600, n_val=40, n_test=40, seed=ar.SEEDS["T3"])
    out = []
    for _ in range(2):
        eng.set_random_seed(ar.SEEDS["T3"])
        out.append(emulator.DirectEmulator(hidden_dims=[64, 128], activation_func="tanh", **data))
    return out


def test_class_surface_compile_derivatives(emulators):
    em, twin = emulators
    for a, b in zip(em.emulator.layers, twin.emulator.layers):
        assert np.array_equal(a.kernel, b.kernel)
    assert em.compile_derivatives() == "ready"
    pars = em.par_test[:9]
    J, Jt = em.jacobian(pars), twin.jacobian(pars)
    st, stt = em._diff_stack(pars)[1], twin._diff_stack(pars)[1]
    assert st.last_jac_route()[0] == "fused_rt" and stt.last_jac_route()[0] == "generic"
    e = jr.rel_frobenius(J, Jt)
    print("JACRT class surface: J against the twin %.3e" % e.max())
    assert e.max() <= F32_BOUND
    F, Ft = em.fisher(pars, 2.0), twin.fisher(pars, 2.0)
    assert st.last_jac_route()[0] == "fused_rt" and set(stt.last_jac_route()[1]) == {"generic"}
    eF = jr.rel_frobenius(F, Ft)
    print("JACRT class surface: F against the twin %.3e" % eF.max())
    assert eF.max() <= F32_BOUND


def test_class_surface_unsupported_models_compute_as_before():
    """a model ending in a ReLU: compile_derivatives says "unsupported", raises nothing, and the model computes as before"""
    emulator, synth, eng = pkg("emulator"), pkg("synth"), pkg("engine")
    data = synth.make_dataset(n_train=600, n_val=40, n_test=40, seed=3)
    eng.set_random_seed(3)
    em = emulator.DirectEmulator(hidden_dims=[32], activation_func="relu", **data)
    em.emulator.layers[-1].activation = "relu"
    pars = em.par_test[:5]
    J0 = em.jacobian(pars)
    st = em._diff_stack(pars)[1]
    assert st.act[-1] == 1 and st.last_jac_route()[0] == "generic"
    assert em.compile_derivatives() == "unsupported"
    J1 = em.jacobian(pars)
    assert em._diff_stack(pars)[1].last_jac_route()[0] == "generic" and np.array_equal(J0, J1)
