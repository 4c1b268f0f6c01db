"""GPU: the ln L variant of fused_fwd<ArchRT, Prec> instantiated at run time (csrc/jit.hip: kJitLnl) -- the
"fused_rt" route of forward-only ln L and of the ensemble and nested samplers, opt-in per handle (Stack.jit_loglike) --
on the small stacks of tests/lnlrt_cases.py: one to fifteen output tiles, partial and dead tiles, in_dim 1 and 15, smooth
activations beside the ln L epilogue, every row count at a wave's and a workgroup's edge.  Every handle here is this
module's own: the named handles of infer_support are shared with modules that expect "two_launch" of NB.

Bound of the route: lnl_ref.LNL_FWD_TOL (6e-7) against the float64 reduction of the device's own forward.  Measured on the
MI355X: see MEASURED below."""
import numpy as np
import pytest

import act_ref as ar
import ensemble_ref as er
import fit_ref as fr
import lnl_ref as lr
import lnlrt_cases as lc
import nested_ref as nr
import shape_cases as sc
from conftest import pkg
from infer_cases import SPREAD
from infer_support import POISON, same, ulp32

pytestmark = pytest.mark.gpu

# worst |lnl - ref| / |ref| over the calls of a case, (f32, f16, bf16), as test_parity printed it on the MI355X: the worst of
# all is 1.86e-7, 0.31 of the bound (K12's cases: 1.56e-7) -- these shapes sum fewer terms than the 451-bin cases the bound
# was sized on, NB as many
MEASURED = {"R0": (1.59e-7, 1.51e-7, 1.23e-7), "R1": (1.40e-7, 1.24e-7, 1.32e-7), "R2": (1.59e-7, 1.31e-7, 1.35e-7),
            "R3b": (1.27e-7, 1.20e-7, 1.36e-7), "R5": (1.24e-7, 1.30e-7, 1.24e-7), "T1": (1.33e-7, 1.23e-7, 1.40e-7),
            "T2": (1.33e-7, 1.28e-7, 1.86e-7), "NB": (1.30e-7, 1.38e-7, 1.18e-7)}


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
    """per case: the handle that asked (every precision; its forward kernel too) and a twin that never asks -- all
    compilations requested first, then waited for"""
    out = {}
    for name in lc.CASES:
        rec = lc.stack(name)
        out[name] = {"st": _handle(ctx, rec), "twin": _handle(ctx, rec), "rec": rec}
        for prec in lc.PRECS:
            out[name]["st"].jit_loglike(prec, 0)
            out[name]["st"].jit(prec, 0)
            out[name]["twin"].jit(prec, 0)
    for name, e in out.items():
        for prec in lc.PRECS:
            assert e["st"].jit_loglike(prec, -1) == "ready", (name, prec)
            assert e["st"].jit(prec, -1) == "ready" and e["twin"].jit(prec, -1) == "ready", (name, prec)
    return out


def _call(rt, name, prec, k, n, tin_on, tout_on, x):
    """the k-th call of a case: the record from the device's own y of a truth row, set on the handle -> (st, flags, d, w, y_dev)"""
    nat = pkg("_native")
    st, rec = rt[name]["st"], rt[name]["rec"]
    flags = _flags(nat, tin_on, tout_on)
    dims = rec["dims"]
    truth = (sc.rows(dims, 8, 900 + k) if tin_on else sc.rows_u(dims, 8, 900 + k)).astype(x.dtype)
    y_truth = st.forward(truth, prec, flags | nat.FWD_FORCE_JIT)[0]
    d, w = lc.record(name, y_truth, float(rec["tout"][0]) if tout_on else 1.0, k)
    st.set_likelihood(d, w)
    y_dev = st.forward(x, prec, flags | nat.FWD_FORCE_JIT)
    assert st.last_route()[0] == "fused_rt", (name, prec, st.last_route())
    return st, flags, d, w, y_dev


# ---- 1. parity
@pytest.mark.parametrize("prec", lc.PRECS)
@pytest.mark.parametrize("name", list(lc.CASES))
def test_parity(rt, name, prec):
    """ln L on route 3, counted once, against float64 -1/2 sum w (d - y_dev)^2 of the same handle's run-time forward, at
    lnl_ref.LNL_FWD_TOL, for every n of lnlrt_cases.ROWS with the transforms alternating; scattered zero weights, a dead
    run inside a tile and (R1) a whole dead tile"""
    worst = 0.0
    for k, (n, tin_on, tout_on, x) in enumerate(lc.calls(name)):
        st, flags, d, w, y_dev = _call(rt, name, prec, k, n, tin_on, tout_on, x)
        tag = "%s %s n=%d %s flags=%d" % (name, prec, n, x.dtype.name, flags)
        c0 = st.last_lnl_route()[1].get("fused_rt", 0)
        lnl = st.loglike_fwd(x, prec, flags)
        last, counts = st.last_lnl_route()
        assert last == "fused_rt" and counts["fused_rt"] == c0 + 1, (tag, last, counts)
        assert lnl.shape == (n,) and lnl.dtype == np.float32 and np.all(np.isfinite(lnl)) and np.all(lnl < 0), tag
        err = lr.rel_err(lnl, lr.lnl64(y_dev, d, w))
        worst = max(worst, float(err.max()))
        print("LNLRT %s: worst %.3e (bound %.1e)" % (tag, err.max(), lr.LNL_FWD_TOL))
        assert err.max() <= lr.LNL_FWD_TOL, (tag, err.max(), int(err.argmax()))
    st.set_likelihood(None, None)
    print("LNLRT %s %s: worst of the calls %.3e" % (name, prec, worst))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_mutations_exceed_the_bound_on_the_device(rt, name):
    """the catalogue applied to the float64 reduction of y_dev moves some row by more than 4x the bound, at 33 and 257 rows"""
    for k, (n, tin_on, tout_on, x) in enumerate(lc.calls(name)):
        if n not in (33, 257):
            continue
        prec = lc.PRECS[k % 3]
        st, flags, d, w, y_dev = _call(rt, name, prec, k, n, tin_on, tout_on, x)
        lnl = st.loglike_fwd(x, prec, flags)
        mean = rt[name]["rec"]["tout"][1] if tout_on else np.ones(y_dev.shape[1])
        for mut, f in lc.MUTATIONS.items():
            e = float(lr.rel_err(lnl, f(y_dev.astype(np.float64), d, w, mean)).max())
            assert e > 4 * lr.LNL_FWD_TOL, (name, prec, n, mut, e)
    rt[name]["st"].set_likelihood(None, None)


@pytest.mark.parametrize("name", [n for n in lc.CASES if n != "R2"])
def test_zero_weight_bins_and_guard_rows(ctx, rt, name):
    """inf in d at three w == 0 bins: finite, the same bits; the _dev form into a buffer poisoned for 64 rows past n: the
    poison stays, the rows equal the host form's.  (R2 has three bins, all live.)"""
    calls = list(lc.calls(name))
    for prec, k in (("f16", 6), ("f32", 3)):   # 129 rows, 33 rows
        n, tin_on, tout_on, x = calls[k]
        x = np.ascontiguousarray(x, np.float32)
        st, flags, d, w, _ = _call(rt, name, prec, k, n, tin_on, tout_on, x)
        zeros = np.flatnonzero(w == 0)
        pick = [int(zeros[0]), int(zeros[len(zeros) // 2]), int(zeros[-1])]
        base = st.loglike_fwd(x, prec, flags)
        d2 = d.copy()
        d2[pick] = np.inf
        with np.errstate(invalid="ignore"):
            st.set_likelihood(d2, w)
        got = st.loglike_fwd(x, prec, flags)
        assert st.last_lnl_route()[0] == "fused_rt" and np.all(np.isfinite(got)) and same(got, base), (name, prec)
        st.set_likelihood(d, w)
        din, g = x.shape[1], 64
        dx, dl = ctx.malloc(x.nbytes), ctx.malloc((n + g) * 4)
        try:
            ctx.h2d(dx, x)
            ctx.memset(dl, 0x7F, (n + g) * 4)
            st.loglike_fwd_dev(dx, din, n, dl, None, 0, prec, flags)
            ctx.sync()
            out = np.empty(n + g, np.float32)
            ctx.d2h(out, dl)
        finally:
            ctx.free(dx)
            ctx.free(dl)
        assert st.last_lnl_route()[0] == "fused_rt"
        assert np.all(out[n:].view(np.uint32) == POISON) and same(out[:n], base), (name, prec)
    st.set_likelihood(None, None)


# ---- 2. data layouts
def test_many_spectra_and_the_two_forms(ctx, rt):
    nat = pkg("_native")
    for name, prec in (("T1", "f16"), ("NB", "f32"), ("R5", "bf16")):
        st, rec = rt[name]["st"], rt[name]["rec"]
        dims = rec["dims"]
        din = dims[0]
        tin_on = sc.has_tin(dims)
        # (V21_FWD_NO_SMALL: the two-launch call's forward takes the run-time kernel too, so both routes reduce the same y)
        flags = _flags(nat, tin_on, True) | nat.FWD_NO_SMALL
        rows = lambda n, seed: (sc.rows(dims, n, seed) if tin_on else sc.rows_u(dims, n, seed)).astype(np.float32)
        yt = st.forward(rows(8, 77), prec, flags | nat.FWD_FORCE_JIT)
        recs = [lc.record(name, yt[m], float(rec["tout"][0]), 5) for m in range(3)]
        w = recs[0][1]
        data = np.stack([r[0] + np.float32(m) for m, r in enumerate(recs)])
        for n, route in ((384, "fused_rt"), (390, "two_launch")):
            R = n // 3
            x = rows(n, 60 + n)
            st.set_likelihood(data[0], w)
            got = st.loglike_fwd(x, prec, flags, data=data)
            assert st.last_lnl_route()[0] == route and got.shape == (n,), (name, n, st.last_lnl_route())
            for m in range(3):
                st.set_likelihood(data[m], w)
                one = st.loglike_fwd(x[m * R:(m + 1) * R], prec, flags)
                assert st.last_lnl_route()[0] == "fused_rt"
                err = lr.rel_err(got[m * R:(m + 1) * R], one.astype(np.float64)).max()
                assert err <= lr.LNL_FWD_TOL, (name, n, m, err)
                if route == "fused_rt":
                    assert same(got[m * R:(m + 1) * R], one), (name, n, m)
        # the host form at 8,193 rows (two chunks) equals the _dev form (rows at a pitch of in_dim + 3) bit for bit
        n = 8193
        x = rows(n, 21)
        st.set_likelihood(data[1], w)
        c0 = st.last_lnl_route()[1]["fused_rt"]
        host = st.loglike_fwd(x, prec, flags)
        assert st.last_lnl_route()[0] == "fused_rt" and st.last_lnl_route()[1]["fused_rt"] == c0 + 1   # once, whatever its chunks
        xp = np.full((n, din + 3), np.nan, np.float32)
        xp[:, :din] = x
        dx, dl = ctx.malloc(xp.nbytes), ctx.malloc(n * 4)
        try:
            ctx.h2d(dx, xp)
            st.loglike_fwd_dev(dx, din + 3, n, dl, None, 0, prec, flags)
            ctx.sync()
            dev = np.empty(n, np.float32)
            ctx.d2h(dev, dl)
        finally:
            ctx.free(dx)
            ctx.free(dl)
        assert st.last_lnl_route()[0] == "fused_rt"
        assert np.all(np.isfinite(host)) and same(host, dev), (name, prec, np.flatnonzero(host != dev)[:5])
        st.set_likelihood(None, None)


# ---- 3. opt-in
def test_opt_in_per_handle(ctx, rt):
    nat = pkg("_native")
    for name, prec in (("NB", "f16"), ("T2", "f32"), ("R0", "bf16")):
        st, twin, rec = rt[name]["st"], rt[name]["twin"], rt[name]["rec"]
        dims = rec["dims"]
        tin_on = sc.has_tin(dims)
        # (V21_FWD_NO_SMALL: the two-launch call's forward takes the run-time kernel too, so both routes reduce the same y)
        flags = _flags(nat, tin_on, True) | nat.FWD_NO_SMALL
        x = (sc.rows(dims, 257, 5) if tin_on else sc.rows_u(dims, 257, 5)).astype(np.float32)
        d, w = lc.record(name, st.forward(x[:8], prec, flags | nat.FWD_FORCE_JIT)[3], float(rec["tout"][0]), 4)
        fresh = _handle(ctx, rec)
        fresh.jit(prec, -1)
        for s in (st, twin, fresh):
            s.set_likelihood(d, w)
        jac = st.last_jac_route()
        a = fresh.loglike_fwd(x, prec, flags)
        assert fresh.last_lnl_route()[0] == "two_launch" and twin.loglike_fwd(x, prec, flags) is not None
        assert twin.last_lnl_route()[0] == "two_launch" and set(twin.last_lnl_route()[1]) == {"two_launch"}
        assert fresh.jit_loglike(prec, -1) == "ready"
        b = fresh.loglike_fwd(x, prec, flags)
        assert fresh.last_lnl_route() == ("fused_rt", {"two_launch": 1, "fused_rt": 1})
        err = float(lr.rel_err(b, a.astype(np.float64)).max())
        print("LNLRT opt-in %s %s: fused_rt against two_launch %.3e (bound %.1e)" % (name, prec, err, 2 * lr.LNL_FWD_TOL))
        assert err <= 2 * lr.LNL_FWD_TOL, (name, prec, err)
        assert same(b, st.loglike_fwd(x, prec, flags)) and st.last_jac_route() == jac
        # forced flags keep their meaning: two-launch, V21_FWD_FORCE_JIT with the run-time forward inside
        for f in (nat.FWD_FORCE_JIT, nat.FWD_FORCE_GENERIC):
            c = st.loglike_fwd(x, prec, flags | f)
            assert st.last_lnl_route()[0] == "two_launch" and np.all(np.isfinite(c))
        assert same(st.loglike_fwd(x, prec, flags | nat.FWD_FORCE_JIT), a)
        # a nuisance record (K = 3) keeps the handle on two-launch after asking (R0: 20 bins, enough live ones)
        fresh.set_nuisance(sc.basis(dims[-1], 3))
        m = fresh.loglike_fwd(x, prec, flags)
        assert fresh.last_lnl_route()[0] == "two_launch" and np.all(np.isfinite(m))
        fresh.set_nuisance(None)
        assert same(fresh.loglike_fwd(x, prec, flags), b) and fresh.last_lnl_route()[0] == "fused_rt"
        for s in (st, twin, fresh):
            s.set_likelihood(None, None)


# ---- 4. refusals and the spilling stack
def test_refusals_leave_the_handle_usable(ctx):
    nat = pkg("_native")
    for key, (dims, act, why) in lc.REFUSALS.items():
        if key == "too_wide":
            continue   # (no forward of that width to compare)
        rec = sc.make_stack(dims, act)
        st = _handle(ctx, rec)
        x = sc.rows_u(dims, 33, 1).astype(np.float32)
        st.set_likelihood(sc.data_for(rec, 3)[0], sc.weights(dims[-1], 3))
        a = st.loglike_fwd(x, "f32", nat.FWD_OUT_TRANSFORM)
        for _ in range(2):
            with pytest.raises(nat.EngineError, match=r"error -3.*no fused ln L kernel for this stack.*" + why):
                st.jit_loglike("f32")
        b = st.loglike_fwd(x, "f32", nat.FWD_OUT_TRANSFORM)
        assert st.last_lnl_route() == ("two_launch", {"two_launch": 2}) and same(a, b), key
        st.set_likelihood(None, None)


def test_a_kernel_with_scratch_leaves_the_handle_on_two_launch(ctx):
    """9-500-512-33 in f16 compiles, spills, and is refused when its code object is loaded -- when the first call after
    jit_loglike decides its route: that call and every later one record "two_launch" and compute what a handle that never
    asked computes, with no error, and nothing is launched that needs scratch memory"""
    nat = pkg("_native")
    rec = sc.make_stack(*lc.SPILLS)
    st, twin = _handle(ctx, rec), _handle(ctx, rec)
    assert st.jit_loglike("f16", -1) == "ready"   # compiled: the registers are counted when it is loaded
    x = sc.rows_u(rec["dims"], 257, 7).astype(np.float32)
    for s in (st, twin):
        s.set_likelihood(sc.data_for(rec, 3)[0], sc.weights(rec["dims"][-1], 3))
    for _ in range(2):
        a = st.loglike_fwd(x, "f16", nat.FWD_OUT_TRANSFORM)
        assert st.last_lnl_route()[0] == "two_launch"
    assert set(st.last_lnl_route()[1]) == {"two_launch"}
    assert same(a, twin.loglike_fwd(x, "f16", nat.FWD_OUT_TRANSFORM))
    with pytest.raises(nat.EngineError, match="register budget"):
        st.jit_loglike("f16")
    assert same(a, st.loglike_fwd(x, "f16", nat.FWD_OUT_TRANSFORM)) and st.last_lnl_route()[0] == "two_launch"
    for s in (st, twin):
        s.set_likelihood(None, None)


# ---- 5. the samplers on route 3
def _problem(rt, name, m=2, seed=8):
    """truths in u, m spectra = y(truth) + noise of 0.02 OUT_STD, weights with a dead head; the record set to spectrum 0"""
    e = rt[name]
    if "prob" not in e:
        rec = e["rec"]
        din, dout = rec["dims"][0], rec["dims"][-1]
        rng = np.random.default_rng(4000 + seed)
        tu = rng.uniform(-0.6, 0.6, size=(m, din))
        sig = 0.02 * sc.OUT_STD
        data = (lc.forward64(rec, tu, False, True) + rng.normal(size=(m, dout)) * sig).astype(np.float32)
        w = np.full(dout, 1.0 / sig ** 2, np.float32)
        w[:dout // 10] = 0.0
        e["prob"] = (tu, data, w)
    for s in (e["st"], e["twin"]):
        s.set_likelihood(e["prob"][1][0], e["prob"][2])
    return e["st"], e["twin"], e["rec"], e["prob"]


def _starts_u(tu, n, seed, scale=SPREAD):
    return np.clip(tu[None, :] + scale * np.random.default_rng(seed).normal(size=(n, tu.size)), -0.999, 0.999)


def _raw(rec, u):
    tin = rec["tin"]
    return fr.untransform(u, tin[0], tin[2], tin[3])


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("name", ["T1", "NB"])
def test_one_ensemble_sweep_against_the_rebuild(rt, name, prec):
    """tests/test_ensemble_gpu.py's test_one_sweep_against_reference on route 3: partners and proposals bit-equal, log alpha
    within one float32 ulp of each of its two ln L, the decisions equal wherever ln U is further than that from log
    alpha (at most 0.5 % excused), lnl_last = loglike_fwd of the same u, bit for bit"""
    nat = pkg("_native")
    st, twin, rec, (tu, data, w) = _problem(rt, name)
    d = rec["dims"][0]
    flags = _flags(nat, True, True)
    a = 2.0
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, nat.FWD_OUT_TRANSFORM)
    for W, E in ((16, 33), (18, 30)):
        n, H = W * E, W // 2
        seed, chain0, step0 = 100 + W, 11, 40
        x0 = _raw(rec, _starts_u(tu[0], n, W))
        c0 = st.last_lnl_route()[1].get("fused_rt", 0)
        u0 = st.sample_ensemble(x0, W, prec, flags, n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
        r = st.sample_ensemble(x0, W, prec, flags, n_steps=1, n_warmup=0, a=a, seed=seed, chain0=chain0, step0=step0, diagnostics=True)
        assert st.last_lnl_route()[0] == "fused_rt" and st.last_lnl_route()[1]["fused_rt"] == c0 + 2   # once per call
        e, h, _ = er.layout(n, W)
        z, k, logu = er.draws(seed, chain0 + np.arange(n), step0, a, H)
        acc_dev = r["accept_rate"] > 0.5
        u, lnl = u0.copy(), lnl_of(u0).astype(np.float64)
        assert st.last_lnl_route()[0] == "fused_rt"
        excused_all = 0
        for hh in (0, 1):
            idx = np.flatnonzero(h == hh)
            pr = e[idx] * W + (1 - hh) * H + k[idx]
            tag = "%s %s W=%d set %d" % (name, prec, W, hh)
            assert np.array_equal(r["last_partner"][idx], pr - e[idx] * W), tag
            y = er.stretch(u[idx], u[pr], z[idx])
            assert same(y.astype(np.float32), r["last_prop_u"][idx]), tag
            inside = np.all(np.abs(y) <= 1.0, axis=1)
            lnl_y = lnl_of(y).astype(np.float64)
            la = np.where(inside, (d - 1) * np.log(z[idx]) + (lnl_y - lnl[idx]), -np.inf)
            bound = ulp32(lnl[idx]) + ulp32(lnl_y)
            la_dev = r["last_log_alpha"][idx]
            assert np.array_equal(np.isneginf(la), np.isneginf(la_dev)), tag
            fin = np.isfinite(la)
            assert np.all(np.abs(la_dev[fin] - la[fin]) <= bound[fin]), tag
            excused = np.abs(logu[idx] - la) <= bound
            excused_all += int(excused.sum())
            assert np.array_equal((logu[idx] < la)[~excused], acc_dev[idx][~excused]), tag
            # (a missing barrier shows only where set 0 moved, a wrong ln L only where it decides)
            by_lnl = np.mean((logu[idx] < (d - 1) * np.log(z[idx])) != acc_dev[idx])
            assert 0.1 < acc_dev[idx].mean() < 0.9 and by_lnl > 0.05, (tag, acc_dev[idx].mean(), by_lnl)
            u[idx] = np.where(acc_dev[idx][:, None], y, u[idx])
            lnl[idx] = np.where(acc_dev[idx], lnl_y, lnl[idx])
        print("LNLRT ensemble %s %s W=%d: accepted %.3f, excused %d of %d" % (name, prec, W, acc_dev.mean(), excused_all, n))
        assert excused_all <= 0.005 * n
        np.testing.assert_allclose(r["x_last"], _raw(rec, u), rtol=1e-12)
        assert same(r["lnl_last"], lnl_of(u)), (name, prec, W)
    for s in (st, twin):
        s.set_likelihood(None, None)


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("name", ["T1", "NB"])
def test_two_nested_iterations_against_the_rebuild(rt, name, prec):
    """tests/test_nested_gpu.py's test_iterations_against_rebuild on route 3: every recorded value and decision bit-equal to
    nested_ref's rebuild from the device's own ln L"""
    nat = pkg("_native")
    st, twin, rec, (tu, data, w) = _problem(rt, name)
    d = rec["dims"][0]
    flags = nat.FWD_OUT_TRANSFORM
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, flags)
    for N, runs in ((16, 33), (18, 30)):
        n, k = N * runs, N // 2
        opts = dict(n_iter=2, n_repeats=2, seed=100 + N, chain0=11 * N, iter0=40)
        u0 = _starts_u(tu[0], n, N).reshape(runs, N, d)
        u0[:, 5] = u0[:, 2]
        u0[:, 9] = u0[:, 2]
        u0 = u0.reshape(n, d)
        c0 = st.last_lnl_route()[1].get("fused_rt", 0)
        r0 = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, n_iter=0)
        r = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, diagnostics=True, **opts)
        assert st.last_lnl_route()[0] == "fused_rt" and st.last_lnl_route()[1]["fused_rt"] == c0 + 2
        ref = nr.nested_ref(lnl_of, u0, N, lnl0=r0["live_lnl"], **opts)
        tag = "%s %s N=%d" % (name, prec, N)
        print("LNLRT nested %s: accepted %.3f" % (tag, r["accept_rate"].mean()))
        assert same(r["dead_lnl"], ref["dead_lnl"].astype(np.float32)), tag
        assert same(r["dead_u"], ref["dead_u"].astype(np.float64)), tag
        assert same(r["lstar"], ref["lstar"].astype(np.float32)) and same(r["lstar"], r["dead_lnl"][:, :, -1]), tag
        assert np.array_equal(r["last_partner"], ref["last_partner"]), tag
        assert same(r["last_prop_u"], ref["last_prop_u"]), tag
        assert np.array_equal(r["accept_rate"], ref["accept_rate"]), tag
        assert same(r["live_u"], ref["live_u"].astype(np.float64)), tag
        assert same(r["live_lnl"], ref["live_lnl"].astype(np.float32)), tag
        assert 0.2 < r["accept_rate"].mean() < 0.8, tag   # (a wrong decision shows only where ln L decides and a fair share moves)
    for s in (st, twin):
        s.set_likelihood(None, None)


@pytest.mark.parametrize("name", ["T1", "NB"])
def test_sampler_routes_first_evaluations_and_splitting(rt, name):
    """2 spectra x one 256-walker ensemble / 256-point run: 128 proposals per spectrum, the uniform layout, route 3 counted
    once per call.  n_steps = 0 / n_iter = 0: the first evaluations' ln L against the same call on the handle that never
    asked, within the bound.  One call over both spectra equals the two per-spectrum calls (chain0 moved on) bit for bit;
    four sweeps equal two and two."""
    nat = pkg("_native")
    st, twin, rec, (tu, data, w) = _problem(rt, name)
    # (V21_FWD_NO_SMALL: the two-launch evaluations' forward is the run-time kernel too, as on route 3)
    flags = _flags(nat, True, True) | nat.FWD_NO_SMALL
    nflags = nat.FWD_OUT_TRANSFORM | nat.FWD_NO_SMALL
    for prec in ("f32", "f16"):
        u = np.vstack([_starts_u(tu[m], 256, 9 + m, 0.01) for m in range(2)])
        x = _raw(rec, u)
        cnt = lambda s: dict(s.last_lnl_route()[1])
        c0 = cnt(st)
        a = st.sample_ensemble(x, 256, prec, flags, data=data[:2], n_steps=0, n_warmup=0)
        assert st.last_lnl_route()[0] == "fused_rt" and cnt(st).get("fused_rt", 0) == c0.get("fused_rt", 0) + 1
        assert cnt(st).get("two_launch", 0) == c0.get("two_launch", 0)
        b = twin.sample_ensemble(x, 256, prec, flags, data=data[:2], n_steps=0, n_warmup=0)
        assert twin.last_lnl_route()[0] == "two_launch" and "fused_rt" not in cnt(twin)
        err = float(lr.rel_err(a["lnl_last"], b["lnl_last"].astype(np.float64)).max())
        na = st.sample_nested(u, n_live=256, precision=prec, flags=nflags, data=data[:2], n_iter=0)
        assert st.last_lnl_route()[0] == "fused_rt"
        nb = twin.sample_nested(u, n_live=256, precision=prec, flags=nflags, data=data[:2], n_iter=0)
        assert twin.last_lnl_route()[0] == "two_launch"
        errn = float(lr.rel_err(na["live_lnl"], nb["live_lnl"].astype(np.float64)).max())
        print("LNLRT samplers %s %s: first evaluations, fused_rt against two_launch %.3e / %.3e (bound %.1e)"
              % (name, prec, err, errn, lr.LNL_FWD_TOL))
        assert err <= lr.LNL_FWD_TOL and errn <= lr.LNL_FWD_TOL, (name, prec, err, errn)
        # splitting and continuation, ensemble
        kw = dict(n_walkers=256, precision=prec, flags=flags, n_warmup=0, seed=5)
        four = st.sample_ensemble(x, data=data[:2], n_steps=4, **kw)
        assert st.last_lnl_route()[0] == "fused_rt"
        first = st.sample_ensemble(x, data=data[:2], n_steps=2, **kw)
        second = st.sample_ensemble(first["x_last"], data=data[:2], n_steps=2, step0=2, **kw)
        assert same(four["samples"], np.concatenate([first["samples"], second["samples"]], axis=1))
        assert same(four["x_last"], second["x_last"]) and same(four["lnl_last"], second["lnl_last"]) and not same(four["x_last"], x)
        for half in (0, 1):
            rows = slice(256 * half, 256 * (half + 1))
            part = st.sample_ensemble(x[rows], data=data[half:half + 1], n_steps=4, chain0=256 * half, **kw)
            assert st.last_lnl_route()[0] == "fused_rt"
            for key in ("x_last", "lnl_last", "accept_rate", "mean_u", "cov_u", "samples"):
                assert same(part[key], four[key][rows]), (name, prec, half, key)
        # ... nested
        kn = dict(n_live=256, precision=prec, flags=nflags, n_repeats=2, seed=5)
        both = st.sample_nested(u, data=data[:2], n_iter=2, **kn)
        assert st.last_lnl_route()[0] == "fused_rt"
        one = st.sample_nested(u, data=data[:2], n_iter=1, **kn)
        two = st.sample_nested(one["live_u"], data=data[:2], n_iter=1, iter0=1, **kn)
        assert same(both["dead_lnl"], np.concatenate([one["dead_lnl"], two["dead_lnl"]])) and same(both["live_u"], two["live_u"])
        for half in (0, 1):
            rows = slice(256 * half, 256 * (half + 1))
            part = st.sample_nested(u[rows], data=data[half:half + 1], n_iter=2, chain0=256 * half, **kn)
            assert same(part["live_u"], both["live_u"][rows]) and same(part["live_lnl"], both["live_lnl"][rows]), (name, prec, half)
            assert same(part["dead_lnl"], both["dead_lnl"][:, half:half + 1]), (name, prec, half)
    for s in (st, twin):
        s.set_likelihood(None, None)


# ---- 6. the class surface
@pytest.fixture(scope="module")
def emulators():
    emulator, synth, eng = pkg("emulator"), pkg("synth"), pkg("engine")
    data = synth.make_dataset(n_train=600, n_val=40, n_test=40, seed=ar.SEEDS["T3"])
    out = []
    for _ in range(2):
        eng.set_random_seed(ar.SEEDS["T3"])
        out.append(emulator.DirectEmulator(hidden_dims=[64, 128], activation_func="tanh", **data))
    return out


def test_class_surface_compile_likelihood(emulators):
    em, twin = emulators
    for a, b in zip(em.emulator.layers, twin.emulator.layers):
        assert np.array_equal(a.kernel, b.kernel)
    assert em.compile_likelihood() == "ready"
    pars = em.par_test[:33]
    truth = np.asarray(em.predict(pars[0]), np.float64)
    sigma = 20.0
    data = (truth + sigma * np.random.default_rng(4).normal(size=truth.shape)).astype(np.float32)
    st, stt = em._diff_stack(pars)[1], twin._diff_stack(pars)[1]
    fwd = em.log_likelihood(pars, data, sigma, forward_only=True)
    assert st.last_lnl_route()[0] == "fused_rt"
    default = em.log_likelihood(pars, data, sigma)
    e = float(lr.rel_err(fwd, np.asarray(default, np.float64)).max())
    print("LNLRT class surface: forward_only on fused_rt against the default call %.3e (bound %.1e)" % (e, 2 * lr.LNL_FWD_TOL))
    assert e <= 2 * lr.LNL_FWD_TOL, e
    tw = twin.log_likelihood(pars, data, sigma, forward_only=True)
    assert stt.last_lnl_route()[0] == "two_launch" and float(lr.rel_err(fwd, tw.astype(np.float64)).max()) <= 2 * lr.LNL_FWD_TOL
    lp = em.log_posterior(data, sigma)
    assert same(lp(pars).astype(np.float32), fwd) and st.last_lnl_route()[0] == "fused_rt"
    # (the class hands the spectrum over as a data matrix: 4 ensembles of 64 walkers are 128 proposals per half-move, a
    #  run of 256 live points 128 per iteration -- the layouts that are uniform per workgroup, as on a compiled stack)
    r = em.sample_ensemble(data, sigma, n_walkers=64, n_ensembles=4, n_steps=4, n_warmup=2, thin=1, p0=pars[0])
    assert st.last_lnl_route()[0] == "fused_rt" and np.all(np.isfinite(r.params))
    r = em.nested_sample(data, sigma, n_live=256, max_iter=8, seed=2)
    assert st.last_lnl_route()[0] == "fused_rt" and np.isfinite(r.log_evidence)
    twin.nested_sample(data, sigma, n_live=256, max_iter=8, seed=2)
    assert set(stt.last_lnl_route()[1]) == {"two_launch"}


def test_class_surface_variational_head_is_unsupported():
    """a model with a GaussianLatent layer: compile_likelihood says "unsupported", raises nothing, and the model computes as before"""
    emulator, synth, eng = pkg("emulator"), pkg("synth"), pkg("engine")
    data = synth.make_dataset(n_train=600, n_val=40, n_test=40, seed=3)
    eng.set_random_seed(3)
    em = emulator.DirectEmulator(hidden_dims=[32], activation_func="relu", **data)
    em.emulator = eng.Sequential([eng.Input(shape=(7,)), eng.Dense(32, activation="relu"), eng.GaussianLatent(4), eng.Dense(451)], name="emulator")
    em.emulator.precision = "f32"
    pars = em.par_test[:5]
    spectrum = np.asarray(em.predict(pars[0]), np.float32) + np.float32(1.0)
    a = em.log_likelihood(pars, spectrum, 5.0, forward_only=True)
    st = em._diff_stack(pars)[1]
    assert st.last_lnl_route()[0] == "two_launch"
    assert em.compile_likelihood() == "unsupported"
    b = em.log_likelihood(pars, spectrum, 5.0, forward_only=True)
    assert em._diff_stack(pars)[1].last_lnl_route()[0] == "two_launch" and same(a, b)
