"""Forward-only log-likelihood on the GPU (include/v21.h: v21_mlp_loglike_fwd[_dev]): the ln L variant of
fused_fwd<Arch, Prec> on the stacks of archs.h against the float64 reduction of the device's own forward (whose bits the
variant reproduces by construction), the mutation catalogue of tests/lnl_ref.py, the select on zero-weight bins, data
matrices, guard regions, host against device entry, the two-launch route on the shapes of tests/shape_cases.py, and the
class surface on the shipped weights.

Bound of the fused route: lnl_ref.LNL_FWD_TOL.  Measured on the MI355X over every case of test_fused_parity: worst relative
error 1.56e-7 (S1 bf16); smallest effect of a mutation 9.0e-4 (drop_bin at 33 rows)."""
import numpy as np
import pytest

import jacobian_ref as jr
import lnl_ref as lr
import marg_ref as mr
import shape_cases as sc
from conftest import pkg
from infer_support import POISON, device_stack, ready, same

pytestmark = pytest.mark.gpu

STATE = -4


def case_of(ctx, name, prec, k, n):
    """the k-th call of a stack: flags alternating as in test_fused_parity_and_primal_bit_identity, rows, the record built
    from the device's own y of a truth row, and y_dev of the rows"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout = lr.stack_of(ctx, name)
    tin_on = dims[0] == 7 and k % 2 == 0
    dtype = np.float64 if k % 4 < 2 else np.float32
    flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | (nat.FWD_OUT_TRANSFORM if k % 3 else 0)
    x = lr.rows_for(dims, n, 10 + k, dtype, tin, tin_on)
    truth = lr.rows_for(dims, 8, 900 + k, dtype, tin, tin_on)
    y_truth = st.forward(truth, prec, flags | nat.FWD_NO_SMALL)[0]
    std = float(tout[0]) if flags & nat.FWD_OUT_TRANSFORM else 1.0
    d, w = lr.record(y_truth, std, k, zero_tail=(k == 4))
    y_dev = st.forward(x, prec, flags | nat.FWD_NO_SMALL)
    assert st.last_route()[0] == "fused"
    mean = tout[1] if flags & nat.FWD_OUT_TRANSFORM else np.ones(dims[-1])
    return st, flags, x, d, w, y_dev, mean


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_fused_parity(ctx, name, prec):
    """S1 = D1, S2 = DE of helpers.STACKS.  lnl against the float64 reduction of the device's own forward at LNL_FWD_TOL"""
    worst = 0.0
    for k, n in enumerate(lr.ROWS):
        st, flags, x, d, w, y_dev, _ = case_of(ctx, name, prec, k, n)
        st.set_likelihood(d, w)
        tag = "%s %s n=%d %s flags=%d" % (name, prec, n, x.dtype.name, flags)
        lnl = st.loglike_fwd(x, prec, flags)
        assert st.last_lnl_route()[0] == "fused", tag
        assert lnl.shape == (n,) and lnl.dtype == np.float32 and np.all(np.isfinite(lnl)) and np.all(lnl < 0), tag
        err = lr.rel_err(lnl, lr.lnl64(y_dev, d, w))
        worst = max(worst, float(err.max()))
        print("LNLFWD %s: worst %.3e (bound %.1e)" % (tag, err.max(), lr.LNL_FWD_TOL))
        assert err.max() <= lr.LNL_FWD_TOL, (tag, err.max(), int(err.argmax()))
    st.set_likelihood(None, None)
    print("LNLFWD %s %s: worst of the rows %.3e" % (name, prec, worst))


@pytest.mark.parametrize("n", [33, 4099])
def test_mutations_exceed_the_bound(ctx, n):
    """each way the in-kernel reduction can go wrong, applied to the float64 reduction of y_dev, moves some row by more
    than 4x the bound -- and the kernel itself stays within the bound of the unmutated reduction"""
    smallest = {}
    for name, prec, k in (("S1", "f16", 1), ("S4", "f32", 2), ("S3", "bf16", 4)):
        st, flags, x, d, w, y_dev, mean = case_of(ctx, name, prec, k, n)
        st.set_likelihood(d, w)
        lnl = st.loglike_fwd(x, prec, flags)
        st.set_likelihood(None, None)
        assert lr.rel_err(lnl, lr.lnl64(y_dev, d, w)).max() <= lr.LNL_FWD_TOL
        for mut, f in lr.MUTATIONS.items():
            e = float(lr.rel_err(lnl, f(y_dev.astype(np.float64), d, w, mean)).max())
            smallest[mut] = min(smallest.get(mut, np.inf), e)
            assert e > 4 * lr.LNL_FWD_TOL, (name, prec, n, mut, e)
    print("LNLFWD mutations n=%d: smallest effect %s" % (n, {m: "%.2e" % e for m, e in smallest.items()}))


def test_zero_weight_bins_are_dropped_by_select(ctx):
    """inf in d at three w == 0 bins (a scattered one, one of the run 32 .. 95, and bin 450 of the last tile): finite, same bits"""
    for name, prec, k in (("S1", "f16", 4), ("S4", "f32", 4), ("S2", "bf16", 4)):
        st, flags, x, d, w, _, _ = case_of(ctx, name, prec, k, 129)
        zeros = np.flatnonzero(w == 0)
        pick = [int(zeros[0]), 64, 450]
        assert all(w[p] == 0 for p in pick)
        st.set_likelihood(d, w)
        base = st.loglike_fwd(x, prec, flags)
        d2 = d.copy()
        d2[pick] = np.inf
        with np.errstate(invalid="ignore"):
            st.set_likelihood(d2, w)
        got = st.loglike_fwd(x, prec, flags)
        st.set_likelihood(None, None)
        assert st.last_lnl_route()[0] == "fused" and np.all(np.isfinite(got)) and same(got, base), (name, prec)


def test_many_spectra(ctx):
    nat = pkg("_native")
    for name, prec in (("S1", "f16"), ("S4", "f32")):
        st, dims, act, Ws, bs, tin, tout = lr.stack_of(ctx, name)
        tin_on = dims[0] == 7
        # (V21_FWD_NO_SMALL: the two-launch call's forward takes the fused kernel too, so both routes reduce the same y)
        flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | nat.FWD_OUT_TRANSFORM | nat.FWD_NO_SMALL
        truth = lr.rows_for(dims, 8, 77, np.float32, tin, tin_on)
        yt = st.forward(truth, prec, flags)
        recs = [lr.record(yt[m], float(tout[0]), 5, False) for m in range(3)]
        w = recs[0][1]
        data = np.stack([np.roll(r[0], 0) + np.float32(m) for m, r in enumerate(recs)])
        for n, route in ((384, "fused"), (390, "two_launch")):
            R = n // 3
            x = lr.rows_for(dims, n, 60 + n, np.float32, tin, tin_on)
            st.set_likelihood(data[0], w)
            assert st.route_loglike_fwd(prec, n, 3, flags) == route
            got = st.loglike_fwd(x, prec, flags, data=data)
            assert st.last_lnl_route()[0] == route and got.shape == (n,), (name, n)
            for m in range(3):
                st.set_likelihood(data[m], w)
                one = st.loglike_fwd(x[m * R:(m + 1) * R], prec, flags)
                assert st.last_lnl_route()[0] == "fused"
                err = lr.rel_err(got[m * R:(m + 1) * R], one.astype(np.float64)).max()
                assert err <= lr.LNL_FWD_TOL, (name, n, m, err)
                if route == "fused":
                    assert same(got[m * R:(m + 1) * R], one), (name, n, m)
        st.set_likelihood(None, None)


def test_guard_region(ctx):
    """loglike_fwd_dev into a buffer poisoned for 64 rows past n: the poison stays, on both routes"""
    nat = pkg("_native")
    for name, prec in (("S1", "f16"), ("S4", "f32"), ("S3", "bf16"), ("NB", "f32")):
        st, dims, act, *_ = lr.stack_of(ctx, name)
        din, dout = dims[0], dims[-1]
        st.set_likelihood(np.zeros(dout, np.float32), np.ones(dout, np.float32))
        for n in (3, 33, 4099):
            x = lr.rows_for(dims, n, 3, np.float32, None, True)
            g = 64
            dx, dl = ctx.malloc(x.nbytes), ctx.malloc((n + g) * 4)
            try:
                ctx.h2d(dx, x)
                ctx.memset(dl, 0x7F, (n + g) * 4)
                st.loglike_fwd_dev(dx, din, n, dl, None, 0, prec, 0)
                ctx.sync()
                lnl = np.empty(n + g, np.float32)
                ctx.d2h(lnl, dl)
                assert np.all(lnl[n:].view(np.uint32) == POISON) and np.all(np.isfinite(lnl[:n])), (name, prec, n)
                assert st.last_lnl_route()[0] == ("two_launch" if name == "NB" else "fused")
                assert same(lnl[:n], st.loglike_fwd(x, prec, 0)), (name, prec, n)
            finally:
                ctx.free(dx)
                ctx.free(dl)
        st.set_likelihood(None, None)


def test_host_and_device_agree(ctx):
    """the host form at 8,193 rows (two chunks) equals the _dev form bit for bit; device rows at a pitch of in_dim + 3"""
    nat = pkg("_native")
    for name, prec in (("S1", "f16"), ("S4", "f32"), ("NB", "f16")):
        st, dims, act, Ws, bs, tin, tout = lr.stack_of(ctx, name)
        din, dout = dims[0], dims[-1]
        tin_on = din == 7
        flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | nat.FWD_OUT_TRANSFORM
        n = 8193
        ready(st, prec)
        x = lr.rows_for(dims, n, 21, np.float32, tin, tin_on)
        yt = st.forward(x[:8], prec, flags | nat.FWD_NO_SMALL)[0]
        st.set_likelihood(*lr.record(yt, float(tout[0]), 9))
        host = st.loglike_fwd(x, prec, flags)
        xp = np.full((n, din + 3), np.nan, np.float32)
        xp[:, :din] = x
        dx, dl = ctx.malloc(xp.nbytes), ctx.malloc(n * 4)
        try:
            ctx.h2d(dx, xp)
            jac_before = st.last_jac_route()
            st.loglike_fwd_dev(dx, din + 3, n, dl, None, 0, prec, flags)
            ctx.sync()
            dev = np.empty(n, np.float32)
            ctx.d2h(dev, dl)
        finally:
            ctx.free(dx)
            ctx.free(dl)
        st.set_likelihood(None, None)
        assert st.last_jac_route() == jac_before  # (these calls do not touch the Jacobian's route record)
        assert np.all(np.isfinite(host)) and same(host, dev), (name, prec, np.flatnonzero(host != dev)[:5])


def test_state_errors_and_empty_calls(ctx):
    nat = pkg("_native")
    st, dims, *_ = lr.stack_of(ctx, "S4")
    st.set_likelihood(None, None)
    x = lr.rows_for(dims, 3, 1, np.float32, None, True)
    with pytest.raises(nat.EngineError, match="v21 error %d" % STATE):
        st.loglike_fwd(x, "f32", 0)                            # no record set
    assert st.loglike_fwd(x[:0], "f32", 0).shape == (0,)       # n = 0: a no-op, whatever the state
    st.set_likelihood(np.zeros(dims[-1], np.float32), np.ones(dims[-1], np.float32))
    with pytest.raises(nat.EngineError):                        # n % n_data != 0 through the C ABI itself
        nat.check(st.lib.v21_mlp_loglike_fwd(st.h, x.ctypes.data, 0, 3, np.zeros((2, dims[-1]), np.float32).ctypes.data_as(nat._F), 2,
                                             np.empty(3, np.float32).ctypes.data_as(nat._F), 0, 0))
    assert np.all(np.isfinite(st.loglike_fwd(x, "f32", 0)))    # the handle stays usable
    st.set_likelihood(None, None)


# ---- the two-launch route
def test_two_launch_on_the_shape_table(ctx):
    """shape_cases i4o65, i5o130, i8o451, i5gauss, i8relu, i1o1 at shape_cases.ROWS, K = 0 and each of the case's modes.
    References on the device's own forward y widened to float64: jacobian_ref.loglike for K = 0 within 1e-5 of ln L (the
    bound of test_likelihood_mode_of_the_generic_kernel), marg_ref.profile_lnl for K > 0 within 1e-5 of the scale r^T W r
    + |b|^2 of the PROJECTED data the device reduces (the bound and scale of infer_support.check_reduction, used by
    test_marginalised_reductions).  Against the old
    loglike(grad=False) of the same stack (the generic Jacobian kernel's own f32 primal): within 2e-5 of ln L resp. of the
    scale -- the sum of the two routes' bounds.  Observed on the MI355X: K = 0 worst 1.08e-7 of ln L against the reference
    and 1.05e-6 against the old route; K > 0 worst 7.2e-8 and 5.8e-8 of the scale."""
    nat = pkg("_native")
    worst = {"ref0": 0.0, "old0": 0.0, "refK": 0.0, "oldK": 0.0}
    for name in ("i4o65", "i5o130", "i8o451", "i5gauss", "i8relu", "i1o1"):
        case = sc.BY_NAME[name]
        st, rec = device_stack(ctx, case.dims, case.act)
        flags = (nat.FWD_IN_TRANSFORM if rec["tin"] is not None else 0) | nat.FWD_OUT_TRANSFORM
        dout = case.dims[-1]
        for K in (0,) + tuple(case.modes):
            w = sc.weights(dout, 3, K)
            data = sc.data_for(rec, 3)[0]
            w64 = w.astype(np.float64)
            st.set_likelihood(data, w)
            A = sc.basis(dout, K) if K else None
            st.set_nuisance(A)
            for n in sc.ROWS:
                x = sc.rows(case.dims, n, 40 + n).astype(np.float32)
                tag = "%s K=%d n=%d" % (name, K, n)
                assert st.route_loglike_fwd("f32", n, 0, flags) == "two_launch", tag
                lnl = st.loglike_fwd(x, "f32", flags)
                assert st.last_lnl_route()[0] == "two_launch" and lnl.shape == (n,) and np.all(np.isfinite(lnl)), tag
                y = st.forward(x, "f32", flags).astype(np.float64)
                old = st.loglike(x, "f32", flags, grad=False).astype(np.float64)
                if K == 0:
                    ref = jr.loglike(y, np.zeros((n, 1, dout)), data, w64)[0]
                    np.testing.assert_allclose(lnl, ref, rtol=1e-5, atol=0, err_msg=tag)
                    np.testing.assert_allclose(lnl, old, rtol=2e-5, atol=0, err_msg=tag)
                    if np.all(ref != 0):
                        worst["ref0"] = max(worst["ref0"], float(np.max(np.abs(lnl - ref) / np.abs(ref))))
                        worst["old0"] = max(worst["old0"], float(np.max(np.abs(lnl - old) / np.abs(ref))))
                else:
                    ref = mr.profile_lnl(y, data, w64, A)[0]
                    scale = lr.marg_scale(y, data, w64, A)
                    er, eo = np.abs(lnl - ref) / scale, np.abs(lnl - old) / scale
                    assert er.max() <= 1e-5 and eo.max() <= 2e-5, (tag, er.max(), eo.max())
                    worst["refK"], worst["oldK"] = max(worst["refK"], float(er.max())), max(worst["oldK"], float(eo.max()))
            st.set_nuisance(None)
        st.set_likelihood(None, None)
    print("LNLFWD two-launch, worst: %s" % {k: "%.2e" % v for k, v in worst.items()})


def test_two_launch_on_named_stacks(ctx):
    """NB (outside archs.h) and VG (a Gauss layer), every precision, with and without a nuisance record, and an archs.h
    stack forced off its fused route by a nuisance record: within the bounds above of the reduction of the device's own y"""
    nat = pkg("_native")
    for name in ("NB", "VG", "S4"):
        st, dims, act, Ws, bs, tin, tout = lr.stack_of(ctx, name)
        tin_on = dims[0] == 7
        flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | nat.FWD_OUT_TRANSFORM
        for prec in ("f32", "f16", "bf16"):
            ready(st, prec)
            for n in (5, 4099):
                x = lr.rows_for(dims, n, 30 + n, np.float32, tin, tin_on)
                y = st.forward(x, prec, flags).astype(np.float64)
                d, w = lr.record(st.forward(x[:8], prec, flags)[1], float(tout[0]), 2)
                st.set_likelihood(d, w)
                for K in (0, 4):
                    if name == "S4" and K == 0:
                        continue
                    A = sc.basis(dims[-1], K) if K else None
                    st.set_nuisance(A)
                    lnl = st.loglike_fwd(x, prec, flags)
                    assert st.last_lnl_route()[0] == "two_launch", (name, prec, n, K)
                    w64 = w.astype(np.float64)
                    if K == 0:
                        np.testing.assert_allclose(lnl, lr.lnl64(y, d, w), rtol=1e-5, atol=0)
                    else:
                        ref = mr.profile_lnl(y, d, w64, A)[0]
                        scale = lr.marg_scale(y, d, w64, A)
                        assert np.max(np.abs(lnl - ref) / scale) <= 1e-5, (name, prec, n, K)
                st.set_nuisance(None)
        st.set_likelihood(None, None)


# ---- the class surface on the shipped weights
def test_class_surface(shipped):
    """the shipped autoencoder-based emulator (its predict chain is archs.h S3), float32"""
    emu, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    em = emu.AutoEncoderEmulator(**synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11))
    em.load_model()
    st = em._diff_stack(np.zeros((1, 7)))[1]
    u = np.random.default_rng(3).uniform(-0.9, 0.9, size=(256, 7))
    theta = pp.par_untransform(u, em.par_train)
    y_all = np.asarray(em.predict(theta), np.float64)
    truth = y_all[:3]
    rng = np.random.default_rng(4)
    sigma = 20.0
    data = (truth + sigma * rng.normal(size=truth.shape)).astype(np.float32)
    for kw in ({}, {"flow": 60.0, "fhigh": 150.0}, {"foreground": 3}):
        default = em.log_likelihood(theta, data[0], sigma, **kw)
        jac_count = dict(st.last_jac_route()[1])
        fwd = em.log_likelihood(theta, data[0], sigma, forward_only=True, **kw)
        assert dict(st.last_jac_route()[1]) == jac_count
        assert st.last_lnl_route()[0] == ("two_launch" if "foreground" in kw else "fused"), kw
        assert fwd.shape == default.shape == (256,) and fwd.dtype == np.float32
        if "foreground" in kw:
            # the two-launch route's bound: 1e-5 of the scale r^T W r + |b|^2 of the projected data (test_two_launch_*).
            # Observed on the MI355X: worst 1.3e-7 of the scale.
            A = emu.foreground_basis(em.frequencies, 451, 3, None, None)
            scale = lr.marg_scale(y_all, data[0], em._band_weights(451, sigma, None, None).astype(np.float64), A)
            e = float(np.max(np.abs(fwd.astype(np.float64) - default) / scale))
            print("LNLFWD class surface, foreground=3: %.3e of the scale (bound 1e-5)" % e)
            assert e <= 1e-5, (kw, e)
        else:
            # the bound itself.  Observed on the MI355X: record 1.9e-7, band 1.6e-7.
            e = float(lr.rel_err(fwd, default.astype(np.float64)).max())
            print("LNLFWD class surface %s: %.3e (bound %.1e)" % (kw, e, lr.LNL_FWD_TOL))
            assert e <= lr.LNL_FWD_TOL, (kw, e)
    one = em.log_likelihood(theta[0], data[0], sigma, forward_only=True)
    assert np.ndim(one) == 0 and one == fwd_one(em, theta[0], data[0], sigma)
    # (M, 451) spectra: (R, 7) against every spectrum, (M, R, 7) block by block
    b = em.log_likelihood(theta, data, sigma, forward_only=True)
    assert b.shape == (3, 256) and st.last_lnl_route()[0] == "fused"
    for m in range(3):
        assert same(b[m], em.log_likelihood(theta, data[m], sigma, forward_only=True)), m
    # 128 rows per spectrum: one data row per workgroup, the fused route, the per-spectrum calls' bits
    t384 = pp.par_untransform(np.random.default_rng(5).uniform(-0.9, 0.9, size=(384, 7)), em.par_train)
    p = em.log_likelihood(t384.reshape(3, 128, 7), data, sigma, forward_only=True)
    assert p.shape == (3, 128) and st.last_lnl_route()[0] == "fused"
    for m in range(3):
        assert same(p[m], em.log_likelihood(t384[128 * m:128 * m + 128], data[m], sigma, forward_only=True)), m
    # 2 rows per spectrum: the two-launch route, whose forward takes the few-row route for six float32 rows -- against
    # the float64 reduction of predict's y of the same rows (the few-row route too) at the two-launch route's bound,
    # 1e-5 of ln L (test_two_launch_on_the_shape_table).  Observed on the MI355X: worst 1.3e-7.
    p = em.log_likelihood(theta[:6].reshape(3, 2, 7), data, sigma, forward_only=True)
    assert p.shape == (3, 2) and st.last_lnl_route()[0] == "two_launch"
    w1 = em._band_weights(451, sigma, None, None)
    y6 = np.asarray(em.predict(theta[:6]), np.float64)
    e = max(float(lr.rel_err(p[m], lr.lnl64(y6[2 * m:2 * m + 2], data[m], w1)).max()) for m in range(3))
    print("LNLFWD class surface, 2 rows per spectrum: %.3e (bound 1e-5)" % e)
    assert e <= 1e-5, e
    # log_posterior: ln L inside the box, -inf outside without a device call
    lp = em.log_posterior(data[0], sigma)
    centre = lp.prior_transform(0.5 * np.ones(7))
    assert np.array_equal(centre, pp.par_untransform(np.zeros(7), em.par_train)[0])
    vals = lp(theta)
    assert vals.dtype == np.float64 and same(vals.astype(np.float32), em.log_likelihood(theta, data[0], sigma, forward_only=True))
    lp(theta[:4])
    counts = dict(st.last_lnl_route()[1])
    outside = pp.par_untransform(np.clip(u[:5] * 1.0, -1, 1) + np.array([0, 0, 0, 2.5, 0, 0, 0]), em.par_train)
    assert np.all(lp(outside) == -np.inf) and lp(outside[0]) == -np.inf
    assert dict(st.last_lnl_route()[1]) == counts  # no call reached the library
    mixed = np.vstack([outside[:2], theta[:3]])
    got = lp(mixed)
    assert np.all(got[:2] == -np.inf) and same(got[2:].astype(np.float32), vals[:3].astype(np.float32))
    assert sum(st.last_lnl_route()[1].values()) == sum(counts.values()) + 1


def fwd_one(em, theta, data, sigma):
    return em.log_likelihood(theta[None, :].repeat(2, axis=0), data, sigma, forward_only=True)[0]
