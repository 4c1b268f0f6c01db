"""The ensemble sampler on the GPU (include/v21.h: v21_mlp_sample_ensemble[_dev]): one sweep rebuilt in float64 from the
device's own evaluations and the same Philox draws, independence of chunking / splitting, the two routes, the uniform
target, statistics against the float64 reference (tests/ensemble_ref.py), edge cases and errors, the emulator classes'
surface.

Measured on the MI355X: one sweep, worst |d log alpha| 7.1e-15 (NB; 8.9e-16 on D1 / S3) against a bound of ~3e-5, 0 of
18,828 decisions excused, 40-63 % of the proposals accepted; fused against two-launch first ln L 2.3e-7 (bound 6e-7);
uniform target accept 0.216 as the reference's, worst z 1.71; device against reference sampler worst z 0.19."""
import ctypes as C

import numpy as np
import pytest

import ensemble_ref as er
import fit_ref as fr
import lnl_ref as lr
import sample_ref as sr
import shape_cases as sc
from conftest import pkg
from infer_cases import N_SE, SPREAD
from infer_support import between_chain, fit_setup, flags_of, ready, run_dev, same, starts_near, u_of, ulp32

pytestmark = pytest.mark.gpu

# SPREAD, the walkers' spread around the truth in u: fit_setup's record (sigma = 0.02 std) is flat at 0.003 (ln L varies by 0.1
# .. 0.2 over the walkers) and steep at 0.1; at 0.05 ln L varies by a few units, so that the likelihood term of log alpha
# decides a fair share of the proposals and a fair share of them is accepted
KEYS = ("x_last", "lnl_last", "accept_rate", "mean_u", "cov_u", "samples", "samples_lnl", "last_prop_u", "last_log_alpha", "last_partner")


# ---- one sweep against the float64 rebuild from the device's own evaluations
SHAPES = ((16, 33),   # 32 ensembles per workgroup, a partial last workgroup
          (18, 30),   # H = 9: 28 ensembles per workgroup, idle threads in every workgroup
          (512, 2))   # H = 256: one ensemble per workgroup


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "S3", "NB"])
def test_one_sweep_against_reference(ctx, name, prec):
    """n_steps = 1 from given starts, D1 / S3 on the fused route and NB on the two-launch route.  last_partner and
    last_prop_u: bit-equal for both sets -- set 1's partners are set 0's positions AFTER its half-move, taken from the
    device's own decisions.  log alpha: within one float32 ulp of each of its two ln L, to first order (the rule of
    infer_support.alpha_bound: the inputs are float32 numbers, the formula is float64).  The decisions agree wherever
    |ln U - log alpha| exceeds that bound; at most 0.5 % may be excused.  lnl_last: loglike_fwd of the same u, bit for bit."""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, name)
    ready(st, prec)
    a, d = 2.0, 7
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, nat.FWD_OUT_TRANSFORM)
    for W, E in SHAPES:
        n, H = W * E, W // 2
        seed, chain0, step0 = 100 + W, 11, 40
        x0 = starts_near(truths[0], tin, n, W, SPREAD)
        u0 = st.sample_ensemble(x0, W, prec, flags_of(nat, True), n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)
        assert np.max(np.abs(u0 - u_of(x0, tin))) <= 2.0 ** -23
        r = st.sample_ensemble(x0, W, prec, flags_of(nat, True), n_steps=1, n_warmup=0, a=a, seed=seed, chain0=chain0, step0=step0, diagnostics=True)
        assert st.last_lnl_route()[0] == ("two_launch" if name == "NB" else "fused")
        e, h, _ = er.layout(n, W)
        z, k, logu = er.draws(seed, chain0 + np.arange(n), step0, a, H)
        acc_dev = r["accept_rate"] > 0.5
        u, lnl = u0.copy(), lnl_of(u0).astype(np.float64)
        worst, excused_all = 0.0, 0
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
            diff = np.abs(la_dev[fin] - la[fin])
            worst = max(worst, float(diff.max()))
            assert np.all(diff <= bound[fin]), (tag, float(np.max(diff / bound[fin])))
            excused = np.abs(logu[idx] - la) <= bound
            excused_all += int(excused.sum())
            assert np.array_equal((logu[idx] < la)[~excused], acc_dev[idx][~excused]), tag
            # (a missing barrier shows only where set 0 moved, a wrong ln L only where it decides)
            by_lnl = np.mean((logu[idx] < (d - 1) * np.log(z[idx])) != acc_dev[idx])
            assert 0.1 < acc_dev[idx].mean() < 0.9 and by_lnl > 0.05, (tag, acc_dev[idx].mean(), by_lnl)
            u[idx] = np.where(acc_dev[idx][:, None], y, u[idx])
            lnl[idx] = np.where(acc_dev[idx], lnl_y, lnl[idx])
        print("ENSEMBLE %s %s W=%d: accepted %.3f, worst |d log alpha| %.3e, excused %d of %d" % (name, prec, W, acc_dev.mean(), worst, excused_all, n))
        assert excused_all <= 0.005 * n
        np.testing.assert_allclose(r["x_last"], fr.untransform(u, tin[0], tin[2], tin[3]), rtol=1e-12)
        assert same(r["lnl_last"], lnl_of(u)), (name, prec, W)
    st.set_likelihood(None, None)


# ---- split invariance
def dev_ensemble(ctx, st, x0, data_rows, W, prec, flags, keys=KEYS, guard=0, **opts):
    """v21_mlp_sample_ensemble_dev on float32 starts -> dict of host arrays; every output has `guard` poisoned bytes
    behind it, which must come back untouched"""
    n, din = x0.shape
    o = st.ensemble_opts(W, **opts)
    keep = o.n_steps // o.thin if o.thin else 0
    shapes = {"x_last": ((n, din), np.float32), "lnl_last": ((n,), np.float32), "samples": ((n, keep, din), np.float32),
              "samples_lnl": ((n, keep), np.float32), "mean_u": ((n, din), np.float64), "cov_u": ((n, din, din), np.float64),
              "accept_rate": ((n,), np.float64), "last_prop_u": ((n, din), np.float32), "last_log_alpha": ((n,), np.float64),
              "last_partner": ((n,), np.int32)}
    n_data = data_rows.shape[0] if data_rows is not None else 0
    call = lambda dx, dd, out: st.sample_ensemble_dev(dx, din, n, dd, n_data, out, W, prec, flags, **opts)
    return run_dev(ctx, shapes, keys, call, x0, data_rows, guard)


def test_split_invariance(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    W = 16
    # the host form of 8,208 rows (513 ensembles: chunks of 8,192 and 16 rows) equals the _dev form
    n = 8208
    assert st.route_ensemble("f16", n, W, host_form=True) == ("fused", 8192)
    x = np.ascontiguousarray(starts_near(truths[0], tin, n, 2, SPREAD).astype(np.float32))
    opts = dict(n_steps=4, n_warmup=2, thin=2, seed=77)
    host = st.sample_ensemble(x, W, "f16", flags, diagnostics=True, **opts)
    dev = dev_ensemble(ctx, st, x, None, W, "f16", flags, guard=256, **opts)
    for k in KEYS:
        assert same(host[k], dev[k]), k
    assert 0.05 < host["accept_rate"].mean() < 0.95
    # 6 sweeps in one call = 3 + 3 continued through a float64 x_last and step0
    x64 = starts_near(truths[0], tin, 4 * W, 3, SPREAD)
    six = st.sample_ensemble(x64, W, "f32", flags, data=data[:2], n_steps=6, n_warmup=0, seed=5)
    first = st.sample_ensemble(x64, W, "f32", flags, data=data[:2], n_steps=3, n_warmup=0, seed=5)
    second = st.sample_ensemble(first["x_last"], W, "f32", flags, data=data[:2], n_steps=3, n_warmup=0, seed=5, step0=3)
    assert same(six["samples"], np.concatenate([first["samples"], second["samples"]], axis=1))
    assert same(six["x_last"], second["x_last"]) and same(six["lnl_last"], second["lnl_last"])
    assert same(six["samples_lnl"], np.concatenate([first["samples_lnl"], second["samples_lnl"]], axis=1))
    assert not same(six["x_last"], x64)
    # two calls over halves of the ensembles, each with its own spectrum and chain0, equal the one call
    for half in (0, 1):
        rows = slice(2 * W * half, 2 * W * (half + 1))
        part = st.sample_ensemble(x64[rows], W, "f32", flags, data=data[half:half + 1], n_steps=6, n_warmup=0, seed=5, chain0=2 * W * half)
        for k in ("x_last", "lnl_last", "accept_rate", "mean_u", "cov_u", "samples", "samples_lnl"):
            assert same(part[k], six[k][rows]), (half, k)
    st.set_likelihood(None, None)


# ---- routes
def test_routes_and_counters(ctx):
    """2 spectra x one 256-walker ensemble: 128 proposals per spectrum, the fused route; 2 x 260 rows: the two-launch
    route.  n_steps = 0: lnl_last is the first evaluations' ln L, which the two routes give within LNL_FWD_TOL (f16: the
    two-launch route's forward is the fused kernel too)."""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    x = starts_near(truths[0], tin, 520, 9, 0.01)
    counts = lambda: dict(st.last_lnl_route()[1])
    jac = st.last_jac_route()
    c0 = counts()
    a = st.sample_ensemble(np.ascontiguousarray(np.vstack([x[:256], x[260:516]])), 256, "f16", flags, data=data[:2], n_steps=0, n_warmup=0)
    assert st.last_lnl_route()[0] == "fused" and counts().get("fused", 0) == c0.get("fused", 0) + 1
    assert counts().get("two_launch", 0) == c0.get("two_launch", 0)
    b = st.sample_ensemble(x, 260, "f16", flags, data=data[:2], n_steps=0, n_warmup=0)
    assert st.last_lnl_route()[0] == "two_launch" and counts().get("two_launch", 0) == c0.get("two_launch", 0) + 1
    common = np.r_[0:256, 260:516]
    err = lr.rel_err(b["lnl_last"][common], a["lnl_last"].astype(np.float64))
    print("ENSEMBLE routes: fused against two-launch, worst %.3e (bound %.1e)" % (err.max(), lr.LNL_FWD_TOL))
    assert err.max() <= lr.LNL_FWD_TOL
    # one count per call, whatever its sweeps and chunks; the Jacobian's record is not touched
    c0 = sum(counts().values())
    st.sample_ensemble(np.ascontiguousarray(np.tile(x[:16], (514, 1))), 16, "f16", flags, n_steps=2, n_warmup=1, thin=0)
    assert sum(counts().values()) == c0 + 1 and st.last_jac_route() == jac
    st.set_likelihood(None, None)


# ---- the uniform target
def test_uniform_target_on_the_device(ctx):
    """all weights 0: ln L = 0 everywhere, acceptance follows (d - 1) ln z alone and the law is uniform on the box"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    st.set_likelihood(data[0], np.zeros(dims[-1], np.float32))
    W, E, d = 16, 64, 7
    n = W * E
    u0 = np.random.default_rng(4).uniform(-1, 1, size=(n, d))
    x0 = fr.untransform(u0, tin[0], tin[2], tin[3])
    opts = dict(n_steps=600, n_warmup=200, seed=5)
    r = st.sample_ensemble(x0, W, "f16", flags_of(nat, True), thin=0, diagnostics=True, **opts)
    assert "samples" not in r and all(np.all(np.isfinite(r[k])) for k in ("mean_u", "cov_u", "accept_rate", "x_last"))
    assert np.all(r["lnl_last"] == 0)
    z = er.draws(5, np.arange(n), 799, 2.0, W // 2)[0]
    fin = np.isfinite(r["last_log_alpha"])
    np.testing.assert_allclose(r["last_log_alpha"][fin], ((d - 1) * np.log(z))[fin], rtol=0, atol=1e-12)
    m, m2 = er.ensemble_estimates(r["mean_u"], r["cov_u"], W)
    zm, z2 = sr.pooled_check(m, 0.0)[1], sr.pooled_check(m2, 1.0 / 3.0)[1]
    ref = er.ensemble_ref(lambda u: np.zeros(u.shape[0]), u_of(x0, tin), W, thin=0, **opts)
    acc_d, acc_r = r["accept_rate"].reshape(E, W).mean(axis=1), ref["accept_rate"].reshape(E, W).mean(axis=1)
    za = abs(acc_d.mean() - acc_r.mean()) / np.sqrt((acc_d.var(ddof=1) + acc_r.var(ddof=1)) / E + 1e-300)
    print("ENSEMBLE uniform target: accept %.3f (reference %.3f, z %.2f), worst z mean %.2f, E[u^2] %.2f"
          % (acc_d.mean(), acc_r.mean(), za, zm.max(), z2.max()))
    assert 0 < acc_d.mean() < 1 and (za < N_SE or acc_d.mean() == acc_r.mean())
    assert np.all(zm < N_SE) and np.all(z2 < N_SE), (zm, z2)
    assert np.all(np.abs(u_of(r["x_last"], tin)) <= 1 + 1e-12)
    st.set_likelihood(None, None)


# ---- statistics against the reference
def test_statistics_against_reference(ctx):
    """NB, f32, 64 ensembles x 16 walkers, 100 + 200 sweeps on the device and in tests/ensemble_ref.py (same starts, same
    draws): per-ensemble pooled mean and second moments within 5 combined between-ensemble standard errors"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, "NB")
    ready(st, "f32")
    W, E = 16, 64
    x0 = starts_near(truths[0], tin, W * E, 1, SPREAD)
    opts = dict(n_steps=200, n_warmup=100, seed=11)
    r = st.sample_ensemble(x0, W, "f32", flags_of(nat, True), thin=0, **opts)
    ref = er.ensemble_ref(er.forward_evaluator(Ws, bs, act, data[0], w, tout), u_of(x0, tin), W, thin=0, **opts)
    worst = {}
    pool = lambda q: q.reshape((E, W) + q.shape[1:]).mean(axis=1)
    sec = lambda q: q["cov_u"] + q["mean_u"][:, :, None] * q["mean_u"][:, None, :]
    for key, dv, rf in (("mean", pool(r["mean_u"]), pool(ref["mean_u"])), ("second moments", pool(sec(r)), pool(sec(ref))),
                        ("accept", pool(r["accept_rate"]), pool(ref["accept_rate"]))):
        (md, vd), (mr, vr) = between_chain(dv), between_chain(rf)
        zz = np.abs(md - mr) / np.sqrt(vd + vr)
        worst[key] = float(np.max(zz))
        assert np.all(zz < N_SE), (key, zz)
    print("ENSEMBLE device vs reference: accept %.3f / %.3f, worst z %s" % (r["accept_rate"].mean(), ref["accept_rate"].mean(), worst))
    assert 0.05 < r["accept_rate"].mean() < 0.95
    st.set_likelihood(None, None)


# ---- edges
def test_edge_cases(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    W = 16
    x0 = starts_near(truths[0], tin, 2 * W, 6, SPREAD)
    # n = 0: a no-op on both entries
    r = st.sample_ensemble(x0[:0], W, "f32", flags, n_steps=2, n_warmup=0)
    assert r["x_last"].shape == (0, 7) and r["samples"].shape == (0, 2, 7)
    dev_ensemble(ctx, st, np.zeros((0, 7), np.float32), None, W, "f32", flags, keys=("x_last",), guard=64, n_steps=1, n_warmup=0)
    # n_steps = 0 returns the clamped start: one outside the box, one with fx = 0 (its floor is the box's lower bound)
    xs = x0.copy()
    xs[1, 3] = 1e6
    xs[2, 2] = 0.0
    r0 = st.sample_ensemble(xs, W, "f32", flags, n_steps=0, n_warmup=0, diagnostics=True)
    uc = np.clip(u_of(xs, tin), -1, 1)
    assert uc[1, 3] == 1.0 and uc[2, 2] == -1.0
    np.testing.assert_allclose(r0["x_last"], fr.untransform(uc, tin[0], tin[2], tin[3]), rtol=1e-6)
    np.testing.assert_array_equal(r0["last_prop_u"], uc.astype(np.float32))
    assert "samples" not in r0 and np.all(r0["last_log_alpha"] == 0) and np.all(r0["accept_rate"] == 0) and np.all(r0["last_partner"] == -1)
    np.testing.assert_array_equal(r0["mean_u"], uc.astype(np.float32).astype(np.float64))
    assert same(r0["lnl_last"], st.loglike_fwd(uc.astype(np.float32), "f32", nat.FWD_OUT_TRANSFORM))
    # thin = 0: no samples, the moments of every kept sweep; thin that does not divide n_steps
    full = st.sample_ensemble(xs, W, "f32", flags, n_steps=10, n_warmup=3, seed=2)
    none = st.sample_ensemble(xs, W, "f32", flags, n_steps=10, n_warmup=3, seed=2, thin=0)
    part = st.sample_ensemble(xs, W, "f32", flags, n_steps=10, n_warmup=3, seed=2, thin=4)
    assert "samples" not in none and same(none["mean_u"], full["mean_u"]) and same(none["cov_u"], full["cov_u"])
    assert part["samples"].shape == (2 * W, 2, 7) and same(part["samples"], full["samples"][:, [3, 7]]) and same(part["x_last"], full["x_last"])
    us = u_of(full["samples"].reshape(-1, 7), tin).reshape(2 * W, 10, 7)
    assert np.all(np.abs(us) <= 1 + 1e-12)
    np.testing.assert_allclose(full["mean_u"], us.mean(axis=1), atol=1e-12)
    np.testing.assert_allclose(full["cov_u"], np.einsum("nki,nkj->nij", us, us) / 10 - np.einsum("ni,nj->nij", us.mean(axis=1), us.mean(axis=1)),
                               atol=1e-12)
    # an ensemble whose walkers all start at one point stays there (the other ensemble moves)
    xd = x0.copy()
    xd[:W] = x0[0]
    rd = st.sample_ensemble(xd, W, "f32", flags, n_steps=5, n_warmup=0, seed=3, diagnostics=True)
    assert all(np.all(np.isfinite(rd[k])) for k in ("x_last", "lnl_last", "mean_u", "cov_u", "samples"))
    assert not np.any(np.isnan(rd["last_log_alpha"])) and np.all(np.isfinite(rd["last_log_alpha"][:W]))
    assert same(rd["samples"][:W], np.broadcast_to(rd["x_last"][:1, None, :], (W, 5, 7))) and np.all(rd["cov_u"][:W] == 0)
    assert not same(rd["x_last"][W:], xd[W:])
    # inf in the data at w == 0 bins changes no bit: the record (the fused route) and a data matrix of 16 rows per spectrum
    # (the two-launch route)
    d2 = data[:2].copy()
    d2[:, :40] = np.inf
    assert np.all(w[:40] == 0)
    runs = []
    for rec, mat, route in ((data[0], None, "fused"), (d2[0], None, "fused"), (data[0], data[:2], "two_launch"), (d2[0], d2[:2], "two_launch")):
        with np.errstate(invalid="ignore"):
            st.set_likelihood(rec, w)
        runs.append(st.sample_ensemble(x0, W, "f16", flags, data=mat, n_steps=4, n_warmup=0, seed=8))
        assert st.last_lnl_route()[0] == route and np.all(np.isfinite(runs[-1]["lnl_last"]))
    for ra, rb in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert same(ra["samples"], rb["samples"]) and same(ra["lnl_last"], rb["lnl_last"]) and same(ra["samples_lnl"], rb["samples_lnl"])
    st.set_likelihood(data[0], w)
    # a nuisance record with K = 3: the two-launch route, ln L marginalised as loglike_fwd's
    st.set_nuisance(sc.basis(dims[-1], 3))
    try:
        rn = st.sample_ensemble(x0, W, "f32", flags, n_steps=3, n_warmup=0, seed=4)
        assert st.last_lnl_route()[0] == "two_launch" and np.all(np.isfinite(rn["samples"]))
        un = u_of(rn["x_last"], tin).astype(np.float32)
        np.testing.assert_allclose(rn["lnl_last"], st.loglike_fwd(un, "f32", nat.FWD_OUT_TRANSFORM), rtol=1e-4)
    finally:
        st.set_nuisance(None)
    # poison guards past every output of the _dev form stay intact (asserted inside dev_ensemble)
    dev_ensemble(ctx, st, np.ascontiguousarray(x0.astype(np.float32)), np.ascontiguousarray(data[:2]), W, "f32", flags, guard=256,
                 n_steps=3, n_warmup=1, seed=1)
    st.set_likelihood(None, None)
    with pytest.raises(nat.EngineError):  # no record
        st.sample_ensemble(x0, W, "f32", flags, n_steps=1, n_warmup=0)


def test_argument_errors_leave_the_handle_usable(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = flags_of(nat, True)
    lib, F, P = st.lib, C.POINTER(C.c_float), C.c_void_p
    x0 = np.ascontiguousarray(starts_near(truths[0], tin, 96, 40, 0.01).astype(np.float32))
    xl = np.empty_like(x0)
    d = np.ascontiguousarray(data[:1])
    out = nat.EnsembleOut(x_last=xl.ctypes.data)

    def opts(**kw):
        o = dict(nat.ENSEMBLE_DEFAULTS, n_walkers=16, n_steps=2, n_warmup=1)
        o.update(kw)
        return nat.EnsembleOpts(*[o[k] for k, _ in nat.EnsembleOpts._fields_])

    host = lambda n, nd, o: lib.v21_mlp_sample_ensemble(st.h, x0.ctypes.data_as(P), 0, n, d.ctypes.data_as(F) if nd else None, nd,
                                                        C.byref(o), C.byref(out), 0, flags)
    d4 = np.ascontiguousarray(np.tile(d, (4, 1)))
    host4 = lambda n, o: lib.v21_mlp_sample_ensemble(st.h, x0.ctypes.data_as(P), 0, n, d4.ctypes.data_as(F), 4, C.byref(o), C.byref(out), 0, flags)
    bad = [(96, opts(n_walkers=17)), (96, opts(n_walkers=14)), (96, opts(n_walkers=514)), (40, opts()), (96, opts(a=1.0)), (96, opts(a=0.5)),
           (96, opts(a=float("nan"))), (96, opts(n_steps=-1)), (96, opts(n_warmup=-1)), (96, opts(thin=-1)), (96, opts(chain0=-1)),
           (96, opts(step0=-1))]
    for n, o in bad:
        assert host(n, 0, o) == -1, (n, o.n_walkers, o.a)
        assert host(96, 0, opts()) == 0  # the handle stays usable after each
    assert host4(96, opts()) == -1       # 24 rows per spectrum: no whole ensembles
    assert host4(64, opts()) == 0
    bufs = [ctx.malloc(x0.nbytes), ctx.malloc(x0.nbytes)]
    try:
        dout = nat.EnsembleOut(x_last=bufs[1])
        dev = lambda n, o: lib.v21_mlp_sample_ensemble_dev(st.h, P(bufs[0]), 7, n, None, 0, C.byref(o), C.byref(dout), 0, flags)
        ctx.h2d(bufs[0], x0)
        for n, o in bad:
            assert dev(n, o) == -1
        assert dev(96, opts()) == 0
        ctx.sync()
        ctx.d2h(xl, bufs[1])
        assert np.all(np.isfinite(xl))
    finally:
        for p in bufs:
            ctx.free(p)
    st.set_likelihood(None, None)


# ---- the class surface on the shipped weights
def test_class_surface(shipped):
    emulator, synth, pp = pkg("emulator"), pkg("synth"), pkg("preprocess")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    u_true = np.random.default_rng(4).uniform(-0.6, 0.6, size=(2, 7))
    truths = pp.par_untransform(u_true, ae.par_train)
    spectra = np.asarray(ae.predict(truths), np.float32)
    lo, hi = pp.par_untransform(-np.ones(7), ae.par_train)[0], pp.par_untransform(np.ones(7), ae.par_train)[0]
    kw = dict(n_walkers=16, n_ensembles=4, n_steps=200, n_warmup=100, thin=10, p0=truths[1], return_lnl=True)
    r = ae.sample_ensemble(spectra[1], 0.05, **kw)
    assert r.params.shape == (4, 16, 20, 7) and r.lnl.shape == (4, 16, 20) and r.accept_rate.shape == (4, 16) and r.step_size is None
    assert r.r_hat.shape == (7,) and r.mean_u.shape == (7,) and r.cov_u.shape == (7, 7)
    assert np.all(r.params >= lo * (1 - 1e-12)) and np.all(r.params <= hi * (1 + 1e-12))
    assert np.all(np.isfinite(r.r_hat)) and np.all(np.isfinite(r.lnl))
    print("ENSEMBLE class surface: r_hat %s, accept %.3f" % (r.r_hat.round(3), r.accept_rate.mean()))
    again = ae.sample_ensemble(spectra[1], 0.05, **kw)
    assert same(r.params, again.params) and same(r.lnl, again.lnl) and same(r.mean_u, again.mean_u)
    other = ae.sample_ensemble(spectra[1], 0.05, **dict(kw, seed=1))
    assert not same(r.params, other.params)
    # several spectra, default starts (the best fit per spectrum), with and without stored samples
    r2 = ae.sample_ensemble(spectra, 1.0, n_walkers=16, n_ensembles=2, n_steps=20, n_warmup=10, thin=0)
    assert r2.params is None and r2.lnl is None and r2.accept_rate.shape == (2, 2, 16) and r2.r_hat.shape == (2, 7) and r2.cov_u.shape == (2, 7, 7)
    r3 = ae.sample_ensemble(spectra, 1.0, n_walkers=16, n_ensembles=2, n_steps=20, n_warmup=10)
    assert r3.params.shape == (2, 2, 16, 20, 7) and r3.lnl is None
    assert hasattr(emulator.DirectEmulator(**data), "sample_ensemble")
    with pytest.raises(ValueError):
        ae.sample_ensemble(np.zeros(450), 1.0)
    with pytest.raises(ValueError):
        ae.sample_ensemble(spectra[0], 1.0, n_walkers=14)
    with pytest.raises(ValueError):
        ae.sample_ensemble(spectra[0], 1.0, a=1.0)
