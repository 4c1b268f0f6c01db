"""The nested sampler on the GPU (include/v21.h: v21_mlp_sample_nested[_dev]): iterations rebuilt exactly from the device's
own evaluations and the same Philox draws (tests/nested_ref.py), independence of chunking / splitting, the evidence against
quadrature and against the float64 reference, given starts and left-out arrays across a host chunk boundary, a flat target,
edge cases and errors, the emulator classes' surface.

Measured on the MI355X: the rebuild bit-equal in all 18 cases, 0 decisions excused, 42-60 % of the proposals accepted;
i1 ln Z -39.0255 +- 0.0339 (quadrature -39.0112, z -0.42), i2 -40.9410 +- 0.0350 (quadrature -40.9389, z -0.06), both equal
to the reference's to the digits shown; the module's 13 tests in 6 s, the two chunk-boundary tests added since under 1 s."""
import ctypes as C

import numpy as np
import pytest

import nested_ref as nr
import shape_cases as sc
from conftest import pkg
from infer_cases import N_SE, QUAD, RUNS, SEED, SPREAD, quadrature_case
from infer_support import device_stack, fit_setup, ready, run_dev, same, starts_near

pytestmark = pytest.mark.gpu

KEYS = ("dead_u", "dead_lnl", "lstar", "live_u", "live_lnl", "accept_rate", "last_partner", "last_prop_u")


def live_near(truth, tin, n, seed, scale=SPREAD):
    """n float64 live points in u: the truth jittered by `scale`, inside the box"""
    return starts_near(truth, tin, n, seed, scale, raw=False)


def stats(r, N):
    """per-run (ln Z, error) of a device result, by the product's own function"""
    em = pkg("emulator")
    runs = r["live_lnl"].shape[0] // N
    lz, err, _, _ = em.nested_evidence(r["dead_lnl"].transpose(1, 0, 2), r["live_lnl"].reshape(runs, N), N)
    return lz, err


# ---- iterations against the exact rebuild from the device's own evaluations
SHAPES = ((16, 33),   # 32 runs per workgroup, a partial last workgroup
          (18, 30),   # k = 9: 28 runs per workgroup, 4 idle threads in every workgroup
          (512, 2))   # k = 256: one run across four waves


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "NB"])
def test_iterations_against_rebuild(ctx, name, prec):
    """Two iterations of two moves from given live points, D1 on the fused route and NB on the two-launch route.  The
    rebuild (tests/nested_ref.py) ranks, records, restarts, draws and proposes in the kernel's float32 operation order and
    takes every ln L from the device -- the starts' from a call of no iterations, the proposals' from loglike_fwd of the
    same compacted rows -- so the rule compares the very float32 values the kernel compared: dead record and its order,
    L*, the survivors' order and the restart copies (the live points), the last partners and proposals, every decision
    (the accept counts and the live points) are BIT-EQUAL, 0 decisions excused.  Rows 5 and 9 of every run duplicate
    row 2: ties, broken on the row index."""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, name)
    ready(st, prec)
    flags = nat.FWD_OUT_TRANSFORM
    lnl_of = lambda u: st.loglike_fwd(np.ascontiguousarray(u, np.float32), prec, flags)
    for N, runs in SHAPES:
        n, k = N * runs, N // 2
        opts = dict(n_iter=2, n_repeats=2, seed=100 + N, chain0=11 * N, iter0=40)
        u0 = live_near(truths[0], tin, n, N).reshape(runs, N, 7)
        u0[:, 5] = u0[:, 2]
        u0[:, 9] = u0[:, 2]
        u0 = u0.reshape(n, 7)
        r0 = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, n_iter=0)
        assert same(r0["live_u"], u0.astype(np.float32).astype(np.float64)) and r0["dead_lnl"].shape == (0, runs, k)
        r = st.sample_nested(u0, n_live=N, precision=prec, flags=flags, diagnostics=True, **opts)
        assert st.last_lnl_route()[0] == ("two_launch" if name == "NB" else "fused")
        ref = nr.nested_ref(lnl_of, u0, N, lnl0=r0["live_lnl"], **opts)
        tag = "%s %s N=%d" % (name, prec, N)
        acc = r["accept_rate"].mean()
        print("NESTED %s: accepted %.3f, L* %s .. %s" % (tag, acc, r["lstar"].min(), r["lstar"].max()))
        assert same(r["dead_lnl"], ref["dead_lnl"].astype(np.float32)), tag
        assert same(r["dead_u"], ref["dead_u"].astype(np.float64)), tag
        assert same(r["lstar"], ref["lstar"].astype(np.float32)) and same(r["lstar"], r["dead_lnl"][:, :, -1]), tag
        assert np.all(np.diff(r["dead_lnl"], axis=2) >= 0), tag
        assert np.array_equal(r["last_partner"], ref["last_partner"]), tag
        assert same(r["last_prop_u"], ref["last_prop_u"]), tag
        assert np.array_equal(r["accept_rate"], ref["accept_rate"]), tag
        assert same(r["live_u"], ref["live_u"].astype(np.float64)), tag
        assert same(r["live_lnl"], ref["live_lnl"].astype(np.float32)), tag
        # (a wrong decision shows only where ln L decides and a fair share moves)
        assert 0.2 < acc < 0.8, (tag, acc)
        # the survivors lie in rank order and every live point is above the last threshold or a copy of one that is
        lv = r["live_lnl"].reshape(runs, N)
        assert np.all(np.diff(lv[:, k:], axis=1) >= 0) and np.all(lv >= r["lstar"][-1][:, None]), tag
    st.set_likelihood(None, None)


# ---- continuation and splitting
def dev_nested(ctx, st, u0, n, data_rows, N, prec, flags, keys=KEYS, guard=0, **opts):
    """v21_mlp_sample_nested_dev on float32 live points (None: drawn) -> dict of host arrays; every output has `guard`
    poisoned bytes behind it, which must come back untouched"""
    din = st.dims[0]
    o = st.nested_opts(N, in_dim=din, **opts)
    runs, k, T = n // N, N // 2, o.n_iter
    shapes = {"dead_u": ((T, runs, k, din), np.float32), "dead_lnl": ((T, runs, k), np.float32), "lstar": ((T, runs), np.float32),
              "live_u": ((n, din), np.float32), "live_lnl": ((n,), np.float32), "accept_rate": ((runs, k), np.float64),
              "last_partner": ((runs, k, 2), np.int32), "last_prop_u": ((runs, k, din), np.float32)}
    n_data = data_rows.shape[0] if data_rows is not None else 0
    call = lambda dx, dd, out: st.sample_nested_dev(dx, din, n, dd, n_data, out, N, prec, flags, **opts)
    return run_dev(ctx, shapes, keys, call, u0, data_rows, guard)


def test_continuation_and_splitting(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = nat.FWD_OUT_TRANSFORM
    N = 16
    # the host form of 8,208 rows (513 runs: chunks of 8,192 and 16 rows) equals the _dev form; drawn starts
    n = 8208
    assert st.route_nested("f16", n, N, host_form=True) == ("fused", 8192)
    opts = dict(n_iter=3, n_repeats=2, seed=77)
    host = st.sample_nested(None, n, N, "f16", flags, diagnostics=True, **opts)
    dev = dev_nested(ctx, st, None, n, None, N, "f16", flags, guard=256, **opts)
    for key in KEYS:
        assert same(host[key].astype(dev[key].dtype), dev[key]), key
    assert same(host["live_u"], host["live_u"].astype(np.float32).astype(np.float64))
    assert 0.02 < host["accept_rate"].mean() < 0.98
    # 4 iterations in one call = 2 + 2 continued through the live points and iter0, against a data matrix
    u = live_near(truths[0], tin, 4 * N, 3)
    kw = dict(n_live=N, precision="f32", flags=flags, data=data[:2], n_repeats=3, seed=5, diagnostics=True)
    four = st.sample_nested(u, n_iter=4, **kw)
    first = st.sample_nested(u, n_iter=2, **kw)
    second = st.sample_nested(first["live_u"], n_iter=2, iter0=2, **kw)
    for key in ("dead_u", "dead_lnl", "lstar"):
        assert same(four[key], np.concatenate([first[key], second[key]])), key
    for key in ("live_u", "live_lnl", "last_partner", "last_prop_u"):
        assert same(four[key], second[key]), key
    np.testing.assert_allclose(four["accept_rate"], (first["accept_rate"] + second["accept_rate"]) / 2, rtol=0, atol=1e-15)
    assert not same(four["live_u"], first["live_u"]) and np.all(four["lstar"][1:] >= four["lstar"][:-1])
    # two calls over halves of the runs, each with its own spectrum and chain0, equal the one call
    for half in (0, 1):
        rows, rr = slice(2 * N * half, 2 * N * (half + 1)), slice(2 * half, 2 * half + 2)
        part = st.sample_nested(u[rows], n_iter=4, chain0=2 * N * half, **dict(kw, data=data[half:half + 1]))
        for key in ("live_u", "live_lnl"):
            assert same(part[key], four[key][rows]), (half, key)
        for key in ("dead_u", "dead_lnl", "lstar"):
            assert same(part[key], four[key][:, rr]), (half, key)
        for key in ("accept_rate", "last_partner", "last_prop_u"):
            assert same(part[key], four[key][rr]), (half, key)
    st.set_likelihood(None, None)


_boundary = {}


def boundary_case(ctx):
    """8,208 given live points (513 runs of 16: host chunks of 8,192 and 16 rows), float64 values that float32 holds
    exactly, three iterations in f16 -> (stack with its record set, float64 starts, options, the host form's full result,
    computed once)"""
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    if not _boundary:
        n, N = 8208, 16
        assert st.route_nested("f16", n, N, host_form=True) == ("fused", 8192)
        u = live_near(truths[0], tin, n, 21).astype(np.float32).astype(np.float64)
        kw = dict(n_live=N, precision="f16", flags=pkg("_native").FWD_OUT_TRANSFORM, n_iter=3, n_repeats=2, seed=78)
        _boundary.update(u=u, kw=kw, full=st.sample_nested(u, diagnostics=True, **kw))
    return st, _boundary["u"], _boundary["kw"], _boundary["full"]


def test_given_starts_across_a_chunk_boundary(ctx):
    """the host form uploads a chunk's given starts as every host form uploads its rows: every output equals the _dev
    form's on the same float32 rows"""
    st, u, kw, full = boundary_case(ctx)
    dev = dev_nested(ctx, st, np.ascontiguousarray(u.astype(np.float32)), u.shape[0], None, kw["n_live"], kw["precision"], kw["flags"],
                     guard=256, n_iter=kw["n_iter"], n_repeats=kw["n_repeats"], seed=kw["seed"])
    for key in KEYS:
        assert full[key].size > 0 and same(full[key].astype(dev[key].dtype), dev[key]), key
    assert 0.02 < full["accept_rate"].mean() < 0.98
    st.set_likelihood(None, None)


def test_optional_arrays_left_out_across_a_chunk_boundary(ctx):
    """without the dead record and the diagnostics -- null slots among the slots of one copy per iteration -- the other
    outputs of the same call do not move"""
    st, u, kw, full = boundary_case(ctx)
    lean = st.sample_nested(u, dead=False, diagnostics=False, **kw)
    assert sorted(lean) == ["accept_rate", "live_lnl", "live_u"]
    for key in lean:
        assert same(lean[key], full[key]), key
    st.set_likelihood(None, None)


# ---- the evidence
@pytest.mark.parametrize("name", ["i1", "i2"])
def test_evidence_against_quadrature_and_reference(ctx, name):
    """the two quadrature problems of tests/infer_cases.py on the device in f32, 64 runs from the drawn starts the
    reference takes too: ln Z within 5 standard errors of the midpoint rule's and within 5 (both sides' errors) of
    tests/nested_ref.py's"""
    nat = pkg("_native")
    p, lz_q, ref, lz_ref = quadrature_case(name)
    N, T = QUAD[name]
    st, rec = device_stack(ctx, p["dims"], p["act"])
    st.set_likelihood(p["data"], p["w"])
    r = st.sample_nested(None, RUNS * N, N, "f32", nat.FWD_OUT_TRANSFORM, n_iter=T, seed=SEED)
    lz, err = stats(r, N)
    se, se_ref = lz.std(ddof=1) / 8, lz_ref.std(ddof=1) / 8
    z_q, z_r = (lz.mean() - lz_q) / se, (lz.mean() - lz_ref.mean()) / np.hypot(se, se_ref)
    print("NESTED %s: ln Z %.4f +- %.4f (quadrature %.4f, z %+.2f; reference %.4f +- %.4f, z %+.2f), formula error %.3f, scatter %.3f, accept %.2f"
          % (name, lz.mean(), se, lz_q, z_q, lz_ref.mean(), se_ref, z_r, err.mean(), lz.std(ddof=1), r["accept_rate"].mean()))
    assert abs(z_q) < N_SE and abs(z_r) < N_SE
    st.set_likelihood(None, None)


def test_flat_target(ctx):
    """all weights 0: every ln L is equal, the strict rule accepts nothing after the start, ln Z is that ln L"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    st.set_likelihood(data[0], np.zeros(dims[-1], np.float32))
    N, runs = 64, 8
    r = st.sample_nested(None, N * runs, N, "f16", nat.FWD_OUT_TRANSFORM, n_iter=5, seed=3, diagnostics=True)
    assert all(np.all(np.isfinite(r[key])) for key in KEYS)
    c = r["live_lnl"][0]
    assert np.all(r["live_lnl"] == c) and np.all(r["dead_lnl"] == c) and np.all(r["lstar"] == c) and np.all(r["accept_rate"] == 0)
    lz, err = stats(r, N)
    np.testing.assert_allclose(lz, float(c), rtol=0, atol=1e-12)
    # ties everywhere: the ranks are the row indices, so iteration 0's dead points are the first half of the drawn starts
    u0 = nr.start_draws(3, np.arange(N * runs), 7).reshape(runs, N, 7)
    assert same(r["dead_u"][0], u0[:, :N // 2].astype(np.float64))
    st.set_likelihood(None, None)


# ---- edges
def test_edge_cases(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = nat.FWD_OUT_TRANSFORM
    N = 64
    u = live_near(truths[0], tin, 2 * N, 6)
    # n = 0: a no-op on both entries
    r = st.sample_nested(u[:0], n_live=N, flags=flags, n_iter=2)
    assert r["live_u"].shape == (0, 7) and r["dead_u"].shape == (2, 0, 32, 7)
    dev_nested(ctx, st, np.zeros((0, 7), np.float32), 0, None, N, "f32", flags, keys=("live_u",), guard=64, n_iter=1)
    # n_iter = 0 returns the start, clamped into the box, with its ln L
    us = u.copy()
    us[1, 3], us[2, 2] = 7.0, np.nan
    r0 = st.sample_nested(us, n_live=N, flags=flags, n_iter=0, diagnostics=True)
    uc = np.where(np.isnan(us), -1.0, np.clip(us, -1, 1)).astype(np.float32)
    assert same(r0["live_u"], uc.astype(np.float64)) and np.all(r0["accept_rate"] == 0) and np.all(r0["last_partner"] == -1)
    assert same(r0["live_lnl"], np.concatenate([st.loglike_fwd(np.ascontiguousarray(uc.reshape(2, 2, 32, 7)[:, h].reshape(-1, 7)), "f32", flags)
                                                .reshape(2, 32) for h in (0, 1)], axis=1).reshape(-1))
    # inf in the data at w == 0 bins changes no bit: the record (the fused route) and a data matrix of 64 rows per spectrum
    # (the two-launch route)
    d2 = data[:2].copy()
    d2[:, :40] = np.inf
    assert np.all(w[:40] == 0)
    runs = []
    for rec, mat, route in ((data[0], None, "fused"), (d2[0], None, "fused"), (data[0], data[:2], "two_launch"), (d2[0], d2[:2], "two_launch")):
        with np.errstate(invalid="ignore"):
            st.set_likelihood(rec, w)
        runs.append(st.sample_nested(u, n_live=N, precision="f16", flags=flags, data=mat, n_iter=3, n_repeats=4, seed=8))
        assert st.last_lnl_route()[0] == route and np.all(np.isfinite(runs[-1]["live_lnl"])) and np.all(np.isfinite(runs[-1]["dead_lnl"]))
    for ra, rb in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert all(same(ra[key], rb[key]) for key in ("dead_u", "dead_lnl", "live_u", "live_lnl", "accept_rate"))
    st.set_likelihood(data[0], w)
    # a nuisance record with K = 3: the two-launch route, ln L marginalised as loglike_fwd's
    st.set_nuisance(sc.basis(dims[-1], 3))
    try:
        rn = st.sample_nested(u, n_live=N, flags=flags, n_iter=3, n_repeats=4, seed=4)
        assert st.last_lnl_route()[0] == "two_launch" and np.all(np.isfinite(rn["dead_lnl"]))
        np.testing.assert_allclose(rn["live_lnl"], st.loglike_fwd(rn["live_u"].astype(np.float32), "f32", flags), rtol=1e-4)
        assert np.all(np.diff(rn["lstar"], axis=0) >= 0)
    finally:
        st.set_nuisance(None)
    # poison guards past every output of the _dev form stay intact (asserted inside dev_nested); given starts, a data matrix
    dev_nested(ctx, st, np.ascontiguousarray(u.astype(np.float32)), 2 * N, np.ascontiguousarray(data[:2]), N, "f32", flags, guard=256,
               n_iter=3, n_repeats=2, seed=1)
    # one count per call, whatever its iterations and chunks; the Jacobian's record is not touched
    counts = lambda: sum(st.last_lnl_route()[1].values())
    c0, jac = counts(), st.last_jac_route()
    st.sample_nested(None, 16 * 514, 16, "f16", flags, n_iter=2, n_repeats=1, dead=False)
    assert counts() == c0 + 1 and st.last_jac_route() == jac
    st.set_likelihood(None, None)
    with pytest.raises(nat.EngineError):  # no record
        st.sample_nested(u, n_live=N, flags=flags, n_iter=1)


def test_argument_errors_leave_the_handle_usable(ctx):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx)
    flags = nat.FWD_OUT_TRANSFORM
    lib, F, P = st.lib, C.POINTER(C.c_float), C.c_void_p
    x0 = np.ascontiguousarray(live_near(truths[0], tin, 256, 40).astype(np.float32))
    xl = np.empty_like(x0)
    d4 = np.ascontiguousarray(np.tile(data[:1], (4, 1)))
    out = nat.NestedOut(live_u=xl.ctypes.data)

    def opts(**kw):
        o = dict(nat.NESTED_DEFAULTS, n_live=64, n_iter=2, n_repeats=2)
        o.update(kw)
        return nat.NestedOpts(*[o[key] for key, _ in nat.NestedOpts._fields_])

    host = lambda n, nd, o: lib.v21_mlp_sample_nested(st.h, x0.ctypes.data_as(P), 0, n, d4.ctypes.data_as(F) if nd else None, nd,
                                                      C.byref(o), C.byref(out), 0, flags)
    bad = [(256, opts(n_live=65)), (252, opts(n_live=14)), (256, opts(n_live=514)), (100, opts()), (256, opts(gamma=-0.5)),
           (256, opts(gamma=float("nan"))), (256, opts(gamma=float("inf"))), (256, opts(n_iter=-1)), (256, opts(n_repeats=-1)),
           (256, opts(iter0=-1)), (256, opts(chain0=-1)), (256, opts(iter0=2 ** 31, n_repeats=2))]
    for n, o in bad:
        assert host(n, 0, o) == -1, (n, o.n_live, o.gamma)
        assert host(256, 0, opts()) == 0  # the handle stays usable after each
    assert host(192, 4, opts()) == -1       # 48 rows per spectrum: no whole runs
    assert host(256, 4, opts()) == 0
    assert np.all(np.isfinite(xl)) and np.all(np.abs(xl) <= 1)
    bufs = [ctx.malloc(x0.nbytes), ctx.malloc(x0.nbytes)]
    try:
        dout = nat.NestedOut(live_u=bufs[1])
        dev = lambda n, o: lib.v21_mlp_sample_nested_dev(st.h, P(bufs[0]), 7, n, None, 0, C.byref(o), C.byref(dout), 0, flags)
        ctx.h2d(bufs[0], x0)
        for n, o in bad:
            assert dev(n, o) == -1
        assert lib.v21_mlp_sample_nested_dev(st.h, P(bufs[0]), 6, 256, None, 0, C.byref(opts()), C.byref(dout), 0, flags) == -1  # pitch
        assert dev(256, opts()) == 0
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
    r = ae.nested_sample(spectra[1], 5.0, n_live=64, dlogz=0.05, seed=2)
    P = r.n_iter * 32 + 64
    assert r.stopped == "dlogz" and r.n_iter % 16 == 0 and r.n_iter < 2000
    assert r.params.shape == (1, P, 7) and r.lnl.shape == (1, P) and r.log_weights.shape == (1, P) and r.accept_rate.shape == (1,)
    assert r.mean_u.shape == (7,) and r.cov_u.shape == (7, 7) and np.all(np.linalg.eigvalsh(r.cov_u) > 0)
    assert np.isfinite(r.log_evidence) and r.log_evidence_err > 0 and r.information > 0
    assert abs(np.sum(np.exp(r.log_weights)) - 1) < 1e-9 and r.n_evals == 64 + 32 * r.n_iter * 21
    assert np.all(r.params >= lo * (1 - 1e-12)) and np.all(r.params <= hi * (1 + 1e-12))
    assert r.log_evidence < r.lnl.max() and 0.05 < r.accept_rate[0] < 0.9
    tp = ae.sample_tempered(spectra[1], 5.0, n_ladders=4, n_steps=200, n_warmup=100, thin=0, p0=truths[1])
    print("NESTED class surface: ln Z %.3f +- %.3f (H %.2f, %d iterations, accept %.2f); sample_tempered's trapezoid %.3f +- %.3f"
          % (r.log_evidence, r.log_evidence_err, r.information, r.n_iter, r.accept_rate[0], tp.log_evidence, tp.log_evidence_err))
    again = ae.nested_sample(spectra[1], 5.0, n_live=64, dlogz=0.05, seed=2)
    assert same(again.params, r.params) and same(again.log_weights, r.log_weights) and again.log_evidence == r.log_evidence
    # the iteration limit, reported; two runs; two spectra; no ln L asked for
    r2 = ae.nested_sample(spectra, 1.0, n_live=64, n_runs=2, max_iter=8, seed=2, return_lnl=False)
    assert r2.stopped == "max_iter" and r2.n_iter == 8 and r2.lnl is None
    assert r2.params.shape == (2, 2, 8 * 32 + 64, 7) and r2.log_weights.shape == (2, 2, 8 * 32 + 64) and r2.accept_rate.shape == (2, 2)
    assert r2.log_evidence.shape == (2,) and np.all(r2.log_evidence_err > 0) and r2.mean_u.shape == (2, 7) and r2.cov_u.shape == (2, 7, 7)
    np.testing.assert_allclose(np.exp(r2.log_weights).reshape(2, -1).sum(axis=1), 1.0, atol=1e-9)
    assert hasattr(emulator.DirectEmulator(**data), "nested_sample")
    with pytest.raises(ValueError):
        ae.nested_sample(np.zeros(450), 1.0)
    with pytest.raises(ValueError):
        ae.nested_sample(spectra[0], 1.0, n_live=48)
    with pytest.raises(ValueError):
        ae.nested_sample(spectra[0], 1.0, n_runs=0)
