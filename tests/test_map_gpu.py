"""MAP fits with held parameters and the Laplace evidence on the GPU (include/v21.h: v21_mlp_fit_map[_dev]): one iteration
rebuilt in float64 from the device's own evaluation, the fit against tests/map_ref.py, the Laplace outputs against the
reference's formulas at the device's own point, what must not have moved, the edges, and the class surface."""
import ctypes as C
import math

import numpy as np
import pytest

import infer_cases as ic
import map_ref as mp
from conftest import pkg
from infer_support import POISON_BYTE, device_eval, device_stack, fit_setup, flags_of, new_stack, run_dev, same, shape_setup, u_of

pytestmark = pytest.mark.gpu
fr, pr, jr = mp.fr, mp.pr, mp.fr.jr

# |device laplace - the reference's formula in float64 at the device's own point| over the cases of
# test_laplace_outputs_against_reference_formulas (NB, i1, i2 in f32, 5 rows each).  Measured on the MI355X: worst 4.5e-5
# (NB; i2 1.4e-5, i1 2.6e-6); the bound is 4 x that, and far below a quarter of the smallest shift a control of
# tests/test_map_cpu.py makes (0.82 / 4 = 0.21).
LAPLACE_TOL = 1.8e-4
SMALLEST_CONTROL_SHIFT = 0.82
ROWS = (1, 5, 257)  # one row, a partial workgroup, one past a 256-thread workgroup


def untransform(u, tin):
    return fr.untransform(np.asarray(u, np.float64), tin[0], tin[2], tin[3])


def device_u(x_hat, tin):
    """the float32 u the device holds behind float64 raw rows it mapped back, exactly"""
    return u_of(x_hat, tin).astype(np.float32).astype(np.float64)


def small_setup(ctx, name):
    """the 1- or 2-input quadrature problem of infer_cases on the device -> (stack handle, problem, tin)"""
    p = ic.problem(name)
    st, rec = device_stack(ctx, p["dims"], p["act"])
    st.set_likelihood(p["data"], p["w"])
    return st, p, rec["tin"]


def setup(ctx, which):
    """-> (stack, tin, d, a centre in u, data matrix or None, evaluator factory row -> float64 ev) of a named stack (D1,
    NB: fit_setup's spectra), a stack of shape_cases (i8o64) or a quadrature problem (i1, i2); the record is set"""
    if which in ("D1", "NB"):
        st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, which, seed=5, m=2)
        return st, tin, 7, u_of(truths[:1], tin)[0], data[:1], lambda: fr.evaluator(Ws, bs, act, data[0], w, tout)
    if which in ("i1", "i2"):
        st, p, tin = small_setup(ctx, which)
        return st, tin, p["dims"][0], p["truth_u"], None, lambda: mp.single(p["ev"])
    st, rec, prob, _ = shape_setup(ctx, which)
    return (st, rec["tin"], rec["dims"][0], prob["truths_u"][0], None,
            lambda: fr.evaluator(rec["Ws"], rec["bs"], rec["act"], prob["data"][0], prob["w"], rec["tout"]))


def tin_of(p):
    """the input transform of a quadrature problem's stack"""
    return p["stack"]["tin"]


def starts_around(centre, n, seed, scale):
    return np.clip(centre[None, :] + scale * np.random.default_rng(seed).normal(size=(n, centre.size)), -0.95, 0.95)


def clamped_start_u(st, nat, x0, prec):
    """the float32 u of the clamped starts as the device holds them (a sample call of no transition hands them out)"""
    return st.sample(x0, prec, flags_of(nat, True), n_steps=0, n_warmup=0, diagnostics=True)["last_prop_u"].astype(np.float64)


def hold_of(d, *cols):
    h = np.zeros(d, bool)
    h[list(cols)] = True
    return h


# ---- 1. one iteration rebuilt from the device's own evaluation
@pytest.mark.parametrize("which,held", [("D1", 2), ("i8o64", 4)])
@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
def test_one_iteration_rebuilt(ctx, which, held, prec):
    """max_iter = 1 under the mixed record (a mode 2 sd outside the box) with one column held -- D1: a uniform column;
    i8o64: the normal column with the outside mode, whose prior then must not be read"""
    nat = pkg("_native")
    st, tin, d, centre, data, _ = setup(ctx, which)
    flags = flags_of(nat, True)
    prior, hold = ic.mixed_prior(d), hold_of(d, held)
    pf = mp.free_prior(prior, hold, True)
    lam0, accepted = 1e-3, 0
    st.set_prior(*prior)
    try:
        for n in ROWS:
            x0 = untransform(starts_around(centre, n, 31 + n, 0.1), tin)
            x0[0, 0] = x0[0, 0] * 1e3  # (a start outside the box: clamped)
            u0 = clamped_start_u(st, nat, x0, prec)
            r0 = st.fit_map(x0, prec, flags, data=data, max_iter=0, use_prior=True, hold=hold)
            r = st.fit_map(x0, prec, flags, data=data, max_iter=1, lambda0=lam0, use_prior=True, hold=hold)
            assert np.allclose(device_u(r0["x_hat"], tin), u0, rtol=0, atol=0), "the clamped start"
            # the proposal in float64 from the device's ln L, gradient and Fisher matrix at the start
            e0 = device_eval(st, nat, u0, prec)
            prop = np.empty_like(u0)
            stepped = np.zeros(n, bool)
            for i in range(n):
                _, _, g, A = mp.system(lambda u: (e0[0][i], e0[1][i], e0[2][i]), pf, hold, u0[i])
                lam, delta = lam0 / 10.0, None
                while delta is None:
                    delta = fr.lm_solve(A, g, lam)
                    lam *= 10.0
                un = np.clip(u0[i] + delta, -1.0, 1.0).astype(np.float32).astype(np.float64)
                un[hold] = u0[i][hold]
                stepped[i] = np.max(np.abs(un - u0[i])) > 1e-7
                prop[i] = un
            # the decision in float64 from the device's ln L at that proposal
            e1 = device_eval(st, nat, prop, prec)
            rose = e1[0] + pr.log_prior(pf, prop) > e0[0] + pr.log_prior(pf, u0)
            accept_ref = stepped & rose
            accept_dev = np.array([not same(r["x_hat"][i], r0["x_hat"][i]) for i in range(n)])
            print("%s %s n=%d: stepped %d, accepted %d (device %d)" % (which, prec, n, stepped.sum(), accept_ref.sum(), accept_dev.sum()))
            assert np.array_equal(accept_dev, accept_ref), (which, prec, n, np.flatnonzero(accept_dev != accept_ref))
            uh = u_of(r["x_hat"], tin)
            tol = np.spacing(np.abs(prop).astype(np.float32)).astype(np.float64) + 1e-12
            err = np.abs(uh - prop)[accept_ref]
            assert np.all(err <= tol[accept_ref]), (which, prec, n, np.max(err / tol[accept_ref]))
            # held coordinates: the start's, bit for bit; ln L stays ln L, ln p is that of the free normal columns
            assert same(r["x_hat"][:, hold], r0["x_hat"][:, hold])
            np.testing.assert_allclose(r["lnl"], np.where(accept_ref, e1[0], e0[0]), rtol=1e-5)
            np.testing.assert_allclose(r["lnp"], pr.log_prior(pf, device_u(r["x_hat"], tin)), rtol=1e-12, atol=1e-300)
            accepted += int(accept_ref.sum())
        assert accepted >= 8, "the accepted branch is exercised"
    finally:
        st.set_prior(None)
        st.set_likelihood(None, None)


# ---- 2. and 3. against map_ref
_ref_cases = {}


def reference_cases(ctx, which):
    """the f32 fit_map of a few starts of one problem under its prior with the reference's run of every row; once"""
    if which not in _ref_cases:
        nat = pkg("_native")
        st, tin, d, centre, data, make_ev = setup(ctx, which)
        if which == "NB":  # two normal columns inside the box, one uniform column held
            kind, mu, sd = np.zeros(7, np.int32), np.zeros(7), np.ones(7)
            kind[[1, 4]], mu[[1, 4]], sd[[1, 4]] = 1, centre[[1, 4]] + 0.1, 0.1
            prior, hold = pr.as_prior(kind, mu, sd), hold_of(7, 2)
            us = starts_around(centre, 5, 12, 0.1)
        else:
            prior, hold = ic.evidence_prior(which), hold_of(d)
            us = np.vstack([np.zeros((1, d)), starts_around(centre, 4, 13, 0.2)])
        x0 = untransform(us, tin)
        st.set_prior(*prior)
        try:
            r = st.fit_map(x0, "f32", flags_of(nat, True), data=data, max_iter=40, use_prior=True, hold=hold)
            r_flat = st.fit_map(x0, "f32", flags_of(nat, True), data=data, max_iter=40, use_prior=False, hold=hold)
        finally:
            st.set_prior(None)
            st.set_likelihood(None, None)
        ev = make_ev()
        u0 = u_of(x0, tin).astype(np.float32).astype(np.float64)
        _ref_cases[which] = dict(tin=tin, d=d, prior=prior, hold=hold, ev=ev, r=r, r_flat=r_flat, u0=u0,
                                 refs=[mp.map_ref(ev, prior, u, hold, True, max_iter=40) for u in u0])
    return _ref_cases[which]


@pytest.mark.parametrize("which", ["NB", "i1", "i2"])
def test_fit_map_against_map_ref(ctx, which):
    c = reference_cases(ctx, which)
    r, ud = c["r"], u_of(c["r"]["x_hat"], c["tin"])
    compared = 0
    for i, ref in enumerate(c["refs"]):
        obj = float(r["lnl"][i]) + r["lnp"][i]
        tol = 1e-4 * max(1.0, abs(ref["obj"]))
        assert obj >= ref["obj"] - tol, (which, i, obj, ref["obj"], r["status"][i], ref["status"])
        free = ~c["hold"]
        A = ref["prec_u"][np.ix_(free, free)]
        if ref["status"] == 1 and np.all(np.abs(ref["u"][free]) < 1 - 1e-3) and np.linalg.cond(A) < 1e6:
            np.testing.assert_allclose(ud[i], ref["u"], atol=1e-4, rtol=0, err_msg="%s row %d" % (which, i))
            compared += 1
    assert compared >= 1, which
    if which == "i1":  # the prior is read: without it the optimum is 1e-2 away
        moved = np.abs(u_of(c["r_flat"]["x_hat"], c["tin"]) - ud)[:, 0]
        print("i1: the prior moves the optimum by", moved)
        assert np.all(moved > 5e-3)


@pytest.mark.parametrize("which", ["NB", "i1", "i2"])
def test_laplace_outputs_against_reference_formulas(ctx, which):
    """laplace, lnp and prec_u against map_ref's formulas in float64 AT THE DEVICE'S OWN POINT: what is left is the float32
    evaluation of ln L and F alone"""
    c = reference_cases(ctx, which)
    r, hold = c["r"], c["hold"]
    uh = device_u(r["x_hat"], c["tin"])
    worst = 0.0
    for i in range(uh.shape[0]):
        f = mp.laplace_at(c["ev"], c["prior"], uh[i], hold, True)
        assert abs(r["lnp"][i] - f["lnp"]) <= 1e-12 * abs(f["lnp"]), (which, i, r["lnp"][i], f["lnp"])
        P = r["prec_u"][i]
        assert same(P, P.T.copy()), "exactly symmetric"
        eye = np.eye(c["d"], dtype=np.float32)
        assert same(P[hold], eye[hold]) and same(P[:, hold], eye[:, hold]), "held rows and columns: the identity's"
        eA = np.linalg.norm(P.astype(np.float64) - f["prec_u"]) / np.linalg.norm(f["prec_u"])
        assert eA <= 1e-5, (which, i, eA)  # (the Fisher reductions' bound, tests/infer_support.py: check_reduction)
        d = abs(r["laplace"][i] - f["laplace"])
        print("%s row %d: |laplace - formula| %.2e, |A - formula| / |A| %.2e, status %d" % (which, i, d, eA, r["status"][i]))
        assert np.isfinite(r["laplace"][i])
        worst = max(worst, d)
    print("%s: worst |laplace - formula| %.3e (bound %.1e)" % (which, worst, LAPLACE_TOL))
    assert LAPLACE_TOL < SMALLEST_CONTROL_SHIFT / 4.0
    assert worst <= LAPLACE_TOL, (which, worst)
    if which == "i1":  # the evidence as the emulator classes define it, against the quadrature
        lz = r["laplace"] - (pr.log_norm(c["prior"]) + c["d"] * math.log(2.0))
        q = ic.evidence_quadrature("i1")[0]
        print("i1: log evidence - quadrature", lz - q)
        assert np.all(np.abs(lz - q) <= 1e-3)


# ---- 4. nothing else moved
FIT_SHAPES = lambda n, d: {"x_hat": ((n, d), np.float32), "lnl": ((n,), np.float32), "lnl_start": ((n,), np.float32),
                           "fisher": ((n, d, d), np.float32), "status": ((n,), np.int32), "lnp": ((n,), np.float64),
                           "laplace": ((n,), np.float64), "prec_u": ((n, d, d), np.float32)}
FIT_KEYS = ("x_hat", "lnl", "lnl_start", "fisher", "status")


def fit_dev(ctx, st, x0, data, prec, flags, keys, map_call, guard=64, ask=None, **kw):
    """v21_mlp_fit_dev (map_call False) or v21_mlp_fit_map_dev on float32 rows -> the buffers `keys`, poisoned before the
    call; ask: the nullable outputs handed to the library (None: all of `keys`), the others stay NULL"""
    n, d = x0.shape

    def call(dx, dd, bufs):
        out = {k: v for k, v in bufs.items() if ask is None or k in ask or k in ("x_hat", "lnl")}
        args = (dx, d, n, dd, 0 if data is None else data.shape[0], out["x_hat"], out["lnl"], out.get("lnl_start"), out.get("fisher"),
                out.get("status"))
        if map_call:
            st.fit_map_dev(*args, out={k: out[k] for k in ("lnp", "laplace", "prec_u") if k in out}, precision=prec, flags=flags, **kw)
        else:
            st.fit_dev(*args, prec, flags, **kw)
    return run_dev(ctx, FIT_SHAPES(n, d), keys, call, x0, data, guard)


@pytest.mark.parametrize("which,prec", [("D1", "f16"), ("NB", "f32")])
def test_without_prior_and_holds_it_is_the_fit(ctx, which, prec):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, truths, data, w = fit_setup(ctx, which, seed=5, m=2)
    flags = flags_of(nat, True)
    x0 = pkg("synth").make_params(8, seed=21, zero_fx_frac=0)
    x32 = np.ascontiguousarray(x0.astype(np.float32))
    try:
        before = (st.fisher(x0, prec, flags), st.loglike(x0, prec, flags))
        want = st.fit(x0, prec, flags, data=data, max_iter=12, fisher=True)
        for kw in (dict(), dict(use_prior=True)):  # (use_prior without a record: the uniform prior)
            got = st.fit_map(x0, prec, flags, data=data, max_iter=12, fisher=True, **kw)
            for k in want:
                assert same(got[k], want[k]), (which, k, kw)
            assert np.all(got["lnp"] == 0.0)
        # the record set but not asked for: still the fit
        st.set_prior(*ic.mixed_prior(7))
        got = st.fit_map(x0, prec, flags, data=data, max_iter=12, fisher=True, use_prior=False)
        st.set_prior(None)
        for k in want:
            assert same(got[k], want[k]), (which, k, "record not asked for")
        # the _dev forms
        wd = fit_dev(ctx, st, x32, data, prec, flags, FIT_KEYS, False, max_iter=12)
        gd = fit_dev(ctx, st, x32, data, prec, flags, FIT_KEYS + ("lnp", "laplace", "prec_u"), True, max_iter=12)
        for k in FIT_KEYS:
            assert same(gd[k], wd[k]), (which, k, "_dev")
        want32 = st.fit(x32, prec, flags, data=data, max_iter=12, fisher=True)
        for k in FIT_KEYS:
            assert same(wd[k], want32[k]), (which, k, "_dev against the host form")
        # rows do not depend on how a call is split, the MAP outputs included
        prior, hold = ic.mixed_prior(7), hold_of(7, 5)
        st.set_prior(*prior)
        whole = st.fit_map(x0, prec, flags, data=data, max_iter=12, fisher=True, use_prior=True, hold=hold)
        for k in range(2):
            part = st.fit_map(x0[4 * k:4 * k + 4], prec, flags, data=data[k:k + 1], max_iter=12, fisher=True, use_prior=True, hold=hold)
            for key in whole:
                assert same(part[key], whole[key][4 * k:4 * k + 4]), (which, k, key)
        assert not same(whole["x_hat"], want["x_hat"]), "the prior and the mask are read"
        st.set_prior(None)
        # after fit_map calls, fit, fisher and loglike return what they returned before
        again = st.fit(x0, prec, flags, data=data, max_iter=12, fisher=True)
        for k in want:
            assert same(again[k], want[k]), (which, k, "fit after fit_map")
        after = (st.fisher(x0, prec, flags), st.loglike(x0, prec, flags))
        assert same(after[0], before[0]) and all(same(a, b) for a, b in zip(after[1], before[1]))
    finally:
        st.set_prior(None)
        st.set_likelihood(None, None)


def test_host_chunks_do_not_move_rows(ctx):
    """8,200 rows of the 2-input problem in the host form: two chunks; rows on both sides of the chunk boundary equal a
    call of their own, every output"""
    nat = pkg("_native")
    st, p, tin = small_setup(ctx, "i2")
    flags = flags_of(nat, True)
    prior, hold = ic.evidence_prior("i2"), hold_of(2, 1)
    n = 8200
    x0 = untransform(starts_around(p["truth_u"], n, 3, 0.2), tin)
    st.set_prior(*prior)
    try:
        whole = st.fit_map(x0, "f32", flags, max_iter=10, fisher=True, use_prior=True, hold=hold)
        for lo, hi in ((0, 5), (8188, 8200)):
            part = st.fit_map(x0[lo:hi], "f32", flags, max_iter=10, fisher=True, use_prior=True, hold=hold)
            for key in whole:
                assert same(part[key], whole[key][lo:hi]), (lo, key)
        assert np.all(np.isfinite(whole["laplace"]))
    finally:
        st.set_prior(None)
        st.set_likelihood(None, None)


def arrays_of(r):
    """the arrays of a host form's result (an array, a tuple or a dict of them), in a fixed order"""
    if isinstance(r, dict):
        return [r[k] for k in sorted(r)]
    return list(r) if isinstance(r, tuple) else [r]


def test_host_forms_share_one_chunk_buffer(ctx):
    """One handle of the 2-input problem takes the host forms in turn -- few rows, then two chunks (a regrow of the chunk
    buffer), few rows again, the nested sampler's per-run slots in between: every result is bit-equal to the same call on a
    handle of its own that has staged nothing before, and the Jacobian of the first call to that of the last"""
    nat = pkg("_native")
    p = ic.problem("i2")
    flags = flags_of(nat, True)
    few = untransform(starts_around(p["truth_u"], 5, 4, 0.2), tin_of(p))
    many = untransform(starts_around(p["truth_u"], 8193, 5, 0.2), tin_of(p))
    calls = [lambda st: st.jacobian(few, "f32", flags, return_outputs=True),
             lambda st: st.fit_map(many, "f32", flags, max_iter=4, fisher=True),
             lambda st: st.loglike(few, "f32", flags),
             lambda st: st.sample_nested(None, 16, 16, "f32", nat.FWD_OUT_TRANSFORM, diagnostics=True, n_iter=2, seed=9),
             lambda st: st.fisher(few, "f32", flags, lnl=True, grad=True),
             lambda st: st.loglike_fwd(many, "f32", flags),
             lambda st: st.jacobian(few, "f32", flags, return_outputs=True)]

    def handle():
        st = new_stack(ctx, p["dims"], p["act"])
        st.set_likelihood(p["data"], p["w"])
        return st

    one = handle()
    got = [arrays_of(call(one)) for call in calls]
    for i, call in enumerate(calls):
        alone = arrays_of(call(handle()))
        assert len(alone) == len(got[i]) and all(a.size > 0 and same(a, b) for a, b in zip(got[i], alone)), i
    assert all(same(a, b) for a, b in zip(got[0], got[-1]))
    assert all(np.all(np.isfinite(a)) for a in got[0])


# ---- 5. edges
def test_edges(ctx):
    nat = pkg("_native")
    st, p, tin = small_setup(ctx, "i2")
    flags = flags_of(nat, True)
    prior = ic.mixed_prior(2)  # (column 0: mu 0.3; column 1: mu -1.4, outside the box)
    x0 = untransform(np.array([[0.3, 1.7], [-0.2, 0.1], [0.0, 0.0]]), tin)
    try:
        st.set_prior(*prior)
        # every column held: the clamped start, status 1, no iteration (lnl = lnl_start), d_free = 0: laplace = ln L
        r = st.fit_map(x0, "f32", flags, use_prior=True, hold=[1, 1])
        r0 = st.fit_map(x0, "f32", flags, max_iter=0)
        assert np.all(r["status"] == 1) and same(r["x_hat"], r0["x_hat"]) and same(r["lnl"], r["lnl_start"])
        assert np.all(r["lnp"] == 0.0) and np.array_equal(r["laplace"], r["lnl"].astype(np.float64))
        assert same(r["prec_u"], np.broadcast_to(np.eye(2, dtype=np.float32), (3, 2, 2)).copy())
        assert np.max(np.abs(u_of(r["x_hat"], tin) - np.clip(u_of(x0, tin), -1, 1))) <= 1e-6
        # all-zero weights: under a normal column the prior's mode, clamped into the box; without a prior no information
        st.set_likelihood(p["data"], np.zeros_like(p["w"]))
        r = st.fit_map(x0, "f32", flags, use_prior=True)
        assert np.all(r["status"] != 3), r["status"]
        np.testing.assert_allclose(u_of(r["x_hat"], tin), np.broadcast_to(np.clip(prior[1], -1.0, 1.0), (3, 2)), atol=1e-6, rtol=0)
        r = st.fit_map(x0, "f32", flags, use_prior=True, hold=[1, 0])  # (column 0 held: column 1 still moves to its mode)
        assert np.all(r["status"] != 3) and same(r["x_hat"][:, 0], r0["x_hat"][:, 0])
        np.testing.assert_allclose(u_of(r["x_hat"], tin)[:, 1], -1.0, atol=1e-6, rtol=0)
        rf, rm = st.fit(x0, "f32", flags), st.fit_map(x0, "f32", flags, use_prior=False)
        assert np.all(rf["status"] == 3) and np.all(rm["status"] == 3) and same(rm["x_hat"], rf["x_hat"])
        assert np.all(np.isnan(rm["laplace"])), "no positive pivot: no Laplace value"
        st.set_likelihood(p["data"], p["w"])
        # an output that is not asked for is not written, nor is anything behind one that is
        x32 = np.ascontiguousarray(x0.astype(np.float32))
        got = fit_dev(ctx, st, x32, None, "f32", flags, ("x_hat", "lnl", "lnp", "laplace", "prec_u", "status"), True, guard=256,
                      ask=("lnp",), use_prior=True, max_iter=5)
        full = st.fit_map(x32, "f32", flags, use_prior=True, max_iter=5)
        assert same(got["lnp"], full["lnp"]) and same(got["x_hat"], full["x_hat"]) and same(got["lnl"], full["lnl"])
        for k in ("laplace", "prec_u", "status"):
            assert np.all(got[k].view(np.uint8) == POISON_BYTE), k
        # a bad hold entry or use_prior: V21_ERR_ARG, the handle usable afterwards
        lib, P, F = st.lib, C.c_void_p, C.POINTER(C.c_float)
        xh, lnl = np.empty_like(x32), np.empty(3, np.float32)

        def raw_call(mo):
            return lib.v21_mlp_fit_map(st.h, x32.ctypes.data_as(P), 0, 3, None, 0, None, C.byref(mo), xh.ctypes.data_as(P), lnl.ctypes.data_as(F),
                                       None, None, None, None, 0, flags)
        hold8 = lambda *v: (C.c_int * 8)(*v)
        assert raw_call(nat.MapOpts(2, hold8())) == -1
        assert raw_call(nat.MapOpts(-1, hold8())) == -1
        assert raw_call(nat.MapOpts(1, hold8(0, 2))) == -1
        assert raw_call(nat.MapOpts(0, hold8(0, 0, 0, 0, 0, 0, 0, -1))) == -1  # (all 8 entries are checked)
        assert raw_call(nat.MapOpts(1, hold8(0, 1))) == 0
        ok = st.fit_map(x32, "f32", flags, use_prior=True, hold=[0, 1])
        assert same(xh, ok["x_hat"]) and same(lnl, ok["lnl"])
    finally:
        st.set_prior(None)
        st.set_likelihood(None, None)


# ---- 6. the class surface on the shipped model
def test_class_surface(shipped):
    emulator, synth, pp, priors = pkg("emulator"), pkg("synth"), pkg("preprocess"), pkg("priors")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    u_true = np.random.default_rng(4).uniform(-0.4, 0.4, size=(1, 7))
    truth = pp.par_untransform(u_true, ae.par_train)[0]
    spectrum = np.asarray(ae.predict(truth[None]), np.float32).reshape(-1)
    lo, hi = float(np.min(ae.par_train[:, 3])), float(np.max(ae.par_train[:, 3]))
    m_u, s_u = u_true[0, 3] + 0.15, 0.02  # (a tight prior on tau, 0.15 in u above the truth)
    spec = {"tau": ("normal", lo + (m_u + 1.0) * (hi - lo) / 2.0, s_u * (hi - lo) / 2.0)}
    P = priors.Prior(spec, ae.par_train)
    sigma = 50.0
    u_of_params = lambda params: pp.par_transform(np.reshape(params, (-1, 7)), ae.par_train)
    kw = dict(n_starts=4, max_iter=30, seed=1)
    ml = ae.fit_parameters(spectrum, sigma, **kw)
    assert ml.log_prior is None and ml.log_evidence is None and ml.cov_u is None and len(ml) == 7
    mapr = ae.fit_parameters(spectrum, sigma, prior=spec, **kw)
    u_ml, u_map = u_of_params(ml.params)[0], u_of_params(mapr.params)[0]
    print("tau in u: ML %.4f, MAP %.4f, prior mean %.4f" % (u_ml[3], u_map[3], m_u))
    assert abs(u_map[3] - m_u) < abs(u_ml[3] - m_u)
    assert mapr.log_prior == pytest.approx(P.log_density_u(u_map), abs=1e-4 * max(1.0, abs(mapr.log_prior)))
    assert float(mapr.lnl) + mapr.log_prior >= float(ml.lnl) + P.log_density_u(u_ml)
    assert mapr.log_evidence is None and mapr.cov_u is None
    # the prior does not leak into the next call
    again = ae.fit_parameters(spectrum, sigma, **kw)
    assert same(again.params, ml.params) and same(again.lnl, ml.lnl)
    # a held parameter comes back as its value, to float32 rounding in u
    v = lo + 0.6 * (hi - lo)
    fx = ae.fit_parameters(spectrum, sigma, fixed={"tau": v}, return_evidence=True, **kw)
    uv = u_of_params(np.where(np.arange(7) == 3, v, truth))[0, 3]
    assert abs(u_of_params(fx.params)[0, 3] - uv) <= np.spacing(np.float32(abs(uv)))
    assert fx.cov_u.shape == (7, 7) and np.all(fx.cov_u[3] == 0) and np.all(fx.cov_u[:, 3] == 0) and abs(fx.log_prior) <= 1e-12
    assert np.allclose(fx.cov_u, fx.cov_u.T, equal_nan=True) and np.ndim(fx.log_evidence) == 0
    ra = ae.fit_parameters(np.stack([spectrum, spectrum]), sigma, prior=P, fixed={"tau": v}, return_evidence=True, return_all=True, **kw)
    assert ra.params.shape == (2, 4, 7) and ra.log_prior.shape == (2, 4) and ra.log_evidence.shape == (2, 4) and ra.cov_u.shape == (2, 4, 7, 7)
    assert np.all(np.abs(ra.log_prior) <= 1e-12), "a held column's prior is not read"
    # the VALUES of log_prior, log_evidence and cov_u: every start of two spectra under a normal on every column (0.3 wide in
    # u, 0.1 off the truth: F + P is then well conditioned) with tau held, against the stack's own results for the same rows
    stats = pp.ParamStats.of(ae.par_train)
    span = stats.hi - stats.lo
    full = {name: ("lognormal" if j in pp.LOG_COLUMNS else "normal", stats.lo[j] + (u_true[0, j] + 1.1) * span[j] / 2.0, 0.3 * span[j] / 2.0)
            for j, name in enumerate(priors.PAR_LABELS)}
    PF = priors.Prior(full, ae.par_train)
    two, hold = np.stack([spectrum, spectrum]), np.arange(7) == 3
    free = np.flatnonzero(~hold)
    ra = ae.fit_parameters(two, sigma, prior=PF, fixed={"tau": v}, return_evidence=True, return_all=True, **kw)
    model, st, flags, _ = ae._diff_stack(truth[None])
    starts = pp.par_untransform(np.vstack([np.zeros((1, 7)), np.random.default_rng(kw["seed"]).uniform(-1.0, 1.0, size=(3, 7))]), ae.par_train)
    starts[:, 3] = v
    st.use_prior(PF.to_u(ae.par_train))
    try:
        r = st.fit_map(np.ascontiguousarray(np.tile(starts, (2, 1))), model.precision, flags, data=two, max_iter=kw["max_iter"], use_prior=True,
                       hold=hold)
    finally:
        st.use_prior(None)
    norm = PF.log_integral_u(~hold)
    assert same(ra.params.reshape(8, 7), r["x_hat"]) and same(ra.lnl.reshape(8), r["lnl"])
    assert np.all(np.isfinite(ra.log_evidence)) and np.all(np.isfinite(ra.cov_u)) and np.all(np.isfinite(ra.log_prior))
    np.testing.assert_allclose(ra.log_evidence.reshape(8), r["laplace"] - norm, rtol=1e-13, atol=0)
    np.testing.assert_allclose(ra.log_prior.reshape(8), r["lnp"] - norm + 6 * math.log(2.0), rtol=1e-12, atol=1e-12)
    # ... which is Prior.log_density_u of the free columns' prior at the result
    p_free = priors.Prior({k: s for k, s in full.items() if k != "tau"}, ae.par_train)
    np.testing.assert_allclose(ra.log_prior.reshape(8), p_free.log_density_u(u_of_params(ra.params)), rtol=1e-9, atol=1e-9)
    cov = ra.cov_u.reshape(8, 7, 7)
    assert np.all(cov[:, 3, :] == 0) and np.all(cov[:, :, 3] == 0)
    for k in range(8):
        A = r["prec_u"][k].astype(np.float64)[np.ix_(free, free)]
        np.testing.assert_allclose(cov[k][np.ix_(free, free)] @ A, np.eye(6), rtol=0, atol=1e-6, err_msg="row %d" % k)
        assert np.all(np.linalg.eigvalsh(cov[k][np.ix_(free, free)]) > 0)
    # the best start per spectrum (the highest ln L + ln p) carries its own three values
    rb = ae.fit_parameters(two, sigma, prior=PF, fixed={"tau": v}, return_evidence=True, **kw)
    best = np.argmax(r["lnl"].astype(np.float64).reshape(2, 4) + r["lnp"].reshape(2, 4), axis=1)
    i2 = np.arange(2)
    assert same(rb.params, ra.params[i2, best]) and same(rb.log_evidence, ra.log_evidence[i2, best])
    assert same(rb.cov_u, ra.cov_u[i2, best]) and same(rb.log_prior, ra.log_prior[i2, best])
    with pytest.raises(ValueError, match="taus"):
        ae.fit_parameters(spectrum, sigma, fixed={"taus": v})
    with pytest.raises(ValueError, match="tau"):
        ae.fit_parameters(spectrum, sigma, fixed={"tau": hi + (hi - lo)})
    # the samplers' default starts under a prior are the MAP fit: no transition, the chains sit at their jittered starts.
    # Through the class: with no kept transition the device's per-chain mean_u is the chain's current point, so the pooled
    # mean_u is the mean of the 16 starts.  Per chain, through the stack on the class's own start rows: x_last is the start,
    # within 5 sd of the N(0, 0.02^2) jitter of the MAP point in every coordinate (112 draws: 6e-5 to miss by chance)
    run = dict(n_chains=16, n_steps=0, n_warmup=0, seed=1)
    s_map = ae.sample_posterior(spectrum, sigma, prior=spec, **run)
    centre = u_of_params(ae.fit_parameters(spectrum, sigma, seed=1, prior=spec).params)[0]
    print("start - MAP point in u:", s_map.mean_u - centre)
    assert np.all(np.abs(s_map.mean_u - centre) <= 0.02)
    assert abs(s_map.mean_u[3] - m_u) < abs(u_ml[3] - m_u)
    x0 = np.ascontiguousarray(ae._sampler_starts(st, spectrum[None], (16,), None, sigma, None, None, 1, None, P))
    st.use_prior(P.to_u(ae.par_train))
    try:
        x_last = st.sample(x0, model.precision, flags, data=spectrum[None], n_steps=0, n_warmup=0, seed=1)["x_last"]
    finally:
        st.use_prior(None)
    off = u_of_params(x_last) - centre
    print("per chain: max |x_last - MAP point| in u %.4f, rms %.4f" % (np.abs(off).max(), off.std()))
    assert off.shape == (16, 7) and np.all(np.abs(off) <= 5 * 0.02)
    np.testing.assert_allclose(off.mean(axis=0), s_map.mean_u - centre, rtol=0, atol=1e-6)
    # without a prior: what it was, a fit_parameters start
    run = dict(n_chains=16, n_steps=20, n_warmup=10, seed=1)
    a = ae.sample_posterior(spectrum, sigma, **run)
    b = ae.sample_posterior(spectrum, sigma, p0=ae.fit_parameters(spectrum, sigma, seed=1).params, **run)
    assert same(a.params, b.params) and same(a.mean_u, b.mean_u)
