"""Fisher matrices and fits, host side: the Python inverse of par_transform, the float64 LM reference (tests/fit_ref.py)
on a small random stack (against scipy's bounded least squares when scipy imports), the new ABI symbols, and argument
checks of the Python surface and the C entry points that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fit_ref as fr
import jacobian_ref as jr
from conftest import ROOT, pkg
from helpers import init_weights

NEW_SYMBOLS = ("v21_mlp_fisher", "v21_mlp_fisher_dev", "v21_mlp_fit", "v21_mlp_fit_dev")


def train_params(seed=5):
    return pkg("synth").make_params(2000, seed=seed, corners=True)


def test_untransform_round_trips_par_transform():
    pp = pkg("preprocess")
    pt = train_params()
    assert np.any(pt[:, 2] == 0)  # the training set holds fx == 0: the fx column's lower bound is the floor
    ps = pp.ParamStats.of(pt)
    x = pkg("synth").make_params(500, seed=9, zero_fx_frac=0.05)
    u = pp.par_transform(x, pt)
    back = pp.par_untransform(u, pt)
    floor = x[:, 2] == 0
    assert floor.any()
    ref = x.copy()
    ref[floor, 2] = 1e-6  # fx == 0 comes back as the floor
    np.testing.assert_allclose(back, ref, rtol=8 * np.finfo(np.float64).eps, atol=0)
    # the other way: u -> raw -> u, to float64 rounding; float32 rows within one ulp of float32
    rng = np.random.default_rng(3)
    u = rng.uniform(-1, 1, size=(400, 7))
    u[:7] = np.eye(7) * 2 - 1  # every column on both bounds
    u2 = pp.par_transform(pp.par_untransform(u, pt), pt)
    assert np.max(np.abs(u2 - u)) <= 8 * np.finfo(np.float64).eps
    # float32 rows (par_transform's float32 branch: float32 floor, log10 rounded to float32) come back within one float32
    # ulp of what that branch emulates: the value of a linear column, the float32 log10 of a log column
    x32 = x.astype(np.float32)
    back32 = pp.par_untransform(pp.par_transform(x32, pt), pt)
    ref32 = x32.astype(np.float64)
    ref32[floor, 2] = np.float32(1e-6)
    lm = np.asarray(ps.log_mask)
    lg32 = np.log10(ref32[:, lm].astype(np.float32))
    assert np.all(np.abs(np.log10(back32[:, lm]) - lg32) <= np.spacing(np.abs(lg32)))
    assert np.all(np.abs(back32[:, ~lm] - ref32[:, ~lm]) <= np.spacing(np.abs(ref32[:, ~lm]).astype(np.float32)))
    # the lower bound of a log column is 10^lo: the floor for fx, never 0
    lower = pp.par_untransform(-np.ones(7), pt)[0]
    assert lower[2] == 10.0 ** ps.lo[2] and abs(lower[2] - 1e-6) <= 1e-6 * 1e-12
    np.testing.assert_array_equal(pp.par_untransform(u, pt), fr.untransform(u, ps.log_mask, ps.lo, ps.hi))


def small_problem(seed=4):
    dims, act = [7, 24, 32, 40], [1, 1, 0]
    Ws, bs, _ = init_weights(dims, seed)
    return dims, act, Ws, bs


def test_lm_ref_recovers_a_truth_inside_the_box():
    dims, act, Ws, bs = small_problem()
    rng = np.random.default_rng(7)
    hits = 0
    for t in range(4):
        u_true = rng.uniform(-0.7, 0.7, size=7)
        data = jr.forward(Ws, bs, act, u_true[None, :])[0]
        w = np.full(dims[-1], 1.0 / 0.01 ** 2)
        ev = fr.evaluator(Ws, bs, act, data, w)
        r = fr.lm_ref(ev, np.zeros(7), max_iter=200)
        assert r["lnl"] >= r["lnl0"]
        assert r["status"] in (0, 1, 2)
        if r["lnl"] > -1e-10:
            hits += 1
            # noiseless data: the truth is a maximum with ln L = 0; a well-conditioned problem recovers it
            F = ev(r["u"])[2]
            if np.linalg.cond(F) < 1e6:
                np.testing.assert_allclose(r["u"], u_true, atol=1e-4)
    assert hits >= 3, hits


def test_lm_ref_agrees_with_scipy_least_squares():
    opt = pytest.importorskip("scipy.optimize")
    dims, act, Ws, bs = small_problem(6)
    rng = np.random.default_rng(8)
    u_true = rng.uniform(-0.5, 0.5, size=7)
    sig = 0.02
    data = jr.forward(Ws, bs, act, u_true[None, :])[0] + rng.normal(size=dims[-1]) * sig
    w = np.full(dims[-1], 1.0 / sig ** 2)
    ev = fr.evaluator(Ws, bs, act, data, w)
    r = fr.lm_ref(ev, np.zeros(7), max_iter=300, xtol=1e-10)

    def resid(u):
        return (jr.forward(Ws, bs, act, u[None, :])[0] - data) / sig

    def jac(u):
        _, J, _ = jr.jvp(Ws, bs, act, u[None, :])
        return J[0].T / sig

    ls = opt.least_squares(resid, np.zeros(7), jac=jac, bounds=(-1.0, 1.0), xtol=1e-14, ftol=1e-14, gtol=1e-14)
    lnl_ls = -0.5 * np.sum(ls.fun ** 2)
    # the same optimum: ln L at least scipy's (its trust region stops a little short on this problem: 1e-4 relative),
    # and the point where the optimum is well conditioned
    assert r["lnl"] >= lnl_ls - 1e-9 * abs(lnl_ls) and abs(r["lnl"] - lnl_ls) <= 1e-3 * abs(lnl_ls), (r["lnl"], lnl_ls)
    if np.linalg.cond(ev(r["u"])[2]) < 1e6:
        np.testing.assert_allclose(r["u"], ls.x, atol=1e-2)


def test_lm_ref_edge_rules():
    dims, act, Ws, bs = small_problem()
    data = jr.forward(Ws, bs, act, np.full((1, 7), 0.2))[0]
    # no information: every weight zero -> status 3, the clamped start kept
    ev = fr.evaluator(Ws, bs, act, data, np.zeros(dims[-1]))
    r = fr.lm_ref(ev, np.full(7, 3.0))
    assert r["status"] == 3 and np.array_equal(r["u"], np.ones(7)) and r["lnl"] == 0.0 and r["iters"] == 0
    # max_iter = 0: the start is the result
    ev = fr.evaluator(Ws, bs, act, data, np.ones(dims[-1]))
    r = fr.lm_ref(ev, np.full(7, -0.3), max_iter=0)
    assert np.array_equal(r["u"], np.full(7, -0.3)) and r["lnl"] == r["lnl0"]


def test_new_symbols_declared_and_bound():
    nat = pkg("_native")
    src = open(os.path.join(ROOT, "include", "v21.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in nat.SIGNATURES, name
    types = open(os.path.join(ROOT, "include", "v21_types.h")).read()
    assert "v21_fit_opts" in types
    assert C.sizeof(nat.FitOpts) == 32  # int, double, double, int: the C layout
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("library not built")
    lib = nat.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    # null arguments are refused before any device work
    assert lib.v21_mlp_fisher(None, None, 0, 1, None, None, None, 0, 0) == -1
    assert lib.v21_mlp_fit(None, None, 0, 1, None, 0, None, None, None, None, None, None, 0, 0) == -1
    assert lib.v21_mlp_fit_dev(None, None, 7, 1, None, 0, None, None, None, None, None, None, 0, 0) == -1
    assert lib.v21_mlp_fisher_dev(None, None, 7, 1, None, None, None, 0, 0) == -1


def _hostless_stack(dims):
    """a Stack object without a device handle: argument checks that run before the library is called"""
    nat = pkg("_native")
    st = nat.Stack.__new__(nat.Stack)
    st.dims, st.act = list(dims), [1] * (len(dims) - 2) + [0]
    st.lib, st.ctx, st.h = None, None, None
    return st


def test_python_surface_validates_arguments():
    st = _hostless_stack([7, 16, 451])
    x = np.zeros((6, 7))
    with pytest.raises(ValueError):
        st.fit(np.zeros((6, 5)))                       # wrong parameter count
    with pytest.raises(ValueError):
        st.fit(x, data=np.zeros((4, 451)))             # 6 rows over 4 spectra
    with pytest.raises(ValueError):
        st.fit(x, data=np.zeros((3, 450)))             # wrong bin count
    with pytest.raises(ValueError):
        st.fisher(np.zeros((2, 6)))
    wide = _hostless_stack([9, 16, 451])
    with pytest.raises(ValueError):
        wide.fit(np.zeros((2, 9)))                     # fits: at most 8 parameters
    o = st.fit_opts(max_iter=3)
    assert (o.max_iter, o.lambda0, o.xtol, o.check_every) == (3, 1e-3, 1e-7, 8)
