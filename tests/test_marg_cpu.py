"""Marginalised foreground modes, host side: the float64 reference (tests/marg_ref.py) against numpy.linalg.lstsq profiling,
finite differences of its own ln L and the invariance under d += A^T a; v21_nuisance_whiten (include/v21.h; pure host
arithmetic) against numpy.linalg.qr of the weighted basis; the float32 projection at foreground scale; the new ABI
symbols and the argument checks of the Python surface that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import marg_ref as mr
from conftest import pkg
from helpers import init_weights

NEW_SYMBOLS = ("v21_nuisance_whiten", "v21_mlp_set_nuisance", "v21_mlp_nuisance_info", "v21_mlp_nuisance_coef")
NU = np.linspace(50.0, 200.0, 451)  # the shipped grid's band in MHz: 451 bins


def band(lo=50.0, hi=100.0, sigma=20.0, holes=True, seed=1):
    """float32 1 / sigma^2 on [lo, hi] MHz, zero outside and (holes) on a tenth of the bins inside"""
    w = np.where((NU >= lo) & (NU <= hi), 1.0 / sigma ** 2, 0.0)
    if holes:
        w[np.random.default_rng(seed).uniform(size=NU.size) < 0.1] = 0.0
    return w.astype(np.float32)


def small_stack(seed=2):
    dims, act = [4, 24, 16, 40], [1, 1, 0]
    Ws, bs, _ = init_weights(dims, seed)
    return dims, act, Ws, bs


def small_case(K=3, seed=4, amp=1e3):
    dims, act, Ws, bs = small_stack()
    rng = np.random.default_rng(seed)
    nu = np.linspace(60.0, 120.0, dims[-1])
    A = pkg("foregrounds").linlog_basis(nu, K)
    w = np.full(dims[-1], 4.0)
    w[:5] = 0.0
    w[rng.uniform(size=dims[-1]) < 0.1] = 0.0
    data = rng.normal(size=dims[-1]) + amp * rng.normal(size=K) @ A
    return Ws, bs, act, data, w, A, rng


def test_reference_is_the_profile_likelihood():
    Ws, bs, act, data, w, A, rng = small_case()
    ev = mr.evaluator_batch(Ws, bs, act, data, w, A)
    u = rng.uniform(-1, 1, size=(6, 4))
    lnl = ev(u)[0]
    y, J, _ = mr.jr.jvp(Ws, bs, act, u)
    prof, a_hat = mr.profile_lnl(y, data, w, A)
    m = mr.marg(y, J, data, w, A)
    # (both sides are sums of terms of size r^T W r: relative to that)
    assert np.all(np.abs(lnl - prof) <= 1e-10 * m["lnl_scale"]), np.max(np.abs(lnl - prof) / m["lnl_scale"])
    np.testing.assert_allclose(m["coef"], a_hat, rtol=1e-8, atol=1e-8 * np.abs(a_hat).max())
    # the formulas as they read (sums 10^6 times their result here) are the same numbers
    ll, gl = mr.marg_literal(y, J, data, w, A)
    assert np.all(np.abs(ll - lnl) <= 1e-12 * m["lnl_scale"]) and np.all(np.abs(gl - m["grad"]) <= 1e-12 * m["grad_scale"])
    # any other amplitudes do worse
    r = data - y
    for _ in range(3):
        a = a_hat + rng.normal(size=a_hat.shape)
        res = r - a @ A
        assert np.all(-0.5 * np.sum(w * res * res, axis=1) <= lnl + 1e-9)


def test_reference_gradient_and_fisher_against_finite_differences():
    # (a foreground of the signal's size: a central difference of float64 sums 10^6 times their result would be noise)
    Ws, bs, act, data, w, A, rng = small_case(amp=1.0)
    ev = mr.evaluator(Ws, bs, act, data, w, A)
    u = rng.uniform(-0.8, 0.8, size=4)
    lnl, g, F = ev(u)
    h = 1e-6
    fd = np.array([(ev(u + h * e)[0] - ev(u - h * e)[0]) / (2 * h) for e in np.eye(4)])
    np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-5 * np.abs(g).max())
    # F_m = J C J^T with C = W - W Q^T Q W: symmetric, positive semi-definite, and below J W J^T
    y, J, _ = mr.jr.jvp(Ws, bs, act, u[None, :])
    Q, _ = mr.whiten(A, w)
    Cm = np.diag(w) - np.diag(w) @ Q.T @ Q @ np.diag(w)
    np.testing.assert_allclose(F, J[0] @ Cm @ J[0].T, rtol=1e-10, atol=1e-10 * np.abs(F).max())
    assert np.all(np.linalg.eigvalsh(F) >= -1e-9 * np.abs(F).max())
    F0 = (J[0] * w) @ J[0].T
    assert np.all(np.linalg.eigvalsh(F0 - F) >= -1e-9 * np.abs(F0).max())
    # the batch form is the single form
    evb = mr.evaluator_batch(Ws, bs, act, data, w, A)
    lb, gb, Fb = evb(np.stack([u, -u]))
    np.testing.assert_allclose([lb[0]], [lnl], rtol=1e-13)
    np.testing.assert_allclose(gb[0], g, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(Fb[0], F, rtol=1e-12, atol=1e-12)


def test_reference_invariant_under_foreground_shift():
    Ws, bs, act, data, w, A, rng = small_case()
    u = rng.uniform(-1, 1, size=(5, 4))
    base = mr.evaluator_batch(Ws, bs, act, data, w, A)(u)
    shifted = mr.evaluator_batch(Ws, bs, act, data + np.array([3e3, -2e3, 5e2]) @ A, w, A)(u)
    y, J, _ = mr.jr.jvp(Ws, bs, act, u)
    # (the shifted sums hold terms 10^6 times the result: relative to r^T W r of the shifted data)
    m = mr.marg(y, J, data + np.array([3e3, -2e3, 5e2]) @ A, w, A)
    assert np.all(np.abs(base[0] - shifted[0]) <= 1e-12 * m["lnl_scale"])
    assert np.all(np.abs(base[1] - shifted[1]) <= 1e-12 * m["grad_scale"])
    np.testing.assert_array_equal(base[2], shifted[2])  # (F_m does not read the data)


def test_reference_evaluators_drive_the_fit_and_sampler_references():
    """evaluator / evaluator_batch have the interfaces of fit_ref.evaluator / sample_ref.evaluator_batch"""
    import fit_ref as fr
    import sample_ref as sr
    Ws, bs, act, data, w, A, rng = small_case()
    u0 = rng.uniform(-0.5, 0.5, size=(3, 4))
    ev = mr.evaluator(Ws, bs, act, data, w, A)
    for i in range(3):
        r = fr.lm_ref(ev, u0[i], max_iter=30)
        assert r["lnl"] >= r["lnl0"] and np.all(np.abs(r["u"]) <= 1)
    # a data matrix: one spectrum per row
    d2 = np.stack([data, data + 5.0 * A[1], data])
    evb = mr.evaluator_batch(Ws, bs, act, d2, w, A)
    lb = evb(u0)[0]
    np.testing.assert_allclose(lb[1], mr.evaluator(Ws, bs, act, d2[1], w, A)(u0[1])[0], rtol=1e-12)
    np.testing.assert_allclose(lb[1], evb(u0)[0][1], rtol=0)
    s = sr.sample_ref(evb, u0, n_steps=20, n_warmup=10, seed=3)
    assert np.all(np.isfinite(s["samples_u"])) and np.all(np.abs(s["samples_u"]) <= 1) and s["accept_rate"].mean() > 0


WHITEN_CASES = [(K, full) for K in (1, 3, 5, 8) for full in (True, False)]


@pytest.mark.parametrize("K,full", WHITEN_CASES)
def test_whiten_against_numpy_qr(K, full):
    nat, fg = pkg("_native"), pkg("foregrounds")
    if full:
        w = np.full(NU.size, 1.0 / 20.0 ** 2, np.float32)
        A = fg.linlog_basis(NU, K)
    else:
        w = band()
        A = fg.band_basis(NU, K, 50.0, 100.0)
    Q, R = nat.nuisance_whiten(A, w)
    w64 = w.astype(np.float64)
    assert Q.shape == (K, NU.size) and R.shape == (K, K)
    assert np.max(np.abs((Q * w64) @ Q.T - np.eye(K))) <= 1e-12
    assert np.all(Q[:, w == 0] == 0)
    Qr, Rr = mr.whiten(A, w64)
    P, Pr = mr.projector(Q, w64), mr.projector(Qr, w64)
    assert np.max(np.abs(P - Pr)) <= 1e-10, np.max(np.abs(P - Pr))
    # R: upper triangular, sqrt(W) A^T = sqrt(W) Q^T R, and numpy's up to the signs of its rows
    assert np.all(np.tril(R, -1) == 0) and np.all(np.diag(R) > 0)
    sw = np.sqrt(w64)
    np.testing.assert_allclose((Q * sw).T @ R, (A * sw).T, rtol=0, atol=1e-12 * np.abs(A * sw).max())
    np.testing.assert_allclose(R, Rr * np.sign(np.diag(Rr))[:, None], rtol=1e-8, atol=1e-10 * np.abs(R).max())


def test_whiten_argument_errors():
    nat, fg = pkg("_native"), pkg("foregrounds")
    lib = nat.load_library()
    w = np.full(NU.size, 0.01, np.float32)
    dp = C.POINTER(C.c_double)

    def call(A, w):
        A = np.ascontiguousarray(A, np.float64)
        q, r = np.zeros_like(A), np.zeros((max(len(A), 1),) * 2)
        return lib.v21_nuisance_whiten(A.ctypes.data_as(dp), w.ctypes.data_as(C.POINTER(C.c_float)), len(A), NU.size,
                                       q.ctypes.data_as(dp), r.ctypes.data_as(dp))
    assert call(fg.linlog_basis(NU, 5), w) == 0
    # n_modes outside 1 .. 8
    assert call(np.zeros((0, NU.size)), w) == -1
    assert call(fg.linlog_basis(NU, 9), w) == -1
    # a rank-deficient basis: a repeated mode, a combination of two others, a mode that lives on zero-weight bins only
    A = fg.linlog_basis(NU, 4)
    assert call(np.vstack([A, A[1:2]]), w) == -1
    assert call(np.vstack([A, 2.0 * A[0:1] - 3.0 * A[2:3]]), w) == -1
    wz = w.copy(); wz[:100] = 0
    e = np.zeros((1, NU.size)); e[0, :100] = 1.0
    assert call(np.vstack([A, e]), wz) == -1
    with pytest.raises(nat.EngineError):
        nat.nuisance_whiten(np.vstack([A, A[1:2]]), w)
    # fewer than n_modes + 1 bins with weight
    w5 = np.zeros(NU.size, np.float32); w5[200:205] = 0.01
    assert call(fg.linlog_basis(NU, 5), w5) == -1
    w6 = w5.copy(); w6[205] = 0.01
    assert call(fg.linlog_basis(NU, 5), w6) == 0
    # a negative or non-finite weight, null pointers
    wn = w.copy(); wn[3] = -1.0
    assert call(A, wn) == -1
    wn[3] = np.nan
    assert call(A, wn) == -1
    assert lib.v21_nuisance_whiten(None, None, 1, NU.size, None, None) == -1


@pytest.mark.parametrize("K", [5, 8])
@pytest.mark.parametrize("lo,hi", [(50.0, 200.0), (50.0, 100.0), (60.0, 120.0)])
def test_float32_data_project_to_signal_size(K, lo, hi):
    """a LinLog foreground of ~2e6 mK at 75 MHz rounded to float32, projected against the library's float64 Q: what is
    left is the rounding of the float32 data.  Bound: the data stay below 2^25 mK, where half a float32 ulp is 1 mK =
    0.05 sigma at sigma = 20 mK (the cases here reach 6e6 mK < 2^23 and leave 2e-3 .. 4e-3 sigma rms), so float32 sums
    over the projected data see residuals of signal size"""
    nat, fg = pkg("_native"), pkg("foregrounds")
    w = band(lo, hi, holes=False)
    A = fg.band_basis(NU, K, lo, hi)
    sel = w > 0
    a = np.zeros(K); a[0] = 2e6 * (75.0 / np.sqrt(NU[sel].min() * NU[sel].max())) ** 2.5
    a[1:] = a[0] * 0.1 * np.random.default_rng(K).normal(size=K - 1) / (1 + np.arange(K - 1))
    d32 = (a @ A).astype(np.float32)
    Q, _ = nat.nuisance_whiten(A, w)
    res = mr.project(d32, Q, w)[sel]
    rms_sigma = np.sqrt(np.mean(res ** 2)) / 20.0
    print("K=%d band %g-%g: residual %.2e sigma rms, foreground max %.2e mK" % (K, lo, hi, rms_sigma, np.abs(d32).max()))
    assert rms_sigma <= 0.05, rms_sigma
    assert np.linalg.cond((A[:, sel] * np.sqrt(w[sel])) / np.linalg.norm(A[:, sel] * np.sqrt(w[sel]), axis=1, keepdims=True)) < 1e5


def test_linlog_basis():
    fg = pkg("foregrounds")
    A = fg.linlog_basis(NU, 4)
    nu0 = np.sqrt(NU[0] * NU[-1])
    assert A.shape == (4, 451) and A.dtype == np.float64
    np.testing.assert_allclose(A[0], (NU / nu0) ** -2.5, rtol=1e-14)
    np.testing.assert_allclose(A[3], (NU / nu0) ** -2.5 * np.log(NU / nu0) ** 3, rtol=1e-13)
    np.testing.assert_allclose(fg.linlog_basis(NU, 2, nu0=75.0, index=-2.0)[1], (NU / 75.0) ** -2.0 * np.log(NU / 75.0), rtol=1e-14)
    B = fg.band_basis(NU, 3, 60.0, 120.0)
    sel = (NU >= 60.0) & (NU <= 120.0)
    assert np.all(B[:, ~sel] == 0)
    np.testing.assert_array_equal(B[:, sel], fg.linlog_basis(NU[sel], 3))
    with pytest.raises(ValueError):
        fg.linlog_basis(NU, 0)
    with pytest.raises(ValueError):
        fg.band_basis(NU, 3, 300.0, 400.0)
    import importlib
    assert importlib.import_module("VeryAccurateEmulator").foregrounds.linlog_basis is fg.linlog_basis


def test_abi_symbols_and_null_checks():
    nat = pkg("_native")
    lib = nat.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
    assert lib.v21_version() == 100
    k = C.c_int32(0)
    assert lib.v21_mlp_set_nuisance(None, None, 0, 0) == -1
    assert lib.v21_mlp_nuisance_info(None, C.byref(k)) == -1
    assert lib.v21_mlp_nuisance_coef(None, None, 0, 0, None, 0, 0) == -1


def test_foreground_argument_needs_frequencies():
    """foreground=<int> selects LinLog terms over the band: without a frequency array that is the ValueError of a band
    selection (raised before any device work)"""
    emulator = pkg("emulator")
    with pytest.raises(ValueError, match="No frequency array"):
        emulator.foreground_basis(None, 451, 5, None, None)
    with pytest.raises(ValueError):
        emulator.foreground_basis(NU, 451, np.zeros((3, 450)), None, None)
    with pytest.raises(ValueError):
        emulator.foreground_basis(NU, 451, 9, None, None)
    assert emulator.foreground_basis(NU, 451, None, None, None) is None
    A = emulator.foreground_basis(NU, 451, 5, 60.0, 120.0)
    np.testing.assert_array_equal(A, pkg("foregrounds").band_basis(NU, 5, 60.0, 120.0))
