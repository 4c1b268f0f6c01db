"""float64 reference of the Fisher matrix and of the projected Levenberg-Marquardt fit (tests/test_fit_*.py), built on
tests/jacobian_ref.py.  lm_ref is the state machine of csrc/fit_kernels.h (fit_lm_kernel) with the same constants:
accept a proposal when ln L rose (the start always) and divide lambda by 10 (not below 1e-12), else multiply it by 10;
solve (F + lambda diag(max(F_ii, tiny))) delta = g by Cholesky; proposal = clip(u + delta, -1, 1); stop on a projected
step <= xtol (1), lambda > 1e12 (2), every F_ii == 0 (3), or after max_iter proposals (0)."""
import numpy as np

import jacobian_ref as jr

LAM_MIN, LAM_MAX, TINY = 1e-12, 1e12, 1e-30


def fisher_ref(J, w):
    """F (n, in, in) = J W J^T of Jacobians J (n, in, out) in the library's layout, W = diag(w)"""
    J = np.asarray(J, np.float64)
    return np.einsum("nik,k,njk->nij", J, np.asarray(w, np.float64), J)


def untransform(u, log_mask, lo, hi):
    """the inverse of preprocess.par_transform in float64: lo + (u + 1) span / 2, then 10^ for a log column"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    t = lo + (np.asarray(u, np.float64) + 1.0) * (hi - lo) / 2.0
    lm = np.asarray(log_mask, bool)
    return np.where(lm, 10.0 ** np.where(lm, t, 0.0), t)


def evaluator(Ws, bs, act, data, w, tout=None):
    """u (in,) -> (ln L, gradient, Fisher matrix) in float64 of the stack on u (no input transform), tout: (std, mean)"""
    std, mean = (1.0, 0.0) if tout is None else (float(tout[0]), np.asarray(tout[1], np.float64))
    d, w = np.asarray(data, np.float64), np.asarray(w, np.float64)

    def ev(u):
        y, J, _ = jr.jvp(Ws, bs, act, np.asarray(u, np.float64)[None, :])
        y, J = y[0] * std + mean, J[0] * std
        r = d - y
        return -0.5 * np.sum(w * r * r), J @ (w * r), (J * w) @ J.T
    return ev


def lm_solve(F, g, lam):
    """delta of (F + lam diag(max(F_ii, tiny))) delta = g, or None when the Cholesky factorisation fails"""
    A = F + lam * np.diag(np.maximum(np.diag(F), TINY))
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, g))


def lm_ref(ev, u0, max_iter=50, lambda0=1e-3, xtol=1e-7):
    """-> dict u (accepted point), lnl, lnl0, status, iters (proposals evaluated after the start)"""
    u_prop = np.clip(np.asarray(u0, np.float64), -1.0, 1.0)
    lam, status, iters = float(lambda0), -1, 0
    u = g = F = None
    lnl = lnl0 = None
    for it in range(max_iter + 1):
        ln, gn, Fn = ev(u_prop)
        if it > 0:
            iters += 1
        if it == 0 or ln > lnl:
            u, g, F, lnl = u_prop.copy(), gn, Fn, ln
            if it == 0:
                lnl0 = ln
            lam = max(lam / 10.0, LAM_MIN)
        else:
            lam *= 10.0
        if not np.any(np.diag(F) != 0):
            status = 3
            break
        delta = None
        while lam <= LAM_MAX:
            delta = lm_solve(F, g, lam)
            if delta is not None:
                break
            lam *= 10.0
        if lam > LAM_MAX:
            status = 2
            break
        un = np.clip(u + delta, -1.0, 1.0)
        if np.max(np.abs(un - u)) <= xtol:
            status = 1
            break
        u_prop = un
    return {"u": u, "lnl": lnl, "lnl0": lnl0, "status": max(status, 0), "iters": iters}


__all__ = ["fisher_ref", "untransform", "evaluator", "lm_ref", "lm_solve", "jr"]
