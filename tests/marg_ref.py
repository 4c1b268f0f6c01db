"""float64 reference of the likelihood marginalised over linear nuisance modes (tests/test_marg_*.py; include/v21.h:
v21_mlp_set_nuisance).  Data model d = y + A^T a + noise, flat prior on a.  With W = diag(w), Q the W-orthonormalised
basis (numpy.linalg.qr of sqrt(W) A^T), r = d - y, b = Q W r, B = Q W J^T:
    lnL_m = -1/2 (r^T W r - |b|^2),   g_m = J W r - B^T b,   F_m = J W J^T - B^T B,   a_hat = R^-1 b.
evaluator / evaluator_batch have the interfaces of fit_ref.evaluator / sample_ref.evaluator_batch."""
import numpy as np

import jacobian_ref as jr


def whiten(A, w):
    """(Q (K, out) with Q W Q^T = I and zeros where w == 0, R (K, K) with sqrt(W) A^T = sqrt(W) Q^T R), by Householder QR"""
    A, w = np.asarray(A, np.float64), np.asarray(w, np.float64)
    sw = np.sqrt(w)
    Qf, R = np.linalg.qr((A * sw).T)  # (out, K), (K, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        Q = np.where(sw > 0, Qf.T / sw, 0.0)
    return Q, R


def projector(Q, w):
    """Q^T Q W (out, out): the W-orthogonal projector onto span(A)"""
    return Q.T @ (Q * np.asarray(w, np.float64))


def project(d, Q, w):
    """d - Q^T (Q W d) along the last axis, float64"""
    d, w = np.asarray(d, np.float64), np.asarray(w, np.float64)
    return d - ((d * w) @ Q.T) @ Q


def marg(y, J, d, w, A):
    """y (n, out), J (n, in, out), d (out,) or (n, out) -> dict lnl (n,), grad (n, in), F (n, in, in), coef (n, K), b (n, K),
    F0 = J W J^T, and the sums of the terms' magnitudes lnl_scale = r^T W r + |b|^2, grad_scale = sum |w r J| + |B^T| |b|.
    ln L and its gradient are formed from the projected residual r - Q^T b -- the same numbers as r^T W r - |b|^2 and
    J W r - B^T b (marg_literal), without the cancellation that costs float64 its digits when d carries a foreground 10^6
    times the signal."""
    y, J, w = np.asarray(y, np.float64), np.asarray(J, np.float64), np.asarray(w, np.float64)
    Q, R = whiten(A, w)
    r = np.asarray(d, np.float64) - y
    wr = w * r
    b = wr @ Q.T                                   # (n, K)
    B = np.einsum("mk,k,njk->nmj", Q, w, J)        # (n, K, in)
    rp = r - b @ Q
    F0 = np.einsum("nik,k,njk->nij", J, w, J)
    return {"lnl": -0.5 * np.sum(w * rp * rp, axis=-1),
            "grad": np.einsum("nk,njk->nj", w * rp, J),
            "F": F0 - np.einsum("nmi,nmj->nij", B, B),
            "coef": np.linalg.solve(R, b.T).T, "b": b, "F0": F0,
            "lnl_scale": np.sum(wr * r, axis=-1) + np.sum(b * b, axis=-1),
            "grad_scale": np.einsum("nk,njk->nj", np.abs(wr), np.abs(J)) + np.einsum("nmj,nm->nj", np.abs(B), np.abs(b))}


def marg_literal(y, J, d, w, A):
    """(lnL_m, g_m) exactly as the formulas read: -1/2 (r^T W r - |b|^2), J W r - B^T b"""
    y, J, w = np.asarray(y, np.float64), np.asarray(J, np.float64), np.asarray(w, np.float64)
    Q, _ = whiten(A, w)
    wr = w * (np.asarray(d, np.float64) - y)
    b = wr @ Q.T
    B = np.einsum("mk,k,njk->nmj", Q, w, J)
    return (-0.5 * (np.sum(wr * (np.asarray(d, np.float64) - y), axis=-1) - np.sum(b * b, axis=-1)),
            np.einsum("nk,njk->nj", wr, J) - np.einsum("nmj,nm->nj", B, b))


def profile_lnl(y, d, w, A):
    """max_a lnL(d - A^T a) per row by numpy.linalg.lstsq on the weighted system -> (lnl (n,), a_hat (n, K))"""
    w = np.asarray(w, np.float64)
    sw = np.sqrt(w)
    r = np.atleast_2d(np.asarray(d, np.float64) - np.asarray(y, np.float64))
    a, *_ = np.linalg.lstsq((np.asarray(A, np.float64) * sw).T, (r * sw).T, rcond=None)
    res = r - a.T @ np.asarray(A, np.float64)
    return -0.5 * np.sum(w * res * res, axis=-1), a.T


def _stack(Ws, bs, act, tout):
    std, mean = (1.0, 0.0) if tout is None else (float(tout[0]), np.asarray(tout[1], np.float64))

    def f(u):
        y, J, _ = jr.jvp(Ws, bs, act, np.asarray(u, np.float64))
        return y * std + mean, J * std
    return f


def evaluator(Ws, bs, act, data, w, A, tout=None):
    """u (in,) -> (lnL_m, g_m, F_m) in float64 of the stack on u (no input transform), tout: (std, mean)"""
    f = _stack(Ws, bs, act, tout)

    def ev(u):
        y, J = f(np.asarray(u, np.float64)[None, :])
        m = marg(y, J, data, w, A)
        return m["lnl"][0], m["grad"][0], m["F"][0]
    return ev


def evaluator_batch(Ws, bs, act, data, w, A, tout=None):
    """u (n, in) -> (lnL_m (n,), g_m (n, in), F_m (n, in, in)); data (out,) or (n, out)"""
    f = _stack(Ws, bs, act, tout)

    def ev(u):
        y, J = f(u)
        m = marg(y, J, data, w, A)
        return m["lnl"], m["grad"], m["F"]
    return ev


__all__ = ["whiten", "projector", "project", "marg", "marg_literal", "profile_lnl", "evaluator", "evaluator_batch"]
