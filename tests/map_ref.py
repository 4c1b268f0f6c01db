"""float64 reference of the MAP fit with held columns and of its Laplace evidence (tests/test_map_*.py; include/v21.h:
v21_mlp_fit_map), built on tests/fit_ref.py and tests/prior_ref.py.

    objective   ln L(u) + ln p(u), ln p = prior_ref.log_prior over the normal columns that are not held
    system      g + grad ln p, A = F + diag(1 / sd^2) on those columns; then for a held column i: g_i = 0,
                A_ij = A_ji = 0 (j != i), A_ii = 1
    laplace     ln L + ln p + d_free / 2 ln 2 pi - 1/2 ln det A at the accepted point (the held pivots are 1)

``map_ref`` is fit_ref.lm_ref on the evaluator wrapped that way.  A held column keeps the float32 value of its clamped
start.  lm_ref decides "no information" on the whole diagonal; the device decides it on the free columns, so the wrapper
leaves the held diagonal at 0 when every free diagonal entry is 0 (and a free column exists): lm_ref then stops with
status 3 as the device does."""
import math

import numpy as np

import fit_ref as fr
import prior_ref as pr

CONTROLS = ("no_prior_in_det", "d_free_plus_one", "held_pivot")


def single(ev_batch):
    """an evaluator of sample_ref (u (n, d) -> batches) as fit_ref takes it (u (d,) -> one evaluation)"""
    def ev(u):
        l, g, F = ev_batch(np.asarray(u, np.float64)[None, :])
        return float(l[0]), g[0], F[0]
    return ev


def free_prior(prior, hold, use_prior):
    """the record the fit works with: the normal columns that are not held (None or use_prior False: all uniform)"""
    hold = np.asarray(hold, bool)
    if prior is None or not use_prior:
        return pr.as_prior(np.zeros(hold.size, np.int64), np.zeros(hold.size), np.ones(hold.size))
    kind, mu, sd = prior
    return pr.as_prior(np.where(hold, 0, kind), mu, sd)


def system(ev, pf, hold, u):
    """-> (ln L, ln p, g, A) at u: the posterior's gradient and matrix with the hold substitution"""
    hold = np.asarray(hold, bool)
    l, g, F = ev(u)
    lp = float(pr.log_prior(pf, u[None, :])[0])
    g = np.where(hold, 0.0, g + pr.grad_log_prior(pf, u[None, :])[0])
    A = np.array(F + pr.precision(pf), np.float64)
    A[hold, :] = 0.0
    A[:, hold] = 0.0
    A[hold, hold] = 1.0
    return l, lp, g, A


def laplace_at(ev, prior, u, hold, use_prior, control=None):
    """the MAP outputs of the formulas above at the point u -> dict lnl, lnp, laplace, prec_u, d_free.  control: one of
    CONTROLS, a deliberately wrong variant (the prior left out of the determinant, d_free miscounted by one, the held
    pivot included) that the tests' bounds must tell from the right one"""
    hold = np.asarray(hold, bool)
    u = np.asarray(u, np.float64)
    pf = free_prior(prior, hold, use_prior)
    l, lp, _, A = system(ev, pf, hold, u)
    d_free = int(np.count_nonzero(~hold))
    D = A
    if control == "no_prior_in_det":
        D = A - np.where(hold[:, None] | hold[None, :], 0.0, pr.precision(pf))
    elif control == "held_pivot":
        D = np.array(ev(u)[2] + pr.precision(pf), np.float64)
    try:
        piv = np.diag(np.linalg.cholesky(D)) ** 2
        ok = bool(np.all(np.isfinite(piv)) and np.all(piv > 0))
    except np.linalg.LinAlgError:
        ok = False
    df = d_free + 1 if control == "d_free_plus_one" else d_free
    lap = l + lp + 0.5 * df * math.log(2.0 * math.pi) - 0.5 * float(np.sum(np.log(piv))) if ok else float("nan")
    return {"lnl": l, "lnp": lp, "laplace": lap, "prec_u": A, "d_free": d_free}


def map_ref(ev, prior, u0, hold, use_prior, max_iter=50, lambda0=1e-3, xtol=1e-7, control=None):
    """-> dict u (accepted point), lnl (ln L alone), lnl0, lnp, obj (ln L + ln p), status, iters, laplace, prec_u, d_free.
    ev: u (d,) -> (ln L, g, F) in float64; prior: a prior_ref triple or None; hold: (d,) bool"""
    hold = np.asarray(hold, bool)
    pf = free_prior(prior, hold, use_prior)
    start = np.clip(np.asarray(u0, np.float64), -1.0, 1.0)
    start[hold] = start[hold].astype(np.float32)  # (the device holds the float32 u of the clamped start)

    def wrapped(u):
        u = np.where(hold, start, u)
        l, lp, g, A = system(ev, pf, hold, u)
        free_diag = np.diag(A)[~hold]
        if free_diag.size and not np.any(free_diag != 0):
            A[hold, hold] = 0.0  # (no information on the free columns: lm_ref's status 3)
        return l + lp, g, A

    r = fr.lm_ref(wrapped, start, max_iter=max_iter, lambda0=lambda0, xtol=xtol)
    u = np.where(hold, start, r["u"])
    out = laplace_at(ev, prior, u, hold, use_prior, control)
    out.update(u=u, obj=r["lnl"], lnl0=ev(start)[0], status=r["status"], iters=r["iters"])
    return out


def posterior_gradient(ev, prior, u, hold, use_prior, lik_terms):
    """-> (the gradient of ln L + ln p over the free columns at u, the sum of the magnitudes of the terms it is made of).
    lik_terms: (d,) sum_k |J_jk w_k r_k|, the magnitudes of the per-bin terms of ln L's gradient at u"""
    hold = np.asarray(hold, bool)
    pf = free_prior(prior, hold, use_prior)
    u = np.asarray(u, np.float64)
    gp = pr.grad_log_prior(pf, u[None, :])[0]
    return (ev(u)[1] + gp)[~hold], float(np.sum(np.asarray(lik_terms)[~hold]) + np.sum(np.abs(gp[~hold])))


__all__ = ["CONTROLS", "single", "free_prior", "system", "laplace_at", "map_ref", "posterior_gradient", "fr", "pr"]
