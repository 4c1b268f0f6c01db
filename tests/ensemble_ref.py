"""float64 reference of the ensemble sampler (tests/test_ensemble_*.py; include/v21.h: v21_mlp_sample_ensemble): Goodman &
Weare's stretch move of csrc/ensemble_kernels.h batched over ensembles, on the Philox helpers of tests/sample_ref.py.

W consecutive rows form one ensemble of two sets of H = W / 2 walkers.  Sweep S is two half-moves, h = 0 then h = 1;
half-move h moves every walker i of set h with the words (w0, w1, w2) of Philox block 0 of (seed, chain0 + row, S):
    z = ((a - 1) U(w0) + 1)^2 / a;   partner k = (H w1) >> 32 in set 1 - h (its CURRENT position);
    y = float32(x_k + z (x_i - x_k));   log alpha = (d - 1) ln z + lnL(y) - lnL(x_i);   accept iff ln U(w2) < log alpha
A y outside [-1, 1]^d is rejected, log alpha = -inf.  Every ln L is evaluated on the rows of one set, ensemble by ensemble
(the device's compacted layout)."""
import numpy as np

import sample_ref as sr


def layout(n, n_walkers):
    """(ensemble, set, index in the set) of every row"""
    W, H = int(n_walkers), int(n_walkers) // 2
    rows = np.arange(n)
    i = rows % W
    return rows // W, i // H, i % H


def draws(seed, chains, step, a, H):
    """(z, partner index in the other set, ln U of the acceptance) of sweep `step` for the global chains"""
    w = sr.block(seed, chains, step, 0)
    z = ((a - 1.0) * sr.uniform(w[:, 0]) + 1.0) ** 2 / a
    k = ((np.uint64(H) * w[:, 1].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    return z, k, np.log(sr.uniform(w[:, 2]))


def stretch(x_i, x_k, z):
    """the proposal as the device rounds it, as float64"""
    return (x_k + z[:, None] * (x_i - x_k)).astype(np.float32).astype(np.float64)


def _lnl(ev, u):
    r = ev(u)
    return np.asarray(r[0] if isinstance(r, tuple) else r, np.float64)


def ensemble_ref(ev, u0, n_walkers, a=2.0, n_steps=1000, n_warmup=500, thin=1, seed=0, chain0=0, step0=0, jacobian=True, clamp=False):
    """The ensembles of csrc/ensemble_kernels.h in float64 (the state is the float32-rounded u, as there).  ev: u (m, d)
    -> ln L (m,), or a tuple whose first entry it is (sample_ref.evaluator_batch).  jacobian=False (the (d - 1) ln z term
    left out) and clamp=True (a proposal outside the box clipped onto it instead of rejected) are deliberately WRONG
    variants, for the controls of the statistical tests.
    -> dict u (n, d), lnl, accept_rate, mean_u, cov_u, samples_u (n, n_steps // thin, d), samples_lnl, last_prop_u,
    last_log_alpha, last_partner, last_accept"""
    u = np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32).astype(np.float64)
    n, d = u.shape
    W, H = int(n_walkers), int(n_walkers) // 2
    assert W % 2 == 0 and n % W == 0
    e, h, _ = layout(n, W)
    sets = [np.flatnonzero(h == hh) for hh in (0, 1)]
    chains = chain0 + np.arange(n)
    lnl = np.zeros(n)
    for idx in sets:
        lnl[idx] = _lnl(ev, u[idx])
    keep = n_steps // thin if thin > 0 else 0
    su, suu, acc = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros(n)
    samples, samples_lnl = np.zeros((n, keep, d)), np.zeros((n, keep))
    prop, la, partner, accept = u.copy(), np.zeros(n), np.full(n, -1), np.ones(n, bool)
    for t in range(n_warmup + n_steps):
        z, k, logu = draws(seed, chains, step0 + t, a, H)
        for hh, idx in enumerate(sets):
            pr = e[idx] * W + (1 - hh) * H + k[idx]
            y = stretch(u[idx], u[pr], z[idx])
            inside = np.all((y >= -1.0) & (y <= 1.0), axis=1)
            if clamp:
                y = np.clip(y, -1.0, 1.0)
                inside[:] = True
            lnl_y = _lnl(ev, y)
            with np.errstate(invalid="ignore"):
                l = ((d - 1) * np.log(z[idx]) if jacobian else 0.0) + (lnl_y - lnl[idx])
            l = np.where(inside & ~np.isnan(l), l, -np.inf)
            ok = logu[idx] < l
            u[idx] = np.where(ok[:, None], y, u[idx])
            lnl[idx] = np.where(ok, lnl_y, lnl[idx])
            prop[idx], la[idx], partner[idx], accept[idx] = y, l, pr - e[idx] * W, ok
            if t >= n_warmup:
                su[idx] += u[idx]
                suu[idx] += u[idx][:, :, None] * u[idx][:, None, :]
                acc[idx] += ok
                kk = t - n_warmup + 1
                if thin > 0 and kk % thin == 0 and kk // thin <= keep:
                    samples[idx, kk // thin - 1], samples_lnl[idx, kk // thin - 1] = u[idx], lnl[idx]
    K = max(n_steps, 1)
    mean = su / K if n_steps else u.copy()
    cov = suu / K - mean[:, :, None] * mean[:, None, :] if n_steps else np.zeros((n, d, d))
    return {"u": u, "lnl": lnl, "accept_rate": acc / K, "mean_u": mean, "cov_u": cov, "samples_u": samples, "samples_lnl": samples_lnl,
            "last_prop_u": prop, "last_log_alpha": la, "last_partner": partner, "last_accept": accept}


def forward_evaluator(Ws, bs, act, data, w, tout=None):
    """u (m, in) -> ln L (m,) in float64 of the stack on u, forward only (sample_ref.evaluator_batch without its Jacobian);
    data (out,)"""
    std, mean = (1.0, 0.0) if tout is None else (float(tout[0]), np.asarray(tout[1], np.float64))
    d, w = np.asarray(data, np.float64), np.asarray(w, np.float64)

    def ev(u):
        h = np.asarray(u, np.float64)
        for W_, b_, a_ in zip(Ws, bs, act):
            h = h @ np.asarray(W_, np.float64) + np.asarray(b_, np.float64)
            h = np.maximum(h, 0.0) if a_ else h
        r = d - (h * std + mean)
        return -0.5 * np.sum(w * r * r, axis=-1)
    return ev


def ensemble_estimates(mean_u, cov_u, n_walkers):
    """per-ensemble estimates of E[u] and E[u^2] (ensembles, d) from the per-walker moments: the walkers of an ensemble
    pooled (they are not independent of each other; ensembles are)"""
    mean_u, cov_u = np.asarray(mean_u, np.float64), np.asarray(cov_u, np.float64)
    d = mean_u.shape[1]
    m = mean_u.reshape(-1, n_walkers, d)
    m2 = (np.diagonal(cov_u, axis1=1, axis2=2) + mean_u ** 2).reshape(-1, n_walkers, d)
    return m.mean(axis=1), m2.mean(axis=1)


__all__ = ["layout", "draws", "stretch", "ensemble_ref", "forward_evaluator", "ensemble_estimates"]
