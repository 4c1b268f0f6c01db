"""float64 reference of the samplers' prior record (tests/test_prior_*.py; include/v21.h: v21_mlp_set_prior): a separable
prior in u in [-1, 1]^d, column i uniform (kind 0) or normal(mu_i, sd_i) truncated to the box (kind 1).

    ln p(u) = -1/2 sum_i ((u_i - mu_i) / sd_i)^2 over the normal columns (unnormalised)
    grad ln p = -(u - mu) / sd^2,   precision = diag(1 / sd^2)

A prior here is the triple (kind (d,), mu (d,), sd (d,)).  ``with_prior(ev, prior)`` wraps an evaluator of sample_ref so
that the plain MALA and ensemble references sample L p unmodified; the tempered and the nested loop below take the prior
beside ev (it is not tempered, and the nested rule needs ln L alone), built from the pieces temper_ref, sample_ref and
nested_ref export."""
import math

import numpy as np
from scipy.special import ndtr, ndtri

import nested_ref as nr
import sample_ref as sr
import temper_ref as tr


def as_prior(kind, mu, sd):
    kind = np.asarray(kind, np.int64)
    return kind, np.where(kind == 1, np.asarray(mu, np.float64), 0.0), np.where(kind == 1, np.asarray(sd, np.float64), 1.0)


def log_prior(prior, u):
    """unnormalised ln p (n,) at u (n, d)"""
    kind, mu, sd = prior
    z = (np.asarray(u, np.float64) - mu) / sd
    return -0.5 * np.sum(np.where(kind == 1, z * z, 0.0), axis=-1)


def grad_log_prior(prior, u):
    kind, mu, sd = prior
    return np.where(kind == 1, -(np.asarray(u, np.float64) - mu) / sd ** 2, 0.0)


def precision(prior):
    """diag(1 / sd^2) (d, d), zero on the uniform columns"""
    kind, mu, sd = prior
    return np.diag(np.where(kind == 1, 1.0 / sd ** 2, 0.0))


def log_norm(prior):
    """ln of the integral of exp(log_prior) over the box, relative to the uniform prior's 2^d: ln[int p du / 2^d]"""
    kind, mu, sd = prior
    out = 0.0
    for i in np.flatnonzero(kind == 1):
        a, b = (-1.0 - mu[i]) / sd[i], (1.0 - mu[i]) / sd[i]
        mass = ndtr(-a) - ndtr(-b) if a + b > 0 else ndtr(b) - ndtr(a)
        out += math.log(math.sqrt(2.0 * math.pi) * sd[i] * mass / 2.0)
    return out


def ppf(prior, c):
    """the prior's inverse CDF column by column: c (n, d) in (0, 1) -> u (n, d) float64.  A uniform column is 2 c - 1; a
    normal column mu + sd z with Phi(z) = Phi(a) + c (Phi(b) - Phi(a)), a, b the standardised box ends, solved in the
    mirrored problem where a + b > 0 so that Phi is taken in the tail nearer the mode; clipped into the box"""
    kind, mu, sd = prior
    c = np.asarray(c, np.float64)
    out = 2.0 * c - 1.0
    for i in np.flatnonzero(kind == 1):
        a, b = (-1.0 - mu[i]) / sd[i], (1.0 - mu[i]) / sd[i]
        if a + b > 0:
            pa, pb = ndtr(-a), ndtr(-b)
            z = -ndtri(pa - c[:, i] * (pa - pb))
        else:
            pa, pb = ndtr(a), ndtr(b)
            z = ndtri(pa + c[:, i] * (pb - pa))
        out[:, i] = np.clip(mu[i] + sd[i] * z, -1.0, 1.0)
    return out


def moments(prior):
    """mean and variance (d,) of every column of the prior on the box, closed form (uniform: 0 and 1 / 3)"""
    kind, mu, sd = prior
    m, v = np.zeros(len(kind)), np.full(len(kind), 1.0 / 3.0)
    phi = lambda x: math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    for i in np.flatnonzero(kind == 1):
        a, b = (-1.0 - mu[i]) / sd[i], (1.0 - mu[i]) / sd[i]
        Z = ndtr(-a) - ndtr(-b) if a + b > 0 else ndtr(b) - ndtr(a)
        r = (phi(a) - phi(b)) / Z
        m[i] = mu[i] + sd[i] * r
        v[i] = sd[i] ** 2 * (1.0 + (a * phi(a) - b * phi(b)) / Z - r * r)
    return m, v


def with_prior(ev, prior):
    """ev: u -> (lnl, g, F) or u -> lnl.  -> the evaluator of L p: (lnl + ln p, g + grad ln p, F + diag(1 / sd^2)), or
    lnl + ln p.  The device's ln L outputs compare with its first entry minus log_prior."""
    P = precision(prior)

    def wrapped(u):
        r = ev(u)
        lp = log_prior(prior, u)
        if isinstance(r, tuple):
            return r[0] + lp, r[1] + grad_log_prior(prior, u), r[2] + P[None]
        return np.asarray(r, np.float64) + lp
    return wrapped


def start_draws(prior, seed, rows, d):
    """the nested sampler's drawn starts under the prior: nested_ref.start_draws' Philox words through ppf, float32"""
    w = np.concatenate([sr.block(seed, rows, 0, 2 + b) for b in range((d + 3) // 4)], axis=1)[:, :d]
    c = sr.uniform(w)
    plain = (2.0 * c - 1.0).astype(np.float32)
    kind = prior[0]
    return np.where(kind == 1, ppf(prior, c).astype(np.float32), plain)


def accept_draws(seed, rows, c):
    """ln U of the prior's acceptance of global move c: word 0 of block 4"""
    w = sr.block(seed, rows.reshape(-1), c, 4)
    return np.log(sr.uniform(w[:, 0])).reshape(rows.shape)


def temper_ref(ev, prior, u0, betas, swap_every=0, n_steps=1000, n_warmup=200, thin=1, eps0=1.0, ridge=1.0, target_accept=0.574, seed=0,
               chain0=0, step0=0, eps_start=None):
    """temper_ref.temper_ref with the prior: gradient, metric and log alpha gain the prior's terms AFTER the beta scaling,
    unscaled; the swap rule and the sums of ln L are unchanged.  -> the same dict"""
    betas = np.asarray(betas, np.float64)
    T = betas.shape[0]
    u = np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32).astype(np.float64)
    n, d = u.shape
    assert n % T == 0
    beta = betas[np.arange(n) % T]
    chains = chain0 + np.arange(n)
    eps = np.full(n, float(eps0)) if eps_start is None else np.asarray(eps_start, np.float64).copy()
    P = precision(prior)[None]
    lnl, g, F = ev(u)
    keep = n_steps // thin if thin > 0 else 0
    su, suu, acc = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros(n)
    sl, sll, proposed, swapped_n = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    samples, samples_lnl = np.zeros((n, keep, d)), np.zeros((n, keep))
    prop, la, accept = u.copy(), np.zeros(n), np.ones(n, bool)
    swaps = 0
    for t in range(n_warmup + n_steps):
        S = step0 + t
        xi = sr.normals(seed, chains, S, d)
        prop, lq_fwd, inside = sr.propose(u, tr.tmul(beta, g) + grad_log_prior(prior, u), tr.tmul(beta, F) + P, eps, xi, ridge)
        lnl_p, g_p, F_p = ev(prop)
        la = sr.log_alpha(u, tr.tmul(beta, lnl) + log_prior(prior, u), lq_fwd, inside, prop, tr.tmul(beta, lnl_p) + log_prior(prior, prop),
                          tr.tmul(beta, g_p) + grad_log_prior(prior, prop), tr.tmul(beta, F_p) + P, eps, ridge)
        accept = np.log(sr.accept_uniform(seed, chains, S)) < la
        u = np.where(accept[:, None], prop, u)
        lnl, g, F = np.where(accept, lnl_p, lnl), np.where(accept[:, None], g_p, g), np.where(accept[:, None, None], F_p, F)
        if t < n_warmup:
            eps = eps * np.exp((t + 1.0) ** -0.6 * (np.exp(np.minimum(la, 0.0)) - target_accept))
        if swap_every > 0 and (S + 1) % swap_every == 0:
            perm, lower, sw, _, _ = tr.swap_event(lnl, betas, (S + 1) // swap_every - 1, seed, chain0, S)
            u, lnl, g, F = u[perm], lnl[perm], g[perm], F[perm]
            swaps += int(sw.sum())
            if t >= n_warmup:
                proposed[lower] += 1
                swapped_n[lower] += sw
        if t >= n_warmup:
            su += u
            suu += u[:, :, None] * u[:, None, :]
            acc += accept
            sl += lnl
            sll += lnl * lnl
            k = t - n_warmup + 1
            if thin > 0 and k % thin == 0 and k // thin <= keep:
                samples[:, k // thin - 1], samples_lnl[:, k // thin - 1] = u, lnl
    K = max(n_steps, 1)
    mean = su / K if n_steps else u.copy()
    cov = suu / K - mean[:, :, None] * mean[:, None, :] if n_steps else np.zeros((n, d, d))
    mean_lnl = sl / K if n_steps else lnl.copy()
    var_lnl = sll / K - mean_lnl ** 2 if n_steps else np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        swap_accept = np.where(proposed > 0, swapped_n / np.maximum(proposed, 1), 0.0)
    return {"u": u, "lnl": lnl, "eps": eps, "accept_rate": acc / K, "mean_u": mean, "cov_u": cov, "samples_u": samples,
            "samples_lnl": samples_lnl, "last_prop_u": prop, "last_log_alpha": la, "last_accept": accept, "mean_lnl": mean_lnl,
            "var_lnl": var_lnl, "swap_accept": swap_accept, "swaps": swaps}


def nested_ref(ev, prior, u0, n_live, n_iter, n_repeats=None, gamma=None, seed=0, iter0=0, chain0=0, lnl0=None, use_prior=True):
    """nested_ref.nested_ref with the prior: a move is accepted iff it is inside the box, ln L(y) > L* and
    ln U < ln p(y) - ln p(x), U from word 0 of block 4 at the move's step; u0 None: the starts are drawn from the prior.
    use_prior=False keeps the starts but leaves the prior's acceptance out, the deliberately WRONG variant of the controls.
    -> nested_ref's dict, last_log_ratio (runs, k): ln p(y) - ln p(x) of the last move, and min_margin: the smallest
    |ln U - (ln p(y) - ln p(x))| over the moves the prior decided"""
    d = len(prior[0])
    N, k, T = int(n_live), int(n_live) // 2, int(n_iter)
    u = np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32)
    n = u.shape[0]
    assert N % 2 == 0 and n % N == 0 and u.shape[1] == d
    runs = n // N
    R = nr.default_repeats(d) if not n_repeats else int(n_repeats)
    g = np.float32(nr.default_gamma(d) if not gamma else gamma)
    u = u.reshape(runs, N, d)
    lnl = (nr._lnl(ev, u.reshape(n, d)) if lnl0 is None else np.asarray(lnl0, np.float64)).reshape(runs, N)
    lnl = np.where(np.isnan(lnl), -np.inf, lnl)
    rows, e = nr.slot_rows(runs, N, chain0), np.arange(runs)[:, None]
    dead_u, dead_lnl, lstar = np.zeros((T, runs, k, d), np.float32), np.zeros((T, runs, k)), np.zeros((T, runs))
    acc = np.zeros((runs, k))
    pa = pb = np.full((runs, k), -1)
    prop, ratio, margin = u[:, k:].copy(), np.zeros((runs, k)), np.inf
    for t in range(T):
        order = nr.rank_order(lnl)
        u, lnl = np.take_along_axis(u, order[:, :, None], axis=1), np.take_along_axis(lnl, order, axis=1)
        dead_u[t], dead_lnl[t], lstar[t] = u[:, :k], lnl[:, :k], lnl[:, k - 1]
        c = nr.restart_draws(seed, rows, iter0 + t, k)
        u[:, :k], lnl[:, :k] = u[e, k + c], lnl[e, k + c]
        for s in range(R):
            mv = (iter0 + t) * R + s
            pa, pb = nr.move_draws(seed, rows, mv, k)
            prop = nr.propose(u[:, :k], u[e, k + pa], u[e, k + pb], g)
            inside = np.all((prop >= -1.0) & (prop <= 1.0), axis=2)
            lnl_y = nr._lnl(ev, prop.reshape(-1, d)).reshape(runs, k)
            with np.errstate(invalid="ignore"):
                above = lnl_y > lstar[t][:, None]
            ratio = log_prior(prior, prop.astype(np.float64)) - log_prior(prior, u[:, :k].astype(np.float64))
            ok = inside & above
            if use_prior:
                logu = accept_draws(seed, rows, mv)
                if ok.any():
                    margin = min(margin, float(np.min(np.abs(logu - ratio)[ok])))
                ok &= logu < ratio
            u[:, :k] = np.where(ok[:, :, None], prop, u[:, :k])
            lnl[:, :k] = np.where(ok, lnl_y, lnl[:, :k])
            acc += ok
    return {"dead_u": dead_u, "dead_lnl": dead_lnl, "lstar": lstar, "live_u": u.reshape(n, d), "live_lnl": lnl.reshape(n),
            "accept_rate": acc / max(T * R, 1), "last_partner": np.stack([pa, pb], axis=-1), "last_prop_u": prop,
            "last_log_ratio": ratio, "min_margin": margin, "n_evals": n + runs * k * T * R}


__all__ = ["as_prior", "log_prior", "grad_log_prior", "precision", "log_norm", "ppf", "moments", "with_prior", "start_draws",
           "accept_draws", "temper_ref", "nested_ref"]
