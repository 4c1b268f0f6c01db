"""float64 reference of the parallel-tempered sampler (tests/test_temper_*.py; include/v21.h: v21_mlp_sample_tempered), on the
pieces of tests/sample_ref.py (Philox, factor, drift, logq, propose, log_alpha), which it does not change.

Rows and rungs: T = len(betas) consecutive rows form one ladder, row r is rung k = r % T at beta = betas[k].  A tempered
transition is sample_ref's with ln L, g and F multiplied by beta (exactly 0 at beta = 0, whatever they hold) wherever they
enter the drift, the metric and log alpha.  With S = step0 + t the global index of transition t, a swap event follows the
decision of S whenever (S + 1) % swap_every == 0; event e = (S + 1) / swap_every - 1 proposes the pairs (k, k + 1) with
k % 2 == e % 2, and a pair swaps iff log U < (beta_k - beta_k+1) (lnL_k+1 - lnL_k), U from word 0 of Philox block 3 of the
lower row's chain at step S.  A swap exchanges (u, ln L, g, F); step size, moments and counters stay with the row.  Moments
and stored samples see the state after the swap, and the next proposal is drawn from it."""
import numpy as np

import sample_ref as sr


def tmul(beta, a):
    """beta a along the first axis, exactly 0 where beta == 0 (non-finite a included)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(beta, np.float64).reshape((-1,) + (1,) * (a.ndim - 1))
    with np.errstate(invalid="ignore"):
        return np.where(b == 0.0, 0.0, b * a)


def swap_uniform(seed, chains, step):
    """word 0 of block 3"""
    return sr.uniform(sr.block(seed, chains, step, 3)[:, 0])


def swap_event(lnl, betas, e, seed, chain0, S):
    """Event number e after transition S on the n rows with ln L `lnl` (ladders of len(betas) rows, the first row global
    chain chain0) -> (perm, lower, swapped, logu, rhs): the state of row r after the event is the state row perm[r] had
    before it; lower: the rows that are the lower one of a proposed pair, and for each of them the decision, log U and
    the right-hand side."""
    lnl, betas = np.asarray(lnl, np.float64), np.asarray(betas, np.float64)
    n, T = lnl.shape[0], betas.shape[0]
    rows = np.arange(n)
    k = rows % T
    lower = rows[(k % 2 == e % 2) & (k + 1 < T)]
    kl = lower % T
    with np.errstate(invalid="ignore"):
        rhs = (betas[kl] - betas[(kl + 1) % T]) * (lnl[(lower + 1) % n] - lnl[lower])
    logu = np.log(swap_uniform(seed, chain0 + lower, S)) if lower.size else np.zeros(0)
    with np.errstate(invalid="ignore"):
        swapped = logu < rhs  # (NaN refuses)
    perm = rows.copy()
    perm[lower[swapped]] = lower[swapped] + 1
    perm[lower[swapped] + 1] = lower[swapped]
    return perm, lower, swapped, logu, rhs


def temper_ref(ev, u0, betas, swap_every=0, n_steps=1000, n_warmup=200, thin=1, eps0=1.0, ridge=1.0, target_accept=0.574, seed=0,
               chain0=0, step0=0, eps_start=None):
    """The rows of csrc/sample_kernels.h's tempered step kernel in float64.  ev: u (n, d) -> (lnl, g, F); u0 (n, d), n a
    multiple of len(betas).
    -> the dict of sample_ref.sample_ref, and mean_lnl, var_lnl, swap_accept (n,), swaps (the number of swaps done)"""
    betas = np.asarray(betas, np.float64)
    T = betas.shape[0]
    u = np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32).astype(np.float64)
    n, d = u.shape
    assert n % T == 0
    beta = betas[np.arange(n) % T]
    chains = chain0 + np.arange(n)
    eps = np.full(n, float(eps0)) if eps_start is None else np.asarray(eps_start, np.float64).copy()
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
        prop, lq_fwd, inside = sr.propose(u, tmul(beta, g), tmul(beta, F), eps, xi, ridge)
        lnl_p, g_p, F_p = ev(prop)
        la = sr.log_alpha(u, tmul(beta, lnl), lq_fwd, inside, prop, tmul(beta, lnl_p), tmul(beta, g_p), tmul(beta, F_p), eps, ridge)
        accept = np.log(sr.accept_uniform(seed, chains, S)) < la
        u = np.where(accept[:, None], prop, u)
        lnl, g, F = np.where(accept, lnl_p, lnl), np.where(accept[:, None], g_p, g), np.where(accept[:, None, None], F_p, F)
        if t < n_warmup:
            eps = eps * np.exp((t + 1.0) ** -0.6 * (np.exp(np.minimum(la, 0.0)) - target_accept))
        if swap_every > 0 and (S + 1) % swap_every == 0:
            perm, lower, sw, _, _ = swap_event(lnl, betas, (S + 1) // swap_every - 1, seed, chain0, S)
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


def trapezoid(betas, E):
    """sum_k (beta_k - beta_k+1) (E_k + E_k+1) / 2 over the trailing axis"""
    b, E = np.asarray(betas, np.float64), np.asarray(E, np.float64)
    return np.sum((b[:-1] - b[1:]) * (E[..., :-1] + E[..., 1:]) / 2.0, axis=-1)


__all__ = ["tmul", "swap_uniform", "swap_event", "temper_ref", "trapezoid"]
