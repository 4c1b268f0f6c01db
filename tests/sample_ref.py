"""float64 reference of the posterior sampler (tests/test_sample_*.py; include/v21.h: v21_mlp_sample): Philox4x32-10, the
word-to-draw mapping, and the Fisher-preconditioned MALA transition of csrc/sample_kernels.h batched over chains, on the
evaluator of tests/fit_ref.py / tests/jacobian_ref.py.

One transition, with G(u) = F(u) + ridge I = L L^T, d parameters, step size e:
    mu(u) = u + e^2 / 2 G(u)^-1 g(u);   u' = float32(mu(u) + e L(u)^-T xi),  xi ~ N(0, I_d)
    log q(b | a) = -|L(a)^T (b - mu(a))|^2 / (2 e^2) + sum_i log L_ii(a) - d / 2 log(2 pi e^2)
    log alpha = lnL(u') - lnL(u) + log q(u | u') - log q(u' | u);   accept iff log(uniform) < log alpha
A proposal outside [-1, 1]^d (or whose G has no Cholesky factor) is rejected, log alpha = -inf.  Warm-up transition
t = 1 .. n_warmup: log e += t^-0.6 (min(1, alpha) - target_accept)."""
import numpy as np

import jacobian_ref as jr

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """counters (..., 4) and keys (..., 2) of 32-bit words -> (..., 4) uint32"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k0 = np.asarray(key)[..., 0].astype(np.uint64) & MASK
    k1 = np.asarray(key)[..., 1].astype(np.uint64) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def block(seed, chains, step, b):
    """the four words of draw block b of transition `step` of the global chains `chains` (n,) -> (n, 4) uint32"""
    chains = np.asarray(chains, np.uint64)
    ctr = np.stack([chains & MASK, chains >> np.uint64(32), np.full_like(chains, int(step)), np.full_like(chains, int(b))], axis=-1)
    seed = int(seed)
    return philox4x32_10(ctr, np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64), ctr.shape[:-1] + (2,)))


def uniform(w):
    return (np.asarray(w, np.float64) + 0.5) * 2.0 ** -32


def normals(seed, chains, step, din):
    """xi (n, din): blocks 0 and 1, Box-Muller on the word pairs (w0, w1) and (w2, w3) of each"""
    cols = []
    for b in range((din + 3) // 4):
        w = block(seed, chains, step, b)
        for h in range(2):
            r, th = np.sqrt(-2.0 * np.log(uniform(w[:, 2 * h]))), 2.0 * np.pi * uniform(w[:, 2 * h + 1])
            cols += [r * np.cos(th), r * np.sin(th)]
    return np.stack(cols, axis=1)[:, :din]


def accept_uniform(seed, chains, step):
    """word 0 of block 2"""
    return uniform(block(seed, chains, step, 2)[:, 0])


def evaluator_batch(Ws, bs, act, data, w, tout=None):
    """u (n, in) -> (ln L (n,), gradient (n, in), Fisher (n, in, in)) in float64 of the stack on u; data (out,) or (n, out)"""
    std, mean = (1.0, 0.0) if tout is None else (float(tout[0]), np.asarray(tout[1], np.float64))
    d, w = np.asarray(data, np.float64), np.asarray(w, np.float64)

    def ev(u):
        y, J, _ = jr.jvp(Ws, bs, act, np.asarray(u, np.float64))
        y, J = y * std + mean, J * std
        r = d - y
        return -0.5 * np.sum(w * r * r, axis=-1), np.einsum("nk,njk->nj", w * r, J), np.einsum("nik,k,njk->nij", J, w, J)
    return ev


def factor(F, ridge):
    """(L (n, d, d), ok (n,)) of G = F + ridge I; rows without a finite factor get the identity and ok False"""
    G = np.asarray(F, np.float64) + ridge * np.eye(F.shape[-1])
    L = np.repeat(np.eye(F.shape[-1])[None], F.shape[0], axis=0)
    ok = np.all(np.isfinite(G), axis=(1, 2))
    try:
        L[ok] = np.linalg.cholesky(G[ok])
    except np.linalg.LinAlgError:  # (some row is not positive definite: one by one)
        for i in np.flatnonzero(ok):
            try:
                L[i] = np.linalg.cholesky(G[i])
            except np.linalg.LinAlgError:
                ok[i] = False
    return L, ok


def drift(L, u, g, eps):
    """(mu, sum log L_ii)"""
    z = np.linalg.solve(L, g[..., None])
    s = np.linalg.solve(np.swapaxes(L, 1, 2), z)[..., 0]
    return u + 0.5 * (eps ** 2)[:, None] * s, np.sum(np.log(np.diagonal(L, axis1=1, axis2=2)), axis=1)


def logq(L, mu, ld, b, eps):
    v = np.einsum("nki,nk->ni", L, b - mu)
    d = L.shape[-1]
    return -np.sum(v * v, axis=1) / (2 * eps ** 2) + ld - 0.5 * d * np.log(2 * np.pi * eps ** 2)


def propose(u, g, F, eps, xi, ridge):
    """-> (u' rounded to float32 (as float64), log q(u' | u), inside the box and drawable)"""
    L, ok = factor(F, ridge)
    mu, ld = drift(L, u, g, eps)
    step = np.linalg.solve(np.swapaxes(L, 1, 2), xi[..., None])[..., 0]
    prop = (mu + eps[:, None] * step).astype(np.float32).astype(np.float64)
    inside = ok & np.all((prop >= -1.0) & (prop <= 1.0), axis=1)
    return prop, logq(L, mu, ld, prop, eps), inside


def log_alpha(u, lnl, lq_fwd, inside, prop, lnl_p, g_p, F_p, eps, ridge):
    """log acceptance ratio of the proposals (-inf where rejected unread)"""
    Lp, okp = factor(F_p, ridge)
    mup, ldp = drift(Lp, prop, g_p, eps)
    with np.errstate(invalid="ignore"):
        la = lnl_p - lnl + logq(Lp, mup, ldp, u, eps) - lq_fwd
    la = np.where(inside & okp & ~np.isnan(la), la, -np.inf)
    return la


def sample_ref(ev, u0, n_steps=1000, n_warmup=200, thin=1, eps0=1.0, ridge=1.0, target_accept=0.574, seed=0, chain0=0, step0=0,
               eps_start=None, clamp=False):
    """The chains of csrc/sample_kernels.h in float64 (the state is the float32-rounded u, as there).  ev: u (n, d) ->
    (lnl, g, F).  clamp=True is a deliberately WRONG variant (a proposal outside the box is clipped onto it instead of
    rejected), for the control of the uniform-target test.
    -> dict u (n, d), lnl, eps, accept_rate, mean_u, cov_u, samples_u (n, n_steps // thin, d), samples_lnl, last_prop_u,
    last_log_alpha, last_accept"""
    u = np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32).astype(np.float64)
    n, d = u.shape
    chains = chain0 + np.arange(n)
    eps = np.full(n, float(eps0)) if eps_start is None else np.asarray(eps_start, np.float64).copy()
    lnl, g, F = ev(u)
    keep = n_steps // thin if thin > 0 else 0
    su, suu, acc = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros(n)
    samples, samples_lnl = np.zeros((n, keep, d)), np.zeros((n, keep))
    prop, la, accept = u.copy(), np.zeros(n), np.ones(n, bool)
    for t in range(n_warmup + n_steps):
        xi = normals(seed, chains, step0 + t, d)
        prop, lq_fwd, inside = propose(u, g, F, eps, xi, ridge)
        if clamp:
            prop = np.clip(prop, -1.0, 1.0)
            inside[:] = True
        lnl_p, g_p, F_p = ev(prop)
        la = log_alpha(u, lnl, lq_fwd, inside, prop, lnl_p, g_p, F_p, eps, ridge)
        accept = np.log(accept_uniform(seed, chains, step0 + t)) < la
        u = np.where(accept[:, None], prop, u)
        lnl, g, F = np.where(accept, lnl_p, lnl), np.where(accept[:, None], g_p, g), np.where(accept[:, None, None], F_p, F)
        if t < n_warmup:
            eps = eps * np.exp((t + 1.0) ** -0.6 * (np.exp(np.minimum(la, 0.0)) - target_accept))
        else:
            su += u
            suu += u[:, :, None] * u[:, None, :]
            acc += accept
            k = t - n_warmup + 1
            if thin > 0 and k % thin == 0 and k // thin <= keep:
                samples[:, k // thin - 1], samples_lnl[:, k // thin - 1] = u, lnl
    K = max(n_steps, 1)
    mean = su / K if n_steps else u.copy()
    cov = suu / K - mean[:, :, None] * mean[:, None, :] if n_steps else np.zeros((n, d, d))
    return {"u": u, "lnl": lnl, "eps": eps, "accept_rate": acc / K, "mean_u": mean, "cov_u": cov, "samples_u": samples,
            "samples_lnl": samples_lnl, "last_prop_u": prop, "last_log_alpha": la, "last_accept": accept}


def r_hat_from_samples(s):
    """the between / within-chain potential scale reduction of samples (chains, steps, d), per coordinate"""
    s = np.asarray(s, np.float64)
    n = s.shape[1]
    W = np.mean(np.var(s, axis=1, ddof=1), axis=0)
    B_over_n = np.var(np.mean(s, axis=1), axis=0, ddof=1)
    return np.sqrt(((n - 1.0) / n * W + B_over_n) / W)


def pooled_check(mean_c, ref_mean, n_se=5.0):
    """per-chain estimates (chains, ...) against a known value: |pooled - ref| in units of the pooled estimate's standard
    error, taken from the between-chain spread -> (pooled, z)"""
    mean_c = np.asarray(mean_c, np.float64)
    pooled = mean_c.mean(axis=0)
    se = mean_c.std(axis=0, ddof=1) / np.sqrt(mean_c.shape[0])
    return pooled, np.abs(pooled - ref_mean) / se


__all__ = ["philox4x32_10", "block", "uniform", "normals", "accept_uniform", "evaluator_batch", "propose", "log_alpha", "sample_ref",
           "r_hat_from_samples", "pooled_check", "factor", "drift", "logq"]
