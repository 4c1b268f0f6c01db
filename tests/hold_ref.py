"""float64 reference of the samplers' hold record (tests/test_hold_*.py; include/v21.h: v21_mlp_set_hold): the four
transitions of sample_ref, temper_ref / prior_ref, ensemble_ref and nested_ref in the FULL d-dimensional space with a
hold mask, written as the kernels are -- the masked system, the ridge on the free pivots, the dropped normal, d_free in
the normalisations -- so that tests/test_hold_cpu.py can pin them to the existing references on the reduced problem
(the held column dropped and its value folded into the evaluator), which is independent code.

A hold is the pair (mask (d,) bool, hu (d,) float64: the float32 the column carries, 0 where free).  A held column is no
parameter: its prior is never read (free_prior), d_free = the columns left.

    MALA / tempered   g_i = 0, F_ij = F_ji = 0, F_ii = 1 after the prior's additions; G = F + ridge diag(free);
                      xi_i = 0; u'_i = hu_i; log q normalised with d_free
    ensemble          log alpha = (d_free - 1) ln z + ...;  the stretch returns hu exactly
    nested            starts carry hu; the difference move returns it exactly"""
import math

import numpy as np

import ensemble_ref as er
import infer_cases as ic
import nested_ref as nr
import prior_ref as pr
import sample_ref as sr
import temper_ref as tr


def as_hold(mask, u):
    """mask (d,) of 0 / 1 and the held coordinates u (d,) float64 (read where held) -> (mask bool, hu: float32(u) as
    float64, 0 where free): rounded once, as the library does"""
    mask = np.asarray(mask).astype(bool)
    return mask, np.where(mask, np.asarray(u, np.float64).astype(np.float32).astype(np.float64), 0.0)


def uniform_prior(d):
    return pr.as_prior(np.zeros(d, np.int64), np.zeros(d), np.ones(d))


def free_prior(prior, hold):
    """the record the kernels get: the held normal columns made uniform"""
    kind, mu, sd = prior
    return pr.as_prior(np.where(hold[0], 0, kind), mu, sd)


def write_held(u, hold):
    """rows u (..., d) with the held coordinates written over theirs (a copy)"""
    return np.where(hold[0], hold[1].astype(np.asarray(u).dtype), u)


def reduce_rows(u, hold):
    """the free columns of rows (..., d)"""
    return np.asarray(u)[..., ~hold[0]]


def reduced_evaluator(ev, hold):
    """ev on d columns -> the evaluator of the reduced problem: the free columns in, the held value folded in, and of a
    (lnl, g, F) evaluator the free block out"""
    free = np.flatnonzero(~hold[0])

    def red(v):
        full = np.empty(v.shape[:-1] + (hold[0].size,))
        full[..., free] = v
        full[..., hold[0]] = hold[1][hold[0]]
        r = ev(full)
        if isinstance(r, tuple):
            return r[0], r[1][:, free], r[2][:, free][:, :, free]
        return r
    return red


def hold_eval(g, F, hold):
    """the masked system: g_i = 0, F_ij = F_ji = 0 (j != i), F_ii = 1 for a held i"""
    m = hold[0]
    g = np.where(m, 0.0, g)
    F = np.where(m[:, None] | m[None, :], np.eye(m.size), F)
    return g, F


def factor(F, ridge, hold):
    """sample_ref.factor of G = F + ridge diag(free): the ridge goes to the free pivots only"""
    G = np.asarray(F, np.float64) + ridge * np.diag((~hold[0]).astype(np.float64))
    return sr.factor(G, 0.0)


def logq(L, mu, ld, b, eps, d_free):
    v = np.einsum("nki,nk->ni", L, b - mu)
    return -np.sum(v * v, axis=1) / (2 * eps ** 2) + ld - 0.5 * d_free * np.log(2 * np.pi * eps ** 2)


def propose(u, g, F, eps, xi, ridge, hold):
    """sample_ref.propose on the masked system (g, F: the posterior's, not yet masked)"""
    g, F = hold_eval(g, F, hold)
    L, ok = factor(F, ridge, hold)
    mu, ld = sr.drift(L, u, g, eps)
    xi = np.where(hold[0], 0.0, xi)
    step = np.linalg.solve(np.swapaxes(L, 1, 2), xi[..., None])[..., 0]
    prop = write_held((mu + eps[:, None] * step).astype(np.float32).astype(np.float64), hold)
    inside = ok & np.all((prop >= -1.0) & (prop <= 1.0), axis=1)
    return prop, logq(L, mu, ld, prop, eps, int(np.sum(~hold[0]))), inside


def log_alpha(u, lnl, lq_fwd, inside, prop, lnl_p, g_p, F_p, eps, ridge, hold):
    g_p, F_p = hold_eval(g_p, F_p, hold)
    Lp, okp = factor(F_p, ridge, hold)
    mup, ldp = sr.drift(Lp, prop, g_p, eps)
    with np.errstate(invalid="ignore"):
        la = lnl_p - lnl + logq(Lp, mup, ldp, u, eps, int(np.sum(~hold[0]))) - lq_fwd
    return np.where(inside & okp & ~np.isnan(la), la, -np.inf)


def temper_ref(ev, prior, hold, u0, betas=(1.0,), swap_every=0, n_steps=1000, n_warmup=200, thin=1, eps0=1.0, ridge=1.0,
               target_accept=0.574, seed=0, chain0=0, step0=0, eps_start=None):
    """prior_ref.temper_ref with the hold (betas (1.0,), swap_every 0: the plain MALA chains of sample_ref under the
    prior).  ev: u (n, d) -> (lnl, g, F).  -> the same dict"""
    betas = np.asarray(betas, np.float64)
    T = betas.shape[0]
    prior = free_prior(prior, hold)
    u = write_held(np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32).astype(np.float64), hold)
    n, d = u.shape
    assert n % T == 0
    beta = betas[np.arange(n) % T]
    chains = chain0 + np.arange(n)
    eps = np.full(n, float(eps0)) if eps_start is None else np.asarray(eps_start, np.float64).copy()
    P = pr.precision(prior)[None]
    lnl, g, F = ev(u)
    keep = n_steps // thin if thin > 0 else 0
    su, suu, acc = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros(n)
    sl, sll, proposed, swapped_n = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    samples, samples_lnl = np.zeros((n, keep, d)), np.zeros((n, keep))
    prop, la, accept = u.copy(), np.zeros(n), np.ones(n, bool)
    for t in range(n_warmup + n_steps):
        S = step0 + t
        xi = sr.normals(seed, chains, S, d)
        prop, lq_fwd, inside = propose(u, tr.tmul(beta, g) + pr.grad_log_prior(prior, u), tr.tmul(beta, F) + P, eps, xi, ridge, hold)
        lnl_p, g_p, F_p = ev(prop)
        la = log_alpha(u, tr.tmul(beta, lnl) + pr.log_prior(prior, u), lq_fwd, inside, prop, tr.tmul(beta, lnl_p) + pr.log_prior(prior, prop),
                       tr.tmul(beta, g_p) + pr.grad_log_prior(prior, prop), tr.tmul(beta, F_p) + P, eps, ridge, hold)
        accept = np.log(sr.accept_uniform(seed, chains, S)) < la
        u = np.where(accept[:, None], prop, u)
        lnl, g, F = np.where(accept, lnl_p, lnl), np.where(accept[:, None], g_p, g), np.where(accept[:, None, None], F_p, F)
        if t < n_warmup:
            eps = eps * np.exp((t + 1.0) ** -0.6 * (np.exp(np.minimum(la, 0.0)) - target_accept))
        if swap_every > 0 and (S + 1) % swap_every == 0:
            perm, lower, sw, _, _ = tr.swap_event(lnl, betas, (S + 1) // swap_every - 1, seed, chain0, S)
            u, lnl, g, F = u[perm], lnl[perm], g[perm], F[perm]
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
    # (the finish kernels: the held mean is the value, its covariances exact zeros)
    mean = write_held(mean, hold)
    cov = np.where(hold[0][:, None] | hold[0][None, :], 0.0, cov)
    mean_lnl = sl / K if n_steps else lnl.copy()
    var_lnl = sll / K - mean_lnl ** 2 if n_steps else np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        swap_accept = np.where(proposed > 0, swapped_n / np.maximum(proposed, 1), 0.0)
    return {"u": u, "lnl": lnl, "eps": eps, "accept_rate": acc / K, "mean_u": mean, "cov_u": cov, "samples_u": samples,
            "samples_lnl": samples_lnl, "last_prop_u": prop, "last_log_alpha": la, "last_accept": accept, "mean_lnl": mean_lnl,
            "var_lnl": var_lnl, "swap_accept": swap_accept}


def ensemble_ref(ev, hold, u0, n_walkers, a=2.0, n_steps=1000, n_warmup=500, thin=1, seed=0, chain0=0, step0=0, prior=None,
                 count_held=False):
    """ensemble_ref.ensemble_ref with the hold (and the prior's ln p(y) - ln p(x), prior None: uniform): the starts carry
    the held value, log alpha takes (d_free - 1) ln z.  count_held=True is the deliberately WRONG variant with
    (d - 1) ln z, for the control.  -> the same dict"""
    u = write_held(np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32).astype(np.float64), hold)
    n, d = u.shape
    prior = free_prior(uniform_prior(d) if prior is None else prior, hold)
    dz = d if count_held else int(np.sum(~hold[0]))
    W, H = int(n_walkers), int(n_walkers) // 2
    assert W % 2 == 0 and n % W == 0
    e, h, _ = er.layout(n, W)
    sets = [np.flatnonzero(h == hh) for hh in (0, 1)]
    chains = chain0 + np.arange(n)
    lnl = np.zeros(n)
    for idx in sets:
        lnl[idx] = er._lnl(ev, u[idx])
    keep = n_steps // thin if thin > 0 else 0
    su, suu, acc = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros(n)
    samples, samples_lnl = np.zeros((n, keep, d)), np.zeros((n, keep))
    prop, la, partner, accept = u.copy(), np.zeros(n), np.full(n, -1), np.ones(n, bool)
    for t in range(n_warmup + n_steps):
        z, k, logu = er.draws(seed, chains, step0 + t, a, H)
        for hh, idx in enumerate(sets):
            prt = e[idx] * W + (1 - hh) * H + k[idx]
            y = er.stretch(u[idx], u[prt], z[idx])
            assert np.array_equal(y[:, hold[0]], u[idx][:, hold[0]])  # (the stretch returns a held coordinate exactly)
            inside = np.all((y >= -1.0) & (y <= 1.0), axis=1)
            lnl_y = er._lnl(ev, y)
            with np.errstate(invalid="ignore"):
                l = (dz - 1) * np.log(z[idx]) + (lnl_y - lnl[idx]) + (pr.log_prior(prior, y) - pr.log_prior(prior, u[idx]))
            l = np.where(inside & ~np.isnan(l), l, -np.inf)
            ok = logu[idx] < l
            u[idx] = np.where(ok[:, None], y, u[idx])
            lnl[idx] = np.where(ok, lnl_y, lnl[idx])
            prop[idx], la[idx], partner[idx], accept[idx] = y, l, prt - e[idx] * W, ok
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
    mean = write_held(mean, hold)
    cov = np.where(hold[0][:, None] | hold[0][None, :], 0.0, cov)
    return {"u": u, "lnl": lnl, "accept_rate": acc / K, "mean_u": mean, "cov_u": cov, "samples_u": samples, "samples_lnl": samples_lnl,
            "last_prop_u": prop, "last_log_alpha": la, "last_partner": partner, "last_accept": accept}


def start_draws(prior, hold, seed, rows, d):
    """the nested sampler's drawn starts with the hold: prior_ref.start_draws' words for the free columns (a held column
    consumes none of its own: the others keep theirs), the held value in the held ones; float32"""
    return write_held(pr.start_draws(free_prior(prior, hold), seed, rows, d), hold)


def nested_ref(ev, prior, hold, u0, n_live, n_iter, n_repeats=None, gamma=None, seed=0, iter0=0, chain0=0, lnl0=None):
    """prior_ref.nested_ref with the hold: the starts (given, or drawn by start_draws) get the held coordinates written, the
    prior is the free columns', and the difference move must return a held coordinate exactly (asserted).  The prior's
    acceptance draw is made only where a free normal column is left, as the launch site picks its kernel.  n_repeats and
    gamma default on d, as the library's do.  -> prior_ref.nested_ref's dict"""
    d = hold[0].size
    fp = free_prior(prior, hold)
    N = int(n_live)
    u0 = write_held(np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32), hold)
    r = pr.nested_ref(ev, fp, u0, N, n_iter, n_repeats=n_repeats or nr.default_repeats(d), gamma=gamma or nr.default_gamma(d), seed=seed,
                      iter0=iter0, chain0=chain0, lnl0=lnl0, use_prior=bool(np.any(fp[0] == 1)))
    for k in ("dead_u", "live_u", "last_prop_u"):
        assert np.array_equal(r[k][..., hold[0]], np.broadcast_to(hold[1][hold[0]].astype(np.float32), r[k][..., hold[0]].shape)), k
    return r


# ---- the cases tests/test_hold_cpu.py and tests/test_hold_gpu.py share
HELD_U = 0.4  # the conditional evidence problem: i2 with column 1 held here
# Cells of its midpoint rule.  The integral is one-dimensional, so this is the 1-D grid of infer_cases (GRID["i1"]), not the
# per-axis count of the 2-D one: with GRID["i2"] = 1,024 cells and half of them the rule differs by 1.3e-5 (the ReLU kinks
# leave it second order in the spacing), which misses the 1e-6 the truth is asked to be known to; with 16,384 and 8,192
# it differs by 5e-8.
QUAD_CELLS = ic.GRID["i1"]
# Its ladder: the tempering tests' power law on 32 rungs, LADDERS ladders, their run.  On their 8 rungs the trapezoid of the
# quadrature's own E_beta[ln L] is 0.142 nats below the integral -- the discretisation bias that sample_tempered's
# docstring describes, 16 of the reference's standard errors here, where one column is left uniform --, on 16 rungs
# 0.031, on 32 rungs 0.007, below one standard error.
HELD_RUNGS = 32
HELD_BETAS = ((HELD_RUNGS - 1.0 - np.arange(HELD_RUNGS)) / (HELD_RUNGS - 1.0)) ** 5


def held_ladder_lz(mean_lnl):
    """per-ladder trapezoids of a run on HELD_BETAS -> (mean, standard error)"""
    lz = tr.trapezoid(HELD_BETAS, np.asarray(mean_lnl, np.float64).reshape(ic.LADDERS, HELD_RUNGS))
    return lz.mean(), lz.std(ddof=1) / math.sqrt(ic.LADDERS)


def held_starts():
    """every rung of a ladder at its ladder's start (infer_cases.problem's, one per ladder)"""
    return np.repeat(ic.problem("i2")["starts_u"][::ic.RUNGS], HELD_RUNGS, axis=0)


# the flat-likelihood ensemble case: infer_cases.FLAT_ENSEMBLE (d = 4, W = 16) sized on the reference until the control of
# tests/test_hold_cpu.py misses by 4 N_SE: at FLAT_ENSEMBLE's own 64 ensembles and 600 kept sweeps the wrong Jacobian's second moments were
# 15.9 to 18.3 standard errors off, and the distance grows as the square root of both counts
FLAT_ENSEMBLE = dict(ic.FLAT_ENSEMBLE, ensembles=128, opts=dict(ic.FLAT_ENSEMBLE["opts"], n_steps=1200))
FLAT_HOLD = ([0, 0, 0, 1], [0.0, 0.0, 0.0, 0.25])

_quad = {}


def held_hold():
    return as_hold([0, 1], [0.0, HELD_U])


def conditional_quadrature():
    """ln Z of i2 with column 1 at float32(0.4): the mean of L over column 0, by the midpoint rule with QUAD_CELLS cells and
    with half of them; and E_beta[ln L] at HELD_BETAS on the fine grid"""
    if "quad" not in _quad:
        p = ic.problem("i2")
        out = []
        for N in (QUAD_CELLS, QUAD_CELLS // 2):
            c = (np.arange(N) + 0.5) * (2.0 / N) - 1.0
            g = p["ev"](np.stack([c, np.full(N, held_hold()[1][1])], -1))[0]
            out.append((g.max() + math.log(np.sum(np.exp(g - g.max())) / N), ic.expectations(g, HELD_BETAS)))
        _quad["quad"] = (out[0][0], out[1][0], out[0][1])
    return _quad["quad"]


__all__ = ["as_hold", "uniform_prior", "free_prior", "write_held", "reduce_rows", "reduced_evaluator", "hold_eval", "factor", "logq",
           "propose", "log_alpha", "temper_ref", "ensemble_ref", "start_draws", "nested_ref"]
