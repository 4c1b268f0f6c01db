"""Cases the inference-side tests share between their CPU and GPU files and with the scripts (no GPU needed): the named
stacks and their transforms, the tempering problems with their quadrature, the nested sampler's sizes and quadrature cases,
the priors with their flat-likelihood runs and evidence problems, and the bounds the sampler tests have in common.  Built on
the float64 references (tests/*_ref.py) and tests/shape_cases.py; whatever is computed here is computed once."""
import math

import numpy as np

import ensemble_ref as er
import helpers
import jacobian_ref as jr
import nested_ref as nr
import prior_ref as pr
import sample_ref as sr
import shape_cases as sc
import temper_ref as tr
from conftest import pkg

N_SE = 5.0     # the statistical tests' bound, in standard errors
SPREAD = 0.05  # the walkers' and live points' spread around the truth in u (tests/test_ensemble_gpu.py says why)

# ---- the named stacks
# a 7-input variational stack: 7 -> 64 -> (gauss 9) -> 32 -> 451
VG = ([7, 64, 9, 32, 451], [1, 2, 1, 0])
# the four stacks with a fused kernel (csrc/archs.h) and their activations
ARCHS = {"S1": helpers.STACKS["D1"], "S2": helpers.STACKS["DE"], "S3": helpers.STACKS["S3"],
         "S4": helpers.STACKS["S4"]}
# Reduced-precision bounds of the forward on Glorot-uniform weights, outputs O(1) (observed r2: f16 max|d| ~1e-4,
# bf16 ~1e-3): max |device - fp64 oracle| and the reference's metric (emulator.py:188-191) in percent.
HALF_BOUNDS = {"f16": dict(max_abs=1e-3, mean_pct=0.05), "bf16": dict(max_abs=1e-2, mean_pct=0.4)}


def vg_weights(seed):
    dims, act = VG
    rng = np.random.default_rng(seed)
    Ws, bs = [], []
    for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
        nw = 2 * n if act[l] == 2 else n
        lim = np.sqrt(6.0 / (k + nw))
        Ws.append(rng.uniform(-lim, lim, size=(k, nw)).astype(np.float32))
        bs.append(rng.normal(scale=0.05, size=nw).astype(np.float32))
    return Ws, bs


def weights_of(name, seed=3):
    if name == "VG":
        return VG[0], VG[1], *vg_weights(seed)
    dims, act = helpers.STACKS[name]
    Ws, bs, _ = helpers.init_weights(dims, seed)
    return dims, act, Ws, bs


def transforms(seed, dtype=np.float64):
    synth, pp = pkg("synth"), pkg("preprocess")
    par_train = synth.make_params(2000, seed=seed, corners=True)
    ps = pp.ParamStats(par_train)
    sig = synth.make_signals(500, seed=seed + 1)
    tin = (ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
    tout = (float(np.std(sig)), np.mean(sig, axis=0))
    return tin, tout, synth.make_params(600, seed=seed + 7, zero_fx_frac=0).astype(dtype)


# ---- parallel tempering
# The two quadrature problems: a 1-input stack of the table and a 2-input stack of the same make, one noisy spectrum of a
# truth inside the box at SIGMA (in units of shape_cases.OUT_STD) on every bin.  Chosen on the reference: at SIGMA = 0.1,
# data seed 17 and 200 + 600 transitions every |z| below stayed under 1.5 (at SIGMA = 0.05 and 200 + 400 the worst was 3.2).
STACKS = {"i1": (sc.BY_NAME["i1o63"].dims, sc.BY_NAME["i1o63"].act), "i2": ([2, 16, 63], [sc.RELU, sc.LINEAR])}
SIGMA, DATA_SEED = 0.1, 17
LADDERS, RUNGS = 64, 8
BETAS = ((RUNGS - 1.0 - np.arange(RUNGS)) / (RUNGS - 1.0)) ** 5
RUN = dict(n_steps=600, n_warmup=200, thin=0, seed=3)
SWAP_EVERY = 5
GRID = {"i1": 16384, "i2": 1024}  # cells per axis of the midpoint rule (and half of it, for the convergence check)

# the swap test: (rungs, ladders) -- 666, 513, 515 and 288 rows, a partial last workgroup at every T -- on i4o65 from
# starts scattered over the box, ladders evenly spaced in beta
SWAP_CASES = [(2, 333), (3, 171), (5, 103), (32, 9)]
SWAP_SEED = 11

_problems, _quad = {}, {}


def swap_betas(T):
    return np.linspace(1.0, 0.0, T)


def scattered_u(d, n, seed):
    """n starts uniform in [-0.9, 0.9]^d"""
    return np.random.default_rng(seed).uniform(-0.9, 0.9, size=(n, d))


def problem(name):
    """-> dict dims, act, stack (shape_cases.make_stack), truth_u (d,), data float32 (out,), w float32 (out,), ev: the
    float64 evaluator u (n, d) -> (lnl, g, F) of sample_ref, starts_u (LADDERS RUNGS, d): every rung of a ladder at its
    ladder's start, the truth jittered by 0.02"""
    if name not in _problems:
        dims, act = STACKS[name]
        st = sc.make_stack(dims, act)
        rng = np.random.default_rng(DATA_SEED)
        tu = rng.uniform(-0.5, 0.5, size=(1, dims[0]))
        y = jr.jvp(st["Ws"], st["bs"], st["act"], tu)[0][0] * st["tout"][0] + st["tout"][1]
        sig = SIGMA * sc.OUT_STD
        data = (y + rng.normal(size=y.shape) * sig).astype(np.float32)
        w = np.full(dims[-1], 1.0 / sig ** 2, np.float32)
        u0 = np.clip(tu + 0.02 * np.random.default_rng(1).normal(size=(LADDERS, dims[0])), -1.0, 1.0)
        _problems[name] = {"dims": dims, "act": act, "stack": st, "truth_u": tu[0], "data": data, "w": w,
                           "ev": sr.evaluator_batch(st["Ws"], st["bs"], st["act"], data, w, st["tout"]),
                           "starts_u": np.repeat(u0, RUNGS, axis=0)}
    return _problems[name]


def lnl_grid(p, N):
    """ln L of the float64 oracle at the midpoints of N^d equal cells of the box"""
    st, d = p["stack"], p["dims"][0]
    c = (np.arange(N) + 0.5) * (2.0 / N) - 1.0
    pts = c[:, None] if d == 1 else np.stack(np.meshgrid(c, c, indexing="ij"), -1).reshape(-1, 2)
    dat, w = p["data"].astype(np.float64), p["w"].astype(np.float64)
    out = []
    for i in range(0, len(pts), 65536):
        y = jr.jvp(st["Ws"], st["bs"], st["act"], pts[i:i + 65536])[0] * st["tout"][0] + st["tout"][1]
        out.append(-0.5 * np.sum(w * (dat - y) ** 2, axis=-1))
    return np.concatenate(out)


def expectations(lnl, betas):
    """E_beta[ln L] = sum ln L L^beta / sum L^beta over equal cells, per beta"""
    out = []
    for b in betas:
        a = b * lnl
        wt = np.exp(a - a.max())
        out.append(np.sum(wt * lnl) / np.sum(wt))
    return np.array(out)


def quadrature(name):
    """-> (E_beta[ln L] at BETAS on the fine grid, the same on a grid of twice the spacing); computed once"""
    if name not in _quad:
        p = problem(name)
        _quad[name] = (expectations(lnl_grid(p, GRID[name]), BETAS), expectations(lnl_grid(p, GRID[name] // 2), BETAS))
    return _quad[name]


def ladder_check(mean_lnl, name):
    """per-row mean ln L (LADDERS RUNGS,) against the quadrature -> (z per rung, z of the trapezoid, standard errors per
    rung): the standard error is the scatter over ladders, the trapezoid's that of the ladders' own trapezoids"""
    q, _ = quadrature(name)
    E = np.asarray(mean_lnl, np.float64).reshape(LADDERS, RUNGS)
    se = E.std(axis=0, ddof=1) / np.sqrt(LADDERS)
    lz = tr.trapezoid(BETAS, E)
    z_lz = (lz.mean() - tr.trapezoid(BETAS, q)) / (lz.std(ddof=1) / np.sqrt(LADDERS))
    return (E.mean(axis=0) - q) / se, z_lz, se


# ---- the nested sampler
RUNS, SEED = 64, 0
QUAD = {"i1": (32, 40), "i2": (64, 40)}  # live points, iterations: X_T = e^-27.7, nothing is left in the live points

_nested_quad = {}


def run_stats(r, N, runs, shrink="harmonic"):
    """per-run (ln Z, error) of a reference or device result"""
    ev = [nr.evidence(r["dead_lnl"][:, e], r["live_lnl"].reshape(runs, N)[e], N, shrink) for e in range(runs)]
    return np.array([v[0] for v in ev]), np.array([v[1] for v in ev])


def z_of(lz, truth):
    return (lz.mean() - truth) / (lz.std(ddof=1) / math.sqrt(len(lz)))


def quadrature_case(name):
    """-> (problem, ln Z by the midpoint rule, the reference's result, its per-run ln Z); computed once"""
    if name not in _nested_quad:
        p = problem(name)
        d, (N, T) = p["dims"][0], QUAD[name]
        g = lnl_grid(p, GRID[name])
        m = g.max()
        lz_q = m + math.log(np.sum(np.exp(g - m))) - d * math.log(GRID[name])
        st = p["stack"]
        ev = er.forward_evaluator(st["Ws"], st["bs"], st["act"], p["data"], p["w"], st["tout"])
        r = nr.nested_ref(ev, nr.start_draws(SEED, np.arange(RUNS * N), d), N, T, seed=SEED)
        _nested_quad[name] = (p, lz_q, r, run_stats(r, N, RUNS)[0])
    return _nested_quad[name]


# ---- the priors
BETAS3 = np.array([1.0, 0.3, 0.0])


def mixed_prior(d):
    """the mixed record of a d-column stack: two normal columns, the second with mu outside the box by 2 sd, the rest
    uniform (d = 1: the one column normal with mu outside the box by 2 sd)"""
    kind, mu, sd = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    if d == 1:
        kind[0], mu[0], sd[0] = 1, 1.3, 0.15
        return pr.as_prior(kind, mu, sd)
    a, b = (1, 4) if d >= 5 else (0, d - 1)
    kind[a], mu[a], sd[a] = 1, 0.3, 0.25
    kind[b], mu[b], sd[b] = 1, -1.4, 0.2
    return pr.as_prior(kind, mu, sd)


# the flat-likelihood runs of test_prior_gpu.test_flat_likelihood_*: (chains or ladders or ensembles, options)
FLAT_MALA = dict(d=7, chains=256, opts=dict(n_steps=600, n_warmup=150, thin=0, seed=5))
FLAT_TEMPER = dict(d=2, ladders=256, swap_every=1, opts=dict(n_steps=600, n_warmup=150, thin=0, seed=6))
FLAT_ENSEMBLE = dict(d=4, W=16, ensembles=64, opts=dict(n_steps=600, n_warmup=300, thin=0, seed=7))


def flat_starts(d, n, seed):
    return scattered_u(d, n, seed)


def moment_z(mean_c, m2_c, prior):
    """z of the per-chain (or per-ensemble) estimates of E[u] and E[u^2] against the prior's closed form"""
    m, v = pr.moments(prior)
    return sr.pooled_check(mean_c, m)[1], sr.pooled_check(m2_c, v + m * m)[1]


def second_moment(r):
    return np.diagonal(r["cov_u"], axis1=1, axis2=2) + r["mean_u"] ** 2


def near(truth_u, n, seed, scale):
    return np.clip(truth_u[None, :] + scale * np.random.default_rng(seed).normal(size=(n, len(truth_u))), -0.999, 0.999)


# the evidence problems: problem(name) under a normal on every column, 0.05 off the truth and 0.05 wide.  (With a
# column left uniform the 8-rung trapezoid of the 2-input problem is 0.26 nats off the integral, 20 standard errors: the
# discretisation bias sample_tempered's docstring describes.  With both columns constrained it is below one.)
def evidence_prior(name):
    p = problem(name)
    d = p["dims"][0]
    return pr.as_prior(np.ones(d, np.int32), np.round(p["truth_u"] + 0.05, 3), np.full(d, 0.05))


_prior_quad, _tref, _nref = {}, {}, {}


def evidence_quadrature(name):
    """-> (ln Z under the prior, ln Z under the uniform prior, E_beta[ln L] under L^beta p at BETAS) by the midpoint rule"""
    if name not in _prior_quad:
        p, prior = problem(name), evidence_prior(name)
        N, d = GRID[name], p["dims"][0]
        c = (np.arange(N) + 0.5) * (2.0 / N) - 1.0
        pts = c[:, None] if d == 1 else np.stack(np.meshgrid(c, c, indexing="ij"), -1).reshape(-1, 2)
        g, lp = lnl_grid(p, N), pr.log_prior(prior, pts)
        lse = lambda a: a.max() + math.log(np.sum(np.exp(a - a.max())))
        E = []
        for b in BETAS:
            a = b * g + lp
            wt = np.exp(a - a.max())
            E.append(np.sum(wt * g) / np.sum(wt))
        _prior_quad[name] = (lse(g + lp) - lse(lp), lse(g) - d * math.log(N), np.array(E))
    return _prior_quad[name]


def tempered_reference(name):
    """prior_ref.temper_ref on the problem at the tempering tests' ladder and run; computed once"""
    if name not in _tref:
        p = problem(name)
        _tref[name] = pr.temper_ref(p["ev"], evidence_prior(name), p["starts_u"], BETAS, swap_every=SWAP_EVERY, **RUN)
    return _tref[name]


def nested_reference(name):
    """prior_ref.nested_ref on the problem from starts drawn from the prior, at the nested tests' sizes; -> (result, ln Z per run)"""
    if name not in _nref:
        p, prior = problem(name), evidence_prior(name)
        d, (N, T) = p["dims"][0], QUAD[name]
        st = p["stack"]
        ev = er.forward_evaluator(st["Ws"], st["bs"], st["act"], p["data"], p["w"], st["tout"])
        r = pr.nested_ref(ev, prior, pr.start_draws(prior, SEED, np.arange(RUNS * N), d), N, T, seed=SEED)
        _nref[name] = (r, run_stats(r, N, RUNS)[0])
    return _nref[name]


def ladder_lz(mean_lnl):
    """per-ladder trapezoids of a tempered run's mean ln L -> (mean, standard error)"""
    lz = tr.trapezoid(BETAS, np.asarray(mean_lnl, np.float64).reshape(LADDERS, RUNGS))
    return lz.mean(), lz.std(ddof=1) / math.sqrt(LADDERS)
