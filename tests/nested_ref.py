"""float64 reference of the nested sampler (tests/test_nested_*.py; include/v21.h: v21_mlp_sample_nested): the iteration of
csrc/nested_kernels.h batched over runs, on the Philox helpers of tests/sample_ref.py, and the evidence from a dead record.

N consecutive rows form one run, k = N / 2.  Iteration t ranks the run's ln L ascending (ties on the row index, NaN as
-inf); the k lowest are the dead points, L* the ln L at rank k - 1, the survivor of rank r moves to row r.  Row j < k then
becomes a copy of survivor floor(k w0 / 2^32) (block 1 of (seed, chain0 + row, t)) and moves n_repeats times:
    y = float32(x + float32(gamma float32(x_a - x_b))),   a = floor(k w0 / 2^32), b = (a + 1 + floor((k - 1) w1 / 2^32)) mod k
from block 0 of (seed, chain0 + row, t n_repeats + s), accepted iff y is inside [-1, 1]^d and ln L(y) > L*.

Run as a script it prints the bias table of the shipped defaults on an analytic Gaussian, the table the lower bound on N
(max(16, 8 d)) rests on."""
import math

import numpy as np

import sample_ref as sr


def default_gamma(d):
    return 2.38 / math.sqrt(2.0 * d)


def default_repeats(d):
    return 3 * d


def slot_rows(runs, N, chain0=0):
    """global rows (runs, k) of the moving slots"""
    return chain0 + np.arange(runs)[:, None] * N + np.arange(N // 2)[None, :]


def rank_order(lnl):
    """(runs, N) ln L -> order (runs, N): order[e, r] is the row of rank r (ascending, ties on the row index, NaN as -inf)"""
    key = np.where(np.isnan(lnl), -np.inf, lnl)
    return np.argsort(key, axis=1, kind="stable")


def _hi(m, w):
    return ((np.uint64(m) * w.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def restart_draws(seed, rows, t, k):
    """the survivor index (runs, k) each moving slot restarts from in global iteration t"""
    w = sr.block(seed, rows.reshape(-1), t, 1)
    return _hi(k, w[:, 0]).reshape(rows.shape)


def move_draws(seed, rows, c, k):
    """the partners (a, b), survivor indices (runs, k), of global move c"""
    w = sr.block(seed, rows.reshape(-1), c, 0)
    a = _hi(k, w[:, 0])
    b = (a + 1 + _hi(k - 1, w[:, 1])) % k
    return a.reshape(rows.shape), b.reshape(rows.shape)


def start_draws(seed, rows, d):
    """drawn start rows (len(rows), d): float32(2 U(w) - 1), coordinate i from word i % 4 of block 2 + i // 4, step 0"""
    w = np.concatenate([sr.block(seed, rows, 0, 2 + b) for b in range((d + 3) // 4)], axis=1)[:, :d]
    return (2.0 * sr.uniform(w) - 1.0).astype(np.float32)


def propose(x, xa, xb, gamma):
    """the difference move in the device's float32 operation order"""
    x, xa, xb = (np.asarray(v, np.float32) for v in (x, xa, xb))
    return x + np.float32(gamma) * (xa - xb)


def _lnl(ev, u):
    r = ev(np.asarray(u, np.float64))
    return np.asarray(r[0] if isinstance(r, tuple) else r, np.float64)


def nested_ref(ev, u0, n_live, n_iter, n_repeats=None, gamma=None, seed=0, iter0=0, chain0=0, slack=None, lnl0=None):
    """The runs of csrc/nested_kernels.h (the state is float32 u, as there; ln L whatever ev returns, widened).  ev: u
    (m, d) -> ln L (m,), or a tuple whose first entry it is.  u0: (n, d) live points.  slack: None, or the deliberately
    WRONG rule that accepts on ln L(y) >= L* - slack, for the controls.  lnl0: the start rows' ln L (n,), instead of ev's.
    -> dict dead_u (T, runs, k, d), dead_lnl, lstar (T, runs), live_u (n, d), live_lnl, accept_rate (runs, k),
    last_partner (runs, k, 2), last_prop_u (runs, k, d), n_evals"""
    u = np.clip(np.asarray(u0, np.float64), -1.0, 1.0).astype(np.float32)
    n, d = u.shape
    N, k, T = int(n_live), int(n_live) // 2, int(n_iter)
    assert N % 2 == 0 and n % N == 0
    runs = n // N
    R = default_repeats(d) if not n_repeats else int(n_repeats)
    g = np.float32(default_gamma(d) if not gamma else gamma)
    u = u.reshape(runs, N, d)
    lnl = (_lnl(ev, u.reshape(n, d)) if lnl0 is None else np.asarray(lnl0, np.float64)).reshape(runs, N)
    lnl = np.where(np.isnan(lnl), -np.inf, lnl)
    rows, e = slot_rows(runs, N, chain0), np.arange(runs)[:, None]
    dead_u, dead_lnl, lstar = np.zeros((T, runs, k, d), np.float32), np.zeros((T, runs, k)), np.zeros((T, runs))
    acc = np.zeros((runs, k))
    pa = pb = np.full((runs, k), -1)
    prop = u[:, k:].copy()
    for t in range(T):
        order = rank_order(lnl)
        u, lnl = np.take_along_axis(u, order[:, :, None], axis=1), np.take_along_axis(lnl, order, axis=1)
        dead_u[t], dead_lnl[t], lstar[t] = u[:, :k], lnl[:, :k], lnl[:, k - 1]
        c = restart_draws(seed, rows, iter0 + t, k)
        u[:, :k], lnl[:, :k] = u[e, k + c], lnl[e, k + c]
        for s in range(R):
            pa, pb = move_draws(seed, rows, (iter0 + t) * R + s, k)
            prop = propose(u[:, :k], u[e, k + pa], u[e, k + pb], g)
            inside = np.all((prop >= -1.0) & (prop <= 1.0), axis=2)
            lnl_y = _lnl(ev, prop.reshape(-1, d)).reshape(runs, k)
            with np.errstate(invalid="ignore"):
                above = lnl_y > lstar[t][:, None] if slack is None else lnl_y >= lstar[t][:, None] - slack
            ok = inside & above
            u[:, :k] = np.where(ok[:, :, None], prop, u[:, :k])
            lnl[:, :k] = np.where(ok, lnl_y, lnl[:, :k])
            acc += ok
    return {"dead_u": dead_u, "dead_lnl": dead_lnl, "lstar": lstar, "live_u": u.reshape(n, d), "live_lnl": lnl.reshape(n),
            "accept_rate": acc / max(T * R, 1), "last_partner": np.stack([pa, pb], axis=-1), "last_prop_u": prop,
            "n_evals": n + runs * k * T * R}


def evidence(dead_lnl, live_lnl, n_live, shrink="harmonic"):
    """ln Z, its error, the information H and the normalised log weights (dead points t-major, then the live points) of
    ONE run: dead_lnl (T, k), live_lnl (N,).  After the death of rank r of iteration t the volume is
    ln X = -t s_k - sum_{i <= r} 1 / (N - i).  shrink="ratio" is the deliberately WRONG rule 1 / N per death (k / N per
    iteration), for the controls."""
    dl, ll = np.asarray(dead_lnl, np.float64), np.asarray(live_lnl, np.float64)
    N = int(n_live)
    T, k = dl.shape
    step = 1.0 / (N - np.arange(k)) if shrink == "harmonic" else np.full(k, 1.0 / N)
    cum = np.cumsum(step)
    s_k, v_k = cum[-1], np.sum(step ** 2)
    prev = -np.arange(T)[:, None] * s_k - np.concatenate([[0.0], cum[:-1]])[None, :]
    lw = np.concatenate([(dl + prev + np.log(-np.expm1(-step))[None, :]).reshape(-1), ll - T * s_k - math.log(N)])
    m = lw.max()
    lz = m + math.log(np.sum(np.exp(lw - m)))
    lw = lw - lz
    both = np.concatenate([dl.reshape(-1), ll])
    w = np.exp(lw)
    H = np.sum(np.where(w > 0, w * np.where(w > 0, both, 0.0), 0.0)) - lz
    return lz, math.sqrt(max(H, 0.0) * v_k / s_k), H, lw


# ---- the analytic target: an isotropic Gaussian of width sigma in u, centred in the box
def gauss_lnl(sigma):
    return lambda u: -0.5 * np.sum(np.asarray(u, np.float64) ** 2, axis=-1) / sigma ** 2


def gauss_lnz(d, sigma):
    """ln of the mean of exp(gauss_lnl) over [-1, 1]^d (the walls included)"""
    return d * math.log(math.sqrt(2.0 * math.pi) * sigma * math.erf(1.0 / (sigma * math.sqrt(2.0))) / 2.0)


def table(cases=((7, 256), (7, 64), (7, 56), (2, 64), (2, 16), (1, 32), (1, 16)), runs=64, sigma=0.1, seed=1):
    """bias of ln Z at the shipped defaults on the Gaussian, in units of the standard error of the mean over the runs"""
    out = []
    for d, N in cases:
        T = int(math.ceil((d * math.log(1.0 / sigma) + 12.0) / np.sum(1.0 / (N - np.arange(N // 2)))))
        u0 = start_draws(seed, np.arange(runs * N), d)
        r = nested_ref(gauss_lnl(sigma), u0, N, T, seed=seed)
        ev = [evidence(r["dead_lnl"][:, e], r["live_lnl"].reshape(runs, N)[e], N) for e in range(runs)]
        lz, err = np.array([v[0] for v in ev]), np.array([v[1] for v in ev])
        se = lz.std(ddof=1) / math.sqrt(runs)
        out.append((d, N, T, lz.mean() - gauss_lnz(d, sigma), se, lz.std(ddof=1), err.mean(), r["accept_rate"].mean()))
    return out


if __name__ == "__main__":
    for row in table():
        print("d=%d N=%3d T=%3d: bias %+.3f +- %.3f (z %+.2f), scatter %.3f, formula %.3f, accept %.2f"
              % (row[:5] + (row[3] / row[4],) + row[5:]))
