"""Helpers of tests/test_lnl_cpu.py and tests/test_lnl_gpu.py: the forward-only log-likelihood (include/v21.h:
v21_mlp_loglike_fwd[_dev]).  The float64 reference is the reduction -1/2 sum w (d - y)^2 of a given y (on the GPU: the
device's own forward, which the fused ln L variant reproduces bit for bit by construction); the mutation catalogue
applies the ways the in-kernel reduction can go wrong to that same float64 reduction, so that the bound of the parity
test is shown to be tight enough to see each of them.  Built on jacobian_ref, marg_ref and shape_cases; modifies none."""
import numpy as np

import jacobian_ref as jr
import shape_cases as sc
from conftest import pkg
from helpers import STACKS, init_weights
from infer_cases import ARCHS, VG, transforms, vg_weights

# The parity bound of the fused route: worst |lnl - ref| / |ref| over every case of test_fused_parity.  Measured on the
# MI355X: worst 1.56e-7 (f32 2^-24 roundings of ~380 positive terms in 15-deep per-lane sums and
# a 6-level tree); the bound is below 4x that (6.2e-7) and below 1/4 of the smallest effect of MUTATIONS (drop_bin: 9.0e-4).
LNL_FWD_TOL = 6e-7

ROWS = (1, 3, 31, 32, 33, 127, 128, 129, 4099)  # lane-half, wave and workgroup edges
NOISE = 0.05

_stacks = {}


def stack_of(ctx, name):
    """the device handle of a named stack (helpers.STACKS, infer_cases.ARCHS / VG) with seeded weights and both
    transforms of infer_cases.transforms(5) (the input transform on 7-input stacks) -> (st, dims, act, Ws, bs, tin, tout)"""
    if name not in _stacks:
        nat = pkg("_native")
        if name == "VG":
            dims, act = VG
            Ws, bs = vg_weights(3)
        else:
            dims, act = ARCHS[name] if name in ARCHS else STACKS[name]
            Ws, bs, _ = init_weights(dims, 3)
        st = nat.Stack(ctx, dims, act)
        st.set_weights(jr.ora.flatten_params(Ws, bs))
        tin, tout, _ = transforms(5)
        if dims[0] == 7:
            st.set_input_transform(*tin)
        st.set_output_transform(tout[0], tout[1].astype(np.float32))
        _stacks[name] = (st, dims, act, Ws, bs, tin, tout)
    return _stacks[name]


def rows_for(dims, n, seed, dtype, tin, tin_on):
    """n rows: raw parameters (7-input stacks with the input transform), else rows of the network's own domain"""
    if dims[0] == 7:
        x = pkg("synth").make_params(max(n, 8), seed=seed)[:n].astype(dtype)
        return x if tin_on else jr.transform(x, *tin)[0].astype(dtype)
    return np.random.default_rng(seed).uniform(-1, 1, size=(n, dims[0])).astype(dtype)


def record(y_truth, std, seed, zero_tail=False):
    """(d float32, w float32) of a 451-bin stack: d = y(truth) + NOISE std noise -- every live bin carries a term of
    comparable size, so a dropped bin cannot hide -- and shape_cases.weights (scattered zeros and the run 32 .. 95);
    zero_tail: bins 448 .. 450, the three live lanes of the last tile, weigh nothing either"""
    nb = np.shape(y_truth)[-1]
    d = (np.asarray(y_truth, np.float64) + NOISE * std * np.random.default_rng(7000 + seed).normal(size=nb)).astype(np.float32)
    w = sc.weights(nb, seed) / np.float32((std / sc.OUT_STD) ** 2)
    if zero_tail:
        w[448:] = 0.0
    return d, w.astype(np.float32)


def lnl64(y, d, w):
    """float64 -1/2 sum_k w_k (d_k - y_k)^2 over the bins with w != 0 (whatever d holds in the others); d (nb,) or (n, nb)"""
    w = np.asarray(w, np.float64)
    live = w != 0
    r = np.asarray(d, np.float64)[..., live] - np.asarray(y, np.float64)[..., live]
    return -0.5 * np.sum(w[live] * r * r, axis=-1)


# ---- the mutation catalogue: name -> f(y (n, nb) float64, d, w, mean) -> the mutated float64 ln L (n,)
def _terms(y, d, w):
    w = np.asarray(w, np.float64)
    r = np.where(w != 0, np.asarray(d, np.float64) - np.asarray(y, np.float64), 0.0)
    return w * r * r  # (n, nb)


def mut_drop_bin(y, d, w, mean):
    """one live bin's term dropped: the first live bin of output tile 7"""
    t = _terms(y, d, w)
    k = 224 + int(np.flatnonzero(np.asarray(w)[224:256] != 0)[0])
    t[:, k] = 0.0
    return -0.5 * t.sum(axis=-1)


def mut_pad_bins(y, d, w, mean):
    """bins 451 .. 479 of tile 14 included, with y = the mean of the output transform's mean, d = 0 and the mean live weight"""
    w = np.asarray(w, np.float64)
    pad = 29 * w[w != 0].mean() * float(np.mean(mean)) ** 2
    return -0.5 * (_terms(y, d, w).sum(axis=-1) + pad)


def mut_half_swap(y, d, w, mean):
    """rows permuted within a wave by swapping the 4 h halves: row j <-> j ^ 4 (where both exist)"""
    l = -0.5 * _terms(y, d, w).sum(axis=-1)
    j = np.arange(l.size) ^ 4
    j = np.where(j < l.size, j, np.arange(l.size))
    return l[j]


def mut_tile_twice(y, d, w, mean):
    """one tile's terms counted twice: tile 5, bins 160 .. 191"""
    t = _terms(y, d, w)
    return -0.5 * (t.sum(axis=-1) + t[:, 160:192].sum(axis=-1))


def mut_neighbour_w(y, d, w, mean):
    """w of the neighbouring bin used: bin k weighed with w[k + 1] (the last with its own); a bin without data keeps 0"""
    w = np.asarray(w, np.float64)
    w2 = np.r_[w[1:], w[-1]]
    r = np.where(w != 0, np.asarray(d, np.float64) - np.asarray(y, np.float64), 0.0)
    return -0.5 * np.sum(w2 * r * r, axis=-1)


MUTATIONS = {"drop_bin": mut_drop_bin, "pad_bins": mut_pad_bins, "half_swap": mut_half_swap, "tile_twice": mut_tile_twice,
             "neighbour_w": mut_neighbour_w}


def mutation_effects(y, d, w, mean):
    """name -> the largest relative change of ln L over the rows (what a comparison of every row against the bound sees)"""
    ref = lnl64(y, d, w)
    return {k: float(np.max(np.abs(f(np.asarray(y, np.float64), d, w, mean) - ref) / np.abs(ref))) for k, f in MUTATIONS.items()}


def marg_scale(y, d, w, A):
    """the sum of the magnitudes of the terms of the marginalised ln L as the device forms it, r^T W r + |b|^2 with r the
    residual of the PROJECTED data (marg_ref.marg's lnl_scale fed marg_ref.project, as test_marg_gpu.reference does)"""
    import marg_ref as mr
    w = np.asarray(w, np.float64)
    Q, _ = mr.whiten(A, w)
    r = mr.project(d, Q, w) - np.asarray(y, np.float64)
    b = (w * r) @ Q.T
    return np.sum(w * r * r, axis=-1) + np.sum(b * b, axis=-1)


def rel_err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref) / np.abs(ref)
