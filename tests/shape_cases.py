"""The table of stack shapes of tests/test_shapes_cpu.py and tests/test_shapes_gpu.py, and its builders.

Every other test of the Jacobian-side kernels (jac_generic.h, reduce_kernels.h, fit_kernels.h, nuisance_kernels.h, sample_kernels.h) runs 7 or
9 inputs against 451 outputs.  The stacks here are tiny and chosen for the branches those shapes never reach: more than
one tangent group on grid.y of jac_generic_kernel and a short last group, its LDS paths (the shrink loop, the 256-float
floor of the likelihood mode's block reduction, a row pitch set by in_dim or out_dim), the lane tails of the reductions
(`for (k = lane; k < dout; k += 64)` at dout below, at and just above 64), their `j < din` padding guards at din = NI, the
identity padding of the fit's and the sampler's Cholesky factor below 8 inputs and the sampler's Philox blocks of four.
None of them is a stack of csrc/archs.h: every one takes the generic route."""
from collections import namedtuple

import numpy as np

import fit_ref as fr
import jacobian_ref as jr
import marg_ref as mr
from helpers import init_weights

LINEAR, RELU, GAUSS = 0, 1, 2
ROWS = (1, 3, 4, 5, 9)  # the reduce kernels run four rows per workgroup: below, at, above one and two workgroups
OUT_STD = 12.5

# modes: the numbers K of nuisance modes the marginalised reductions run with; fit: also fitted and sampled (in_dim <= 8)
Case = namedtuple("Case", "name dims act modes fit")

CASES = [
    # in_dim = 1 with out_dim = 1, every width below 32: grid.y = 1 with one tangent, 2 (tc + 1) maxw = 16 floats -- the
    # 256-float LDS floor of the likelihood mode; 63 lanes of the reductions never enter the bin loop but still shuffle
    Case("i1o1", [1, 4, 1], [1, 0], (), False),
    # in_dim = 1, the minimum of fit_lm_kernel and sample_step_kernel (seven rows of identity padding in the Cholesky
    # factor, one Philox block of which one normal is used); out_dim = 63: lane 63 never enters the bin loop
    Case("i1o63", [1, 16, 63], [1, 0], (1, 4), True),
    # in_dim = 2, out_dim = 1, every width below 32 (the issue's example): the LDS floor again, with two tangents
    Case("i2o1", [2, 3, 1], [1, 0], (), False),
    # a hidden width above 256: the `o += blockDim.x` loop of jac_generic_kernel runs twice for 44 threads; out_dim = 65
    Case("i2w300", [2, 300, 65], [1, 0], (4,), False),
    # a one-layer stack ending in a ReLU: the output layer's mask on primal and tangents, maxw = out_dim = 65
    Case("i3relu1", [3, 65], [1], (5,), False),
    # out_dim = 3: 61 idle lanes; two live bins allow K = 1 and refuse K = 4
    Case("i4o3", [4, 8, 3], [1, 0], (1,), False),
    # in_dim = 4: exactly one Philox block; out_dim = 65 = 64 + 1: one lane runs the bin loop twice; every K instantiation
    Case("i4o65", [4, 32, 65], [1, 0], (1, 4, 5, 8), True),
    # in_dim = 5: two Philox blocks, three of the second's normals unused; out_dim = 130 = 2 * 64 + 2 with a run of 64
    # zero-weight bins (a whole pass of the bin loop skipped by every lane); maxw = out_dim
    Case("i5o130", [5, 64, 130], [1, 0], (5, 8), True),
    # a one-layer linear stack: no hidden layer, out_dim = 63, maxw = out_dim
    Case("i5lin1", [5, 63], [0], (4,), False),
    # one Gauss layer (z = z_mean: the first half of its columns, row pitch nw = 2 n) away from in_dim = 7
    Case("i5gauss", [5, 32, 6, 16, 63], [1, 2, 1, 0], (1,), False),
    # [7, 3000, 5]: 2 (7 + 1) 3000 floats exceed 160 KB, the shrink loop stops at tc = 5: tangent groups 5 + 2
    Case("i7w3000", [7, 3000, 5], [1, 0], (), False),
    # in_dim = 8: tangent groups 7 + 1 (blockIdx.y = 1 with a single tangent), NI = 8 without padding in
    # jac_reduce_kernel<8, ., .>, fit_lm_kernel and the sampler (the fit limit, two full Philox blocks); out_dim = 64: every
    # lane runs the bin loop exactly once
    Case("i8o64", [8, 33, 64], [1, 0], (4, 8), True),
    # the one 451-bin case, at in_dim = 8, two hidden layers
    Case("i8o451", [8, 64, 48, 451], [1, 1, 0], (5,), False),
    # in_dim = 9: the first NI = 15 instantiations on the generic route (groups 7 + 2); served by fisher, refused by fit
    # and sample; no input transform from here on
    Case("i9o65", [9, 24, 65], [1, 0], (1, 8), False),
    # in_dim = 14: two full tangent groups 7 + 7; out_dim = 3
    Case("i14o3", [14, 20, 3], [1, 0], (1,), False),
    # in_dim = 15 with out_dim = 65: groups 7 + 7 + 1, NI = 15 without padding (the Fisher limit), 120 accumulators
    Case("i15o65", [15, 40, 65], [1, 0], (4, 8), False),
    # in_dim = 16, maxw = in_dim: the LDS row pitch is set by the input; groups 7 + 7 + 2; past the Fisher limit --
    # Jacobian and loglike are still served, every reduction of reduce_kernels.h is refused
    Case("i16o3", [16, 8, 3], [1, 0], (), False),
    # in_dim = 17: groups 7 + 7 + 3; out_dim = 64
    Case("i17o64", [17, 31, 64], [1, 0], (), False),
    # a ReLU-ended stack with a hidden layer at in_dim = 8, out_dim = 130 (maxw = out_dim, the mask on groups 7 + 1)
    Case("i8relu", [8, 20, 130], [1, 1], (8,), False),
]
BY_NAME = {c.name: c for c in CASES}

# refused with V21_ERR_UNSUPPORTED, the handle stays usable: 2 (1 + 1) 10241 floats = 163,856 bytes, 16 more than the
# 160 KB of LDS a workgroup can have, with one tangent per workgroup already (10,240 is the widest layer served)
TOO_WIDE = ([2, 10241, 1], [1, 0])
# the 65,535-row launch split of jac_run at 65,537 rows (grid.x of the second launch: 2)
SPLIT = ([2, 4, 3], [1, 0])
SPLIT_ROWS = 65537


def has_tin(dims):
    return dims[0] <= 8


def _weights(dims, act, seed):
    """helpers.init_weights, or the recipe of infer_cases.vg_weights for a stack with a Gauss layer (2 n columns)"""
    if GAUSS not in act:
        Ws, bs, _ = init_weights(dims, seed)
        return Ws, bs
    rng = np.random.default_rng(seed)
    Ws, bs = [], []
    for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
        nw = 2 * n if act[l] == GAUSS else n
        lim = np.sqrt(6.0 / (k + nw))
        Ws.append(rng.uniform(-lim, lim, size=(k, nw)).astype(np.float32))
        bs.append(rng.normal(scale=0.05, size=nw).astype(np.float32))
    return Ws, bs


def input_transform(din):
    """(log_mask, zero_floor, lo, hi) of `din` <= 8 columns: every third column log10, column 0 with a zero floor of 1e-6
    whose log10 is the box's lower bound (as fx in the reference's parameters), lo < hi everywhere"""
    j = np.arange(din)
    log_mask = (j % 3 == 0).astype(np.int32)
    zero_floor = np.where(j == 0, 1e-6, 0.0)
    lo = np.where(log_mask == 1, np.where(j == 0, -6.0, -1.0), -3.0 + j)
    hi = np.where(log_mask == 1, np.where(j == 0, 1.0, 2.0), 5.0 + 2.0 * j)
    return log_mask, zero_floor, lo.astype(np.float64), hi.astype(np.float64)


def output_transform(dout):
    k = np.arange(dout)
    return OUT_STD, (-30.0 + 20.0 * np.sin(0.37 * k) + 0.05 * k).astype(np.float32).astype(np.float64)


_stacks = {}


def make_stack(dims, act, seed=3):
    """-> dict dims, act, Ws, bs, flat, tin (None above 8 inputs), tout; cached, never modified"""
    key = (tuple(dims), tuple(act), seed)
    if key not in _stacks:
        Ws, bs = _weights(dims, act, seed)
        _stacks[key] = {"dims": list(dims), "act": list(act), "Ws": Ws, "bs": bs, "flat": jr.ora.flatten_params(Ws, bs),
                        "tin": input_transform(dims[0]) if has_tin(dims) else None, "tout": output_transform(dims[-1])}
    return _stacks[key]


def rows_u(dims, n, seed):
    """n rows in the network's own domain, float64, inside [-0.9, 0.9]"""
    return np.random.default_rng(1000 + seed).uniform(-0.9, 0.9, size=(n, dims[0]))


def rows(dims, n, seed):
    """n raw float64 rows inside the box of input_transform (rows_u mapped back; every second row from row 1 on has
    exactly 0 in the column with the zero floor); above 8 inputs, where there is no transform, rows_u itself"""
    u = rows_u(dims, n, seed)
    if not has_tin(dims):
        return u
    log_mask, _, lo, hi = input_transform(dims[0])
    x = fr.untransform(u, log_mask, lo, hi)
    x[1::2, 0] = 0.0
    return x


def weights(dout, seed, K=0):
    """1 / sigma^2 per bin (sigma between 0.05 and 0.075 of OUT_STD) with zeros: about one bin in six, scattered, and
    where dout >= 128 also the 64 consecutive bins 32 .. 95; below 8 bins a single zero (none at dout = 1).  At least
    K + 1 bins stay live."""
    rng = np.random.default_rng(2000 + seed)
    k = np.arange(dout)
    w = 1.0 / (0.05 * OUT_STD * (1.0 + 0.5 * k / dout)) ** 2
    if dout >= 8:
        w[rng.uniform(size=dout) < 1.0 / 6.0] = 0.0
    elif dout > 1:
        w[seed % dout] = 0.0
    if dout >= 128:
        w[32:96] = 0.0
    assert np.count_nonzero(w) >= K + 1, (dout, K, np.count_nonzero(w))
    return w.astype(np.float32)


def basis(dout, K):
    """(K, dout) float64: the Chebyshev polynomials T_0 .. T_(K-1) of the bin index mapped to [-1, 1]"""
    t = np.linspace(-1.0, 1.0, dout) if dout > 1 else np.zeros(1)
    return np.polynomial.chebyshev.chebvander(t, K - 1).T.copy()


def basis_condition(dout, K, w):
    """cond(R) of marg_ref.whiten: the condition number of the weighted basis"""
    return np.linalg.cond(mr.whiten(basis(dout, K), np.asarray(w, np.float64))[1])


def data_for(stack, seed, noise=0.05):
    """(data float32 (dout,), its truth row): the float64 outputs of one row of rows() plus noise of `noise` OUT_STD"""
    dims = stack["dims"]
    x1 = rows(dims, 1, 90 + seed)
    y = jr.jacobian(stack["Ws"], stack["bs"], stack["act"], x1, stack["tin"], stack["tout"])[0][0]
    return (y + np.random.default_rng(3000 + seed).normal(size=dims[-1]) * noise * OUT_STD).astype(np.float32), x1[0]


# ---- fits and chains (in_dim <= 8): truths inside the box, a few starts per truth
FIT_TRUTHS, FIT_STARTS, FIT_SIGMA = 2, 3, 0.02


def fit_problem(case, seed=8):
    """-> dict truths_u (m, din), data float32 (m, dout) = y(truth) + noise of FIT_SIGMA OUT_STD, w, x0 raw float64
    (m FIT_STARTS, din) -- the truths moved by 0.1 in u -- and u0, the float32 u of the starts as the device holds them"""
    st = make_stack(case.dims, case.act)
    din, dout = case.dims[0], case.dims[-1]
    rng = np.random.default_rng(4000 + seed)
    tu = rng.uniform(-0.6, 0.6, size=(FIT_TRUTHS, din))
    y = jr.jvp(st["Ws"], st["bs"], st["act"], tu)[0] * st["tout"][0] + st["tout"][1]
    sig = FIT_SIGMA * OUT_STD
    data = (y + rng.normal(size=y.shape) * sig).astype(np.float32)
    w = np.where(weights(dout, seed) > 0, 1.0 / sig ** 2, 0.0).astype(np.float32)
    us = np.clip(np.repeat(tu, FIT_STARTS, axis=0) + 0.1 * rng.normal(size=(FIT_TRUTHS * FIT_STARTS, din)), -0.95, 0.95)
    tin = st["tin"]
    x0 = fr.untransform(us, tin[0], tin[2], tin[3])
    u0 = jr.transform(x0, *tin)[0].astype(np.float32).astype(np.float64)
    return {"truths_u": tu, "data": data, "w": w, "x0": x0, "u0": u0}


CHAINS = 384  # 0.5 % of them is one decision


def chain_starts(case, prob, seed=7, scale=0.03):
    """CHAINS raw float64 starts: the first truth jittered by `scale` in u, inside the box (test_sample_gpu.starts_near)"""
    tin = make_stack(case.dims, case.act)["tin"]
    u = np.clip(prob["truths_u"][:1] + scale * np.random.default_rng(seed).normal(size=(CHAINS, case.dims[0])), -0.999, 0.999)
    return fr.untransform(u, tin[0], tin[2], tin[3])


# rows of the 3000-wide stack from another draw: of 3000 units x 22 rows the default draw leaves two rows with a unit within
# 1e-5 of its kink in float64 (test_shapes_cpu: the share of such rows is held at zero on the reference)
ROW_SEED = {"i7w3000": 400}


def jac_inputs(case):
    """the calls of the Jacobian test: (n, input transform on, output transform on, rows in their dtype) for every n of
    ROWS -- with and without each transform, float64 and float32 rows"""
    for k, n in enumerate(ROWS):
        tin_on = has_tin(case.dims) and k % 2 == 0
        dtype = np.float64 if k % 4 < 2 else np.float32
        seed = 10 + k + ROW_SEED.get(case.name, 0)
        x = rows(case.dims, n, seed) if tin_on else rows_u(case.dims, n, seed)
        yield n, tin_on, k % 3 != 0, x.astype(dtype)


# the one transition the sampler test rebuilds: every counter word non-zero
SEED, CHAIN0, STEP0, EPS0, RIDGE = (5 << 32) + 1234, 7, 40, 0.7, 1.0
