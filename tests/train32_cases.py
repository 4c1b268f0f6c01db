"""The table of stack shapes of tests/test_train32_cpu.py and tests/test_train32_gpu.py, its builders and its checks.

Every other f32 training test runs the reference widths (7, 9, 32, 224, 288, 352, 451) or three stacks whose hidden widths
are all below 64.  One f32 optimizer step's branches are decided by the widths and the row count: 32-feature tiles
(train_chain32.h) against 64-feature tiles (train_chain32s.h), their k-steps in chunks (chain32_frags, chain32s_frags), the
host's c32s_split per layer, the contraction split of single-tile layers, the 32 x 32 (or 64 x 64) tiles of [dW; db] with
M = K + 1, the 256-row slabs of dw_adam32.h and the 16-byte quad-transpose store of stream format 4 against its scalar
tail.  The stacks here are tiny and chosen for those branches; the arms force every forward route and every update route
onto each of them.

The gradient check is STRICT: every layer's block by relative L2, the whole arena by cosine and norm ratio, nothing else.
It can be, because the data of every (case, rows) entry is drawn from a seed (DATA_SEED) at which no float64
pre-activation of a ReLU layer lies within 1e-5 of its kink (test_train32_cpu holds that count at zero), so the device
cannot legitimately take a ReLU the other way."""
from collections import namedtuple

import numpy as np

import train_support as ts
from helpers import TOL, init_weights, layer_errors, oracle_step
from oracle import ref_numpy as ora

LINEAR, RELU = 0, 1
Case = namedtuple("Case", "name dims act rows y_is_x")

CASES = [
    # one layer: 2 L - 1 = 1 chain step and no backward rows in the job table; K = 1 has only the scalar stream path; M = 2
    Case("o1", [1, 1], [0], (1, 9), False),
    # one input, a 3-wide ReLU, one output: every tile of every layer is mostly padding
    Case("i1h3", [1, 3, 1], [1, 0], (5, 17), False),
    # K = 5: one vector quad, a scalar tail row and the bias row in one 32-tile; N = 33 = 32 + 1 and 65 = 64 + 1: a
    # one-feature last tile in both tilings, chain32_frags(33) is the first width with a second chunk; rows below, at and above
    # the 4-, 8- and 16-row blocks and one 256-row slab
    Case("tails", [5, 33, 65, 3], [1, 1, 0], (1, 3, 4, 5, 8, 9, 16, 17, 257), False),
    # no tail anywhere; the bias row opens a tile row of its own (M = 65); exactly one slab
    Case("full64", [64, 64, 64], [1, 0], (8, 16, 256), True),
    # 512 -> 9: NT == 1, the contraction split into 16 chunks (the maximum, every wave), c32s_split(1, 32); 9 -> 512: 16
    # tiles of 32 and 8 of 64; backward KT == 1
    Case("latent", [512, 9, 512], [1, 0], (1, 9, 17, 257), True),
    # chain32s_frags 16 against 17 (4 -> 8 fragments); 129 = 2 x 64 + 1 = 4 x 32 + 1; a linear layer inside; 300 rows: a
    # second, short slab
    Case("k16", [16, 128, 17, 129, 16], [1, 0, 1, 0], (7, 33, 300), False),
    # 3 x 9 x 8 = 216 gradient tiles >= 192: dw32_tile = 64, gemm_nt_dwadam_kernel<2> and the 64-tile sliced launch; K = 37
    # is no multiple of 8
    Case("big64", [512, 512, 512, 512], [1, 1, 0], (37,), False),
    # every layer linear: no ReLU kink at any row count; slab boundaries; kDw32MaxRows; 513 rows with V21_DW32_LDS=0: two
    # slices, Adam folds the slabs itself (nslab > 1)
    Case("slabs", [7, 40, 31, 9], [0, 0, 0], (255, 256, 257, 513, 2048), False),
]
BY_NAME = {c.name: c for c in CASES}

# ---- arms: the environment a Trainer is created and stepped under (a trainer commits to its kind and stream format at
# creation; the update switches are read per step)
SWITCHES = ("V21_TRAIN_CHAIN", "V21_CHAIN32S", "V21_C32S_ROWS", "V21_DW32_LDS", "V21_DW32_ADAM")
FWD_ARMS = {
    "chain32": {"V21_CHAIN32S": "0"},
    "chain32s_8": {"V21_CHAIN32S": "1", "V21_C32S_ROWS": "8"},
    "chain32s_4": {"V21_CHAIN32S": "1", "V21_C32S_ROWS": "4"},
    "per_layer": {"V21_TRAIN_CHAIN": "0"},
}
UPD_ARMS = {"default": {}, "lds0": {"V21_DW32_LDS": "0"}, "adam0": {"V21_DW32_ADAM": "0"}}
# the ten arms: three forward routes x three update arms, and the per-layer path
ARMS = [(f, u) for f in ("chain32", "chain32s_8", "chain32s_4") for u in UPD_ARMS] + [("per_layer", "default")]


def upd_arms_of(fwd):
    return [u for f, u in ARMS if f == fwd]


def arm_env(fwd, upd):
    e = dict(FWD_ARMS[fwd])
    e.update(UPD_ARMS[upd])
    return e


def set_arm(monkeypatch, fwd, upd):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in arm_env(fwd, upd).items():
        monkeypatch.setenv(k, v)


# ---- the route table: the update route's name per (case, update arm), one entry per rows entry of the case (a single name:
# every rows entry).  The forward route's name is the forward arm's; the per-layer arm is ("per_layer", "per_layer").
# default: 32 x 32 tiles and <= 2,048 rows: dwadam32; big64 has 216 tiles: 64 x 64, one contraction slice: nt_dwadam.
# lds0: register operands, one contraction slice up to 512 rows (nt_dwadam), slices of <= 512 rows above (nt_sliced).
# adam0: no Adam in a gradient launch's epilogue: nt_sliced.  No arm refuses a rows entry.
UPD_ROUTES = {
    "o1": {"default": "dwadam32", "lds0": "nt_dwadam", "adam0": "nt_sliced"},
    "i1h3": {"default": "dwadam32", "lds0": "nt_dwadam", "adam0": "nt_sliced"},
    "tails": {"default": "dwadam32", "lds0": "nt_dwadam", "adam0": "nt_sliced"},
    "full64": {"default": "dwadam32", "lds0": "nt_dwadam", "adam0": "nt_sliced"},
    "latent": {"default": "dwadam32", "lds0": "nt_dwadam", "adam0": "nt_sliced"},
    "k16": {"default": "dwadam32", "lds0": "nt_dwadam", "adam0": "nt_sliced"},
    "big64": {"default": "nt_dwadam", "lds0": "nt_dwadam", "adam0": "nt_sliced"},
    "slabs": {"default": "dwadam32", "lds0": ("nt_dwadam", "nt_dwadam", "nt_dwadam", "nt_sliced", "nt_sliced"), "adam0": "nt_sliced"},
}


def expected_route(case, k, fwd, upd):
    """(forward route, update route) of rows entry k of `case` under arm (fwd, upd)"""
    if fwd == "per_layer":
        return ("per_layer", "per_layer")
    u = UPD_ROUTES[case.name][upd]
    return (fwd, u if isinstance(u, str) else u[k])


# ---- data.  The recipe of scripts/diag/train_fuzz.py: x uniform in [-1, 1], y normal, row weights uniform(0.5, 1.5) /
# out_dim, weights from helpers.init_weights; a permutation on every second rows entry; max_batch = rows + 5 on every
# other one (the operand pitch then differs from the row count: the `koff + 4 c + 4 > lda` guard of dwadam32_body).
# DATA_SEED: the seed of (case, rows) -- the first of 100, 101, ... at which no ReLU pre-activation is a kink candidate at
# the weights of any of the three steps (test_train32_cpu follows them on the host); entries not listed take 100.  One
# step of k16 at 300 rows has 77,100 ReLU pre-activations and 6 % of the seeds leave it without a candidate, 0.03 % all
# three steps: hence 6585.  (o1, 1) is off seed 100 for another reason: there the one row's residual p - y falls to 4e-3 of
# |y| by the third step (loss 1.2e-3 -> 1.3e-5), and a float32 subtraction then carries 1.4e-5 of it -- numpy float32 itself
# misses the loss and layer bounds there (test_train32_cpu holds the float32 reference inside them on every entry).
WEIGHT_SEED = 100
LR = 1e-2
STEPS = 3
DATA_SEED = {("o1", 1): 101, ("tails", 257): 159, ("full64", 256): 103, ("latent", 257): 101, ("k16", 33): 102, ("k16", 300): 6585, ("big64", 37): 155}


def make_data(case, k, seed=None):
    """-> dict of rows entry k: x, y (None: y = x), w, perm (None or int32), max_batch, xv / yv / wv (the validation split:
    rows // 2 + 1 other rows)"""
    rows = case.rows[k]
    rng = np.random.default_rng(DATA_SEED.get((case.name, rows), 100) if seed is None else seed)
    din, dout = case.dims[0], case.dims[-1]
    nv = rows // 2 + 1
    x = rng.uniform(-1, 1, size=(rows + nv, din)).astype(np.float32)
    y = None if case.y_is_x else rng.normal(size=(rows + nv, dout)).astype(np.float32)
    w = (rng.uniform(0.5, 1.5, size=rows + nv) / dout).astype(np.float32)
    perm = rng.permutation(rows).astype(np.int32) if k % 2 == 1 else None
    return {"rows": rows, "x": x[:rows], "y": None if y is None else y[:rows], "w": w[:rows], "perm": perm,
            "max_batch": rows + (5 if k % 2 == 0 else 0),
            "xv": x[rows:], "yv": None if y is None else y[rows:], "wv": w[rows:]}


_data = {}


def data(case, k):
    """make_data, cached and never modified"""
    if (case.name, k) not in _data:
        _data[(case.name, k)] = make_data(case, k)
    return _data[(case.name, k)]


def step_rows(d):
    """(x, target, w) of the one step of an epoch over the whole split, in the order the step takes them"""
    idx = d["perm"] if d["perm"] is not None else np.arange(d["rows"])
    tgt = d["x"] if d["y"] is None else d["y"]
    return d["x"][idx], tgt[idx], d["w"][idx]


def short_rows(rows):
    """The rows of the shorter step taken after a step of `rows` rows at the same weights: the largest count below `rows` that
    is 1 .. 4 past a multiple of 8 (0: none, rows = 1).  The 4-row blocks of train_chain32s.h then rewrite the gradient
    operands only up to the next multiple of 4, and the last k-step of 8 of the weight-gradient kernels runs over what the
    longer step left there: their `kk + e >= K` selects are all that keeps it out."""
    return max([n for n in range(1, rows) if 1 <= n % 8 <= 4], default=0)


def start_weights(case):
    """(Ws, bs, flat) every trainer of `case` starts from"""
    return init_weights(case.dims, WEIGHT_SEED)


def oracle(case, flat, x, tgt, w):
    """float64 (loss, flat gradient) of one step at the float32 arena `flat`"""
    Ws, bs = ora.unflatten_params(np.asarray(flat), case.dims)
    return oracle_step(Ws, bs, case.act, x, tgt, w)


def forward64(case, flat, x):
    Ws, bs = ora.unflatten_params(np.asarray(flat, np.float64), case.dims)
    return ts.forward64(Ws, bs, case.act, x)


def val_loss64(case, flat, d):
    p = forward64(case, flat, d["xv"])
    t = d["xv"] if d["yv"] is None else d["yv"]
    return float(np.sum(ora.per_sample_loss(p, t, d["wv"].astype(np.float64))) / len(p))


def step32(case, flat, x, tgt, w):
    """the same step in numpy float32: (loss, flat gradient) -- the reference alone must stay inside the bounds"""
    f = np.float32
    Ws, bs = ora.unflatten_params(np.asarray(flat, f), case.dims)
    acts = [x.astype(f)]
    for W_, b_, a_ in zip(Ws, bs, case.act):
        z = acts[-1] @ W_ + b_
        acts.append(np.maximum(z, f(0)) if a_ else z)
    B = f(len(x))
    d = acts[-1] - tgt.astype(f)
    loss = float(np.sum(w.astype(f) * np.sum(d * d, axis=1, dtype=f), dtype=f) / B)
    dz = (f(2) / B) * w.astype(f)[:, None] * d
    L = len(case.act)
    dWs, dbs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        dWs[l] = acts[l].T @ dz
        dbs[l] = dz.sum(0, dtype=f)
        dh = dz @ Ws[l].T
        dz = dh * (acts[l] > 0) if l > 0 and case.act[l - 1] else dh
    return loss, ora.flatten_params(dWs, dbs)


def kink_candidates(case, flat, x, rel_thr=1e-5):
    """float64 pre-activations of ReLU layers with |z| < rel_thr x the layer's largest |z| (the candidates of
    helpers.kink_adjusted_oracle)"""
    Ws, bs = ora.unflatten_params(np.asarray(flat, np.float64), case.dims)
    return sum(int((np.abs(z) < rel_thr * np.abs(z).max()).sum())
               for a_, (z, _) in zip(case.act, ts.layers64(Ws, bs, case.act, x)) if a_)


# ---- the strict check.  Loss 2e-5 and cosine 0.999999: helpers.TOL["f32"]; every layer's block 2e-6: the f32 bound of
# helpers.per_layer_gradient_check (summation noise 1.2e-7 .. 4e-7 from 1 to 40,001 rows); norm ratio 2e-4: 10 x the loss
# tolerance, as helpers.assert_step_matches_oracle has it for the other precisions.  No kink excuse, no column fallback.
TOL_LOSS, TOL_COS = TOL["f32"]
TOL_LAYER = 2e-6
TOL_RATIO = 10 * TOL_LOSS


def strict_errors(dims, loss, g, lo, go):
    """-> dict loss (relative), layer (worst block's relative L2), cos1 (1 - cosine over the arena), ratio (|norm ratio - 1|)"""
    g, go = np.asarray(g, np.float64), np.asarray(go, np.float64)
    ng, no = np.linalg.norm(g), np.linalg.norm(go)
    # 1 - cos from the difference of the unit vectors: the dot product itself cannot resolve 1e-12
    cos1 = 0.5 * float(np.linalg.norm(g / max(ng, 1e-300) - go / max(no, 1e-300)) ** 2)
    return {"loss": abs(loss - lo) / max(1e-300, abs(lo)), "layer": max(e[0] for e in layer_errors(dims, g, go)),
            "cos1": cos1, "ratio": abs(float(ng / max(1e-300, no)) - 1.0)}


def strict_excess(e):
    """the errors over their bounds: the step passes when every one is <= 1"""
    return {"loss": e["loss"] / TOL_LOSS, "layer": e["layer"] / TOL_LAYER, "cos1": e["cos1"] / (1.0 - TOL_COS), "ratio": e["ratio"] / TOL_RATIO}


def strict_ok(e):
    return np.isfinite(list(e.values())).all() and e["loss"] <= TOL_LOSS and e["layer"] <= TOL_LAYER and e["cos1"] < 1.0 - TOL_COS and e["ratio"] < TOL_RATIO


# ---- mutations of the float64 (loss, gradient): what a kernel that is subtly wrong would give.  Each returns None where it
# does not apply, else (loss, gradient).
def _offs(dims):
    return np.cumsum([0] + [a * b + b for a, b in zip(dims[:-1], dims[1:])])


def _block(dims, g, l):
    o = _offs(dims)
    return g[o[l]:o[l + 1]].reshape(dims[l] + 1, dims[l + 1])   # (a view: writing it writes g)


def _rows_dropped(case, flat, x, tgt, w, keep):
    """loss and gradient with only the rows `keep` summed, the step's denominator unchanged"""
    B = len(x)
    lo, go = oracle(case, flat, x[keep], tgt[keep], w[keep])
    s = len(x[keep]) / B
    return lo * s, go * s


def mut_last_row(case, flat, x, tgt, w, lo, go):
    return _rows_dropped(case, flat, x, tgt, w, slice(0, len(x) - 1)) if len(x) > 1 else (0.0, np.zeros_like(go))


def mut_rows_from_256(case, flat, x, tgt, w, lo, go):
    return _rows_dropped(case, flat, x, tgt, w, slice(0, 256)) if len(x) > 256 else None


def mut_bias_row(case, flat, x, tgt, w, lo, go, l):
    g = go.copy()
    _block(case.dims, g, l)[-1, :] = 0.0
    return lo, g


def mut_last_element(case, flat, x, tgt, w, lo, go, l):
    g = go.copy()
    b = _block(case.dims, g, l)
    if b[-1, -1] == 0.0:   # (a ReLU unit no row of the step switches on: nothing to zero)
        return None
    b[-1, -1] = 0.0
    return lo, g


def mut_relu_mask(case, flat, x, tgt, w, lo, go, l):
    """the derivative of ONE unit of ReLU layer l taken as 1 on every row: the first unit some row of the step switches off"""
    if not case.act[l]:
        return None
    Ws, bs = ora.unflatten_params(np.asarray(flat, np.float64), case.dims)
    L = len(case.act)
    acts = [np.asarray(x, np.float64)]
    for W_, b_, a_ in zip(Ws, bs, case.act):
        z = acts[-1] @ W_ + b_
        acts.append(np.maximum(z, 0) if a_ else z)
    off = np.where((acts[l + 1] <= 0).any(0))[0]
    if not len(off):
        return None
    _, dz = ora.batch_loss_and_grad(acts[-1], np.asarray(tgt, np.float64), np.asarray(w, np.float64))
    dWs, dbs = [None] * L, [None] * L
    for li in range(L - 1, -1, -1):
        dWs[li] = acts[li].T @ dz
        dbs[li] = dz.sum(0)
        dh = dz @ Ws[li].T
        if li > 0 and case.act[li - 1]:
            m = acts[li] > 0
            if li - 1 == l:
                m = m.copy()
                m[:, off[0]] = True
            dz = dh * m
        else:
            dz = dh
    g = ora.flatten_params(dWs, dbs)
    return (lo, g) if not np.array_equal(g, go) else None


def mut_tile(case, flat, x, tgt, w, lo, go, l):
    """the first 32 x 32 tile of layer l's [dW; db] taken from its neighbour: the next tile of columns, or of rows"""
    g = go.copy()
    b = _block(case.dims, g, l)
    M, N = b.shape
    if N >= 64:
        b[:min(M, 32), 0:32] = b[:min(M, 32), 32:64]
    elif M >= 64:
        b[0:32, :min(N, 32)] = b[32:64, :min(N, 32)]
    else:
        return None
    return lo, g


def mutations(case):
    """[(name, function of (case, flat, x, tgt, w, lo, go))]: the catalogue, per layer where a mutation names one"""
    L = len(case.act)
    out = [("last_row", mut_last_row), ("rows_from_256", mut_rows_from_256)]
    for name, fn in (("bias_row", mut_bias_row), ("last_element", mut_last_element), ("relu_mask", mut_relu_mask), ("tile", mut_tile)):
        for l in range(L):
            out.append(("%s_l%d" % (name, l), lambda *a, fn=fn, l=l: fn(*a, l)))
    return out


# ---- Adam.  csrc/train_kernels.h: adam_update_element, its exact expressions:
#   m = pm + (g - pm) omb1;  v = pv + (g g - pv) omb2;  w = pw - (m alpha) / (sqrt(v) + eps)
# with omb1 = 1 - beta1, omb2 = 1 - beta2 and alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) all evaluated in float32
# (csrc/api_trainer.hip: adam_alpha, adam_args).  Errors are relative to the sum of the magnitudes of each formula's terms
# (plus the smallest normal float32: below it a float32 has no relative precision).
BETA1, BETA2, EPS = 0.9, 0.999, 1e-7
FLT_MIN = float(np.finfo(np.float32).tiny)


def adam_consts(t, lr=LR, beta1=BETA1, beta2=BETA2):
    """(alpha of step t, 1 - beta1, 1 - beta2, eps) as the float32 values the device holds"""
    f = np.float32
    return ora.adam_alpha(lr, beta1, beta2, t, f), f(1) - f(beta1), f(1) - f(beta2), f(EPS)


def adam_eval(pw, pm, pv, g, t, dtype, variant=None):
    """(m, v, w) after step t from float32 (pw, pm, pv, g), evaluated in `dtype`.  variant: one of ADAM_CONTROLS"""
    alpha, omb1, omb2, eps = adam_consts(t + 1 if variant == "alpha_next" else t)
    if variant == "betas_swapped":
        omb1, omb2 = omb2, omb1
    c = lambda a: np.asarray(a, np.float32).astype(dtype)
    pw, pm, pv, g = c(pw), c(pm), c(pv), c(g)
    alpha, omb1, omb2, eps = dtype(alpha), dtype(omb1), dtype(omb2), dtype(eps)
    m = pm + (g - pm) * omb1
    v = pv + (g * g - pv) * omb2
    mu = pm if variant == "m_stale" else m
    den = np.sqrt(v + eps) if variant == "eps_in_sqrt" else np.sqrt(v) + eps
    return m, v, pw - (mu * alpha) / den


ADAM_CONTROLS = ("alpha_next", "eps_in_sqrt", "betas_swapped", "m_stale")


def adam_errors(pw, pm, pv, g, t, m, v, w):
    """worst element's error of (m, v, w) against the float64 evaluation, each relative to its formula's terms -> (em, ev, ew)"""
    alpha, omb1, omb2, eps = (float(c) for c in adam_consts(t))
    d = lambda a: np.asarray(a, np.float32).astype(np.float64)
    pw, pm, pv, g = d(pw), d(pm), d(pv), d(g)
    m64, v64, w64 = adam_eval(pw, pm, pv, g, t, np.float64)
    dm = np.abs(pm) + omb1 * (np.abs(g) + np.abs(pm)) + FLT_MIN
    dv = pv + omb2 * (g * g + pv) + FLT_MIN
    dw = np.abs(pw) + np.abs(alpha * m64 / (np.sqrt(v64) + eps)) + FLT_MIN
    worst = lambda a, ref, den: float((np.abs(np.asarray(a, np.float64) - ref) / den).max())
    return worst(m, m64, dm), worst(v, v64, dv), worst(w, w64, dw)


def model_steps(case, k, d=None):
    """The STEPS steps of rows entry k on the host: the float64 gradient at the float32 arena, rounded to float32, drives the
    numpy float32 evaluation of Adam.  Yields (t, arena before, pm, pv, x, tgt, w, float64 loss, float64 gradient, (m, v, w) after)."""
    d = data(case, k) if d is None else d
    x, tgt, w = step_rows(d)
    flat = start_weights(case)[2].astype(np.float32)
    pm, pv = np.zeros_like(flat), np.zeros_like(flat)
    for t in range(1, STEPS + 1):
        lo, go = oracle(case, flat, x, tgt, w)
        m, v, wn = adam_eval(flat, pm, pv, go.astype(np.float32), t, np.float32)
        yield t, flat, pm, pv, x, tgt, w, lo, go, (m, v, wn)
        flat, pm, pv = wn, m, v


# the worst errors of the numpy float32 evaluation of those expressions over the three steps of every (case, rows) entry of
# the table (test_train32_cpu computes and pins them): m 1.491e-7, v 2.081e-7, w 2.674e-6.  The bounds are 4 x those: FMA
# contraction and an ulp of sqrtf and of the division.  (w: an element whose m nearly cancels, 0.9 pm = -0.1 g, on a weight
# near zero: the rounding of m is then all of the update and little stands beside it in the denominator.)
ADAM_MODEL_WORST = {"m": 1.50e-7, "v": 2.09e-7, "w": 2.68e-6}
ADAM_TOL = {k: 4 * e for k, e in ADAM_MODEL_WORST.items()}
