"""The reference of the smooth activations (include/v21.h: V21_ACT_TANH .. V21_ACT_SOFTPLUS; oracle/ref_numpy.py knows ReLU
only): forward, one training step (loss with the MSE / row-weight conventions of helpers.oracle_step, and the FULL
gradient) and the parameter Jacobian of a stack with ANY per-layer code list (0 linear, 1 ReLU, 3 tanh, 4 sigmoid, 5 elu,
6 softplus), in float64.  Each also runs in float32 (`dtype=np.float32`: numpy in float32, numpy's own tanh / exp / log1p /
expm1, the derivative taken from the stored output as the per-layer trainer takes it) -- used ONLY to size bounds: how far
float32 arithmetic alone is from float64 at a test's shapes and seeds.  And the stacks, weights and data of
tests/test_act_gpu.py, so that tests/test_act_cpu.py sizes the bounds at exactly those.  Needs no GPU."""
import numpy as np

from oracle import ref_numpy as ora

LINEAR, RELU, TANH, SIGMOID, ELU, SOFTPLUS = 0, 1, 3, 4, 5, 6
NAMES = {LINEAR: "linear", RELU: "relu", TANH: "tanh", SIGMOID: "sigmoid", ELU: "elu", SOFTPLUS: "softplus"}
SMOOTH = (TANH, SIGMOID, ELU, SOFTPLUS)


# ---- the activations (no overflow for any finite z, in either dtype: every exponential has a non-positive argument)
def act(code, z):
    if code == LINEAR:
        return z
    if code == RELU:
        return np.maximum(z, 0)
    if code == TANH:
        return np.tanh(z)
    if code == SIGMOID:
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(z.dtype)
    if code == ELU:
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0))).astype(z.dtype)
    if code == SOFTPLUS:
        return (np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))).astype(z.dtype)
    raise ValueError("activation code %r" % (code,))


def deriv(code, z):
    """dh/dz from z: the float64 reference's (and the Jacobian kernel's) form"""
    one = np.ones_like(z)
    if code == LINEAR:
        return one
    if code == RELU:
        return (z > 0).astype(z.dtype)
    if code == TANH:
        e = np.exp(-2 * np.abs(z))
        return (4 * e / (1 + e) ** 2).astype(z.dtype)
    if code == SIGMOID:
        e = np.exp(-np.abs(z))
        return (e / (1 + e) ** 2).astype(z.dtype)
    if code == ELU:
        return np.where(z > 0, one, np.exp(np.minimum(z, 0))).astype(z.dtype)
    if code == SOFTPLUS:
        return act(SIGMOID, z)
    raise ValueError("activation code %r" % (code,))


def deriv_out(code, h):
    """dh/dz from the stored output h = act(z): what the per-layer trainer has (the table of include/v21.h)"""
    one = np.ones_like(h)
    if code == LINEAR:
        return one
    if code == RELU:
        return (h > 0).astype(h.dtype)
    if code == TANH:
        return 1 - h * h
    if code == SIGMOID:
        return h * (1 - h)
    if code == ELU:
        return np.where(h > 0, one, h + 1).astype(h.dtype)
    if code == SOFTPLUS:
        return (-np.expm1(-h)).astype(h.dtype)
    raise ValueError("activation code %r" % (code,))


def _cast(Ws, bs, dtype):
    return [np.asarray(W, dtype) for W in Ws], [np.asarray(b, dtype) for b in bs]


# ---- forward
def layers(Ws, bs, codes, x, dtype=np.float64):
    """[(z, h)] of every layer"""
    W, b = _cast(Ws, bs, dtype)
    h = np.asarray(x, dtype)
    out = []
    for W_, b_, c in zip(W, b, codes):
        z = h @ W_ + b_
        h = act(c, z)
        out.append((z, h))
    return out


def forward(Ws, bs, codes, x, dtype=np.float64):
    return layers(Ws, bs, codes, x, dtype)[-1][1]


# ---- one training step: loss = mean over the rows of w_i sum_j (p - y)^2 (helpers.oracle_step's convention), full gradient
def step(Ws, bs, codes, x, tgt, w, dtype=np.float64):
    """-> (loss, flat gradient in Keras' order W0, b0, W1, b1, ...).  float64: the derivative from z; float32: from the
    stored output, as the device's per-layer route forms it."""
    W, _ = _cast(Ws, bs, dtype)
    zh = layers(Ws, bs, codes, x, dtype)
    hs = [np.asarray(x, dtype)] + [h for _, h in zh]
    lo, dz = ora.batch_loss_and_grad(hs[-1], np.asarray(tgt, dtype), np.asarray(w, dtype))
    dz = dz.astype(dtype)
    L = len(codes)
    dWs, dbs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        dWs[l] = hs[l].T @ dz
        dbs[l] = dz.sum(0)
        if l > 0:
            dh = dz @ W[l].T
            d = deriv(codes[l - 1], zh[l - 1][0]) if dtype == np.float64 else deriv_out(codes[l - 1], hs[l])
            dz = (dh * d).astype(dtype)
    return lo, ora.flatten_params(dWs, dbs)


def loss_only(flat, dims, codes, x, tgt, w):
    Ws, bs = ora.unflatten_params(np.asarray(flat, np.float64), dims)
    p = forward(Ws, bs, codes, x)
    return float(np.mean(ora.per_sample_loss(p, np.asarray(tgt, np.float64), np.asarray(w, np.float64))))


# ---- the Jacobian dy_o / dx_j, (n, in, out)
def jacobian(Ws, bs, codes, x, dtype=np.float64):
    W, b = _cast(Ws, bs, dtype)
    h = np.asarray(x, dtype)
    n, din = h.shape
    T = np.broadcast_to(np.eye(din, dtype=dtype), (n, din, din)).copy()   # (n, tangent, feature)
    for W_, b_, c in zip(W, b, codes):
        z = h @ W_ + b_
        T = (T @ W_) * deriv(c, z)[:, None, :]
        h = act(c, z)
    return T.astype(dtype)


def per_layer_rel_l2(dims, g, go):
    """||g - go|| / ||go|| per layer's [W; b] block of the flat arena"""
    offs = np.cumsum([0] + [a * b + b for a, b in zip(dims[:-1], dims[1:])])
    out = []
    for i in range(len(dims) - 1):
        a, b = np.asarray(g[offs[i]:offs[i + 1]], np.float64), np.asarray(go[offs[i]:offs[i + 1]], np.float64)
        out.append(float(np.linalg.norm(a - b) / max(1e-300, np.linalg.norm(b))))
    return out


def jac_row_rel_l2(J, Jo):
    """max over the rows of ||J_row - Jo_row|| / ||Jo_row||"""
    d = (np.asarray(J, np.float64) - np.asarray(Jo, np.float64)).reshape(len(Jo), -1)
    return float(np.max(np.linalg.norm(d, axis=1) / np.linalg.norm(np.asarray(Jo, np.float64).reshape(len(Jo), -1), axis=1)))


# ---- the stacks of tests/test_act_gpu.py.  Hidden widths 40 and 72: no multiple of 16 or 32 (partial tiles, non-zero
# padding: sigmoid(0) = 0.5, softplus(0) = ln 2); output 37: two output tiles of the fused kernel, fed by more than 32
# features; input 5.  T3: the sample notebook's stack with tanh, with the transforms.
T1 = ([5, 40, 72, 37], [TANH, SIGMOID, LINEAR])
T2 = ([5, 40, 72, 37], [ELU, SOFTPLUS, LINEAR])
T3 = ([7, 64, 128, 451], [TANH, TANH, LINEAR])
J1 = ([9, 40, 37], [TANH, LINEAR])   # in_dim 9: two tangent groups of jac_generic_kernel
RELU_CONTROL = ([5, 40, 72, 37], [RELU, RELU, LINEAR])
SEEDS = {"T1": 11, "T2": 12, "T3": 13, "J1": 14, "RELU": 15}
# the float32 restatement's own Jacobian error against float64 at the shapes and seeds of the GPU test (3 rows; max over the
# rows of relative L2), measured on the CPU: 1.335e-7 and 2.103e-7.  tests/test_act_cpu.py holds the restatement to these
# figures; the device's bound in tests/test_act_gpu.py is 8 x them.
JAC_F32_ERR = {"J1": 1.34e-7, "T2": 2.11e-7}
SAT_BIAS = 90.0   # two units of every hidden layer: exp(+-180) in a naive tanh is inf / inf


def stack_weights(dims, seed, saturate=True):
    """-> (Ws, bs, flat): Glorot kernels, N(0, 0.05) biases; saturate: in every hidden layer unit 1 gets bias +90 and unit 2
    bias -90 (their derivative is 0 to rounding, their output the saturated value)"""
    rng = np.random.default_rng(seed)
    Ws = [ora.glorot_uniform(rng, k, n) for k, n in zip(dims[:-1], dims[1:])]
    bs = [rng.normal(scale=0.05, size=n).astype(np.float32) for n in dims[1:]]
    if saturate:
        for b in bs[:-1]:
            b[1], b[2] = SAT_BIAS, -SAT_BIAS
    return Ws, bs, ora.flatten_params(Ws, bs)


def step_data(dims, rows, seed):
    """-> (x in [-1, 1], targets ~ N(0, 1), plain-MSE row weights as float32)"""
    rng = np.random.default_rng(seed + 500)
    x = rng.uniform(-1, 1, size=(rows, dims[0])).astype(np.float32)
    y = rng.normal(size=(rows, dims[-1])).astype(np.float32)
    return x, y, ora.mse_row_weight(y).astype(np.float32)


def adam_reference(flat, g, lr):
    """the weights after ONE Keras Adam update from zero moments, in float32 (oracle/ref_numpy.py: adam_step)"""
    st = ora.AdamState(flat.size, lr=lr)
    return ora.adam_step(np.array(flat, np.float32), np.asarray(g, np.float32), st)
