"""What the training-side GPU tests share (test_train_gpu, test_poison_gpu, train32_cases): the float64 forward pass and
loss of a plain stack (the loss AND gradient of one step is helpers.oracle_step), the two comparisons every file makes, the
environment a trainer is created under, the one place that builds a stack + trainer, and the pre-processed signals with
their relative-MSE row weights.  Importing this needs no GPU; calling what takes a `ctx` does."""
import contextlib
import os

import numpy as np

from conftest import pkg
from oracle import ref_numpy as ora


# ---- float64 forward
def layers64(Ws, bs, act, x, layers=None):
    """(pre-activation, activation) of every layer (of the first `layers`) in float64; act: 1 = ReLU, 0 = linear"""
    h = np.asarray(x, np.float64)
    for W_, b_, a_ in list(zip(Ws, bs, act))[:layers]:
        z = h @ np.asarray(W_, np.float64) + np.asarray(b_, np.float64)
        h = np.maximum(z, 0) if a_ else z
        yield z, h


def forward64(Ws, bs, act, x, layers=None):
    """the last activation of the float64 forward pass (of the first `layers` layers: an encoder alone)"""
    h = np.asarray(x, np.float64)
    for _, h in layers64(Ws, bs, act, x, layers):
        pass
    return h


def loss64(Ws, bs, act, x, tgt, w):
    """float64 forward loss of the rows: the mean of the per-sample losses"""
    return float(np.mean(ora.per_sample_loss(forward64(Ws, bs, act, x), np.asarray(tgt, np.float64), np.asarray(w, np.float64))))


# ---- comparisons
def cos(a, b):
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def close(a, b, rtol, what):
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b).max() / scale
    assert err < rtol, "%s: max err / scale = %.3e (limit %.1e)" % (what, err, rtol)


# ---- trainers
@contextlib.contextmanager
def forced_env(**env):
    """the variables set for the body (a trainer commits to its route when it is created), then exactly what was there
    before: the old value, or absent"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def new_trainer(ctx, dims, act, flat, prec, max_batch, lr=None, env=None):
    """-> (stack holding the arena `flat`, its trainer); created under forced_env(**env); lr: Adam at that learning rate"""
    native = pkg("_native")
    with forced_env(**(env or {})):
        st = native.Stack(ctx, dims, act)
        st.set_weights(flat)
        tr = native.Trainer(st, prec, max_batch)
    if lr is not None:
        tr.set_adam(lr=lr)
    return st, tr


def vae_weights(dims, gl, seed):
    """-> (act, Ws, bs) of a stack whose layer `gl` is the (z_mean | z_log_var) head: dims = widths the NEXT layer sees, so
    that layer's kernel is (dims[gl], 2*dims[gl+1]); Glorot kernels and N(0, 0.05) biases from one generator"""
    rng = np.random.default_rng(seed)
    L = len(dims) - 1
    act = [2 if l == gl else (1 if l < L - 1 else 0) for l in range(L)]
    Ws, bs = [], []
    for l in range(L):
        nout = dims[l + 1] * (2 if l == gl else 1)
        Ws.append(ora.glorot_uniform(rng, dims[l], nout))
        bs.append(rng.normal(scale=0.05, size=nout).astype(np.float32))
    return act, Ws, bs


# ---- data
def signal_rows(n, seed, stats_from=None):
    """-> (n pre-processed signals, their relative-MSE row weights as float32).  stats_from: pre-processed against the
    first `stats_from` >= n signals of the seed (one row alone pre-processes to zeros)"""
    sig_all = pkg("synth").make_signals(stats_from or n, seed=seed)
    y = ora.preproc(sig_all[:n], sig_all)
    return y, ora.relative_mse_row_weight(y, sig_all).astype(np.float32)
