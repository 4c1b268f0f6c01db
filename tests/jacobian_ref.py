"""float64 reference of the parameter Jacobian and the Gaussian log-likelihood (tests/test_jacobian_*.py).

Forward-mode through the stack as the oracle's forward computes it (oracle/ref_numpy.py: act(h W + b), ReLU z > 0, a
V21_ACT_GAUSS layer evaluated as z = z_mean -- the first half of its columns), the chain-rule factor of
preprocess.par_transform (taken at the value after the fx zero floor, floored in the dtype of the rows) and std of the
output transform."""
import numpy as np

import half_ref
from oracle import ref_numpy as ora

RELU, GAUSS = 1, 2


def layer_params(Ws, bs, act):
    """(W, b) float64 as the forward uses them: a V21_ACT_GAUSS layer's z_mean columns only."""
    out = []
    for W, b, a in zip(Ws, bs, act):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        if a == GAUSS:
            k = W.shape[1] // 2
            W, b = W[:, :k], b[:k]
        out.append((W, b))
    return out


def forward(Ws, bs, act, xt):
    h = np.asarray(xt, np.float64)
    for (W, b), a in zip(layer_params(Ws, bs, act), act):
        z = h @ W + b
        h = np.maximum(z, 0) if a == RELU else z
    return h


def round16(a, prec):
    """float64 -> the nearest f16 / bf16 value (round to nearest even), as float64 (half_ref.round16)"""
    return half_ref.round16(a, prec)


def masks16(Ws, bs, act, xt, prec, with_z=False):
    """the ReLU decisions of a 16-bit primal as the fused kernels form it: operands (input, weights, activations) rounded
    to f16 / bf16, products summed wide, the f32 bias added, z > 0 -- per layer a bool (n, units) array or None (and the
    pre-activations with with_z).  One definition: half_ref.masks16."""
    return half_ref.masks16(Ws, bs, act, xt, prec, with_z=with_z)


def jvp(Ws, bs, act, xt, flips=None, masks=None):
    """(y (n, out), J (n, in, out) = d y / d xt, pre-activations per layer).  flips: per layer None or a bool (n, units)
    array of ReLU decisions to invert (kink analysis); masks: per layer the ReLU decisions to use instead of z > 0 (the
    derivative of the function a 16-bit primal computes, masks16)."""
    h = np.asarray(xt, np.float64)
    n, din = h.shape
    T = np.repeat(np.eye(din)[None], n, axis=0)
    zs = []
    for l, ((W, b), a) in enumerate(zip(layer_params(Ws, bs, act), act)):
        z = h @ W + b
        Tz = T @ W
        zs.append(z)
        if a == RELU:
            m = z > 0 if masks is None else masks[l]
            if flips is not None and flips[l] is not None:
                m = m ^ flips[l]
            h = np.where(m, z, 0.0)
            T = Tz * m[:, None, :]
        else:
            h, T = z, Tz
    return h, T, zs


def transform(x, log_mask, zero_floor, lo, hi):
    """(xt, fac) float64: preprocess.par_transform of raw rows and its derivative d xt / d x at the floored value.  The
    floor is rounded to the dtype of the rows (float32 rows: (float)1e-6), as the reference floors in that dtype."""
    x = np.asarray(x)
    t = x.astype(np.float64)
    for j, zf in enumerate(zero_floor):
        if zf > 0:
            fl = float(np.float32(zf)) if x.dtype == np.float32 else float(zf)
            t[x[:, j] == 0, j] = fl
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    span = hi - lo
    lm = np.asarray(log_mask, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(lm, np.log10(np.where(lm, t, 1.0)), t)
        fac = np.where(lm, 2.0 / (span * t * np.log(10.0)), 2.0 / span)
    return (q - lo) / span * 2 - 1, fac


def jacobian(Ws, bs, act, x, tin=None, tout=None, flips=None, mask_prec=None):
    """(y, jac (n, in, out)) of raw rows x.  tin: (log_mask, zero_floor, lo, hi) or None; tout: (std, mean) or None;
    mask_prec "f16" / "bf16": with the ReLU decisions of that precision's primal (masks16)."""
    if tin is not None:
        xt, fac = transform(x, *tin)
    else:
        xt, fac = np.asarray(x, np.float64), np.ones(np.shape(x))
    masks = masks16(Ws, bs, act, xt.astype(np.float32), mask_prec) if mask_prec else None
    if masks is not None and flips is not None:
        masks = [m if f is None or m is None else m ^ f for m, f in zip(masks, flips)]
        flips = None
    y, J, _ = jvp(Ws, bs, act, xt, flips, masks)
    std, mean = (1.0, 0.0) if tout is None else (float(tout[0]), np.asarray(tout[1], np.float64))
    return y * std + mean, J * fac[:, :, None] * std


def jvp16(Ws, bs, act, xt, prec, **kw):
    """half_ref.jvp: the forward-mode pass that rounds where fused_jac rounds (prec None: jvp above, bit for bit)"""
    return half_ref.jvp(Ws, bs, act, xt, prec, **kw)


def operands16(x, tin=None, tout=None):
    """what fused_jac is handed for raw rows x: (xt float32 -- the float64 transform rounded once, csrc/par_transform.h --,
    fac as the float32 jac_prep_kernel stores, the float32 std of the output transform or None)"""
    if tin is not None:
        xt, fac = transform(x, *tin)
        if np.asarray(x).dtype == np.float32:  # par_transform_f32: the log10 of a float32 row is a float32
            lm, lo, span = np.asarray(tin[0], bool), np.asarray(tin[2], np.float64), np.asarray(tin[3], np.float64) - np.asarray(tin[2], np.float64)
            t = np.asarray(x, np.float64).copy()
            for j, zf in enumerate(tin[1]):
                if zf > 0:
                    t[np.asarray(x)[:, j] == 0, j] = float(np.float32(zf))
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(lm, np.log10(np.where(lm, t, 1.0)).astype(np.float32).astype(np.float64), t)
            xt = (q - lo) / span * 2 - 1
    else:
        xt, fac = np.asarray(x, np.float64), np.ones(np.shape(x))
    std = None if tout is None else float(np.float32(tout[0]))
    return xt.astype(np.float32), fac.astype(np.float32).astype(np.float64), std


def jacobian16(Ws, bs, act, x, prec, tin=None, tout=None, acc="f64", mut=None):
    """(y, J (n, in, out)) of raw rows x as fused_jac<., prec> forms them (half_ref.jvp), float64: tin / tout as in
    jacobian; y as half_ref.forward forms it.  acc "f32": the CPU device model; mut: an entry of half_ref.JAC_MUTATIONS."""
    xt, fac, std = operands16(x, tin, tout)
    y, J, _ = half_ref.jvp(Ws, bs, act, xt, prec, acc=acc, fac=fac if tin is not None else None, std=std, mut=mut)
    if tout is not None:
        y = y * float(tout[0]) + np.asarray(tout[1], np.float64)
    return y, J


def loglike(y, jac, data, inv_var):
    """lnl (n,), grad (n, in) of ln L = -1/2 sum w (d - y)^2 from outputs and their Jacobian."""
    r = np.asarray(data, np.float64) - np.asarray(y, np.float64)
    w = np.asarray(inv_var, np.float64)
    return -0.5 * np.sum(w * r * r, axis=-1), np.einsum("nk,njk->nj", w * r, np.asarray(jac, np.float64))


def oracle_outputs(Ws, bs, act, x, tin=None, tout=None):
    """the float64 forward of raw rows through ora.par_transform-equivalent and unpreproc-equivalent transforms"""
    xt = transform(x, *tin)[0] if tin is not None else np.asarray(x, np.float64)
    y = forward(Ws, bs, act, xt)
    return y if tout is None else y * float(tout[0]) + np.asarray(tout[1], np.float64)


def min_relative_preactivation(Ws, bs, act, xt):
    """per row: min over hidden ReLU units of |z| / max|z| of that layer"""
    _, _, zs = jvp(Ws, bs, act, xt)
    out = np.full(np.shape(xt)[0], np.inf)
    for z, a in zip(zs[:-1], act[:-1]):
        if a == RELU:
            out = np.minimum(out, np.min(np.abs(z), axis=1) / np.max(np.abs(z), axis=1))
    return out


def near_kinks(Ws, bs, act, xt, rel=1e-5):
    """per layer: bool (n, units) of ReLU units whose float64 pre-activation is zero to rel x max|z| of that layer"""
    _, _, zs = jvp(Ws, bs, act, xt)
    return [(np.abs(z) <= rel * np.max(np.abs(z), axis=1, keepdims=True)) if a == RELU else None for z, a in zip(zs, act)]


def rel_frobenius(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ax = tuple(range(1, ref.ndim))
    return np.sqrt(np.sum((got - ref) ** 2, axis=ax)) / np.maximum(np.sqrt(np.sum(ref ** 2, axis=ax)), 1e-300)


__all__ = ["jvp", "jvp16", "operands16", "jacobian16", "masks16", "round16", "jacobian", "loglike", "transform", "forward", "oracle_outputs", "near_kinks", "rel_frobenius",
           "min_relative_preactivation", "ora"]
