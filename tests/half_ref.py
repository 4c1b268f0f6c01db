"""float64 reference of the 16-bit kernels that rounds where they round (forward, loss, full gradient, ReLU decisions).

The plain float64 oracle (helpers.oracle_step, jacobian_ref.forward) differs from an f16 / bf16 result by the rounding of
the matrix-product operands: ~1e-3 per layer of gradient, ~1e-4 of output.  A bound that wide also passes a kernel that
drops a batch block, rounds a layer the wrong way or loses a row of the loss.  This module rounds the operands as the
kernels do and sums exactly, so what is left of a device result is the f32 summation order (and the one-ulp hidden values
that order moves across a 16-bit rounding midpoint).

Where the kernels round (every 16-bit route; csrc/):
  * matrix-product operands are rounded to 16 bits, round to nearest even: the input rows after par_transform
    (fused_fwd.h:444, fused_train.h:276, fused_train16.h:266, the chain kernel's operand image), the weights (the packed
    streams: adam_repack_kernel / wt_pack_kernel) and the hidden activations after ReLU (fused_fwd.h:490-493,
    train_chain.h:505-518, fused_train.h:314-325, fused_train16.h:296-303; per_layer / small / generic: gemm_nt.h:215
    casts the f32 activation when it loads it -- the same value, since rounding is monotonic);
  * products are summed in f32 (MFMA); the f32 bias is the accumulator's initial value (fused_fwd.h:556,
    train_chain.h:479) or added to the sum (gemm_nt.h:337-339, gemm.h:163-164) -- the same in exact arithmetic;
  * the output layer is not rounded; the output transform is (acc + b) * std + mean (fused_fwd.h:513-516,
    gemm_nt.h:339, train_chain.h:543);
  * the loss is formed from the unrounded output, the f32 targets and row weights (train_kernels.h:130-153
    loss_grad_t_kernel, train_chain.h:554-568, fused_train.h:350-354, fused_train16.h:322-326);
  * gradient operands are multiplied by gs = grad_opscale(brows, dout) (api_trainer.hip:393) before they are rounded:
    dZ16 = round16(gs dz) (train_chain.h:567, fused_train.h:354, gemm_nt.h: b_scale / a_scale = gs);
    dX = dZ16 round16(W)^T / gs, masked by the forward's ReLU decisions, and the dZ16 of the layer below is
    round16(gs dX) (train_chain.h:662-674, fused_train.h:357-370; per_layer: out_scale 1/gs, then a_scale gs);
    [dW; db] = [H16; 1]^T dZ16 / gs (the gemm_dw16 / dw16_adam out_scale, api_trainer.hip dw16_problems; per_layer
    NT_DW).

One thing differs between routes, the ReLU decision the backward pass uses (`mask`):
  "sum"     -- z > 0 on the f32 sum: chain16 (train_chain.h:511 tests the f32 accumulator), per_layer (gemm_nt.h
               NT_DX_MASK reads the f32 activation), and the forward of every route (a value that rounds to +0 is 0);
  "rounded" -- round16(z) > 0: fused128 and fused64 (fused_train.h:320-325, fused_train16.h:297-303: the mask of the
               packed pair, so a pre-activation that underflows to +0 passes no gradient).
route_model() names the model of each training route.

jvp() is the forward-mode pass of the fused 16-bit Jacobian (csrc/fused_jac.h), rounded where that kernel rounds -- its
own section below lists the sites -- with JAC_MUTATIONS the catalogue of its tangents (tests/test_jac16_*.py).

`acc="f32"` is the DEVICE MODEL the CPU self-tests use: the same computation with numpy's f32 accumulation standing in
for the kernels' summation order.  MUTATIONS is the catalogue of plausible kernel mistakes the new checks must refuse;
the CPU tests apply it to the device model, the GPU tests to the device's own returned arrays (apply_* below: the
difference the mistake makes to the reference, added on the host)."""
import math

import numpy as np

from oracle import ref_numpy as ora

RELU, GAUSS = 1, 2


# ---- rounding ----------------------------------------------------------------------------------------------------------

def round16(a, prec):
    """float64 -> the nearest f16 / bf16 value (round to nearest even, overflow to +-inf, subnormals kept, -0 kept), as
    float64.  prec None: unchanged (the rounding switched off).  bf16 rounds the float32 value (what the kernels hold)."""
    a = np.asarray(a, np.float64)
    if prec is None:
        return a
    if prec == "f16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(np.float64)
    if prec != "bf16":
        raise ValueError(prec)
    with np.errstate(over="ignore"):
        u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    out = u.astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(nan, np.nan, out)


def round16_toward_zero(a, prec):
    """the same grid, rounded toward zero (a MUTATION: the kernels round to nearest)"""
    a = np.asarray(a, np.float64)
    if prec == "f16":
        r = a.astype(np.float16).astype(np.float64)
        over = np.abs(r) > np.abs(a)
        step = np.nextafter(r.astype(np.float16), np.float16(0)).astype(np.float64)
        return np.where(over, step, r)
    u = a.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def grad_opscale(brows, dout):
    """api_trainer.hip:393: 2^clamp(lround(log2(max(1, brows dout / 16))), 0, 24).  C lround rounds halves away from zero
    (the argument is >= 0 here: floor(x + 0.5))."""
    s = float(brows) * float(dout) / 16.0
    e = int(math.floor(math.log2(max(1.0, s)) + 0.5))
    return float(2.0 ** max(0, min(24, e)))


def route_model(route):
    """the ReLU-decision model a 16-bit training route follows (module docstring) -> "sum" / "rounded".  route: the name
    of Trainer.last_route()[0][0] (or the tuple itself)."""
    fwd = route[0] if isinstance(route, tuple) else route
    if fwd in ("fused128", "fused64"):
        return "rounded"
    if fwd in ("chain16", "per_layer"):
        return "sum"
    raise ValueError("no 16-bit model for route %r" % (route,))


# ---- the mutation catalogue ----------------------------------------------------------------------------------------------
# name -> (what it changes, precisions it applies to).  Each is one plausible mistake of a 16-bit kernel; the layer / block /
# tile it touches is fixed by mutation_site() so that the CPU and the GPU tests mean the same edit.
MUTATIONS = {
    "hidden_rtz": ("forward", ("f16", "bf16")),   # one hidden layer's activations rounded toward zero, not to nearest
    "bias16": ("forward", ("f16", "bf16")),       # the bias rounded to 16 bits before it is added
    "dw_block": ("grad", ("f16", "bf16")),        # one 32-row batch block missing from one layer's [dW; db]
    "dw_tile": ("grad", ("f16", "bf16")),         # one 16-wide column tile of one layer's [dW; db] scaled by 1 + 2^-8
    "loss_row": ("loss", ("f16", "bf16")),        # the loss without one row
    "dz_nogs": ("grad", ("f16",)),                # one layer's dZ rounded without gs (bf16: gs changes nothing)
}
# What the STEP check (loss + gradient) cannot be asked to refuse, and why:
#   bias16 -- a bias of ~0.05 rounded to f16 moves an f16 step's loss by 5e-7 .. 8e-7 (D1, AE at 4,096 rows), inside the
#             loss bound the device needs (1.2e-6); the forward check refuses it by its median (1e-5 against 8e-8);
#   dz_nogs unless rows x outputs >= 2^20 -- gs (grad_opscale) lifts dz ~ 2 w (p - y) / rows out of the f16 subnormals
#             where that product is large (D1 / AE at >= 4,096 rows: 1e-2 of a layer without it); for 256-row steps, the
#             9-wide latent emulator or a 33-wide output dz is normal anyway and rounding it without gs moves a layer by
#             3e-4 .. 8e-4 (measured on the MI355X) -- inside the bounds;
#   dw_block above 8,192 rows -- one 32-row block is < 0.4 % of a layer, under the f16 noise of the device's one-ulp
#             hidden-activation flips (~1e-3 of a layer).
STEP_CHECK_MIN_ELEMENTS = {"dz_nogs": 1 << 20}   # rows x outputs
STEP_CHECK_MAX_ROWS = {"dw_block": 8192}


def mutations_for(prec, kind=None):
    """names of the catalogue that apply to prec (and change `kind`: "forward" entries change forward, loss and gradient)"""
    out = []
    for name, (what, precs) in MUTATIONS.items():
        if prec in precs and (kind is None or what == kind or (kind in ("loss", "grad") and what == "forward")):
            out.append(name)
    return out


def step_mutations(prec, rows, dout, act=None):
    """the catalogue entries the step check must refuse on a step of `rows` rows and `dout` outputs (see above); a stack
    without a hidden ReLU layer has no hidden activations to round the wrong way"""
    no_hidden = act is not None and mutation_site(act, rows)[0] is None
    return [m for m in mutations_for(prec) if m != "bias16" and rows * dout >= STEP_CHECK_MIN_ELEMENTS.get(m, 0)
            and rows <= STEP_CHECK_MAX_ROWS.get(m, 1 << 40) and not (m == "hidden_rtz" and no_hidden)]


def mutation_site(act, rows):
    """(hidden layer, gradient layer, batch block rows, dz layer, loss row) the catalogue edits"""
    L = len(act)
    hidden = [l for l in range(L - 1) if act[l] == RELU]
    hl = hidden[len(hidden) // 2] if hidden else None
    gl = L // 2
    b0 = 32 if rows > 64 else 0
    return hl, gl, (b0, min(rows, b0 + 32)), L - 1, rows - 1


# ---- forward --------------------------------------------------------------------------------------------------------------

def _layer_params(Ws, bs, act):
    """(W, b) float64 as the forward uses them: a V21_ACT_GAUSS layer's z_mean columns only (include/v21.h)"""
    out = []
    for W, b, a in zip(Ws, bs, act):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        if a == GAUSS:
            k = W.shape[1] // 2
            W, b = W[:, :k], b[:k]
        out.append((W, b))
    return out


def _mm(a, b, acc):
    if acc == "f32":   # the device model: f32 products summed in f32 (numpy's sgemm order stands in for the MFMA's)
        return (a.astype(np.float32) @ b.astype(np.float32)).astype(np.float64)
    return a @ b


def forward(Ws, bs, act, xt, prec, tout=None, acc="f64", mut=None, keep=False):
    """outputs of rows xt (after par_transform, float64 or float32): every product operand round16, products summed
    exactly (acc "f64") or in f32 (acc "f32": the device model), the f32 bias added, ReLU on that sum; the output layer
    unrounded, then (acc + b) * std + mean with tout = (std, mean).
    keep: (y, hs16 = the operands of every layer, zs = the pre-activations)."""
    h = np.asarray(xt, np.float64) if prec is None else round16(np.asarray(xt, np.float32).astype(np.float64), prec)
    hs, zs = [h], []
    L = len(act)
    site = mutation_site(act, len(h))[0] if mut == "hidden_rtz" else None
    for l, ((W, b), a) in enumerate(zip(_layer_params(Ws, bs, act), act)):
        if mut == "bias16":
            b = round16(b, prec)
        z = _mm(h, round16(W, prec), acc) + b
        if acc == "f32":
            z = z.astype(np.float32).astype(np.float64)
        zs.append(z)
        if l < L - 1:
            r = np.maximum(z, 0) if a == RELU else z
            h = round16_toward_zero(r, prec) if l == site else round16(r, prec)
            hs.append(h)
        else:
            h = np.maximum(z, 0) if a == RELU else z
    y = h
    if tout is not None:
        y = y * float(tout[0]) + np.asarray(tout[1], np.float64)
    return (y, hs, zs) if keep else y


def masks16(Ws, bs, act, xt, prec, with_z=False):
    """the ReLU decisions of a 16-bit primal (the fused forward kernels: z > 0 on the sum) -- per layer a bool (n, units)
    array or None (and the pre-activations with with_z).  jacobian_ref.masks16 is this function."""
    _, _, zs = forward(Ws, bs, act, xt, prec, keep=True)
    out = [z > 0 if a == RELU else None for z, a in zip(zs, act)]
    return (out, zs) if with_z else out


# ---- forward-mode tangents: the fused 16-bit Jacobian (csrc/fused_jac.h) --------------------------------------
# Where fused_jac<Arch, Prec> rounds (read off the kernel):
#   * layer-0 operand: the primal column holds the transformed f32 row rounded to 16 bits (P::pack2, fused_jac.h:97-108);
#     the tangent columns are exact unit vectors, so the layer-0 tangents are rows of round16(W0), exact in f32;
#   * weights: round16(W) of the forward's packed stream; the f32 bias is the accumulator's initial value on the primal
#     columns only (:245), products are summed in f32 (MFMA);
#   * hidden layers: the ReLU decision is z > 0 on the PRIMAL's f32 sum (:145-148) and masks primal and tangents alike;
#     then primal AND tangents are rounded to 16 bits by P::pack2 (:150-151) -- a linear hidden layer (S3's 224 -> 9)
#     included;
#   * output layer: nothing is rounded; tangents are multiplied by out_std (the f32 the handle holds) and then by the f32
#     chain-rule factor of the input transform (:176-179); y takes the forward's epilogue (half_ref.forward).
# The mutation catalogue of the tangents, in the scheme of MUTATIONS: the mistake is made inside the reference and the
# difference it makes is added to the device's own J (apply_jac_mutation).  jac_mutation_site() fixes the layer.
JAC_MUTATIONS = {
    "tan_rtz": ("f16", "bf16"),          # the middle hidden layer's tangents rounded toward zero, not to nearest
    "tan_tile": ("f16", "bf16"),         # its units 16..31, last input's tangent only, scaled by 1 + 2^-8 before rounding
    "fac16": ("f16", "bf16"),            # the chain-rule factor rounded to 16 bits before the output multiply (needs fac)
    "out_tile": ("f16", "bf16"),         # bins 32..63 of the last input's Jacobian row scaled by 1 + 2^-8 (the epilogue)
    "prim_unrounded": ("f16", "bf16"),   # the layer-0 primal operand left in f32: moves the masks and y
}
# What the Jacobian's median check is NOT asked to refuse, and why (tests/test_jac16_cpu.py holds the numbers):
#   prim_unrounded -- it changes the PRIMAL: y moves by ~1e-5 / 1e-4 of its scale (f16 / bf16) in the median row, which the
#             primal's bit-identity with fused_fwd (tests/test_jacobian_gpu.py) and the forward's own rounding check
#             (tests/test_half_ref_gpu.py) refuse outright.  On J it acts only through the ReLU units the moved primal
#             switches: whole rows at a time, none in most rows of most cells -- the per-cell MEDIAN of a stack is 0 or
#             far below 16x the device model (the CPU module asserts which), so the entry is kept for the primal and left
#             out of jac_mutations().
JAC_CHECK_SKIPS = ("prim_unrounded",)


def jac_mutation_site(act):
    """the hidden layer the tangent entries edit: the middle hidden ReLU layer (mutation_site's rule).  Never layer 0 on
    a stack with two or more hidden ReLU layers -- layer 0's tangents are rows of round16(W0), which no rounding moves."""
    return mutation_site(act, 0)[0]


def jac_mutations(prec, with_fac, act=None):
    """names of JAC_MUTATIONS the Jacobian's median check must refuse for a call: fac16 only with an input transform (a
    factor of 1 rounds to 1), the hidden-layer entries only on a stack with a hidden ReLU layer above layer 0"""
    no_site = act is not None and not jac_mutation_site(act)
    return [m for m, precs in JAC_MUTATIONS.items() if prec in precs and m not in JAC_CHECK_SKIPS
            and (with_fac or m != "fac16") and not (no_site and m in ("tan_rtz", "tan_tile"))]


def jvp(Ws, bs, act, xt, prec, acc="f64", flips=None, masks=None, fac=None, std=None, mut=None):
    """(y (n, out), J (n, in, out) = d y / d xt, pre-activations per layer) of rows xt (after par_transform), rounded
    where fused_jac rounds (above): acc "f64" sums exactly (the reference), "f32" is the CPU device model.  prec None:
    jacobian_ref.jvp bit for bit.  flips / masks as in jacobian_ref.jvp.  fac (n, in), std: the output layer's tangents
    times std times fac (the kernel's order), both as the kernel holds them (f32 values); y stays in the network's units.
    mut: an entry of JAC_MUTATIONS."""
    h = np.asarray(xt, np.float64)
    if prec is not None and mut != "prim_unrounded":
        h = round16(np.asarray(xt, np.float32).astype(np.float64), prec)
    elif prec is not None:
        h = np.asarray(xt, np.float32).astype(np.float64)
    n, din = h.shape
    T = np.repeat(np.eye(din)[None], n, axis=0)
    zs = []
    L = len(act)
    site = jac_mutation_site(act) if mut in ("tan_rtz", "tan_tile") else None
    for l, ((W, b), a) in enumerate(zip(_layer_params(Ws, bs, act), act)):
        Wr = round16(W, prec)
        z = _mm(h, Wr, acc) + b
        Tz = _mm(T, Wr, acc)
        if acc == "f32":
            z = z.astype(np.float32).astype(np.float64)
        zs.append(z)
        if a == RELU:
            m = z > 0 if masks is None else masks[l]
            if flips is not None and flips[l] is not None:
                m = m ^ flips[l]
            h = np.where(m, z, 0.0)
            T = Tz * m[:, None, :]
        else:
            h, T = z, Tz
        if l < L - 1:
            if mut == "tan_tile" and l == site:
                T = T.copy()
                T[:, din - 1, 16:32] *= 1 + 2.0 ** -8
            h = round16(h, prec)
            T = round16_toward_zero(T, prec) if (mut == "tan_rtz" and l == site) else round16(T, prec)
    if std is not None:
        T = T * float(std)
    if fac is not None:
        f = np.asarray(fac, np.float64)
        T = T * (round16(f, prec) if mut == "fac16" else f)[:, :, None]
    if mut == "out_tile":
        T = T.copy()
        T[:, din - 1, 32:64] *= 1 + 2.0 ** -8
    return h, T, zs


def apply_jac_mutation(name, J, Ws, bs, act, xt, prec, fac=None, std=None, Jref=None):
    """J (a device result of rows xt) edited as if fused_jac made mistake `name`: J + (reference with it - without it)"""
    if Jref is None:
        Jref = jvp(Ws, bs, act, xt, prec, fac=fac, std=std)[1]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(J, np.float64) + (jvp(Ws, bs, act, xt, prec, fac=fac, std=std, mut=name)[1] - Jref)


def jac_cell_errors(J, Jref, tile=32):
    """(n, in, ceil(out / tile)): ||J - Jref||_2 / ||Jref||_2 over the bins of every (row, input, 32-bin output tile)
    cell; a cell that is not finite counts as infinitely wrong"""
    J, Jref = np.asarray(J, np.float64), np.asarray(Jref, np.float64)
    n, din, dout = Jref.shape
    nt = -(-dout // tile)
    pad = nt * tile - dout
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = np.pad((J - Jref) ** 2, ((0, 0), (0, 0), (0, pad))).reshape(n, din, nt, tile).sum(-1)
    r2 = np.pad(Jref ** 2, ((0, 0), (0, 0), (0, pad))).reshape(n, din, nt, tile).sum(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.sqrt(d2) / np.sqrt(np.maximum(r2, 1e-300))
    return np.where(np.isfinite(e), e, np.inf)


JAC_POOL_BELOW = 31   # rows: a median over fewer could be decided by one row with a unit at its kink


def jac_worst_cell_median(J, Jref, tile=32):
    """the Jacobian check's statistic: the median over rows of every cell's error, the worst cell of them; calls of fewer
    than JAC_POOL_BELOW rows: the median of all the call's cell errors pooled"""
    e = jac_cell_errors(J, Jref, tile)
    if e.shape[0] < JAC_POOL_BELOW:
        return float(np.median(e))
    return float(np.median(e, axis=0).max())


# ---- one optimizer step: loss and full gradient ---------------------------------------------------------------------------

def step(Ws, bs, act, x, tgt, w, prec, mask="sum", brows=None, acc="f64", mut=None, flips=None, keep=False):
    """(loss, flat gradient [W0, b0, W1, ...]) of one step of rows x against targets tgt with row weights w, as the 16-bit
    kernels form them (module docstring).  prec None: the plain float64 oracle.  brows: the rows the loss is averaged over
    (default len(x)).  flips: {(layer, row, unit)} whose ReLU derivative is taken the other way (kink analysis).
    keep: also the per-row losses."""
    L = len(act)
    rows = len(x)
    B = rows if brows is None else brows
    y, hs, zs = forward(Ws, bs, act, x, prec, acc=acc, mut=mut if mut in ("hidden_rtz", "bias16") else None, keep=True)
    Wr = [round16(np.asarray(W, np.float64), prec) for W, _ in _layer_params(Ws, bs, act)]
    t64, w64 = np.asarray(tgt, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    d = y - t64
    if acc == "f32":
        d = d.astype(np.float32).astype(np.float64)
    rowloss = w64 * np.sum(d * d, axis=1)
    hl, gl, (b0, b1), zl, lr = mutation_site(act, rows)
    loss = float((rowloss.sum() - (rowloss[lr] if mut == "loss_row" else 0.0)) / B)
    dz = (2.0 / B) * w64[:, None] * d
    gs = grad_opscale(B, y.shape[1]) if prec is not None else 1.0
    dz16 = gs * round16(dz, prec) if (mut == "dz_nogs" and zl == L - 1) else round16(gs * dz, prec)
    dWs, dbs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        H = hs[l]
        if mut == "dw_block" and l == gl:
            keep_rows = np.r_[0:b0, b1:rows]
            dWs[l] = _mm(H[keep_rows].T, dz16[keep_rows], acc) / gs
            dbs[l] = dz16[keep_rows].sum(0) / gs
        else:
            dWs[l] = _mm(H.T, dz16, acc) / gs
            dbs[l] = dz16.sum(0) / gs
        if mut == "dw_tile" and l == gl:
            c0 = 16 if dWs[l].shape[1] >= 32 else 0
            dWs[l][:, c0:c0 + 16] *= 1 + 2.0 ** -8
            dbs[l][c0:c0 + 16] *= 1 + 2.0 ** -8
        if l == 0:
            break
        dx = _mm(dz16, Wr[l].T, acc)
        if act[l - 1] == RELU:
            z = zs[l - 1]
            m = (z > 0) if mask == "sum" else (round16(z, prec) > 0)
            if flips:
                m = m.copy()
                for (fl, fr, fu) in flips:
                    if fl == l - 1:
                        m[fr, fu] = not m[fr, fu]
            dx = dx * m
        dz16 = round16(dx, prec) if not (mut == "dz_nogs" and zl == l - 1) else gs * round16(dx / gs, prec)
    g = ora.flatten_params(dWs, dbs)
    return (loss, g, rowloss) if keep else (loss, g)


# ---- the checks' statistics -------------------------------------------------------------------------------------------------

def forward_stats(y, yref, scale=1.0):
    """(median, p99, max) of |y - yref| / scale"""
    d = np.abs(np.asarray(y, np.float64) - np.asarray(yref, np.float64)).ravel() / scale
    return float(np.median(d)), float(np.percentile(d, 99)), float(d.max())


def layer_rel_l2(dims, g, gref):
    """per layer's [W; b] block of the flat arena: ||g - gref|| / ||gref||"""
    offs = np.cumsum([0] + [a * b + b for a, b in zip(dims[:-1], dims[1:])])
    out = []
    for i in range(len(dims) - 1):
        a, b = np.asarray(g[offs[i]:offs[i + 1]], np.float64), np.asarray(gref[offs[i]:offs[i + 1]], np.float64)
        out.append(float(np.linalg.norm(a - b) / max(1e-300, np.linalg.norm(b))))
    return out


def tile_rel_l2(dims, g, gref, width=16):
    """per layer: the worst relative L2 over its 16-column tiles of [W; b] (one tile scaled by 1 + 2^-8 is 3.9e-3 there,
    ~1e-3 of the whole layer -- inside the f16 noise of the per-layer figure)"""
    offs = np.cumsum([0] + [a * b + b for a, b in zip(dims[:-1], dims[1:])])
    out = []
    for i in range(len(dims) - 1):
        K, N = dims[i] + 1, dims[i + 1]
        a = np.asarray(g[offs[i]:offs[i + 1]], np.float64).reshape(K, N)
        b = np.asarray(gref[offs[i]:offs[i + 1]], np.float64).reshape(K, N)
        worst = 0.0
        for c in range(0, N, width):
            worst = max(worst, float(np.linalg.norm(a[:, c:c + width] - b[:, c:c + width]) / max(1e-300, np.linalg.norm(b[:, c:c + width]))))
        out.append(worst)
    return out


def step_errors(dims, loss, g, lref, gref):
    """(relative loss error, worst per-layer relative L2 of the gradient, worst 16-column tile's relative L2)"""
    return abs(float(loss) - lref) / abs(lref), max(layer_rel_l2(dims, g, gref)), max(tile_rel_l2(dims, g, gref))


# ---- the catalogue applied to results ---------------------------------------------------------------------------------------

def apply_forward_mutation(name, y, Ws, bs, act, xt, prec, tout=None, yref=None):
    """y (a device result of rows xt) edited as if its kernel made mistake `name`: y + (reference with it - without it)"""
    if yref is None:
        yref = forward(Ws, bs, act, xt, prec, tout=tout)
    return np.asarray(y, np.float64) + (forward(Ws, bs, act, xt, prec, tout=tout, mut=name) - yref)


def apply_step_mutation(name, loss, g, Ws, bs, act, x, tgt, w, prec, mask="sum", brows=None, ref=None):
    """(loss, g) of a device step edited as if its kernels made mistake `name` (the difference it makes to the reference)"""
    if ref is None:
        ref = step(Ws, bs, act, x, tgt, w, prec, mask=mask, brows=brows)
    lm, gm = step(Ws, bs, act, x, tgt, w, prec, mask=mask, brows=brows, mut=name)
    return float(loss) + (lm - ref[0]), np.asarray(g, np.float64) + (gm - ref[1])


# ---- ReLU kinks --------------------------------------------------------------------------------------------------------------

def kink_adjusted(Ws, bs, act, x, tgt, w, prec, g_dev, gref, mask="sum", brows=None, rel_thr=1e-3, max_entries=400):
    """The rounding reference's gradient for the assignment of d relu / dz that the DEVICE made at pre-activations that
    are zero to within its rounding (helpers.kink_adjusted_oracle, on this reference): every (layer, row, unit) with
    |z| < rel_thr x the layer's largest |z| is a candidate; one is taken when the residual of ITS OWN column of [W; b]
    contains the one-row delta of flipping it with coefficient 1 (0.95 .. 1.05).  Upper layers first (a flip changes its
    own layer's column and the layers below, nothing above).  -> (adjusted flat gradient, [(layer, row, unit, z)]), or
    (gref, None) with too many candidates."""
    L = len(act)
    _, _, zs = forward(Ws, bs, act, x, prec, keep=True)
    cand = []
    for l in range(L - 1):
        if act[l] != RELU:
            continue
        thr = rel_thr * float(np.abs(zs[l]).max())
        rr, uu = np.where(np.abs(zs[l]) < thr)
        cand += [(l, int(r), int(u)) for r, u in zip(rr, uu)]
    if len(cand) > max_entries:
        return gref, None
    B = len(x) if brows is None else brows
    dims = [np.shape(Ws[0])[0]] + [np.shape(W)[1] for W in Ws]
    offs = np.cumsum([0] + [a * b + b for a, b in zip(dims[:-1], dims[1:])])

    def row_grad(r, flips):
        fl = {(l, 0, u) for (l, u) in flips}
        return step(Ws, bs, act, x[r:r + 1], tgt[r:r + 1], w[r:r + 1], prec, mask=mask, brows=B, flips=fl)[1]

    res = np.asarray(g_dev, np.float64) - gref
    adj = np.array(gref, np.float64)
    taken = []
    by_col = {}
    for (l, r, u) in cand:
        by_col.setdefault((l, u), []).append(r)
    for (l, u) in sorted(by_col, key=lambda c: -c[0]):
        K, N = dims[l], dims[l + 1]
        col = lambda v: v[offs[l]:offs[l + 1]].reshape(K + 1, N)[:, u]
        rows_left = list(by_col[(l, u)])
        while rows_left:
            rescol = col(res)
            best = None
            for r in rows_left:
                flips_r = {(tl, tu) for (tl, tr_, tu, _) in taken if tr_ == r}
                delta = row_grad(r, flips_r | {(l, u)}) - row_grad(r, flips_r)
                dcol = col(delta)
                n2 = float(dcol @ dcol)
                if n2 <= 0:
                    continue
                fit = float(rescol @ dcol) / n2
                if abs(fit - 1.0) < 0.05 and (best is None or n2 > best[0]):
                    best = (n2, r, delta)
            if best is None:
                break
            _, r, delta = best
            res -= delta
            adj += delta
            taken.append((l, r, u, float(zs[l][r, u])))
            rows_left.remove(r)
    return adj, taken
