"""The cases of tests/test_jacrt_cpu.py and tests/test_jacrt_gpu.py: fused_jac<ArchRT, Prec> instantiated at run time
(csrc/jit.hip: kJitJac) on small stacks, their row counts, their refusals, the kink rule of the f32 check
and the float64 restatement of the 16-bit kernel on a stack with smooth activations.  Needs no GPU.

Stacks (weights as act_ref.stack_weights / shape_cases.make_stack build them):
    R0  5-20         lin                 one layer, one output tile: no hidden epilogue at all
    R1  5-40-72-37   relu relu lin       G = 8; partial tiles 40 / 72; two output tiles, the last partial
    R2  1-20-3       relu lin            in_dim 1 (7 padding columns), widths < 32, one output tile
    R3  7-64-9-32-48 relu LIN relu lin   REFUSED, by name: two output tiles fed by 32 features are 2 k-steps of 16 in f16 /
                                         bf16, and fused_jac's (and fused_fwd's) static_assert on the aux double buffer wants
                                         more than the read-ahead depth of 2 -- the rule that refuses [5, 63]; jit_jac_eligible
                                         takes no precision, so f32 (4 k-steps of 8) is refused with it
    R3b 7-64-9-40-48 relu LIN relu lin   what R3 was to reach: G = 8 full; a linear hidden layer (S3's 224 -> 9)
    R4  8-33-64      relu lin            the first G = 16; width 33
    R5  15-40-65     relu lin            G = 16 full
    T1, T2  5-40-72-37  tanh sigmoid / elu softplus, two units per hidden layer at bias +-90
    J1  9-40-37      tanh                smooth with G = 16
    S4  csrc/archs.h                     run time against compiled

Rows.  Both precision forms of the Jacobian family (csrc/fused_families.h: FamilyJac on PrecF32 / PrecF16x2sp / PrecBF16x2sp)
run WAVES = 4 waves of CT = 1 column tile of 32 virtual rows: 128 virtual rows per workgroup, jac_group = 8 (in_dim <= 7) or
16 of them per signal."""
import numpy as np

import act_ref as ar
import half_ref as hr
import jacobian_ref as jr
import shape_cases as sc

WAVES, CT, TILE = 4, 1, 32


def group(in_dim):
    """csrc/fused_jac.h: jac_group"""
    return 8 if in_dim <= 7 else 16


def signals(in_dim):
    """(signals per wave, signals per workgroup)"""
    g = group(in_dim)
    return CT * TILE // g, WAVES * CT * TILE // g


def row_counts(in_dim):
    """one signal; one below / at / one above a wave; one below / at / one above a workgroup; two workgroups and one
    signal; 130 rows (8 or 16 workgroups and two signals).  G = 8: (1, 3, 4, 5, 15, 16, 17, 33, 130); G = 16: (1, 2, 3, 7,
    8, 9, 17, 130) -- the sets of the issue, from FamilyJac's numbers."""
    spw, wg = signals(in_dim)
    return tuple(sorted({1, spw - 1, spw, spw + 1, wg - 1, wg, wg + 1, 2 * wg + 1, 130} - {0}))


assert row_counts(5) == (1, 3, 4, 5, 15, 16, 17, 33, 130) and row_counts(9) == (1, 2, 3, 7, 8, 9, 17, 130)

RELU_CASES = {
    "R0": ([5, 20], [0]),
    "R1": ar.RELU_CONTROL,
    "R2": ([1, 20, 3], [1, 0]),
    "R3b": ([7, 64, 9, 40, 48], [1, 0, 1, 0]),
    "R4": ([8, 33, 64], [1, 0]),
    "R5": ([15, 40, 65], [1, 0]),
}
SMOOTH_CASES = {"T1": ar.T1, "T2": ar.T2, "J1": ar.J1}
CASES = dict(RELU_CASES, **SMOOTH_CASES)
S4 = ([9, 32, 352, 451], [1, 1, 0])
# compiles, needs scratch memory in f16 (the forward's kernel of this stack does too: __graft_entry__.PREBUILT_STACKS) and is
# refused when it is loaded: the handle stays on the generic route
SPILLS = ([9, 500, 512, 33], [1, 1, 0])
PRECS = ("f32", "f16", "bf16")
# weights of R2 .. R5: shape_cases.make_stack's seed.  (Changed here, never the cap, should test_jacrt_cpu's kink share fail.)
SEED = {"R0": 3, "R2": 3, "R3b": 3, "R4": 3, "R5": 3}

# (dims, act, the reason jit_jac_eligible gives)
REFUSALS = {
    "i16o3": (sc.BY_NAME["i16o3"].dims, sc.BY_NAME["i16o3"].act, "at most 15 inputs"),
    "i8relu": (sc.BY_NAME["i8relu"].dims, sc.BY_NAME["i8relu"].act, "output layer is linear"),
    "i5gauss": (sc.BY_NAME["i5gauss"].dims, sc.BY_NAME["i5gauss"].act, "no variational head"),
    "i5lin1": ([5, 63], [0], "too narrow for the fused kernel's aux double buffer"),
    "R3": ([7, 64, 9, 32, 48], [1, 0, 1, 0], "too narrow for the fused kernel's aux double buffer"),
    "too_wide": (sc.TOO_WIDE[0], sc.TOO_WIDE[1], r"layer width not in \[1, 1024\]"),
}

_stacks = {}


def stack(name):
    """-> dict dims, act, Ws, bs, flat, tin (None above 8 inputs), tout; cached, never modified"""
    if name not in _stacks:
        dims, act = S4 if name == "S4" else CASES[name]
        if name in SEED or name == "S4":
            _stacks[name] = sc.make_stack(dims, act, SEED.get(name, 3))
        else:
            Ws, bs, flat = ar.stack_weights(dims, ar.SEEDS["RELU" if name == "R1" else name], saturate=name != "R1")
            _stacks[name] = {"dims": list(dims), "act": list(act), "Ws": Ws, "bs": bs, "flat": flat,
                             "tin": sc.input_transform(dims[0]) if sc.has_tin(dims) else None, "tout": sc.output_transform(dims[-1])}
    return _stacks[name]


def smooth(act):
    return any(a in ar.SMOOTH for a in act)


def calls(name):
    """the calls of a case: (n, input transform on, output transform on, rows in their dtype) for every row count -- with
    and without either transform where the case has one, float64 and float32 rows (shape_cases.jac_inputs' pattern)"""
    dims = stack(name)["dims"]
    for k, n in enumerate(row_counts(dims[0])):
        tin_on = sc.has_tin(dims) and k % 2 == 0
        dtype = np.float64 if k % 4 < 2 else np.float32
        x = sc.rows(dims, n, 10 + k) if tin_on else sc.rows_u(dims, n, 10 + k)
        yield n, tin_on, k % 3 != 0, x.astype(dtype)


def transformed(rec, x, tin_on):
    return jr.transform(x, *rec["tin"])[0] if tin_on else np.asarray(x, np.float64)


# ---- the f32 check's kink rule (helpers.kink_adjusted_oracle's criterion): a row is excluded when a float64
# pre-activation of a hidden ReLU unit lies within 1e-5 of its layer's largest magnitude in the call
KINK_REL = 1e-5


def kink_rows(rec, xt):
    """bool (n,): rows with a hidden ReLU unit at its kink in float64"""
    zs = [z for z, _ in ar.layers(rec["Ws"], rec["bs"], rec["act"], xt)]
    out = np.zeros(len(xt), bool)
    for z, a in zip(zs[:-1], rec["act"][:-1]):
        if a == ar.RELU:
            out |= (np.abs(z) < KINK_REL * np.abs(z).max()).any(axis=1)
    return out


def reference64(rec, x, tin_on, tout_on):
    """(y, J (n, in, out)) float64 of raw rows: jacobian_ref for ReLU stacks, act_ref.jacobian for smooth ones"""
    tin, tout = (rec["tin"] if tin_on else None), (rec["tout"] if tout_on else None)
    if not smooth(rec["act"]):
        return jr.jacobian(rec["Ws"], rec["bs"], rec["act"], x, tin, tout)
    xt, fac = jr.transform(x, *tin) if tin_on else (np.asarray(x, np.float64), np.ones(np.shape(x)))
    y = ar.forward(rec["Ws"], rec["bs"], rec["act"], xt)
    J = ar.jacobian(rec["Ws"], rec["bs"], rec["act"], xt)
    std, mean = (1.0, 0.0) if tout is None else (float(tout[0]), np.asarray(tout[1], np.float64))
    return y * std + mean, J * fac[:, :, None] * std


# ---- the 16-bit kernel on a stack with smooth layers, restated in float64 (half_ref.jvp has ReLU and linear only).
# Where fused_jac rounds ("Where fused_jac rounds"; half_ref.py:211-220), and after a smooth layer (K18):
# h = act(z) and t act'(z) are formed in f32 from the f32 sums z and t -- act' from the PRIMAL's z -- and THEN rounded to
# 16 bits by the pack.  Sums are exact here (float64); what is left of a correct kernel is its f32 summation order and the
# device's expf / log1pf (~1 ulp of f32), both far below a 16-bit rounding step: single roundings flip, medians do not.
SMOOTH_MUTATIONS = (
    "deriv_out",   # the derivative taken from the ROUNDED output h (1 - h^2 ...) instead of z
    "tan_tile",    # the site's units 16 .. 31, last input's tangent, scaled by 1 + 2^-8 before rounding (half_ref's entry)
    "deriv16",     # the derivative rounded to 16 bits before the multiply
)


def smooth_site(act):
    """the hidden layer the mutations edit: the last smooth hidden layer"""
    return max(l for l, a in enumerate(act[:-1]) if a in ar.SMOOTH)


def jvp16_smooth(Ws, bs, act, xt, prec, fac=None, std=None, mut=None):
    """(y, J (n, in, out)) of rows xt (float32, after par_transform) as fused_jac<ArchRT, prec> forms them; fac, std as
    half_ref.jvp takes them; y in the network's units."""
    h = hr.round16(np.asarray(xt, np.float32).astype(np.float64), prec)
    n, din = h.shape
    T = np.repeat(np.eye(din)[None], n, axis=0)
    L = len(act)
    site = smooth_site(act) if mut else None
    for l, (W, b, a) in enumerate(zip(Ws, bs, act)):
        Wr = hr.round16(np.asarray(W, np.float64), prec)
        z = h @ Wr + np.asarray(b, np.float64)
        Tz = T @ Wr
        if a in ar.SMOOTH:
            hh = ar.act(a, z)
            d = ar.deriv(a, z)
            if l == site and mut == "deriv_out":
                d = ar.deriv_out(a, hr.round16(hh, prec))
            if l == site and mut == "deriv16":
                d = hr.round16(d, prec)
            h, T = hh, Tz * d[:, None, :]
        elif a == ar.RELU:
            m = z > 0
            h, T = np.where(m, z, 0.0), Tz * m[:, None, :]
        else:
            h, T = z, Tz
        if l < L - 1:
            if l == site and mut == "tan_tile":
                T = T.copy()
                T[:, din - 1, 16:32] *= 1 + 2.0 ** -8
            h, T = hr.round16(h, prec), hr.round16(T, prec)
    if std is not None:
        T = T * float(std)
    if fac is not None:
        T = T * np.asarray(fac, np.float64)[:, :, None]
    return h, T


def jacobian16(rec, x, prec, tin_on, tout_on, mut=None):
    """the rounding reference of a case's call: jacobian_ref.jacobian16 for ReLU / linear stacks (mut: an entry of
    half_ref.JAC_MUTATIONS), the restatement above for smooth ones (mut: an entry of SMOOTH_MUTATIONS)"""
    tin, tout = (rec["tin"] if tin_on else None), (rec["tout"] if tout_on else None)
    if not smooth(rec["act"]):
        return jr.jacobian16(rec["Ws"], rec["bs"], rec["act"], x, prec, tin, tout, mut=mut)
    xt, fac, std = jr.operands16(x, tin, tout)
    y, J = jvp16_smooth(rec["Ws"], rec["bs"], rec["act"], xt, prec, fac if tin_on else None, std, mut)
    if tout is not None:
        y = y * float(tout[0]) + np.asarray(tout[1], np.float64)
    return y, J


# The bound of the smooth 16-bit check (worst-cell median, half_ref.jac_worst_cell_median), by DESIGN.md K6's rule: at most
# 4x the worst measured on the MI355X, at most 1/4 of what the cheapest entry of SMOOTH_MUTATIONS moves the statistic.
# Measured over every call of T1, T2, J1, f16 / bf16:
#     worst                                   1.156e-7 (T1, 130 rows) / 8.08e-8 (T2, 130 rows)
#     mutations on the device's own J, least over the calls of >= 31 rows (below, cells are pooled and one tile's
#     scaling does not move the pooled median):
#         deriv_out 6.62e-5 / 4.96e-4     tan_tile 2.59e-3 / 3.42e-3     deriv16 2.69e-4 / 1.72e-3
# 4 x worst = 4.6e-7 / 3.2e-7; 1/4 of the cheapest mutation = 1.65e-5 / 1.24e-4: the first decides.
SMOOTH16_MEASURED = {"f16": 1.156e-7, "bf16": 8.08e-8}
SMOOTH16_TOL = {"f16": 4.5e-7, "bf16": 3.2e-7}
