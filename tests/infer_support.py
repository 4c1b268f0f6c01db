"""Device-side helpers the inference-side GPU tests share (Jacobian, likelihood, Fisher, fits and the four samplers): the
named and the tabled stacks with their records, the comparisons every file makes (bit equality, float32 ulps, the poison
pattern, the Jacobian's and the reductions' bounds, log alpha and its first-order bound) and one runner for the samplers'
_dev entries.  Importing this needs no GPU; calling what takes a `ctx` or a stack handle does."""
import numpy as np

import fit_ref as fr
import jacobian_ref as jr
import marg_ref as mr
import prior_ref as pr
import sample_ref as sr
import shape_cases as sc
import temper_ref as tr
from conftest import pkg
from helpers import STACKS, init_weights
from infer_cases import ARCHS, VG, scattered_u, transforms, vg_weights

FUSED, GENERIC = ("D1", "DE", "S3", "S4"), ("NB", "W6")
BOUND = {"f32": None, "f16": (1e-2, 3e-2), "bf16": (5e-2, 1e-1)}  # (p99, max) against the 16-bit primal's masks
# the pattern outputs and guard regions are filled with before a _dev call: as the byte memset takes, and as a 32-bit word
POISON_BYTE = 0x7F
POISON = np.frombuffer(bytes([POISON_BYTE] * 4), np.uint32)[0]
NU = np.linspace(50.0, 200.0, 451)

_named, _tabled = {}, {}


# ---- comparisons
def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def between_chain(a):
    """(pooled value, squared standard error) of per-chain estimates (chains, ...)"""
    a = np.asarray(a, np.float64)
    return a.mean(axis=0), a.var(axis=0, ddof=1) / a.shape[0]


def flags_of(nat, tin_on):
    return (nat.FWD_IN_TRANSFORM if tin_on else 0) | nat.FWD_OUT_TRANSFORM


# ---- the named stacks (helpers.STACKS, infer_cases.ARCHS / VG) and their records
def stack_of(ctx, name):
    if name not in _named:
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
        _named[name] = (st, dims, act, Ws, bs, tin, tout)
    return _named[name]


def rows_for(dims, n, seed, dtype):
    if dims[0] == 7:
        x = pkg("synth").make_params(max(n, 8), seed=seed)[:n]
    else:
        x = np.random.default_rng(seed).uniform(-1, 1, size=(n, dims[0]))
    return x.astype(dtype)


def band_weights(dout, tout, seed=1):
    """1 / sigma^2 on a band of bins, zero outside it and on a few scattered bins"""
    rng = np.random.default_rng(seed)
    w = np.full(dout, 1.0 / (0.05 * tout[0]) ** 2)
    w[: dout // 5] = 0.0
    w[rng.uniform(size=dout) < 0.1] = 0.0
    return w.astype(np.float32)


def setup(ctx, name, seed=1):
    st, dims, act, Ws, bs, tin, tout = stack_of(ctx, name)
    dout = dims[-1]
    w = band_weights(dout, tout, seed)
    x1 = rows_for(dims, 1, 99, np.float64)
    data = (jr.jacobian(Ws, bs, act, x1, tin if dims[0] == 7 else None, tout)[0][0]
            + np.random.default_rng(seed).normal(size=dout) * 0.05 * tout[0]).astype(np.float32)
    st.set_likelihood(data, w)
    return st, dims, act, Ws, bs, tin, tout, data, w


def fit_setup(ctx, name="D1", seed=3, m=3):
    """stack, its references, `m` spectra of truths drawn in the box (with noise), the record set to their weights"""
    st, dims, act, Ws, bs, tin, tout = stack_of(ctx, name)
    dout = dims[-1]
    truths = pkg("synth").make_params(m, seed=seed, zero_fx_frac=0)
    sig = 0.02 * tout[0]
    rng = np.random.default_rng(seed)
    data = (jr.jacobian(Ws, bs, act, truths, tin, tout)[0] + rng.normal(size=(m, dout)) * sig).astype(np.float32)
    w = np.full(dout, 1.0 / sig ** 2, np.float32)
    w[:40] = 0.0
    st.set_likelihood(data[0], w)
    return st, dims, act, Ws, bs, tin, tout, truths, data, w


def u_of(x, tin):
    return jr.transform(np.asarray(x, np.float64), *tin)[0]


def pick(n):
    """rows to compare: both ends, both sides of the 16,384-row slice boundary, a few more"""
    edges = [i for i in (16383, 16384, 32767, 32768) if i < n]
    return np.unique(np.r_[0, n - 1, edges, np.arange(0, n, max(1, n // 40))].astype(np.int64))


def ready(st, prec):
    """a stack outside archs.h that can have a run-time instantiated forward kernel has it before the comparison starts:
    the forward inside the call and the forward of the reference then take one route"""
    nat = pkg("_native")
    try:
        st.jit(prec, -1)
    except nat.EngineError:
        pass  # (not eligible: a Gauss layer)


# ---- the stacks of tests/shape_cases.py and their records
def new_stack(ctx, dims, act):
    """a handle of its own of a stack of the table, with its weights and transforms set (no input transform above 8 inputs)"""
    rec = sc.make_stack(dims, act)
    st = pkg("_native").Stack(ctx, dims, act)
    st.set_weights(rec["flat"])
    if rec["tin"] is not None:
        st.set_input_transform(*rec["tin"])
    st.set_output_transform(rec["tout"][0], rec["tout"][1].astype(np.float32))
    return st


def device_stack(ctx, dims, act):
    """the one shared handle of a stack of the table (new_stack), and its host record"""
    key = (tuple(dims), tuple(act))
    if key not in _tabled:
        _tabled[key] = new_stack(ctx, dims, act)
    # (no record of an earlier test, should that one have failed half way: clearing the likelihood clears the nuisance too)
    _tabled[key].set_likelihood(None, None)
    _tabled[key].set_prior(None)
    return _tabled[key], sc.make_stack(dims, act)


def shape_setup(ctx, name):
    """a stack of shape_cases with its first fit problem as the record -> (stack handle, host record, problem, flags)"""
    case = sc.BY_NAME[name]
    st, rec = device_stack(ctx, case.dims, case.act)
    prob = sc.fit_problem(case)
    st.set_likelihood(prob["data"][0], prob["w"])
    return st, rec, prob, flags_of(pkg("_native"), True)


# ---- starts
def starts_near(truth, tin, n, seed, scale=0.03, raw=True):
    """n float64 starts: the truth jittered by `scale` in u, inside the box; raw parameters, or (raw False) left in u"""
    u = np.clip(u_of(truth[None, :], tin) + scale * np.random.default_rng(seed).normal(size=(n, 7)), -0.999, 0.999)
    return fr.untransform(u, tin[0], tin[2], tin[3]) if raw else u


def starts_in_box(rec, prob, n, seed, scale):
    """n raw float64 starts: the first truth jittered by `scale` in u (scale None: infer_cases.scattered_u)"""
    d = rec["dims"][0]
    u = scattered_u(d, n, seed) if scale is None else np.clip(prob["truths_u"][:1] + scale * np.random.default_rng(seed).normal(size=(n, d)),
                                                              -0.999, 0.999)
    tin = rec["tin"]
    return fr.untransform(u, tin[0], tin[2], tin[3])


# ---- the Jacobian's rows
def check_rows(tag, prec, got, ref, Ws, bs, act, xt, tin_on, x, tin, tout):
    err = jr.rel_frobenius(got, ref)
    assert np.all(np.isfinite(err)), (tag, int(np.sum(~np.isfinite(err))))
    if prec != "f32":
        # 16-bit: the ReLU mask follows the device's 16-bit primal (z > 0 of the f16 / bf16 operands' sum), and a unit
        # whose float64 pre-activation lies within that rounding of zero switches: one switched unit of a 224-wide last
        # hidden layer moves J by ~1 / sqrt(224) ~ 7 %.  So the operand-rounding bounds hold against the
        # float64 Jacobian WITH the 16-bit primal's masks (tests/jacobian_ref.py: masks16); against the plain float64
        # Jacobian the switched rows are only reported.
        _, Jm = jr.jacobian(Ws, bs, act, x, tin if tin_on else None, tout, mask_prec=prec)
        em = jr.rel_frobenius(got, Jm)
        p99, mx = BOUND[prec]
        print("%s: vs 16-bit masks p99 %.2e max %.2e; vs float64 median %.2e, rows > %.0e: %d of %d"
              % (tag, np.percentile(em, 99), em.max(), np.median(err), mx, int(np.sum(err > mx)), err.size))
        assert np.percentile(em, 99) <= p99, (tag, np.percentile(em, 99))
        # a row beyond the max bound (at most 0.5 %): the emulation sums the 16-bit operands in float64 and rounds each
        # layer's output once, the device sums in f32 -- one layer output rounded to the neighbouring 16-bit value moves
        # the next pre-activations by ~1 ulp (2^-11 / 2^-8) of their scale, so a unit the emulation puts within 2 ulp of
        # zero may be decided the other way; such a unit must exist in the row
        bad = np.flatnonzero(em > mx)
        assert bad.size <= max(1, int(0.005 * em.size)), (tag, bad.size, em.max())
        for i in bad:
            xt1 = (jr.transform(x[i:i + 1], *tin)[0] if tin_on else x[i:i + 1].astype(np.float64)).astype(np.float32)
            _, z16 = jr.masks16(Ws, bs, act, xt1, prec, with_z=True)
            rel = 2.0 ** -10 if prec == "f16" else 2.0 ** -7
            assert any(a == jr.RELU and np.any(np.abs(z) <= rel * np.max(np.abs(z))) for z, a in zip(z16, act)), (tag, i, em[i])
        return
    bad = np.flatnonzero(err > 1e-5)
    assert bad.size <= max(1, int(0.005 * err.size)), (tag, bad.size, err.max())
    for i in bad:  # each must come within the bound once the reference flips the units at their kink -- all of them
        kinks = jr.near_kinks(Ws, bs, act, xt[i:i + 1])
        assert any(k is not None and k.any() for k in kinks), (tag, i, err[i])
        _, Jf = jr.jacobian(Ws, bs, act, x[i:i + 1], tin if tin_on else None, tout, kinks)
        assert jr.rel_frobenius(got[i:i + 1], Jf)[0] <= 1e-5, (tag, i, err[i], jr.rel_frobenius(got[i:i + 1], Jf)[0])


# ---- the marginalised reductions
def basis(K):
    return pkg("foregrounds").linlog_basis(NU, K)


def reference(y, jac, d, w, A):
    """marg_ref on the device's y and J with the float32 data as they are, and the scales of the projected residual"""
    w64 = np.asarray(w, np.float64)
    ref = mr.marg(y, jac, d, w64, A)
    Q, R = mr.whiten(A, w64)
    sc_ = mr.marg(y, jac, mr.project(d, Q, w64), w64, A)
    Ri = np.abs(np.linalg.inv(R))
    rt = np.abs(mr.project(d, Q, w64) - np.asarray(y, np.float64))
    coef_tol = (1e-5 * (rt * w64) @ np.abs(Q).T) @ Ri.T + 1e-12 * np.abs((w64 * np.asarray(d, np.float64)) @ Q.T) @ Ri.T
    return ref, sc_["lnl_scale"], sc_["grad_scale"], coef_tol


def check_reduction(tag, F, lnl, g, coef, ref, lnl_scale, grad_scale, coef_tol, worst):
    eF = np.sqrt(np.sum((F - ref["F"]) ** 2, axis=(1, 2))) / np.sqrt(np.sum(ref["F0"] ** 2, axis=(1, 2)))
    el = np.abs(lnl - ref["lnl"]) / lnl_scale
    eg = np.abs(g - ref["grad"]) / grad_scale
    worst["F"], worst["lnl"], worst["grad"] = max(worst["F"], eF.max()), max(worst["lnl"], el.max()), max(worst["grad"], eg.max())
    print("%s: F %.2e lnl %.2e grad %.2e (of 1e-5)" % (tag, eF.max(), el.max(), eg.max()))
    assert eF.max() <= 1e-5, (tag, eF.max())
    assert el.max() <= 1e-5, (tag, el.max())
    assert eg.max() <= 1e-5, (tag, eg.max())
    if coef is not None:
        ec = np.abs(coef - ref["coef"]) / coef_tol
        worst["coef"] = max(worst["coef"], ec.max())
        assert ec.max() <= 1.0, (tag, ec.max())


# ---- one Langevin transition in float64
def device_eval(st, nat, u, prec):
    """the device's own ln L, gradient and Fisher matrix at float32 points u (no input transform), as float64"""
    F, lnl, g = st.fisher(np.ascontiguousarray(u, np.float32), prec, nat.FWD_OUT_TRANSFORM, lnl=True, grad=True)
    return lnl.astype(np.float64), g.astype(np.float64), F.astype(np.float64)


def alpha_of(u0, e0, prop, e1, eps, ridge):
    """log alpha in float64 of the move u0 -> prop from the evaluations e = (lnl, g, F) at both"""
    L0, ok0 = sr.factor(e0[2], ridge)
    mu0, ld0 = sr.drift(L0, u0, e0[1], eps)
    inside = ok0 & np.all(np.abs(prop) <= 1.0, axis=1)
    return sr.log_alpha(u0, e0[0], sr.logq(L0, mu0, ld0, prop, eps), inside, prop, e1[0], e1[1], e1[2], eps, ridge)


def alpha_bound(u0, e0, prop, e1, eps, ridge, la):
    """what one float32 ulp of every input (ln L, each gradient component, each Fisher entry, at both points) moves log
    alpha by, to first order, summed in magnitude: the inputs are float32 numbers, the formula is float64"""
    bound = ulp32(e0[0]) + ulp32(e1[0])
    d = u0.shape[1]

    def moved(e):
        with np.errstate(invalid="ignore"):  # (-inf - -inf: a rejected proposal stays rejected)
            return np.abs(np.nan_to_num(alpha_of(u0, e[0], prop, e[1], eps, ridge) - la, nan=0.0, posinf=0.0, neginf=0.0))
    for side in (0, 1):
        for j in range(d):
            e = [[a.copy() for a in e0], [a.copy() for a in e1]]
            e[side][1][:, j] += ulp32(e[side][1][:, j])
            bound += moved(e)
            for k in range(j, d):
                e = [[a.copy() for a in e0], [a.copy() for a in e1]]
                h = ulp32(e[side][2][:, j, k])
                e[side][2][:, j, k] += h
                if k != j:
                    e[side][2][:, k, j] += h
                bound += moved(e)
    return bound


def posterior_eval(e, u, beta, prior):
    """an evaluation (lnl, g, F) of ln L at u as the transition at the rows' beta under the prior sees it"""
    return (tr.tmul(beta, e[0]) + pr.log_prior(prior, u), tr.tmul(beta, e[1]) + pr.grad_log_prior(prior, u),
            tr.tmul(beta, e[2]) + pr.precision(prior)[None])


def alpha_bound_prior(u0, e0, prop, e1, eps, ridge, la, beta, prior):
    """test_temper_gpu.alpha_bound_tempered with the prior's float64 terms inside the perturbed function: what one float32
    ulp of every evaluated input (ln L, each gradient component, each Fisher entry, at both points) moves log alpha by,
    to first order, summed in magnitude"""
    d = u0.shape[1]

    def moved(e):
        with np.errstate(invalid="ignore"):
            a = alpha_of(u0, posterior_eval(e[0], u0, beta, prior), prop, posterior_eval(e[1], prop, beta, prior), eps, ridge)
            return np.abs(np.nan_to_num(a - la, nan=0.0, posinf=0.0, neginf=0.0))
    bound = tr.tmul(beta, ulp32(e0[0]) + ulp32(e1[0]))
    for side in (0, 1):
        for j in range(d):
            e = [[a.copy() for a in e0], [a.copy() for a in e1]]
            e[side][1][:, j] += ulp32(e[side][1][:, j])
            bound += moved(e)
            for k in range(j, d):
                e = [[a.copy() for a in e0], [a.copy() for a in e1]]
                h = ulp32(e[side][2][:, j, k])
                e[side][2][:, j, k] += h
                if k != j:
                    e[side][2][:, k, j] += h
                bound += moved(e)
    return bound


# ---- the samplers' _dev entries
def run_dev(ctx, shapes, keys, call, x0=None, data_rows=None, guard=0):
    """One call of a sampler's _dev entry -> dict of host arrays.  `shapes`: output name -> (shape, dtype), of which `keys`
    are asked for; x0: float32 start rows (None: the entry draws them); data_rows: a float32 data matrix (None: the
    record's data); call(dx, dd, out) makes the st.sample*_dev call from the device pointers, out: name -> pointer.
    Every output and the `guard` bytes behind it are poisoned before the call, and the guard must come back untouched."""
    host = {k: np.empty(*shapes[k]) for k in keys}
    sizes = {k: max(a.nbytes + guard, 8) for k, a in host.items()}
    bufs = []

    def alloc(nbytes):
        bufs.append(ctx.malloc(max(nbytes, 8)))
        return bufs[-1]

    try:
        dx = None if x0 is None else alloc(x0.nbytes)
        dd = None if data_rows is None else alloc(data_rows.nbytes)
        out = {k: alloc(nb) for k, nb in sizes.items()}
        for k, nb in sizes.items():
            ctx.memset(out[k], POISON_BYTE, nb)
        if x0 is not None and x0.nbytes:
            ctx.h2d(dx, x0)
        if data_rows is not None:
            ctx.h2d(dd, data_rows)
        call(dx, dd, out)
        ctx.sync()
        for k, a in host.items():
            raw = np.empty(sizes[k], np.uint8)
            ctx.d2h(raw, out[k])
            a.view(np.uint8).reshape(-1)[:] = raw[:a.nbytes]
            touched = np.flatnonzero(raw[a.nbytes:a.nbytes + guard] != POISON_BYTE)
            assert touched.size == 0, "%s: %d guard bytes overwritten, the first at +%d" % (k, touched.size, touched[0])
    finally:
        for p in bufs:
            ctx.free(p)
    return host


def dev_tempered(ctx, st, x0, prec, flags, T, betas, swap_every, guard=0, **opts):
    """v21_mlp_sample_tempered_dev on float32 starts against the record -> x_last, lnl_last, mean_lnl, swap_accept"""
    n, din = x0.shape
    shapes = {"x_last": ((n, din), np.float32), "lnl_last": ((n,), np.float32), "mean_lnl": ((n,), np.float64), "swap_accept": ((n,), np.float64)}

    def call(dx, dd, out):
        sample_out, temper_out = ({k: out[k] for k in ks} for ks in (("x_last", "lnl_last"), ("mean_lnl", "swap_accept")))
        st.sample_tempered_dev(dx, din, n, None, 0, sample_out, temper_out, T, betas, swap_every, None, prec, flags, **opts)
    return run_dev(ctx, shapes, tuple(shapes), call, x0, None, guard)
