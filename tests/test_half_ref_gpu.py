"""Every 16-bit forward route against the float64 reference that rounds where the kernels round (tests/half_ref.py).

The float64 oracle's bounds (infer_cases.HALF_BOUNDS: max |d| 1e-3 f16, 1e-2 bf16) cover operand rounding, and so
also a kernel that rounds a hidden layer toward zero or rounds its bias (max |d| 1.4e-4 / 1.3e-3 from a correct one).
Against the rounding reference a correct kernel differs by its f32 summation order only, and in a few rows by the one-ulp
hidden values that order moves across a 16-bit rounding midpoint -- so the checks bound the MEDIAN and the 99th percentile
of |d| (single rows decide a max) and keep the float64 max.  Every route of the table, f16 and
bf16, at 1, 31, 33, 4,097 and 65,536 rows (the last on a 2,048-row sample), with and without the input and output
transforms; the route taken is asserted, and the mutation catalogue (half_ref.MUTATIONS, its forward entries) applied to
the device's own outputs must be refused.

Bounds (helpers.FWD16_TOL; |d| in pre-processed units: divided by the output transform's std), at most 4x the worst
measured on the MI355X over every case here: f16 median 2.0e-8, p99 2.2e-5, max 1.6e-4; bf16 median 1.6e-8, p99 2.8e-6, max 8.8e-4.  (Per route,
f16 / bf16 median: fused 2.0e-8 / 1.6e-8, fused_rt 1.6e-8 / 1.5e-8, table 1.4e-8 / 1.3e-8, small 1.3e-8 / 1.3e-8, generic
1.5e-8 / 1.3e-8; a hidden layer rounded toward zero or a rounded bias moves the median to ~1e-5 / ~1e-4.)"""
import numpy as np
import pytest

import half_ref as hr
from conftest import pkg
from helpers import FWD16_TOL, STACKS
from infer_cases import ARCHS as FUSED_STACKS, HALF_BOUNDS
from oracle import ref_numpy as ora

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 33, 4097, 65536)
SAMPLE = 2048


def _weights(dims, act, seed):
    Ws, bs = ora.init_mlp(dims, seed=seed)
    rng = np.random.default_rng(seed + 100)
    bs = [rng.normal(scale=0.05, size=b.shape).astype(np.float32) for b in bs]
    return Ws, bs


def _transforms(st, dims):
    """the class surface's par_transform / unpreproc on a 7 -> 451 stack -> (flags, tin for the reference, tout)"""
    synth, pp, native = pkg("synth"), pkg("preprocess"), pkg("_native")
    par_train = synth.make_params(2000, seed=1, corners=True)
    ps, ss = pp.ParamStats.of(par_train), pp.SignalStats.of(synth.make_signals(512, seed=3))
    st.set_input_transform(ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
    st.set_output_transform(ss.std, ss.mean)
    return native.FWD_IN_TRANSFORM | native.FWD_OUT_TRANSFORM, par_train, (float(ss.std), np.asarray(ss.mean, np.float64))


def _check(tag, y, x, Ws, bs, act, prec, par_train=None, tout=None, seen=None):
    """device outputs y of raw rows x: stats against the rounding reference, the float64 bound, the mutations refused"""
    n = len(x)
    pick = np.arange(n) if n <= 4097 else np.r_[np.random.default_rng(n).choice(n - 16, SAMPLE - 16, replace=False), n - 16:n]
    xs, ys = x[pick], np.asarray(y, np.float64)[pick]
    xt = ora.par_transform(xs, par_train).astype(np.float32) if par_train is not None else xs
    scale = 1.0 if tout is None else tout[0]
    yref = hr.forward(Ws, bs, act, xt, prec, tout=tout)
    med, p99, mx = hr.forward_stats(ys, yref, scale)
    tm, tp, tx = FWD16_TOL[prec]
    print("HALFREF forward %s %s rows=%d median %.2e p99 %.2e max %.2e" % (tag, prec, n, med, p99, mx))
    if seen is not None:
        seen.append((med, p99, mx))
    assert med <= tm and p99 <= tp and mx <= tx, (tag, prec, n, "vs rounding reference", med, p99, mx)
    y64 = hr.forward(Ws, bs, act, np.asarray(xt, np.float64), None, tout=tout)   # the plain float64 oracle, as before
    assert np.abs(ys - y64).max() / scale <= HALF_BOUNDS[prec]["max_abs"], (tag, prec, n, "vs float64")
    for name in hr.mutations_for(prec, "forward"):
        ym = hr.apply_forward_mutation(name, ys, Ws, bs, act, xt, prec, tout=tout, yref=yref)
        mm, pm, xm = hr.forward_stats(ym, yref, scale)
        assert not (mm <= tm and pm <= tp and xm <= tx), (tag, prec, n, "mutation not refused", name, mm, pm, xm)


def _rows(n, d, seed, par_train=None):
    if par_train is not None:
        return pkg("synth").make_params(n, seed=seed, dtype=np.float32)
    return np.random.default_rng(seed).uniform(-1, 1, size=(n, d)).astype(np.float32)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("arch", ["S1", "S2", "S3", "S4"])
def test_fused_forward_matches_rounding_reference(ctx, arch, prec):
    """fused_fwd<S1..S4> (D1, DE, the autoencoder-path stack S3, the decoder-path S4): 1 .. 4,097 rows (65,536 on D1), with
    and without the transforms (stacks of 7 inputs and 451 outputs)."""
    native = pkg("_native")
    dims, act = FUSED_STACKS[arch]
    Ws, bs = _weights(dims, act, seed=3)
    for tf in (False, True):
        if tf and not (dims[0] == 7 and dims[-1] == 451):
            continue
        st = native.Stack(ctx, dims, act)
        st.set_weights(ora.flatten_params(Ws, bs))
        flags, par_train, tout = _transforms(st, dims) if tf else (0, None, None)
        for n in ROWS:
            if n == 65536 and (arch != "S1" or tf):
                continue
            x = _rows(n, dims[0], n, par_train)
            y = st.forward(x, prec, flags=flags)
            assert st.last_route()[0] == "fused", (arch, st.last_route())
            _check((arch, tf), y, x, Ws, bs, act, prec, par_train, tout)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_custom_stack_routes_match_rounding_reference(ctx, prec):
    """The notebook's stack NB (no compiled kernel): the few-row route (1 .. 33 rows), the table-driven one-launch kernel
    (FWD_FORCE_CHAIN, 1 .. 65,536 rows) and the run-time instantiated fused kernel (4,097 and 65,536 rows); with and without
    the transforms."""
    native = pkg("_native")
    dims, act = STACKS["NB"]
    Ws, bs = _weights(dims, act, seed=4)
    for tf in (False, True):
        st = native.Stack(ctx, dims, act)
        st.set_weights(ora.flatten_params(Ws, bs))
        flags, par_train, tout = _transforms(st, dims) if tf else (0, None, None)
        for n in (1, 31, 33):
            x = _rows(n, dims[0], n, par_train)
            y = st.forward(x, prec, flags=flags)
            assert st.last_route()[0] == "small", st.last_route()
            _check(("NB small", tf), y, x, Ws, bs, act, prec, par_train, tout)
        for n in (1, 31, 33, 4097, 65536):
            x = _rows(n, dims[0], n + 1, par_train)
            y = st.forward(x, prec, flags=flags | native.FWD_FORCE_CHAIN)
            assert st.last_route()[0] == "table", st.last_route()
            _check(("NB table", tf), y, x, Ws, bs, act, prec, par_train, tout)
        assert st.jit(prec) == "ready"
        for n in (4097, 65536):
            x = _rows(n, dims[0], n + 2, par_train)
            y = st.forward(x, prec, flags=flags)
            assert st.last_route()[0] == "fused_rt", st.last_route()
            _check(("NB fused_rt", tf), y, x, Ws, bs, act, prec, par_train, tout)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_generic_route_matches_rounding_reference(ctx, prec):
    """W6 (600 wide: beyond the one-launch kernels and the few-row route): the per-layer K-loop GEMM at every row count,
    with and without the transforms.  Forced by its flag: the default route of a W6 call above 4,096 rows asks for a
    run-time kernel, and test_routes.py's W6 rows expect none in this session."""
    native = pkg("_native")
    dims, act = STACKS["W6"]
    Ws, bs = _weights(dims, act, seed=5)
    for tf in (False, True):
        st = native.Stack(ctx, dims, act)
        st.set_weights(ora.flatten_params(Ws, bs))
        flags, par_train, tout = _transforms(st, dims) if tf else (0, None, None)
        for n in (1, 31, 33, 4097, 65536):
            x = _rows(n, dims[0], n + 3, par_train)
            y = st.forward(x, prec, flags=flags | native.FWD_FORCE_GENERIC)   # (the default route is the same, but a call of
            assert st.last_route()[0] == "generic", st.last_route()               # > 4,096 rows asks for a run-time kernel)
            _check(("W6 generic", tf), y, x, Ws, bs, act, prec, par_train, tout)
