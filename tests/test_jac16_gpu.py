"""fused_jac<Arch, f16 | bf16> against the float64 forward-mode reference that rounds where it rounds (half_ref.jvp through
jacobian_ref.jacobian16), and the likelihood reductions built on it against the same reference.

The bounds of tests/test_jacobian_gpu.py (p99 1e-2 / max 3e-2 in f16, 5e-2 / 1e-1 in bf16, against float64 tangents with
the 16-bit primal's ReLU decisions) have to cover the rounding of every tangent operand -- and so cover a kernel that
rounds a layer's tangents toward zero, scales a tile or rounds the chain-rule factor.  Against the rounding reference what
is left of a correct kernel is its f32 summation order, and in single rows the ReLU units that order decides the other
way: so the check bounds MEDIANS over rows, one per (input, 32-bin output tile) cell of J, and asserts the worst cell
(half_ref.jac_worst_cell_median; calls of fewer than 31 rows pool their cells); the p99 / max conditions stay as they are
(infer_support.check_rows, called here).  Every entry of half_ref.JAC_MUTATIONS the check answers for, applied to the
device's own J, must be refused -- and lie at least 4x beyond the bound.

Bounds (helpers.JAC16_TOL, LNL16_TOL, FISHER16_TOL): at most 4x the worst measured on the MI355X over every case here, at
most 1/4 of the least any catalogue entry makes.  Measured worst (f16 / bf16):
    J, worst-cell median    S1 1.26e-7 / 7.07e-8   S2 1.46e-7 / 7.39e-8   S3 1.60e-7 / 8.56e-8   S4 1.86e-7 / 8.22e-8
    ln L, median            D1 4.76e-8 / 3.57e-8   S3 5.21e-8 / 4.38e-8   S4 3.67e-8 / 3.61e-8
    g, worst input's median D1 4.21e-8 / 2.96e-8   S3 3.20e-8 / 2.38e-8   S4 2.75e-8 / 2.74e-8
    F, median               D1 4.97e-8 / 3.12e-8   S3 5.77e-8 / 3.36e-8   S4 4.99e-8 / 4.38e-8
    marginalised (D1 f16, K = 5): ln L 1.42e-8, g 8.9e-9, F 5.85e-8
    catalogue on the device's J, least over the cases: tan_rtz 5.7e-4 / 5.0e-3, tan_tile 1.0e-3 / 1.0e-3, fac16 2.9e-4 /
    2.5e-3, out_tile 3.9e-3 / 3.9e-3; through the reductions tan_rtz and fac16 move g to >= 1.7e-5 / 1.3e-4, F to >= 2.7e-4
    / 2.0e-3
The module takes 6 s on the MI355X (15 tests, the slowest 0.6 s)."""
import numpy as np
import pytest

import fit_ref as fr
import half_ref as hr
import jacobian_ref as jr
from conftest import pkg
from helpers import FISHER16_TOL, JAC16_TOL, LNL16_TOL
from infer_support import basis, check_rows, flags_of, reference, rows_for, setup, stack_of

pytestmark = pytest.mark.gpu

# (rows, input transform, output transform, dtype of the rows): one, under-full and over-full 32-column tiles at 8
# virtual rows per signal (S4: 16), then several workgroups with a ragged last one.  Rows and dtypes of test_jacobian_gpu's
# cases of the same counts (seed 10 + k).
CASES = [(1, True, False, np.float64), (3, False, True, np.float64), (4, True, True, np.float32), (5, False, False, np.float32),
         (31, False, True, np.float64), (33, True, False, np.float64), (4099, True, True, np.float32)]
CMP_ROWS = 512       # rows compared of a larger call: the first, the last and a random sample
MUT_ROWS = 128       # rows of those the catalogue is applied to
MUTATED = (33, 4099)


def sample(n):
    return np.arange(n) if n <= CMP_ROWS else np.unique(np.r_[0, n - 1, np.random.default_rng(n).choice(n, CMP_ROWS - 2, replace=False)])


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "DE", "S3", "S4"])
def test_fused_jacobian_matches_rounding_reference(ctx, name, prec):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout = stack_of(ctx, name)
    worst = 0.0
    for k, (n, tin_on, tout_on, dtype) in enumerate(CASES):
        tin_on = tin_on and dims[0] == 7
        flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | (nat.FWD_OUT_TRANSFORM if tout_on else 0)
        x = rows_for(dims, n, 10 + k, dtype)
        if dims[0] == 7 and not tin_on:  # without the input transform: rows in the network's own domain [-1, 1]
            x = jr.transform(x, *tin)[0].astype(dtype)
        tag = "%s %s n=%d %s flags=%d" % (name, prec, n, dtype.__name__, flags)
        jac = st.jacobian(x, prec, flags)
        assert st.last_jac_route()[0] == "fused", tag
        assert jac.shape == (n, dims[0], dims[-1]), tag
        idx = sample(n)
        xs, got = x[idx], jac[idx]
        ti, to = (tin if tin_on else None), (tout if tout_on else None)
        _, J16 = jr.jacobian16(Ws, bs, act, xs, prec, ti, to)
        stat = hr.jac_worst_cell_median(got, J16)
        worst = max(worst, stat)
        print("JAC16 %s: worst-cell median %.3e (bound %.1e)" % (tag, stat, JAC16_TOL[prec]))
        assert stat <= JAC16_TOL[prec], (tag, stat)
        # the p99 and max conditions against the mask-only reference, as they are
        _, Jr = jr.jacobian(Ws, bs, act, xs, ti, to)
        xt = jr.transform(xs, *tin)[0] if tin_on else xs.astype(np.float64)
        check_rows(tag, prec, got, Jr, Ws, bs, act, xt, tin_on, xs, tin, to)
        if n in MUTATED:
            sub = np.arange(len(idx)) if len(idx) <= MUT_ROWS else np.unique(np.r_[0, len(idx) - 1, np.arange(0, len(idx), len(idx) // (MUT_ROWS - 2))])
            xt32, fac, std = jr.operands16(xs[sub], ti, to)
            base = hr.jac_worst_cell_median(got[sub], J16[sub])
            assert base <= JAC16_TOL[prec], (tag, base)
            muts = hr.jac_mutations(prec, tin_on, act)
            assert len(muts) == (4 if tin_on else 3), muts
            for mut in muts:
                Jm = hr.apply_jac_mutation(mut, got[sub], Ws, bs, act, xt32, prec, fac=fac if tin_on else None, std=std, Jref=J16[sub])
                v = hr.jac_worst_cell_median(Jm, J16[sub])
                print("JAC16 %s: %s worst-cell median %.3e" % (tag, mut, v))
                assert not v <= JAC16_TOL[prec], (tag, "mutation not refused", mut, v)
                assert v >= 4 * JAC16_TOL[prec], (tag, "the bound is more than 1/4 of what the mutation makes", mut, v)
    print("JAC16 worst %s %s: %.3e" % (name, prec, worst))


def _median(e, axis=None):
    """a median in which a value that is not finite counts as infinitely wrong"""
    return np.median(np.where(np.isfinite(e), e, np.inf), axis=axis)


def reduction_errors(lnl, g, F, lr, gr, Fr, gscale):
    """medians over rows of: |ln L - ref| / |ref|; |g_j - ref| over the sum of its terms' magnitudes (a sum with
    cancellation, as test_jacobian_gpu.test_loglike scales it), one median per input j and the worst input of them (the
    max over a row's inputs would be decided by the one tangent value per row that the summation order moves across a
    16-bit rounding midpoint); F's relative Frobenius error"""
    with np.errstate(invalid="ignore", over="ignore"):
        el = np.abs(np.asarray(lnl, np.float64) - lr) / np.abs(lr)
        eg = np.abs(np.asarray(g, np.float64) - gr) / gscale
        eF = jr.rel_frobenius(F, Fr)
    return float(_median(el)), float(_median(eg, axis=0).max()), float(_median(eF))


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "S3", "S4"])
def test_loglike_and_fisher_match_rounding_reference(ctx, name, prec):
    """Stack.loglike and Stack.fisher(lnl, grad) on 600 rows with band weights (zero on a fifth of the bins): ln L, g and F
    against the float64 reductions of the rounding reference's y and J; tan_rtz and fac16 applied to the device's J and
    pushed through the same float64 reductions must move g and F beyond the bounds"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout, data, w = setup(ctx, name)
    try:
        flags = flags_of(nat, dims[0] == 7)
        tin_on = dims[0] == 7
        ti = tin if tin_on else None
        x = rows_for(dims, 600, 77, np.float64)
        lnl, g = st.loglike(x, prec, flags)
        F, lnl_f, g_f = st.fisher(x, prec, flags, lnl=True, grad=True)
        assert st.last_jac_route()[0] == "fused"
        y16, J16 = jr.jacobian16(Ws, bs, act, x, prec, ti, tout)
        w64, d64 = w.astype(np.float64), data.astype(np.float64)
        lr, gr = jr.loglike(y16, J16, d64, w64)
        Fr = fr.fisher_ref(J16, w64)
        gscale = np.einsum("nk,njk->nj", np.abs(w64 * (d64 - y16)), np.abs(J16))
        tl, tg, tF = LNL16_TOL[prec]["lnl"], LNL16_TOL[prec]["grad"], FISHER16_TOL[prec]
        for what, (l_, g_) in (("loglike", (lnl, g)), ("fisher", (lnl_f, g_f))):
            el, eg, eF = reduction_errors(l_, g_, F, lr, gr, Fr, gscale)
            print("LNL16 %s %s %s: lnl %.3e (bound %.1e) grad %.3e (%.1e) F %.3e (%.1e)" % (name, prec, what, el, tl, eg, tg, eF, tF))
            assert el <= tl and eg <= tg and eF <= tF, (name, prec, what, el, eg, eF)
        # the catalogue: the device's own y and J, the mistake added, reduced in float64
        y, jac = st.jacobian(x, prec, flags, return_outputs=True)
        xt32, fac, std = jr.operands16(x, ti, tout)
        for mut in ("tan_rtz",) + (("fac16",) if tin_on else ()):
            Jm = hr.apply_jac_mutation(mut, jac, Ws, bs, act, xt32, prec, fac=fac if tin_on else None, std=std, Jref=J16)
            lm, gm = jr.loglike(y, Jm, d64, w64)
            el, eg, eF = reduction_errors(lm, gm, fr.fisher_ref(Jm, w64), lr, gr, Fr, gscale)
            print("LNL16 %s %s %s: grad %.3e F %.3e" % (name, prec, mut, eg, eF))
            assert not eg <= tg and not eF <= tF, (name, prec, "mutation not refused", mut, eg, eF)
            assert eg >= 4 * tg and eF >= 4 * tF, (name, prec, "a bound is more than 1/4 of what the mutation makes", mut, eg, eF)
    finally:
        st.set_likelihood(None, None)


def test_marginalised_reductions_match_rounding_reference(ctx):
    """jac_reduce_kernel with nuisance modes (the sampler's reduction, 4x the plain one) on D1 in f16 with K = 5 foreground modes, 64 rows: F,
    ln L and g against marg_ref fed the rounding reference's y and J, medians over rows (g: per input, the worst input).
    Every error is relative to the sum of the magnitudes of the terms the kernel sums, as tests/test_marg_gpu.py scales
    them: the kernel works on the PROJECTED data d~ = d - Q^T (Q W d) (nuis_project_kernel), so ln L_m = -1/2 (r~ W r~ -
    |b~|^2) is a difference of two float32 sums that are each ~150x ln L_m with these data (r~ carries the smooth part
    of y that the raw residual does not), and F_m = F0 - B^T B is scaled by F0 = J W J^T."""
    nat = pkg("_native")
    prec = "f16"
    st, dims, act, Ws, bs, tin, tout, data, w = setup(ctx, "D1")
    try:
        flags = flags_of(nat, dims[0] == 7)
        A = basis(5)
        st.set_nuisance(A)
        assert st.nuisance_modes() == 5
        x = rows_for(dims, 64, 78, np.float64)
        F, lnl, g = st.fisher(x, prec, flags, lnl=True, grad=True)
        assert st.last_jac_route()[0] == "fused"
        l_ll, g_ll = st.loglike(x, prec, flags)
        y16, J16 = jr.jacobian16(Ws, bs, act, x, prec, tin, tout)
        ref, lnl_scale, grad_scale, _ = reference(y16, J16, data, w, A)
        eF = _median(np.sqrt(np.sum((F - ref["F"]) ** 2, axis=(1, 2))) / np.sqrt(np.sum(ref["F0"] ** 2, axis=(1, 2))))
        for what, (l_, g_) in (("fisher", (lnl, g)), ("loglike", (l_ll, g_ll))):
            el = _median(np.abs(l_ - ref["lnl"]) / lnl_scale)
            eg = _median(np.abs(g_ - ref["grad"]) / grad_scale, axis=0).max()
            print("LNL16 marginalised D1 f16 %s: lnl %.3e grad %.3e F %.3e" % (what, el, eg, eF))
            assert el <= LNL16_TOL[prec]["lnl"] and eg <= LNL16_TOL[prec]["grad"], (what, el, eg)
        assert eF <= FISHER16_TOL[prec], eF
    finally:
        st.set_nuisance(None)
        st.set_likelihood(None, None)
