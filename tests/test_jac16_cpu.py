"""The rounding reference of the fused 16-bit Jacobian (half_ref.jvp, jacobian_ref.jacobian16) on the CPU: with the rounding
switched off it IS jacobian_ref.jvp; its primal is half_ref.forward and its ReLU decisions are masks16; the worst-cell
median (half_ref.jac_worst_cell_median) accepts the DEVICE MODEL (the same pass with f32 accumulation) and every entry of
the tangent catalogue (half_ref.JAC_MUTATIONS) the Jacobian check answers for moves it to at least 16x the model's; and a
tangent on a 16-bit rounding midpoint goes to the even neighbour.

Measured here (256 rows, worst-cell median; f16 / bf16): the device model D1 2.0e-7 / 6.5e-8, S3 2.3e-7 / 7.8e-8, S4
2.3e-7 / 8.0e-8; tan_rtz >= 5.6e-4 / 4.8e-3, tan_tile >= 9.9e-4 / 1.1e-3, fac16 2.9e-4 / 2.5e-3, out_tile 3.9e-3 / 3.9e-3.
prim_unrounded leaves the f16 median where it was (1.0 .. 1.1x the model on D1, S3, S4) and bf16's on S4 (1.4x), while
it moves y by 6e-6 .. 1.6e-5 (f16) / 5e-5 .. 1.3e-4 (bf16) of its scale -- it is the primal checks' to refuse (half_ref.JAC_CHECK_SKIPS)."""
import numpy as np
import pytest

import half_ref as hr
import jacobian_ref as jr
from conftest import pkg
from helpers import FWD16_TOL, JAC16_TOL, STACKS, init_weights
from infer_cases import ARCHS, VG, transforms, vg_weights

_cache = {}


def case(name, n=256, seed=10):
    """(dims, act, Ws, bs, x float64, tin or None, tout) -- weights and transforms as test_jacobian_gpu.stack_of makes them"""
    if (name, n, seed) not in _cache:
        if name == "VG":
            (dims, act), (Ws, bs) = VG, vg_weights(3)
        elif name == "RE":   # a stack ending in a ReLU
            dims, act = [7, 64, 128, 451], [1, 1, 1]
            Ws, bs, _ = init_weights(dims, 4)
        else:
            dims, act = ARCHS[name] if name in ARCHS else STACKS[name]
            Ws, bs, _ = init_weights(dims, 3)
        tin, tout, _ = transforms(5)
        if dims[0] == 7:
            x = pkg("synth").make_params(max(n, 8), seed=seed)[:n].astype(np.float64)
        else:
            x, tin = np.random.default_rng(seed).uniform(-1, 1, size=(n, dims[0])), None
        _cache[(name, n, seed)] = (dims, act, Ws, bs, x, tin, tout)
    return _cache[(name, n, seed)]


@pytest.mark.parametrize("name", ["D1", "S3", "S4", "VG", "RE"])
def test_rounding_off_is_jacobian_ref_jvp_bit_for_bit(name):
    dims, act, Ws, bs, x, tin, tout = case(name, 40)
    xt = jr.transform(x, *tin)[0] if tin is not None else x
    want = jr.jvp(Ws, bs, act, xt)
    got = hr.jvp(Ws, bs, act, xt, None)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))
    # masks= and flips= as jacobian_ref.jvp takes them
    masks = jr.masks16(Ws, bs, act, xt.astype(np.float32), "bf16")
    flips = [None if m is None else (np.arange(m.size).reshape(m.shape) % 97 == 0) for m in masks]
    for kw in (dict(masks=masks), dict(flips=flips), dict(masks=masks, flips=flips)):
        want = jr.jvp(Ws, bs, act, xt, **kw)
        got = hr.jvp(Ws, bs, act, xt, None, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), sorted(kw)
    assert not np.array_equal(hr.jvp(Ws, bs, act, xt, None, flips=flips)[1], hr.jvp(Ws, bs, act, xt, None)[1])


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "S3", "S4"])
def test_primal_is_half_ref_forward_and_masks_are_masks16(name, prec):
    dims, act, Ws, bs, x, tin, tout = case(name, 40)
    xt, fac, std = jr.operands16(x, tin, tout)
    for acc in ("f64", "f32"):
        y, J, zs = hr.jvp(Ws, bs, act, xt, prec, acc=acc)
        assert np.array_equal(y, hr.forward(Ws, bs, act, xt, prec, acc=acc)), acc
    masks = hr.masks16(Ws, bs, act, xt, prec)
    zs = hr.jvp(Ws, bs, act, xt, prec)[2]
    assert all((m is None and a != hr.RELU) or np.array_equal(m, z > 0) for m, z, a in zip(masks, zs, act))
    y16, J16 = jr.jacobian16(Ws, bs, act, x, prec, tin, tout)
    assert np.array_equal(y16, hr.forward(Ws, bs, act, xt, prec, tout=tout))
    # J is the tangent pass times the float32 std and factor the kernel holds, in that order
    want = hr.jvp(Ws, bs, act, xt, prec)[1] * std
    if tin is not None:
        want = want * fac[:, :, None]
        assert fac.dtype == np.float64 and np.array_equal(fac, fac.astype(np.float32)) and not np.all(fac == 1)
    assert np.array_equal(J16, want) and std == float(np.float32(tout[0]))
    # the masked tangents: a unit the primal switches off passes nothing
    _, T, zs = hr.jvp(Ws, bs, act[:1], xt, prec)
    assert np.all(T[np.broadcast_to((zs[0] <= 0)[:, None, :], T.shape)] == 0)


def test_float32_rows_take_the_float32_transform():
    """par_transform_f32 (csrc/par_transform.h): the log10 of a float32 row is rounded to float32 before the affine map"""
    dims, act, Ws, bs, x, tin, tout = case("D1", 40)
    x32 = x.astype(np.float32)
    xt = jr.operands16(x32, tin, tout)[0]
    lm = np.asarray(tin[0], bool)
    t = x32.astype(np.float64)
    for j, zf in enumerate(tin[1]):
        if zf > 0:
            t[x32[:, j] == 0, j] = float(np.float32(zf))
    q = np.where(lm, np.log10(np.where(lm, t, 1.0)).astype(np.float32).astype(np.float64), t)
    lo, hi = np.asarray(tin[2], np.float64), np.asarray(tin[3], np.float64)
    assert np.array_equal(xt, (((q - lo) / (hi - lo)) * 2 - 1).astype(np.float32)) and lm.any()
    assert np.array_equal(jr.operands16(x, tin, tout)[0], jr.transform(x, *tin)[0].astype(np.float32))


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "S3", "S4"])
def test_median_check_accepts_the_device_model_and_every_mutation_is_16x_beyond_it(name, prec):
    dims, act, Ws, bs, x, tin, tout = case(name)
    y16, J16 = jr.jacobian16(Ws, bs, act, x, prec, tin, tout)
    yd, Jd = jr.jacobian16(Ws, bs, act, x, prec, tin, tout, acc="f32")
    base = hr.jac_worst_cell_median(Jd, J16)
    print("JAC16 model %s %s worst-cell median %.2e" % (name, prec, base))
    assert 0 < base <= JAC16_TOL[prec], (name, prec, base)
    muts = hr.jac_mutations(prec, tin is not None, act)
    assert set(muts) == set(hr.JAC_MUTATIONS) - {"prim_unrounded"} - (set() if tin is not None else {"fac16"})
    xt, fac, std = jr.operands16(x, tin, tout)
    for mut in muts:
        _, Jm = jr.jacobian16(Ws, bs, act, x, prec, tin, tout, acc="f32", mut=mut)
        v = hr.jac_worst_cell_median(Jm, J16)
        print("JAC16 model %s %s %s worst-cell median %.2e (%.0fx)" % (name, prec, mut, v, v / base))
        assert v >= 16 * base, (name, prec, mut, v, base)
        assert v >= 4 * JAC16_TOL[prec], (name, prec, mut, v)   # ... and the bound is at most 1/4 of it
        # the same entry applied on the host to a device result (what the GPU tests do)
        Ja = hr.apply_jac_mutation(mut, Jd, Ws, bs, act, xt, prec, fac=fac if tin is not None else None, std=std, Jref=J16)
        va = hr.jac_worst_cell_median(Ja, J16)
        assert va >= 16 * base and va >= 4 * JAC16_TOL[prec], (name, prec, mut, va)
    # tan_tile and out_tile touch one input's tangent in 16 units / 32 bins: the median over the whole matrix is blind
    for mut in ("tan_tile", "out_tile"):
        _, Jm = jr.jacobian16(Ws, bs, act, x, prec, tin, tout, acc="f32", mut=mut)
        assert np.median(hr.jac_cell_errors(Jm, J16)) <= 1.1 * np.median(hr.jac_cell_errors(Jd, J16)), mut
    # prim_unrounded: refused by the primal's checks (y moves far beyond the forward's median bound), not by this one
    ym, Jm = jr.jacobian16(Ws, bs, act, x, prec, tin, tout, acc="f32", mut="prim_unrounded")
    scale = float(tout[0])
    med_y = hr.forward_stats(ym, y16, scale)[0]
    print("JAC16 model %s %s prim_unrounded: y median %.2e, J worst-cell median %.2e" % (name, prec, med_y, hr.jac_worst_cell_median(Jm, J16)))
    assert med_y > 16 * FWD16_TOL[prec][0], (name, prec, med_y)
    assert hr.forward_stats(yd, y16, scale)[0] <= FWD16_TOL[prec][0]
    if prec == "f16" or name == "S4":
        assert hr.jac_worst_cell_median(Jm, J16) < 16 * base, (name, prec)


def test_pooled_median_below_31_rows():
    dims, act, Ws, bs, x, tin, tout = case("D1", 40)
    _, J16 = jr.jacobian16(Ws, bs, act, x, "f16", tin, tout)
    Jm = J16.copy()
    Jm[:16] *= 1 + 2.0 ** -8            # 16 rows wrong
    e = hr.jac_cell_errors(Jm, J16)
    assert e.shape == (40, 7, 15)       # 451 bins: 14 whole tiles and one of 3 bins
    assert hr.jac_worst_cell_median(Jm, J16) == 0.0                                # 16 of 40: under half of every cell
    assert abs(hr.jac_worst_cell_median(Jm[:30], J16[:30]) - 2.0 ** -8) < 1e-12    # 16 of 30, pooled
    Jn = J16.copy()
    Jn[:, 6, 448:] *= 1 + 2.0 ** -8     # the ragged last tile of one input
    assert abs(hr.jac_worst_cell_median(Jn, J16) - 2.0 ** -8) < 1e-12
    assert hr.jac_worst_cell_median(Jn[:30], J16[:30]) == 0.0                      # one cell of 105: the pooled median is blind
    Jn[3, 2, 5] = np.nan
    assert np.isinf(hr.jac_cell_errors(Jn, J16)[3, 2, 0])


@pytest.mark.parametrize("prec,u", [("f16", 2.0 ** -10), ("bf16", 2.0 ** -7)])
def test_a_tangent_on_a_rounding_midpoint_goes_to_even(prec, u):
    """1 -> 3 -> 2 -> 2, every unit on: the second hidden layer's tangents are 1 + u/2 (half way between 1 and 1 + u: to
    the even 1) and 1 + 3u/2 (half way between 1 + u and 1 + 2u: to the even 1 + 2u); rounded toward zero, 1 and 1 + u"""
    act = [1, 1, 0]
    Ws = [np.array([[1.0, u / 2, 3 * u / 2]]), np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]), np.eye(2)]
    bs = [np.ones(3), np.ones(2), np.zeros(2)]
    assert all(np.array_equal(hr.round16(W, prec), W) for W in Ws)   # the weights are 16-bit values
    assert hr.jac_mutation_site(act) == 1
    x = np.array([[1.0]])
    for acc in ("f64", "f32"):
        y, J, zs = hr.jvp(Ws, bs, act, x, prec, acc=acc)
        assert J.shape == (1, 1, 2) and J[0, 0].tolist() == [1.0, 1 + 2 * u], (acc, J)
        assert hr.jvp(Ws, bs, act, x, prec, acc=acc, mut="tan_rtz")[1][0, 0].tolist() == [1.0, 1 + u]
    assert hr.jvp(Ws, bs, act, x, None)[1][0, 0].tolist() == [1 + u / 2, 1 + 3 * u / 2]
    assert np.array_equal(y, hr.forward(Ws, bs, act, x, prec))
    # a unit the primal switches off passes no tangent, rounded or not
    bs_off = [np.ones(3), np.array([1.0, -9.0]), np.zeros(2)]
    assert hr.jvp(Ws, bs_off, act, x, prec)[1][0, 0].tolist() == [1.0, 0.0]
