"""The rounding reference (tests/half_ref.py) on the CPU: with the rounding switched off it IS the float64 oracle; round16
is numpy's float16 / torch's bfloat16; and its checks accept the DEVICE MODEL (the same computation with f32 accumulation)
and refuse every entry of the mutation catalogue applied to it."""
import numpy as np
import pytest

import half_ref as hr
import jacobian_ref as jr
from helpers import FWD16_TOL, HALF_STEP_TOL, STACKS, half_step_check, init_weights, oracle_step, stack_data


def test_rounding_off_is_the_float64_oracle():
    for name in ("D1", "AE", "NB"):
        dims, act = STACKS[name]
        x, y, w = stack_data(dims, 200, 5)
        tgt = x if y is None else y
        Ws, bs, _ = init_weights(dims, 3)
        lo, go = oracle_step(Ws, bs, act, x, tgt, w)
        l, g = hr.step(Ws, bs, act, x, tgt, w, None)
        assert abs(l - lo) <= 1e-12 * abs(lo)
        assert np.abs(g - go).max() <= 1e-12 * np.abs(go).max()
        y0 = jr.forward(Ws, bs, act, x)
        assert np.abs(hr.forward(Ws, bs, act, x, None) - y0).max() <= 1e-12 * np.abs(y0).max()
    # a variational head's forward (z = z_mean) as jacobian_ref has it
    dims, act = [451, 96, 9, 32, 451], [1, 2, 1, 0]
    rng = np.random.default_rng(1)
    Ws = [rng.uniform(-0.1, 0.1, size=(k, 2 * n if a == 2 else n)).astype(np.float32) for k, n, a in zip(dims[:-1], dims[1:], act)]
    bs = [rng.normal(scale=0.05, size=W.shape[1]).astype(np.float32) for W in Ws]
    x = rng.normal(size=(50, 451)).astype(np.float32)
    assert np.abs(hr.forward(Ws, bs, act, x, None) - jr.forward(Ws, bs, act, x)).max() <= 1e-12


def test_round16_f16_is_numpy_float16():
    rng = np.random.default_rng(0)
    mx = float(np.finfo(np.float16).max)
    tiny = 2.0 ** -24                         # the smallest subnormal
    ulp1 = 2.0 ** -10
    a = np.r_[rng.normal(size=2000) * 10.0 ** rng.uniform(-9, 5, size=2000),
              1 + ulp1 / 2, 1 + 3 * ulp1 / 2, -(1 + ulp1 / 2),     # ties: to even
              tiny / 2, 3 * tiny / 2, tiny * 0.49, -tiny / 2,       # subnormal ties and underflow (to +-0)
              mx, mx + 2.0 ** 4, mx + 2.0 ** 4 + 1e-3, 1e6, -1e6,   # the largest value, the tie above it, overflow
              0.0, -0.0, np.inf, -np.inf]
    r = hr.round16(a, "f16")
    with np.errstate(over="ignore"):
        want = a.astype(np.float16).astype(np.float64)
    assert np.array_equal(r, want) and np.array_equal(np.signbit(r), np.signbit(want))
    assert r[2007] == mx and r[2008] == np.inf and r[2009] == np.inf and r[2011] == -np.inf   # the tie above max -> inf
    assert r[2000] == 1.0 and r[2001] == 1 + 2 * ulp1 and r[2002] == -1.0
    assert r[2003] == 0.0 and r[2004] == 2 * tiny and r[2006] == 0.0 and np.signbit(r[2006]) and np.signbit(r[2013])


def test_round16_bf16_is_torch_bfloat16():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1)
    ulp1 = 2.0 ** -7
    tiny = float(np.finfo(np.float32).smallest_subnormal)
    mx = float(torch.finfo(torch.bfloat16).max)
    a = np.r_[rng.normal(size=2000) * 10.0 ** rng.uniform(-30, 30, size=2000),
              1 + ulp1 / 2, 1 + 3 * ulp1 / 2, -(1 + ulp1 / 2),
              1e-39, -1e-39, 2.0 ** -133 * 3, tiny,                 # f32 subnormals (bf16 keeps them)
              mx, 3.3e38, -3.4e38, 0.0, -0.0, np.inf, -np.inf]
    a32 = a.astype(np.float32)
    want = torch.from_numpy(a32).to(torch.bfloat16).to(torch.float64).numpy()
    r = hr.round16(a32, "bf16")
    assert np.array_equal(r, want) and np.array_equal(np.signbit(r), np.signbit(want))
    assert r[2000] == 1.0 and r[2001] == 1 + 2 * ulp1 and r[2007] == mx and r[2009] == -np.inf and np.signbit(r[2011])


def test_grad_opscale_is_the_nearest_power_of_two_clamped():
    """api_trainer.hip:393 in exact integer arithmetic, without logarithms: 2^e with e the integer nearest log2(s),
    s = brows dout / 16, i.e. 2^(2e - 1) <= s^2 < 2^(2e + 1) (lround's halves, log2 s = e + 1/2, would need s^2 = 2^(2e+1)
    exactly, which an integer ratio squared is not unless s is a power of two times sqrt(2) -- so the half-up rule shows at
    the boundary s^2 = 2^(2e+1) - epsilon on either side); clamped to 2^0 .. 2^24."""
    def exact(brows, dout):
        p2 = (brows * dout) ** 2          # s^2 = p2 / 256
        e = 0
        while 256 * 2 ** (2 * e + 1) <= p2:  # s^2 >= 2^(2e + 1): the nearest power is above 2^e
            e += 1
        return 2.0 ** min(24, e)
    rng = np.random.default_rng(3)
    cases = [(b, d) for b in (1, 2, 15, 16, 22, 23, 45, 46, 181, 182, 256, 4096, 8193, 16389, 32768, 1 << 20)
             for d in (1, 3, 9, 17, 33, 451)]
    cases += [(int(b), int(d)) for b, d in zip(rng.integers(1, 70000, 400), rng.integers(1, 600, 400))]
    # the rounding boundary itself: s just below and just above 2^(e + 1/2) (22.627 = 2^4.5; 45.25 = 2^5.5)
    cases += [(362, 1), (363, 1), (724, 1), (725, 1)]
    for b, d in cases:
        assert hr.grad_opscale(b, d) == exact(b, d), (b, d, hr.grad_opscale(b, d), exact(b, d))
    assert hr.grad_opscale(362, 1) == 16.0 and hr.grad_opscale(363, 1) == 32.0    # 22.625 -> 2^4, 22.6875 -> 2^5


def _masks16_before(Ws, bs, act, xt, prec):
    """jacobian_ref.masks16 as it was before it became a call into half_ref (its own rounding: numpy float16 and a bf16
    bit trick), for the pinned comparison below"""
    def r16(a):
        a = np.asarray(a, np.float64)
        if prec == "f16":
            return a.astype(np.float16).astype(np.float64)
        u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32).astype(np.float64)
    h = r16(xt)
    out = []
    for W, b, a in zip(Ws, bs, act):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        z = h @ r16(W) + b
        out.append(z > 0 if a == 1 else None)
        h = r16(np.maximum(z, 0) if a == 1 else z)
    return out


def test_masks16_keeps_its_decisions():
    dims, act = STACKS["D1"]
    Ws, bs, _ = init_weights(dims, 3)
    x = np.random.default_rng(2).uniform(-1, 1, size=(300, 7)).astype(np.float32)
    for prec in ("f16", "bf16"):
        want = _masks16_before(Ws, bs, act, x, prec)
        got = jr.masks16(Ws, bs, act, x, prec)
        assert all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(got, want)), prec
    # and a hand-made case: z = 1 + 2^-12 - 1 rounds its operand 1 + 2^-12 to 1 in f16 (z = 0: off), not in bf16 either;
    # z = 2^-11 + 2^-11 x ... -- one row, one unit: x = [1 + 2^-12, -1], W = [[1], [1]], b = 0
    Wm, bm, am = [np.array([[1.0], [1.0]], np.float32)], [np.zeros(1, np.float32)], [1]
    xm = np.array([[1 + 2.0 ** -12, -1.0], [1 + 2.0 ** -9, -1.0]], np.float32)
    for prec, want in (("f16", [False, True]), ("bf16", [False, False])):
        assert jr.masks16(Wm, bm, am, xm, prec)[0][:, 0].tolist() == want, prec
    assert _masks16_before(Wm, bm, am, xm, "f16")[0][:, 0].tolist() == [False, True]


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name,rows", [("D1", 4096), ("AE", 4096), ("D1", 33), ("NB", 31)])
def test_step_checks_accept_the_device_model_and_refuse_every_mutation(name, rows, prec):
    """The device model (f32 accumulation) passes half_step_check under HALF_STEP_TOL for both ReLU models; each catalogue
    entry the step check answers for (half_ref.step_mutations), applied to the device model, is refused."""
    dims, act = STACKS[name]
    x, y, w = stack_data(dims, rows, 5)
    tgt = x if y is None else y
    Ws, bs, _ = init_weights(dims, 3)
    for model in ("sum", "rounded"):
        ref = hr.step(Ws, bs, act, x, tgt, w, prec, mask=model)
        ld, gd = hr.step(Ws, bs, act, x, tgt, w, prec, mask=model, acc="f32")
        ok, note, _ = half_step_check(dims, act, Ws, bs, x, tgt, w, ld, gd, prec, model, ref=ref, mutate=False)
        assert ok, (name, rows, prec, model, note)
        for mut in hr.step_mutations(prec, rows, dims[-1], act):
            lm, gm = hr.step(Ws, bs, act, x, tgt, w, prec, mask=model, acc="f32", mut=mut)
            ok, note, e = half_step_check(dims, act, Ws, bs, x, tgt, w, lm, gm, prec, model, ref=ref, mutate=False)
            assert not ok, (name, rows, prec, model, mut, "not refused", note)
        # ... and the same catalogue applied to a device result on the host (what the GPU tests do) is refused too
        ok, note, _ = half_step_check(dims, act, Ws, bs, x, tgt, w, ld, gd, prec, model, ref=ref, mutate=True)
        assert ok and "every mutation refused" in note, note


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_forward_checks_accept_the_device_model_and_refuse_every_mutation(prec):
    dims, act = STACKS["D1"]
    Ws, bs, _ = init_weights(dims, 3)
    x = np.random.default_rng(7).uniform(-1, 1, size=(8192, 7)).astype(np.float32)
    tm, tp, tx = FWD16_TOL[prec]
    yref = hr.forward(Ws, bs, act, x, prec)
    med, p99, mx = hr.forward_stats(hr.forward(Ws, bs, act, x, prec, acc="f32"), yref)
    assert med <= tm and p99 <= tp and mx <= tx, (med, p99, mx)
    for mut in hr.mutations_for(prec, "forward"):
        mm, pm, xm = hr.forward_stats(hr.forward(Ws, bs, act, x, prec, acc="f32", mut=mut), yref)
        assert not (mm <= tm and pm <= tp and xm <= tx), (mut, mm, pm, xm)
        assert mm > 100 * med, (mut, mm, med)


def test_the_catalogue_is_complete():
    assert set(hr.mutations_for("f16", "forward")) == {"hidden_rtz", "bias16"}     # the forward check's entries
    assert set(hr.step_mutations("f16", 4096, 451)) == set(hr.MUTATIONS) - {"bias16"}
    assert set(hr.step_mutations("f16", 256, 451)) == set(hr.MUTATIONS) - {"bias16", "dz_nogs"}
    assert "hidden_rtz" not in hr.step_mutations("f16", 70, 451, [0])          # one linear layer: no hidden activations
    assert set(hr.mutations_for("f16")) == set(hr.MUTATIONS)
    assert set(hr.mutations_for("bf16")) == set(hr.MUTATIONS) - {"dz_nogs"}
    assert set(HALF_STEP_TOL) == {"f16", "bf16"}


def test_slices_with_the_global_row_count_sum_to_the_whole_step():
    """brows (a data-parallel rank's slice: loss scale 2 / brows and gs of brows): two slices stepped with the global row
    count sum to the whole step -- every row's contribution is the same rounded value -- and a slice stepped with its own
    row count is a different step"""
    dims, act = STACKS["AE"]
    x, _, w = stack_data(dims, 200, 5)
    Ws, bs, _ = init_weights(dims, 3)
    for prec in ("f16", "bf16"):
        l, g = hr.step(Ws, bs, act, x, x, w, prec)
        la, ga = hr.step(Ws, bs, act, x[:77], x[:77], w[:77], prec, brows=200)
        lb, gb = hr.step(Ws, bs, act, x[77:], x[77:], w[77:], prec, brows=200)
        assert abs(la + lb - l) <= 1e-12 * l
        assert np.abs(ga + gb - g).max() <= 1e-12 * np.abs(g).max()
        lo, go = hr.step(Ws, bs, act, x[:77], x[:77], w[:77], prec)
        assert abs(lo * 77 / 200 - la) <= 1e-12 * la
        assert hr.grad_opscale(77, 451) != hr.grad_opscale(200, 451) and not np.allclose(go * 77 / 200, ga, rtol=0, atol=0)
