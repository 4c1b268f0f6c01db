"""GPU: the smooth activations (include/v21.h: V21_ACT_TANH .. V21_ACT_SOFTPLUS) on every route that takes them, against
the float64 reference of tests/act_ref.py.  The stacks are the smallest at which these kernels can go wrong (act_ref.T1 /
T2: hidden widths 40 and 72 -- partial tiles and non-zero padding --, 37 outputs in two tiles, 5 inputs; two units per
hidden layer at biases +-90), the bounds the project's own (helpers.TOL, infer_cases.HALF_BOUNDS); tests/test_act_cpu.py
shows on the CPU that float32 arithmetic alone stays a factor 4 inside the per-layer bound at exactly these shapes and seeds."""
import numpy as np
import pytest

import act_ref as ar
from conftest import pkg
from helpers import TOL
from infer_cases import HALF_BOUNDS
from oracle import ref_numpy as ora
from train_support import new_trainer

pytestmark = pytest.mark.gpu

TOL_LAYER = 2e-6   # f32 per layer relative L2 (helpers.per_layer_gradient_check)
PRECS = ["f32", "f16", "bf16"]


def _stack(ctx, name, seed=None):
    native = pkg("_native")
    dims, codes = getattr(ar, name) if isinstance(name, str) else name
    Ws, bs, flat = ar.stack_weights(dims, ar.SEEDS[name] if seed is None else seed)
    st = native.Stack(ctx, dims, codes)
    st.set_weights(flat)
    return st, dims, codes, Ws, bs, flat


def _check_forward(y, ref, prec, what):
    assert np.isfinite(y).all(), what
    if prec == "f32":
        np.testing.assert_allclose(y, ref, atol=2e-5, rtol=1e-5, err_msg=str(what))
    else:
        d, bound = np.abs(y - ref).max(), HALF_BOUNDS[prec]["max_abs"] * max(1.0, float(np.abs(ref).max()))
        assert d <= bound, (what, d, bound)


# ---- 1. forward on every route
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["T1", "T2"])
def test_forward_routes_against_float64(ctx, name, prec):
    native = pkg("_native")
    st, dims, codes, Ws, bs, _ = _stack(ctx, name)
    x = np.random.default_rng(7).uniform(-1, 1, size=(300, dims[0])).astype(np.float32)
    ref = ar.forward(Ws, bs, codes, x)
    assert np.isfinite(ref).all()
    ys = st.forward(x[:1], prec)                                   # the default below 4,097 rows: one NT launch per layer
    assert st.last_route()[0] == "small"
    _check_forward(ys, ref[:1], prec, (name, prec, "small", 1))
    gen = {}
    for n in (1, 127, 129, 300):                                   # the 128-row workgroup edge, a partial last workgroup
        gen[n] = st.forward(x[:n], prec, native.FWD_FORCE_GENERIC)
        assert st.last_route()[0] == "generic"
        _check_forward(gen[n], ref[:n], prec, (name, prec, "generic", n))
        ys = st.forward(x[:n], prec)
        assert st.last_route()[0] == "small"
        _check_forward(ys, ref[:n], prec, (name, prec, "small", n))
    # the chain kernels know ReLU and linear only: forcing them must not return a linear-layer result
    yc = st.forward(x, prec, native.FWD_FORCE_CHAIN)
    assert st.last_route()[0] == "generic" and np.array_equal(yc, gen[300])
    assert st.jit(prec) == "ready"
    for n in (1, 127, 129, 300):
        yj = st.forward(x[:n], prec, native.FWD_FORCE_JIT)
        assert st.last_route()[0] == "fused_rt"
        _check_forward(yj, ref[:n], prec, (name, prec, "fused_rt", n))
        yd = st.forward(x[:n], prec, native.FWD_NO_SMALL)          # the default above the few-row route, once the kernel is there
        assert st.last_route()[0] == "fused_rt" and np.array_equal(yd, yj), (name, prec, n)


# ---- 2. the class surface
def test_direct_emulator_predict_with_tanh(ctx):
    emulator, synth, eng = pkg("emulator"), pkg("synth"), pkg("engine")
    data = synth.make_dataset(n_train=600, n_val=40, n_test=300, seed=ar.SEEDS["T3"])
    eng.set_random_seed(ar.SEEDS["T3"])
    em = emulator.DirectEmulator(hidden_dims=[64, 128], activation_func="tanh", **data)
    ls = em.emulator.layers
    assert [l._act_code for l in ls] == ar.T3[1] and [ls[0].input_dim] + [l.units for l in ls] == ar.T3[0]
    Ws, bs = [l.kernel for l in ls], [l.bias for l in ls]
    xt = ora.par_transform(em.par_test, em.par_train).astype(np.float32)
    ref = ora.unpreproc(ar.forward(Ws, bs, ar.T3[1], xt).astype(np.float32), em.signal_train)
    pred = em.predict(em.par_test)
    assert pred.shape == (300, 451) and pred.dtype == np.float32
    # (the bounds of tests/test_emulator_gpu.py::test_direct_emulator_predict_contract)
    np.testing.assert_allclose(pred, ref, atol=2e-5 * float(np.std(em.signal_train)) + 1e-4, rtol=1e-5)
    assert np.allclose(em.predict(em.par_test[0]), pred[0], atol=5e-5)


# ---- 3. one training step on the per-layer route
def _step(ctx, dims, codes, flat, prec, x, y, w, rows, env=None):
    st, tr = new_trainer(ctx, dims, codes, flat, prec, rows, lr=1e-3, env=env)
    tr.set_data(0, x, y, w)
    loss = tr.run_epoch(None, rows)
    return loss, tr.get_grad(), st.get_weights(), tr.last_route()[0]


def _check_step(tag, prec, rows, dims, flat, got, twin, lo, go):
    loss, g, wts, route = got
    assert route == ("per_layer", "per_layer"), (tag, route)
    tol_l, tol_c = TOL[prec]
    assert np.isfinite(g).all() and np.isfinite(wts).all(), tag
    errs = ar.per_layer_rel_l2(dims, g, go)
    cos = float(g @ go / (np.linalg.norm(g) * np.linalg.norm(go)))
    print("ACT step %s: loss err %.2e, cos %.7f, per layer %s" % (tag, abs(loss - lo) / lo, cos, ["%.2e" % e for e in errs]))
    assert abs(loss - lo) <= tol_l * abs(lo), (tag, "loss", loss, lo)
    assert cos > tol_c, (tag, "cosine", cos)
    layer_tol = TOL_LAYER if prec == "f32" else (0.5 if rows < 64 else (0.1 if prec == "f16" else 0.25))
    assert max(errs) <= layer_tol, (tag, "per layer", errs, layer_tol)
    # one Keras Adam update from zero moments, applied to the device's own gradient in float32 (two implementations of the
    # same float32 arithmetic: the tolerance of tests/test_oracle.py's Adam comparison)
    np.testing.assert_allclose(wts, ar.adam_reference(flat, g, 1e-3), rtol=2e-6, atol=1e-7, err_msg=str(tag))
    # ... which moved every weight whose gradient is well above Adam's epsilon by about lr (lr g / (|g| + 3.2e-6)), none by more
    big = np.abs(go) > 1e-4
    assert big.any() and np.all(np.abs(wts - flat)[big] > 0.9e-3) and np.abs(wts - flat).max() < 1.1e-3, tag
    l2, g2, w2, _ = twin   # the same step on a second trainer: the same launches on the same bits
    assert loss == l2 and np.array_equal(g, g2) and np.array_equal(wts, w2), (tag, "bitwise twin differs")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows", [37, 600])   # 600: two contraction slices of the weight gradient and the slab sum
@pytest.mark.parametrize("name", ["T1", "T2"])
def test_training_step_against_float64(ctx, name, rows, prec):
    dims, codes = getattr(ar, name)
    Ws, bs, flat = ar.stack_weights(dims, ar.SEEDS[name])
    x, y, w = ar.step_data(dims, rows, ar.SEEDS[name])
    lo, go = ar.step(Ws, bs, codes, x, y, w)
    got = _step(ctx, dims, codes, flat, prec, x, y, w, rows)
    twin = _step(ctx, dims, codes, flat, prec, x, y, w, rows)
    _check_step((name, rows, prec), prec, rows, dims, flat, got, twin, lo, go)


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_relu_control_on_the_shared_epilogue_path(ctx, prec):
    """the same dims with ReLU through V21_TRAIN_CHAIN=0: the per-layer route's ReLU / linear epilogues, which share the
    kernel with the new ones, against the project's own oracle and bounds"""
    from helpers import oracle_step
    dims, codes = ar.RELU_CONTROL
    Ws, bs, flat = ar.stack_weights(dims, ar.SEEDS["RELU"], saturate=False)
    x, y, w = ar.step_data(dims, 600, ar.SEEDS["RELU"])
    lo, go = oracle_step(Ws, bs, codes, x, y, w)
    lo2, go2 = ar.step(Ws, bs, codes, x, y, w)
    assert lo == lo2 and np.array_equal(go, go2)   # (act_ref restates the project's oracle for ReLU stacks)
    loss, g, _, route = _step(ctx, dims, codes, flat, prec, x, y, w, 600, env={"V21_TRAIN_CHAIN": "0"})
    assert route == ("per_layer", "per_layer")
    tol_l, tol_c = TOL[prec]
    assert abs(loss - lo) <= tol_l * lo
    assert float(g @ go / (np.linalg.norm(g) * np.linalg.norm(go))) > tol_c
    if prec == "f32":
        from helpers import per_layer_gradient_check
        ok, note = per_layer_gradient_check(dims, codes, Ws, bs, x, g, go, prec, tgt=y, w=w)
        assert ok, note


# ---- 4. refusals, sweep, joint
def test_refusals_and_sweep(ctx):
    native = pkg("_native")
    dims = ar.T1[0]
    Ws, bs, flat = ar.stack_weights(dims, 3)
    st = native.Stack(ctx, dims, [ar.TANH, ar.SIGMOID, ar.TANH])   # a smooth OUTPUT layer: created, run forward, not trained
    st.set_weights(flat)
    x, y, w = ar.step_data(dims, 64, 3)
    with pytest.raises(native.EngineError, match=r"layer 2.*tanh"):
        native.Trainer(st, "f32", 64)
    ref = ar.forward(Ws, bs, [ar.TANH, ar.SIGMOID, ar.TANH], x)
    np.testing.assert_allclose(st.forward(x, "f32"), ref, atol=2e-5, rtol=1e-5)   # the handle stays usable
    np.testing.assert_allclose(st.forward(x, "f32", native.FWD_FORCE_GENERIC), ref, atol=2e-5, rtol=1e-5)
    with pytest.raises(native.EngineError, match="no fused kernel for this stack"):
        st.jit("f16")
    # joint: refused, naming the activation (the joint step runs on the chain kernels)
    ae_dims, em_dims = [37, 40, 9, 40, 37], [5, 40, 9]
    _, ae = new_trainer(ctx, ae_dims, [ar.TANH, 0, ar.TANH, 0], ar.stack_weights(ae_dims, 4)[2], "f32", 64)
    _, em = new_trainer(ctx, em_dims, [ar.TANH, 0], ar.stack_weights(em_dims, 5)[2], "f32", 64)
    with pytest.raises(native.EngineError, match="tanh"):
        native.Joint(ae, em, 1)
    # sweep: works as for any per-layer trainer, and every member equals its solo trainer
    codes = ar.T1[1]
    flats = [ar.stack_weights(dims, 20 + k)[2] for k in range(3)]
    solo = []
    for f in flats:
        s1, t1 = new_trainer(ctx, dims, codes, f, "f32", 64, lr=1e-3)
        t1.set_data(0, x, y, w)
        solo.append((t1.run_epoch(None, 64), s1.get_weights()))
    members = [new_trainer(ctx, dims, codes, f, "f32", 64, lr=1e-3) for f in flats]
    members[0][1].set_data(0, x, y, w)
    sw = native.Sweep([t for _, t in members])
    losses = sw.run_epoch(None, 64)
    for (l1, w1), l2, (s2, _) in zip(solo, losses, members):
        assert abs(l1 - l2) <= 1e-6 * abs(l1)
        np.testing.assert_allclose(s2.get_weights(), w1, rtol=1e-5, atol=1e-7)


# ---- 5. the Jacobian and what rests on it
# float32 restatement against float64 at these shapes and seeds, measured on the CPU (tests/test_act_cpu.py holds it there):
# J1 1.34e-7, T2 2.11e-7 (max over rows of relative L2).  The device's bound is 8 x that: the kernel's k-ordered fmaf chains
# and the device's exp differ from numpy's.
JAC_F32_ERR = ar.JAC_F32_ERR
assert JAC_F32_ERR == {"J1": 1.34e-7, "T2": 2.11e-7}


@pytest.mark.parametrize("name", ["J1", "T2"])
def test_jacobian_against_float64(ctx, name):
    st, dims, codes, Ws, bs, _ = _stack(ctx, name)
    x = ar.step_data(dims, 3, ar.SEEDS[name])[0]
    y, J = st.jacobian(x, "f32", return_outputs=True)
    assert st.last_jac_route()[0] == "generic"
    np.testing.assert_allclose(y, ar.forward(Ws, bs, codes, x), atol=2e-5, rtol=1e-5)
    e = ar.jac_row_rel_l2(J, ar.jacobian(Ws, bs, codes, x))
    print("ACT jacobian %s: device %.3e, float32 restatement %.3e" % (name, e, JAC_F32_ERR[name]))
    assert np.isfinite(J).all() and e <= 8 * JAC_F32_ERR[name], (name, e)


@pytest.fixture(scope="module")
def tanh_emulator():
    emulator, synth, eng = pkg("emulator"), pkg("synth"), pkg("engine")
    data = synth.make_dataset(n_train=600, n_val=40, n_test=40, seed=ar.SEEDS["T3"])
    eng.set_random_seed(ar.SEEDS["T3"])
    return emulator.DirectEmulator(hidden_dims=[64, 128], activation_func="tanh", **data)


def test_fit_recovers_a_point_of_the_tanh_model(tanh_emulator):
    """a noiseless spectrum the model makes itself at an interior point, sigma = 1 mK, 8 starts: recovered to the tolerance of
    tests/test_fit_gpu.py::test_fit_recovers_truths_on_trained_weights (best ln L >= -0.5)"""
    em, pp = tanh_emulator, pkg("preprocess")
    truth = pp.par_untransform(np.random.default_rng(4).uniform(-0.5, 0.5, size=(1, 7)), em.par_train)
    spectrum = np.asarray(em.predict(truth), np.float32).reshape(1, 451)
    res = em.fit_parameters(spectrum, 1.0, n_starts=8, max_iter=100, return_all=True)
    lnl = np.asarray(res.lnl).reshape(-1)
    print("ACT fit: ln L of the 8 starts %s" % lnl)
    assert np.isfinite(lnl).all() and lnl.max() >= -0.5, lnl


def test_forward_only_lnl_equals_the_jacobian_route(tanh_emulator):
    em = tanh_emulator
    pars = em.par_test[:5]
    data = np.asarray(em.predict(em.par_test[7]), np.float32) + 0.5
    a = em.log_likelihood(pars, data, 2.0)
    b = em.log_likelihood(pars, data, 2.0, forward_only=True)
    _, st, _, _ = em._diff_stack(pars)
    assert st.last_lnl_route()[0] == "two_launch" and st.last_jac_route()[0] == "generic"
    np.testing.assert_allclose(b, a, rtol=1e-5)


# ---- 6. the variational head with smooth hidden layers
def test_variational_tanh_autoencoder_without_noise_equals_the_plain_one(ctx):
    emulator, eng = pkg("emulator"), pkg("engine")
    sig = np.random.default_rng(9).normal(size=(64, 37)).astype(np.float32)
    eng.set_random_seed(9)
    vae = emulator.AutoEncoder(sig, enc_hidden_dims=[40], dec_hidden_dims=[40], latent_dim=9, activation_func="tanh", variational=True)
    vae.build((None, 37))
    ls = vae.encoder.layers + vae.decoder.layers
    codes = [l._act_code for l in ls]
    assert codes == [ar.TANH, 2, ar.TANH, ar.LINEAR]
    dims = [37, 40, 9, 40, 37]
    rng = np.random.default_rng(10)
    Ws = [l.kernel.copy() for l in ls]
    bs = [rng.normal(scale=0.05, size=l.bias.shape).astype(np.float32) for l in ls]
    y, w = sig, ora.mse_row_weight(sig).astype(np.float32)
    _, tr = new_trainer(ctx, dims, codes, ora.flatten_params(Ws, bs), "f32", 64, lr=1e-3)
    tr.set_vae(0.0, sample=False, seed=1)
    tr.set_data(0, y, None, w)
    loss = tr.run_epoch(None, 64)
    g = tr.get_grad()
    assert tr.last_route()[0] == ("per_layer", "per_layer")
    Wp = [Ws[0], np.ascontiguousarray(Ws[1][:, :9]), Ws[2], Ws[3]]
    bp = [bs[0], bs[1][:9].copy(), bs[2], bs[3]]
    plain = [ar.TANH, ar.LINEAR, ar.TANH, ar.LINEAR]
    _, tr2 = new_trainer(ctx, dims, plain, ora.flatten_params(Wp, bp), "f32", 64, lr=1e-3)
    tr2.set_data(0, y, None, w)
    loss2 = tr2.run_epoch(None, 64)
    g2 = tr2.get_grad()
    assert loss == loss2
    lo, go = ar.step(Wp, bp, plain, y, y, w)
    assert abs(loss2 - lo) <= TOL["f32"][0] * lo and max(ar.per_layer_rel_l2(dims, g2, go)) <= TOL_LAYER
    o = o2 = 0
    for l, (W_, b_) in enumerate(zip(Ws, bs)):
        gw = g[o:o + W_.size].reshape(W_.shape); o += W_.size
        gb = g[o:o + b_.size]; o += b_.size
        gw2 = g2[o2:o2 + Wp[l].size].reshape(Wp[l].shape); o2 += Wp[l].size
        gb2 = g2[o2:o2 + bp[l].size]; o2 += bp[l].size
        if l == 1:
            np.testing.assert_array_equal(gw[:, 9:], 0); np.testing.assert_array_equal(gb[9:], 0)
            gw, gb = gw[:, :9], gb[:9]
        np.testing.assert_allclose(gw, gw2, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(gb, gb2, rtol=1e-6, atol=1e-9)
