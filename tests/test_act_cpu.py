"""The smooth activations (include/v21.h: V21_ACT_TANH .. V21_ACT_SOFTPLUS) where no GPU is needed: the float64 reference
of tests/act_ref.py against central differences, the routes of csrc/routes.h, run-time compilation of the fused forward
kernel (hiprtc), the Python surface (Dense, DirectEmulator, Model.save -> h5lite), and the SIZING of the bounds that
tests/test_act_gpu.py holds the device to: the float32 restatement against float64 at exactly its shapes and seeds."""
import ctypes.util
import os
import subprocess
import sys

import numpy as np
import pytest

import act_ref as ar
from conftest import ROOT, pkg

HAVE_HIPRTC = os.path.exists("/opt/rocm/lib/libhiprtc.so") or ctypes.util.find_library("hiprtc") is not None
needs_hiprtc = pytest.mark.skipif(not HAVE_HIPRTC, reason="libhiprtc is not installed here")

HEADLINE = [7, 352, 352, 352, 224, 451]
SMALL = [5, 40, 72, 37]


def _codes(dims, code):
    return [code] * (len(dims) - 2) + [ar.LINEAR]


# ---- the reference itself
@pytest.mark.parametrize("code", ar.SMOOTH)
def test_reference_gradient_and_jacobian_match_central_differences(code):
    dims, codes = SMALL, _codes(SMALL, code)
    Ws, bs, flat = ar.stack_weights(dims, seed=100 + code, saturate=False)
    x, y, w = ar.step_data(dims, 6, seed=code)
    _, g = ar.step(Ws, bs, codes, x, y, w)
    flat64 = flat.astype(np.float64)
    rng = np.random.default_rng(code)
    idx = rng.choice(flat.size, 60, replace=False)
    h = 1e-5
    fd = np.empty(len(idx))
    for k, i in enumerate(idx):
        p, m = flat64.copy(), flat64.copy()
        p[i] += h; m[i] -= h
        fd[k] = (ar.loss_only(p, dims, codes, x, y, w) - ar.loss_only(m, dims, codes, x, y, w)) / (2 * h)
    assert np.linalg.norm(fd - g[idx]) <= 1e-6 * np.linalg.norm(g[idx]), (np.linalg.norm(fd - g[idx]) / np.linalg.norm(g[idx]))
    J = ar.jacobian(Ws, bs, codes, x)
    x64 = x.astype(np.float64)
    Jfd = np.empty_like(J)
    for j in range(dims[0]):
        p, m = x64.copy(), x64.copy()
        p[:, j] += h; m[:, j] -= h
        Jfd[:, j, :] = (ar.forward(Ws, bs, codes, p) - ar.forward(Ws, bs, codes, m)) / (2 * h)
    assert np.linalg.norm(Jfd - J) <= 1e-6 * np.linalg.norm(J), np.linalg.norm(Jfd - J) / np.linalg.norm(J)


def test_reference_is_finite_where_a_naive_formula_is_not():
    z = np.array([-200.0, -90.0, -1e-3, 0.0, 1e-3, 90.0, 200.0])
    for dt in (np.float64, np.float32):
        with np.errstate(all="raise"):   # no overflow anywhere (an underflow to 0 is the saturated value itself)
            with np.errstate(under="ignore"):
                for code in ar.SMOOTH:
                    for f in (ar.act, ar.deriv):
                        assert np.isfinite(f(code, z.astype(dt))).all(), (code, dt)
    assert np.allclose(ar.act(ar.SIGMOID, np.zeros(1)), 0.5) and np.allclose(ar.act(ar.SOFTPLUS, np.zeros(1)), np.log(2))
    h = ar.act(ar.TANH, z)
    assert np.allclose(ar.deriv_out(ar.TANH, h), ar.deriv(ar.TANH, z), atol=1e-12)
    for code in ar.SMOOTH:   # the derivative from the output is the derivative
        zz = np.linspace(-6, 6, 241)
        assert np.allclose(ar.deriv_out(code, ar.act(code, zz)), ar.deriv(code, zz), rtol=1e-9, atol=1e-12), code


# ---- routes (csrc/routes.h through the C ABI)
@pytest.mark.parametrize("code", ar.SMOOTH)
@pytest.mark.parametrize("dims", [HEADLINE, SMALL], ids=["headline", "small"])
def test_routes_of_smooth_stacks(dims, code):
    native = pkg("_native")
    act = _codes(dims, code)
    for prec in ("f32", "f16"):
        for rows in (256, 4096, 16384):
            assert native.route_train(dims, act, prec, rows, rows) == ("per_layer", "per_layer"), (prec, rows)
            assert native.route_train(dims, act, prec, 16384, rows, rt_ready=True) == ("per_layer", "per_layer"), (prec, rows)
    for prec in ("f32", "f16", "bf16"):
        for n in (1, 300, 65536):
            assert native.route_forward(dims, act, prec, n, native.FWD_NO_SMALL, rt_ready=True) == "fused_rt", (prec, n)
            for flags in (0, native.FWD_NO_SMALL, native.FWD_FORCE_CHAIN, native.FWD_FORCE_GENERIC):
                r = native.route_forward(dims, act, prec, n, flags)
                assert r in ("generic", "small") and r != "table", (prec, n, flags, r)
            assert native.route_forward(dims, act, prec, n, native.FWD_FORCE_CHAIN, rt_ready=True) == "generic"
        assert native.route_jacobian(dims, act, prec, 300) == "generic"
        assert native.route_loglike_fwd(dims, act, prec, 300) == "two_launch"
    # a smooth OUTPUT layer: no fused kernel, whatever rt_ready says
    assert native.route_forward(dims, [code] * (len(dims) - 1), "f16", 65536, rt_ready=True) == "generic"
    with pytest.raises(native.EngineError, match="unknown"):
        native.route_forward(dims, [7] * (len(dims) - 1), "f16", 300)


def test_relu_routes_are_what_they_were():
    native = pkg("_native")
    assert native.route_train(HEADLINE, [1, 1, 1, 1, 0], "f16", 4096, 4096)[0] == "chain16"
    assert native.route_train(SMALL, [1, 1, 0], "f32", 256, 256)[0].startswith("chain32")
    assert native.route_forward(SMALL, [1, 1, 0], "f16", 65536) == "table"


# ---- run-time compilation (hiprtc, no GPU)
def _prebuild_in_a_fresh_process(dims, act, prec, d):
    code = ("import importlib, sys; sys.path.insert(0, %r); n = importlib.import_module('21cmvae_amd._native'); "
            "n.jit_prebuild(%r, %r, %r, %r)" % (ROOT, dims, act, prec, d))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]


@needs_hiprtc
@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
def test_fused_forward_compiles_for_smooth_stacks(tmp_path, prec):
    d = str(tmp_path / "kc")
    _prebuild_in_a_fresh_process(SMALL, [3, 4, 0], prec, d)
    _prebuild_in_a_fresh_process(SMALL, [5, 6, 0], prec, d)
    files = sorted(os.listdir(d))
    assert len(files) == 2 and files[0] != files[1], files
    assert files[0].startswith("fused_5x40x72x37_a340_") and files[1].startswith("fused_5x40x72x37_a560_"), files


def test_jit_eligibility_of_smooth_stacks(tmp_path):
    native = pkg("_native")
    with pytest.raises(native.EngineError, match="output layer is linear"):
        native.jit_prebuild(SMALL, [3, 3, 3], "f16", str(tmp_path))
    with pytest.raises(native.EngineError, match="ReLU and linear layers only"):
        native.jit_prebuild_train(SMALL, [3, 3, 0], "f16", str(tmp_path))


# ---- the Python surface
def test_dense_accepts_the_names_and_callables():
    eng, native = pkg("engine"), pkg("_native")
    want = {"tanh": native.ACT_TANH, "sigmoid": native.ACT_SIGMOID, "elu": native.ACT_ELU, "softplus": native.ACT_SOFTPLUS,
            "relu": native.ACT_RELU, "linear": native.ACT_LINEAR}
    assert (native.ACT_TANH, native.ACT_SIGMOID, native.ACT_ELU, native.ACT_SOFTPLUS) == (3, 4, 5, 6)
    for name, code in want.items():
        assert eng.Dense(8, name)._act_code == code

    def tanh(x):
        return np.tanh(x)

    assert eng.Dense(8, tanh)._act_code == native.ACT_TANH and eng.Dense(8, None)._act_code == native.ACT_LINEAR
    with pytest.raises(NotImplementedError) as e:
        eng.Dense(8, "gelu")
    for name in want:
        assert repr(name) in str(e.value), str(e.value)


def test_direct_emulator_builds_tanh_layers():
    emulator, synth = pkg("emulator"), pkg("synth")
    data = synth.make_dataset(n_train=40, n_val=8, n_test=8, seed=3)
    em = emulator.DirectEmulator(hidden_dims=[64, 128], activation_func="tanh", **data)
    assert [l._act_code for l in em.emulator.layers] == [3, 3, 0]
    assert [l.units for l in em.emulator.layers] == [64, 128, 451]


@pytest.mark.parametrize("ext", ["h5", "npz"])
def test_save_and_load_keep_the_activation_names(tmp_path, ext):
    eng, h5 = pkg("engine"), pkg("h5lite")
    Ws, bs, _ = ar.stack_weights(SMALL, seed=5)
    m = eng.sequential_from_arrays(Ws, bs, acts=["tanh", "softplus", "linear"])
    p = str(tmp_path / ("m." + ext))
    m.save(p)
    back = h5.load_model(p)
    assert [l.activation for l in back.layers] == ["tanh", "softplus", "linear"]
    assert [l._act_code for l in back.layers] == [3, 6, 0]
    for a, b in zip(m.get_weights(), back.get_weights()):
        assert np.array_equal(a, b)
    if ext == "h5":
        info = h5.read_keras_h5(p)
        assert [l[3] for l in info["layers"]] == ["tanh", "softplus", "linear"]


# ---- bound sizing: what float32 arithmetic ALONE costs at the GPU tests' shapes and seeds
STEP_CONDITION = 5e-7   # float32 restatement against float64, per layer; the device's bound is 2e-6 (helpers: TOL_LAYER): factor 4


@pytest.mark.parametrize("name", ["T1", "T2"])
@pytest.mark.parametrize("rows", [37, 600])
def test_float32_step_is_within_the_condition(name, rows):
    dims, codes = getattr(ar, name)
    Ws, bs, _ = ar.stack_weights(dims, ar.SEEDS[name])
    x, y, w = ar.step_data(dims, rows, ar.SEEDS[name])
    lo, go = ar.step(Ws, bs, codes, x, y, w)
    l32, g32 = ar.step(Ws, bs, codes, x, y, w, dtype=np.float32)
    errs = ar.per_layer_rel_l2(dims, g32, go)
    print("float32 restatement %s rows=%d: loss %.2e, per layer %s" % (name, rows, abs(l32 - lo) / lo, ["%.2e" % e for e in errs]))
    assert np.isfinite(g32).all() and np.isfinite(go).all()
    assert max(errs) <= STEP_CONDITION, errs
    assert abs(l32 - lo) <= 2e-6 * lo


# the Jacobian: the float32 restatement's own error (max over rows of relative L2), measured here; the device's bound in
# tests/test_act_gpu.py is 8 x the figures recorded there, and this test holds the restatement to those figures
JAC_F32_ERR = ar.JAC_F32_ERR


@pytest.mark.parametrize("name", ["J1", "T2"])
def test_float32_jacobian_error_is_the_recorded_one(name):
    dims, codes = getattr(ar, name)
    Ws, bs, _ = ar.stack_weights(dims, ar.SEEDS[name])
    x = ar.step_data(dims, 3, ar.SEEDS[name])[0]
    e = ar.jac_row_rel_l2(ar.jacobian(Ws, bs, codes, x, dtype=np.float32), ar.jacobian(Ws, bs, codes, x))
    print("float32 restatement Jacobian %s: %.3e" % (name, e))
    assert e <= JAC_F32_ERR[name], e
