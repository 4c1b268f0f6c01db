"""Parameter Jacobian and Gaussian log-likelihood, host side: the float64 reference (tests/jacobian_ref.py) against
central finite differences of the oracle's forward, the route decision (csrc/routes.h: decide_jacobian through
v21_route_jacobian) and the ABI's new symbols.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import jacobian_ref as jr
from conftest import ROOT, pkg
from helpers import STACKS
from infer_cases import ARCHS, VG, transforms, weights_of


@pytest.mark.parametrize("name", ["D1", "NB", "VG"])
def test_reference_jacobian_matches_finite_differences(name):
    dims, act, Ws, bs = weights_of(name)
    tin, tout, x = transforms(5)
    xt = jr.transform(x, *tin)[0]
    keep = jr.min_relative_preactivation(Ws, bs, act, xt) >= 1e-3  # no unit near its kink: differences are smooth
    x = x[keep][:24]
    assert x.shape[0] >= 8, "too few rows away from every kink"
    y, J = jr.jacobian(Ws, bs, act, x, tin, tout)
    np.testing.assert_allclose(y, jr.oracle_outputs(Ws, bs, act, x, tin, tout), rtol=0, atol=0)
    fd = np.empty_like(J)
    for j in range(x.shape[1]):
        h = 1e-6 * np.abs(x[:, j])
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        fd[:, j, :] = (jr.oracle_outputs(Ws, bs, act, xp, tin, tout) - jr.oracle_outputs(Ws, bs, act, xm, tin, tout)) / (2 * h)[:, None]
    err = jr.rel_frobenius(J, fd)
    assert err.max() <= 1e-6, err.max()
    # ln L gradient: the same against differences of ln L itself
    rng = np.random.default_rng(1)
    data = y[0] + rng.normal(size=dims[-1]) * 0.1 * tout[0]
    w = np.where(rng.uniform(size=dims[-1]) < 0.2, 0.0, 1.0 / (0.05 * tout[0]) ** 2)
    lnl, g = jr.loglike(y, J, data, w)
    gfd = np.empty_like(g)
    for j in range(x.shape[1]):
        h = 1e-6 * np.abs(x[:, j])
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        lp = jr.loglike(jr.oracle_outputs(Ws, bs, act, xp, tin, tout), J, data, w)[0]
        lm = jr.loglike(jr.oracle_outputs(Ws, bs, act, xm, tin, tout), J, data, w)[0]
        gfd[:, j] = (lp - lm) / (2 * h)
    assert jr.rel_frobenius(g, gfd).max() <= 1e-6


def test_route_decisions():
    nat = pkg("_native")
    for name, (dims, act) in ARCHS.items():
        for prec in ("f32", "f16", "bf16"):
            for n in (1, 4099, 65536):
                assert nat.route_jacobian(dims, act, prec, n) == "fused", (name, prec, n)
                assert nat.route_jacobian(dims, act, prec, n, flags=nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM) == "fused"
        assert nat.route_jacobian(dims, act, "f32", 100, flags=nat.FWD_FORCE_GENERIC) == "generic"
    for dims, act in (STACKS["NB"], STACKS["W6"], VG, ([7, 64, 128, 451], [1, 1, 1])):
        for prec in ("f32", "f16", "bf16"):
            assert nat.route_jacobian(dims, act, prec, 100) == "generic"


def test_new_symbols_are_declared_exported_and_typed():
    nat = pkg("_native")
    lib = nat.load_library()
    hdr = open(os.path.join(ROOT, "include", "v21.h")).read()
    names = ["v21_mlp_jacobian", "v21_mlp_jacobian_dev", "v21_mlp_set_likelihood", "v21_mlp_loglike", "v21_mlp_loglike_dev",
             "v21_route_jacobian", "v21_mlp_last_jac_route"]
    for s in names:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in nat.SIGNATURES, s
        assert isinstance(getattr(lib, s), ctypes._CFuncPtr), s
    assert lib.v21_version() == 100


def test_reference_floor_derivative():
    """fx == 0 is differentiated at the floor: d xt / d fx = 2 / (span t ln 10), t = 1e-6 in the rows' dtype"""
    tin, _, x = transforms(2)
    x = x[:3].copy()
    x[:, 2] = 0
    for dt in (np.float64, np.float32):
        xt, fac = jr.transform(x.astype(dt), *tin)
        t = float(np.float32(1e-6)) if dt == np.float32 else 1e-6
        span = tin[3][2] - tin[2][2]
        np.testing.assert_allclose(fac[:, 2], 2 / (span * t * np.log(10)), rtol=1e-15)
