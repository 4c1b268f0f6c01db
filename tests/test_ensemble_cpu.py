"""The ensemble sampler, host side (no GPU): the float64 reference (tests/ensemble_ref.py) on a uniform and on a Gaussian
target, two deliberately wrong variants that the same bounds catch, the route and chunk decision (csrc/routes.h:
decide_ensemble through v21_route_ensemble) and the refusals of ``Stack.ensemble_opts``.

Bounds: N_SE = 5 between-ensemble standard errors (ensembles are independent of each other; the walkers of one are not).
A plain numpy stretch move gave worst |z| 1.7 .. 2.1 on the uniform target and 1.8 / 1.3 on the Gaussian one; without the
(d - 1) ln z term 43 .. 200 and 80."""
import numpy as np
import pytest

import ensemble_ref as er
import sample_ref as sr
from conftest import pkg
from helpers import STACKS
from infer_cases import ARCHS

N_SE = 5.0
MISS = 4 * N_SE  # what a wrong variant must miss by at least: "far more than the bound"


def uniform_run(W, **kw):
    d, E = 7, 64
    u0 = np.random.default_rng(W).uniform(-1, 1, size=(E * W, d))
    r = er.ensemble_ref(lambda u: np.zeros(u.shape[0]), u0, W, n_steps=600, n_warmup=200, thin=0, seed=17 + W, **kw)
    m, m2 = er.ensemble_estimates(r["mean_u"], r["cov_u"], W)
    return r, sr.pooled_check(m, 0.0)[1], sr.pooled_check(m2, 1.0 / 3.0)[1]


@pytest.mark.parametrize("W", [16, 64])
def test_reference_on_a_uniform_target(W):
    r, zm, z2 = uniform_run(W)
    print("uniform target, W = %d: accept %.3f, worst z mean %.2f, E[u^2] %.2f" % (W, r["accept_rate"].mean(), zm.max(), z2.max()))
    assert np.all(np.abs(r["u"]) <= 1.0)
    assert np.all(zm < N_SE) and np.all(z2 < N_SE), (zm, z2)
    # without the (d - 1) ln z term every proposal inside the box is accepted, and the law is not uniform
    r, zm, z2 = uniform_run(W, jacobian=False)
    print("   without (d - 1) ln z: worst z of E[u^2] %.1f" % z2.max())
    assert z2.max() > MISS, z2
    # proposals clipped onto the box instead of rejected: mass on its faces
    r, zm, z2 = uniform_run(W, clamp=True)
    print("   clamped: worst z of E[u^2] %.1f" % z2.max())
    assert z2.max() > MISS, z2


def gaussian_evaluator(sigma):
    """a one-layer linear stack y = u scored against d = 0 with w = 1 / sigma^2: ln L = -|u|^2 / (2 sigma^2)"""
    d = 7
    return sr.evaluator_batch([np.eye(d)], [np.zeros(d)], [0], np.zeros(d), np.full(d, 1.0 / sigma ** 2))


def gaussian_run(**kw):
    W, E, d, sigma = 16, 64, 7, 0.1
    u0 = 0.05 * np.random.default_rng(3).normal(size=(E * W, d))
    r = er.ensemble_ref(gaussian_evaluator(sigma), u0, W, n_steps=800, n_warmup=300, thin=0, seed=23, **kw)
    m, m2 = er.ensemble_estimates(r["mean_u"], r["cov_u"], W)
    return r, sr.pooled_check(m, 0.0)[1], sr.pooled_check(m2, sigma ** 2)[1]


def test_reference_on_a_gaussian_target():
    r, zm, zv = gaussian_run()
    print("Gaussian target: accept %.3f, worst z mean %.2f, variance %.2f" % (r["accept_rate"].mean(), zm.max(), zv.max()))
    assert np.all(zm < N_SE) and np.all(zv < N_SE), (zm, zv)
    r, zm, zv = gaussian_run(jacobian=False)
    print("   without (d - 1) ln z: worst z of the variance %.1f" % zv.max())
    assert zv.max() > MISS, zv


def test_reference_draws():
    """the stretch factor lies in [1 / a, a] with density 1 / sqrt(z), the partner in 0 .. H - 1, uniformly"""
    a, H, n = 2.0, 9, 200000
    z, k, logu = er.draws(5, np.arange(n), 3, a, H)
    assert z.min() >= 1 / a and z.max() <= a and k.min() == 0 and k.max() == H - 1 and np.all(logu < 0)
    # E[z] under g(z) ~ z^-1/2 on [1 / a, a]: (a^1.5 - a^-1.5) / (3 (a^0.5 - a^-0.5))
    ez = (a ** 1.5 - a ** -1.5) / (3 * (a ** 0.5 - a ** -0.5))
    assert abs(z.mean() - ez) < N_SE * z.std() / np.sqrt(n)
    counts = np.bincount(k, minlength=H)
    assert np.all(np.abs(counts - n / H) < N_SE * np.sqrt(n / H))


def test_route_table():
    nat = pkg("_native")
    F = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    arch, other = ARCHS["S1"], STACKS["NB"]
    table = [
        # stack, n, W, n_data, K, flags, host form -> route, chunk rows
        (arch, 65536, 256, 0, 0, F, False, "fused", 65536),          # the record
        (arch, 528, 16, 0, 0, F, False, "fused", 528),
        (arch, 512, 256, 2, 0, F, False, "fused", 512),              # half layout: 128 rows per spectrum
        (arch, 520, 260, 2, 0, F, False, "two_launch", 520),         # 130 rows per spectrum
        (arch, 2048, 16, 4, 0, F, False, "fused", 2048),             # 16 ensembles of 8 per spectrum
        (arch, 2112, 16, 4, 0, F, False, "two_launch", 2112),
        (arch, 65536, 256, 0, 4, F, False, "two_launch", 65536),     # a nuisance record
        (arch, 65536, 256, 0, 0, F | nat.FWD_FORCE_GENERIC, False, "two_launch", 65536),
        (arch, 65536, 256, 0, 0, F | nat.FWD_FORCE_CHAIN, False, "two_launch", 65536),
        (other, 65536, 256, 0, 0, F, False, "two_launch", 65536),    # outside archs.h
        (ARCHS["S2"], 65536, 256, 0, 0, F, False, "fused", 65536),   # the other stacks of archs.h that a sampler
        (ARCHS["S3"], 8208, 16, 0, 0, F, True, "fused", 8192),       # takes (S4 has 9 inputs: refused before any route)
        # host chunks: whole ensembles, not above 8,192 rows
        (arch, 8208, 16, 0, 0, F, True, "fused", 8192),
        (arch, 48 * 400, 48, 0, 0, F, True, "fused", 8160),
        (other, 48 * 400, 48, 0, 0, F, True, "two_launch", 8160),
        # ... whole spectra when they fit
        (arch, 4 * 2560, 16, 4, 0, F, True, "fused", 7680),
        (other, 4 * 2400, 48, 4, 0, F, True, "two_launch", 7200),
        # ... a fused call against a data matrix in multiples of lcm(W, 256) rows; spectra larger than a chunk
        (arch, 2 * 12288, 48, 2, 0, F, True, "fused", 7680),
        (arch, 2 * 16384, 16, 2, 0, F, True, "fused", 8192),
        (other, 2 * 12288, 48, 2, 0, F, True, "two_launch", 8160),
        # ... and two-launch where no such chunk fits: lcm(510, 256) = 65,280
        (arch, 2 * 65280, 510, 2, 0, F, True, "two_launch", 8160),
        (arch, 2 * 65280, 510, 2, 0, F, False, "fused", 2 * 65280),
    ]
    for (dims, act), n, W, nd, K, flags, host, route, chunk in table:
        for prec in ("f32", "f16", "bf16"):
            assert nat.route_ensemble(dims, act, prec, n, W, nd, K, flags, host) == (route, chunk), (dims, n, W, nd, K, flags, host, prec)


def test_route_argument_errors():
    nat = pkg("_native")
    dims, act = ARCHS["S1"]
    for n, W, nd in ((34, 17, 0),        # W odd
                     (28, 14, 0),        # W < 2 (d + 1)
                     (1028, 514, 0),     # W > 512
                     (40, 16, 0),        # n % W != 0
                     (96, 16, 4),        # 24 rows per spectrum: no whole ensembles
                     (96, 16, 5)):       # n % n_data != 0
        with pytest.raises(nat.EngineError):
            nat.route_ensemble(dims, act, "f32", n, W, nd)
    with pytest.raises(nat.EngineError):
        nat.route_ensemble(dims, act, "f32", 64, 16, n_modes=9)
    with pytest.raises(ValueError):
        nat.route_ensemble(dims, act, "f64", 64, 16)
    # the checks every route query shares refuse a width below 1 for the training query as for the others
    zero_wide = [dims[0], 0] + list(dims[2:])
    with pytest.raises(nat.EngineError, match=r"dims\[1\] = 0"):
        nat.route_ensemble(zero_wide, act, "f32", 64, 16)
    with pytest.raises(nat.EngineError, match=r"dims\[1\] = 0"):
        nat.route_train(zero_wide, act, "f16", 256, 256)
    assert nat.route_ensemble(dims, act, "f32", 0, 16) == ("fused", 0)
    assert nat.route_ensemble(dims, act, "f32", 64, 16) == ("fused", 64)  # the library stays usable


def test_options():
    nat = pkg("_native")
    o = nat.Stack.ensemble_opts()
    assert (o.n_walkers, o.a, o.n_steps, o.n_warmup, o.thin, o.seed, o.chain0, o.step0) == (64, 2.0, 1000, 500, 1, 0, 0, 0)
    o = nat.Stack.ensemble_opts(16, a=1.5, n_steps=3, n_warmup=0, thin=0, seed=2 ** 63, chain0=5, step0=7, n=64, n_data=2, in_dim=7)
    assert (o.n_walkers, o.a, o.n_steps, o.thin, o.seed, o.chain0, o.step0) == (16, 1.5, 3, 0, 2 ** 63, 5, 7)
    bad = [dict(n_walkers=17), dict(n_walkers=0), dict(n_walkers=514), dict(n_walkers=14, in_dim=7), dict(a=1.0), dict(a=0.5),
           dict(a=float("inf")), dict(a=float("nan")), dict(n_steps=-1), dict(n_warmup=-1), dict(thin=-1), dict(chain0=-1), dict(step0=-1),
           dict(n_steps=1.5), dict(step0=2 ** 32 - 10, n_steps=10, n_warmup=0), dict(n_walkers=16, n=40), dict(n_walkers=16, n=96, n_data=4)]
    for kw in bad:
        with pytest.raises(ValueError):
            nat.Stack.ensemble_opts(**kw)
    assert nat.Stack.ensemble_opts(n_walkers=14, in_dim=6).n_walkers == 14
    # the binding refuses rows that are no whole ensembles or spectra before the library sees them
    st = object.__new__(nat.Stack)
    st.dims = [7, 451]
    with pytest.raises(ValueError, match="whole ensembles"):
        st.sample_ensemble(np.zeros((40, 7)), 16)
    with pytest.raises(ValueError, match="data must be"):
        st.sample_ensemble(np.zeros((32, 7)), 16, data=np.zeros((2, 450), np.float32))
    with pytest.raises(ValueError, match="multiple"):
        st.sample_ensemble(np.zeros((32, 7)), 16, data=np.zeros((3, 451), np.float32))
