"""The nested sampler, host side (no GPU): ``nested_evidence`` on constructed records, the float64 reference
(tests/nested_ref.py) on an analytic Gaussian in the box and on the two quadrature problems of tests/infer_cases.py,
two deliberately wrong variants that the same bound catches, the route decision (v21_route_nested) and the refusals of
``Stack.nested_opts``.  The quadrature cases (tests/infer_cases.py) are computed once and shared with tests/test_nested_gpu.py.

Bound: N_SE = 5 standard errors of the mean over 64 independent runs (their scatter / 8).  Measured with the shipped
defaults (n_repeats = 3 d, gamma = 2.38 / sqrt(2 d)), sigma = 0.1, seed 0: d = 7, N = 256 bias +0.056 +- 0.032; d = 7,
N = 64 +0.162 +- 0.059 -- a real bias of a third of one run's error, 2.8 standard errors of 64 runs (seeds 2 and 3 of the
table in tests/nested_ref.py: 1.9 and 2.3) --; d = 2, N = 64 -0.005 +- 0.038.  The k / N shrinkage misses by 144 standard
errors, the rule ln L >= L* - 1 by 55.  Quadrature: i1 z -0.42, i2 z -0.06."""
import math

import numpy as np
import pytest

import nested_ref as nr
from conftest import pkg
from infer_cases import ARCHS, N_SE, RUNS, SEED, quadrature_case, run_stats, z_of

SIGMA = 0.1  # the analytic Gaussian's width in u

_gauss = {}


def gauss_run(d, N, **kw):
    """the reference on the Gaussian from drawn starts, as many iterations as leave e^-12 of the bulk in the live points"""
    key = (d, N) + tuple(sorted(kw.items()))
    if key not in _gauss:
        T = int(math.ceil((d * math.log(1.0 / SIGMA) + 12.0) / np.sum(1.0 / (N - np.arange(N // 2)))))
        u0 = nr.start_draws(SEED, np.arange(RUNS * N), d)
        _gauss[key] = nr.nested_ref(nr.gauss_lnl(SIGMA), u0, N, T, seed=SEED, **kw)
    return _gauss[key]


# ---- nested_evidence
def test_evidence_of_one_iteration_by_hand():
    em = pkg("emulator")
    dead, live = np.log([[1.0, 2.0]]), np.log([3.0, 4.0, 5.0, 6.0])
    x1, x2 = math.exp(-1 / 4), math.exp(-1 / 4 - 1 / 3)
    parts = np.array([1.0 * (1 - x1), 2.0 * (x1 - x2)] + [v * x2 / 4 for v in (3.0, 4.0, 5.0, 6.0)])
    Z = parts.sum()
    lz, err, H, lw = em.nested_evidence(dead, live, 4)
    assert abs(lz - math.log(Z)) < 1e-14 and lw.shape == (6,)
    np.testing.assert_allclose(np.exp(lw), parts / Z, rtol=1e-13)
    Hh = np.sum(parts / Z * np.log([1, 2, 3, 4, 5, 6])) - math.log(Z)
    assert abs(H - Hh) < 1e-13
    s_k, v_k = 1 / 4 + 1 / 3, 1 / 16 + 1 / 9
    assert abs(err - math.sqrt(Hh * v_k / s_k)) < 1e-13
    # leading axes are runs; the reference's own evidence agrees
    lz2, err2, H2, lw2 = em.nested_evidence(np.stack([dead, dead + 1]), np.stack([live, live + 1]), 4)
    np.testing.assert_allclose(lz2, [lz, lz + 1], rtol=0, atol=1e-14)
    np.testing.assert_allclose(lw2[1], lw, rtol=0, atol=1e-13)
    ref = nr.evidence(dead, live, 4)
    assert abs(ref[0] - lz) < 1e-14 and abs(ref[1] - err) < 1e-14 and abs(ref[2] - H) < 1e-13
    with pytest.raises(ValueError):
        em.nested_evidence(dead, live[:3], 4)


def test_evidence_of_a_flat_record_and_of_minus_infinity():
    em = pkg("emulator")
    lz, err, H, lw = em.nested_evidence(np.full((7, 8), -3.25), np.full(16, -3.25), 16)
    assert abs(lz + 3.25) < 1e-12 and abs(H) < 1e-12 and abs(np.sum(np.exp(lw)) - 1) < 1e-12
    dead = np.full((2, 8), -1.0)
    dead[0, :3] = -np.inf
    lz, err, H, lw = em.nested_evidence(dead, np.zeros(16), 16)
    assert np.isfinite(lz) and np.isfinite(H) and np.all(lw[:3] == -np.inf) and abs(np.sum(np.exp(lw)) - 1) < 1e-12


def test_evidence_of_a_constructed_gaussian_record():
    """dead ln L set to ln L(X) of a d-dimensional Gaussian at the expected volumes X_{t,r}, live points at the midpoints of
    N equal parts of [0, X_T]: ln Z and H within the rectangle rule's own error -- the difference between the rule on the
    intervals' upper ends (what the estimate is) and on their lower ends -- of the analytic values"""
    em = pkg("emulator")
    d, sigma, N, T = 2, 0.1, 64, 40
    k = N // 2
    vd = math.pi ** (d / 2) / math.gamma(d / 2 + 1)
    lnl_of = lambda X: -0.5 * (X * 2.0 ** d / vd) ** (2.0 / d) / sigma ** 2
    step = 1.0 / (N - np.arange(k))
    lnx = (-np.arange(T)[:, None] * step.sum() - np.cumsum(step)[None, :]).reshape(-1)
    X = np.exp(lnx)
    xl = X[-1] * (np.arange(N) + 0.5) / N
    lz, err, H, lw = em.nested_evidence(lnl_of(X).reshape(T, k), lnl_of(xl), N)
    assert abs(np.sum(np.exp(lw)) - 1) < 1e-12
    # the same integrals with every interval's ln L taken at its other end
    edges = np.concatenate([[1.0], X])
    width = edges[:-1] - edges[1:]
    lo_l = lnl_of(edges[:-1])
    z_est = np.sum(np.exp(lnl_of(X)) * width) + X[-1] * np.mean(np.exp(lnl_of(xl)))
    z_low = np.sum(np.exp(lo_l) * width) + X[-1] * np.mean(np.exp(lnl_of(xl)))
    h_low = (np.sum(np.exp(lo_l) * lo_l * width) + X[-1] * np.mean(np.exp(lnl_of(xl)) * lnl_of(xl))) / z_low - math.log(z_low)
    lz_true = d / 2 * math.log(2 * math.pi * sigma ** 2) - d * math.log(2.0)
    h_true = -d / 2 - lz_true
    up_l = lnl_of(X)
    h_est = (np.sum(np.exp(up_l) * up_l * width) + X[-1] * np.mean(np.exp(lnl_of(xl)) * lnl_of(xl))) / z_est - math.log(z_est)
    assert abs(H - h_est) < 1e-10
    tol_z, tol_h = abs(math.log(z_est) - math.log(z_low)), abs(h_est - h_low)
    print("constructed record: ln Z %.5f (analytic %.5f, rule's error %.5f), H %.5f (analytic %.5f, rule's error %.5f)"
          % (lz, lz_true, tol_z, H, h_true, tol_h))
    assert abs(lz - math.log(z_est)) < 1e-12
    assert abs(lz - lz_true) <= tol_z and abs(H - h_true) <= tol_h
    assert tol_z < 0.05 and tol_h < 0.05


# ---- the reference on the analytic Gaussian
@pytest.mark.parametrize("d,N", [(7, 256), (7, 64), (2, 64)])
def test_reference_on_a_gaussian(d, N):
    r = gauss_run(d, N)
    lz, err = run_stats(r, N, RUNS)
    z, scatter = z_of(lz, nr.gauss_lnz(d, SIGMA)), lz.std(ddof=1)
    print("nested_ref d=%d N=%d: bias %+.3f +- %.3f (z %+.2f), scatter %.3f, mean formula error %.3f, accept %.2f"
          % (d, N, lz.mean() - nr.gauss_lnz(d, SIGMA), scatter / 8, z, scatter, err.mean(), r["accept_rate"].mean()))
    assert abs(z) < N_SE
    assert scatter / 1.5 < err.mean() < scatter * 1.5
    assert 0.1 < r["accept_rate"].mean() < 0.7


def test_wrong_variants_fail_the_same_bound():
    d, N = 7, 256
    truth = nr.gauss_lnz(d, SIGMA)
    z_ratio = z_of(run_stats(gauss_run(d, N), N, RUNS, shrink="ratio")[0], truth)
    z_slack = z_of(run_stats(gauss_run(d, N, slack=1.0), N, RUNS)[0], truth)
    print("wrong variants: k / N shrinkage z %+.1f, ln L >= L* - 1 z %+.1f" % (z_ratio, z_slack))
    assert abs(z_ratio) > N_SE and abs(z_slack) > N_SE


@pytest.mark.parametrize("name", ["i1", "i2"])
def test_reference_against_quadrature(name):
    p, lz_q, r, lz = quadrature_case(name)
    z = z_of(lz, lz_q)
    print("nested_ref %s: ln Z %.4f +- %.4f, quadrature %.4f (z %+.2f), accept %.2f" % (name, lz.mean(), lz.std(ddof=1) / 8, lz_q, z,
                                                                                      r["accept_rate"].mean()))
    assert abs(z) < N_SE


def test_reference_draws_and_ranks():
    a, b = nr.move_draws(3, nr.slot_rows(40, 16), 5, 8)
    assert a.shape == (40, 8) and np.all(a != b) and a.min() == 0 and a.max() == 7 and b.min() == 0 and b.max() == 7
    c = nr.restart_draws(3, nr.slot_rows(40, 16), 5, 8)
    assert c.min() == 0 and c.max() == 7 and not np.array_equal(c, a)
    u = nr.start_draws(1, np.arange(4096), 7)
    assert u.dtype == np.float32 and np.all(np.abs(u) <= 1) and abs(u.mean()) < 0.02 and abs((u ** 2).mean() - 1 / 3) < 0.02
    order = nr.rank_order(np.array([[2.0, np.nan, 1.0, 1.0, -np.inf, 3.0]]))
    assert order.tolist() == [[1, 4, 2, 3, 0, 5]]


# ---- the binding
def test_signatures_and_options():
    nat = pkg("_native")
    for name in ("v21_mlp_sample_nested", "v21_mlp_sample_nested_dev", "v21_route_nested"):
        assert name in nat.SIGNATURES and hasattr(nat.load_library(), name)
    o = nat.Stack.nested_opts()
    assert (o.n_live, o.n_repeats, o.n_iter, o.gamma, o.seed, o.iter0, o.chain0) == (256, 0, 100, 0.0, 0, 0, 0)
    o = nat.Stack.nested_opts(64, n_repeats=5, n_iter=3, gamma=0.5, seed=2 ** 63, iter0=7, chain0=128, n=256, n_data=2, in_dim=7)
    assert (o.n_live, o.n_repeats, o.n_iter, o.gamma, o.seed, o.iter0, o.chain0) == (64, 5, 3, 0.5, 2 ** 63, 7, 128)
    bad = [dict(n_live=17), dict(n_live=14), dict(n_live=514), dict(gamma=-1.0), dict(gamma=float("nan")),
           dict(gamma=float("inf")), dict(n_repeats=-1), dict(n_iter=-1), dict(iter0=-1), dict(chain0=-1), dict(n_iter=1.5),
           dict(iter0=2 ** 32 - 10, n_iter=10, n_repeats=1), dict(n_iter=2 ** 30, n_repeats=8), dict(n_live=16, n=40),
           dict(n_live=16, n=96, n_data=4)]
    for kw in bad:
        with pytest.raises(ValueError):
            nat.Stack.nested_opts(**kw)
    assert nat.Stack.nested_opts(n_live=16, in_dim=7).n_live == 16
    st = object.__new__(nat.Stack)
    st.dims = [7, 451]
    with pytest.raises(ValueError, match="whole runs"):
        st.sample_nested(np.zeros((100, 7)), n_live=64)
    with pytest.raises(ValueError, match="their number"):
        st.sample_nested()
    with pytest.raises(ValueError, match="multiple"):
        st.sample_nested(n=192, n_live=64, data=np.zeros((5, 451), np.float32))


def test_route_without_a_gpu():
    """v21_route_nested is v21_route_ensemble's decision and chunk rule with n_live in the place of n_walkers"""
    nat = pkg("_native")
    dims, act = ARCHS["S1"]
    other = ([7, 33, 451], [1, 0])
    for (dm, ac), n, N, nd, K, host in (((dims, act), 65536, 512, 0, 0, False), ((dims, act), 1024, 256, 0, 0, False),
                                        ((dims, act), 65536, 256, 0, 3, False), ((dims, act), 2 * 256, 256, 2, 0, False),
                                        ((dims, act), 2 * 64, 64, 2, 0, False), (other, 65536, 256, 0, 0, False),
                                        ((dims, act), 64 * 200, 64, 0, 0, True), ((dims, act), 4 * 2560, 64, 4, 0, True),
                                        ((dims, act), 2 * 65280, 510, 2, 0, True), (ARCHS["S2"], 65536, 512, 0, 0, False),
                                        (ARCHS["S3"], 64 * 200, 64, 0, 0, True)):
        for prec in ("f32", "f16", "bf16"):
            assert nat.route_nested(dm, ac, prec, n, N, nd, K, 0, host) == nat.route_ensemble(dm, ac, prec, n, N, nd, K, 0, host)
    assert nat.route_nested(dims, act, "f16", 65536, 512) == ("fused", 65536)
    assert nat.route_nested(dims, act, "f16", 2 * 64, 64, 2) == ("two_launch", 128)
    assert nat.route_nested(dims, act, "f16", 64 * 200, 64, host_form=True) == ("fused", 8192)
    for n, N, nd in ((114, 57, 0), (28, 14, 0), (1028, 514, 0), (100, 64, 0), (4 * 96, 64, 4), (256, 64, 3)):
        with pytest.raises(nat.EngineError):
            nat.route_nested(dims, act, "f32", n, N, nd)
    assert nat.route_nested(dims, act, "f32", 0, 64) == ("fused", 0)
    assert nat.route_nested(dims, act, "f32", 64, 16) == ("fused", 64)
    assert nat.route_nested(dims, act, "f32", 128, 64) == ("fused", 128)  # the library stays usable
