"""CPU: the float64 reference of the MAP fit and its Laplace evidence (tests/map_ref.py) against quadrature, with the
controls that show the bounds discriminate, and the surface of v21_mlp_fit_map (no GPU needed)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import infer_cases as ic
import map_ref as mp
from conftest import ROOT, pkg

pr, jr = mp.pr, mp.fr.jr
NEW_SYMBOLS = ["v21_mlp_fit_map", "v21_mlp_fit_map_dev"]
SEEDS = (1, 2, 3)
HELD_U, HELD_CELLS = 0.4, 65536

_i1, _held = {}, {}


def i1_runs():
    """the i1 problem under its evidence prior from the box centre and three seeded starts; computed once"""
    if not _i1:
        p, prior = ic.problem("i1"), ic.evidence_prior("i1")
        ev = mp.single(p["ev"])
        starts = [np.zeros(1)] + [np.random.default_rng(s).uniform(-1.0, 1.0, size=1) for s in SEEDS]
        _i1.update(p=p, prior=prior, ev=ev, starts=starts, norm=pr.log_norm(prior) + math.log(2.0),
                   runs=[mp.map_ref(ev, prior, u0, [False], True) for u0 in starts])
    return _i1


def held_case():
    """i2 with column 1 held at u = 0.4: the reference and the midpoint rule along the free column; computed once"""
    if not _held:
        p, prior = ic.problem("i2"), ic.evidence_prior("i2")
        ev, hold, u0 = mp.single(p["ev"]), np.array([False, True]), np.array([0.0, HELD_U])
        c = (np.arange(HELD_CELLS) + 0.5) * (2.0 / HELD_CELLS) - 1.0
        pts = np.stack([c, np.full(HELD_CELLS, float(np.float32(HELD_U)))], -1)
        a = p["ev"](pts)[0] + pr.log_prior(mp.free_prior(prior, hold, True), pts)
        quad = a.max() + math.log(np.sum(np.exp(a - a.max())) * 2.0 / HELD_CELLS)
        _held.update(p=p, prior=prior, ev=ev, hold=hold, u0=u0, quad=quad, run=mp.map_ref(ev, prior, u0, hold, True))
    return _held


def lik_terms(p, u):
    """sum_k |J_jk w_k r_k| (d,): the magnitudes of the per-bin terms of ln L's gradient at u"""
    st = p["stack"]
    y, J, _ = jr.jvp(st["Ws"], st["bs"], st["act"], np.asarray(u, np.float64)[None, :])
    r = p["data"].astype(np.float64) - (y[0] * st["tout"][0] + st["tout"][1])
    return np.sum(np.abs(J[0] * st["tout"][0] * p["w"].astype(np.float64) * r), axis=-1)


def test_reference_evidence_matches_quadrature_i1():
    c = i1_runs()
    q_prior, q_uniform, _ = ic.evidence_quadrature("i1")
    for u0, r in zip(c["starts"], c["runs"]):
        d = r["laplace"] - c["norm"] - q_prior
        print("i1 from %+.4f: u %.5f status %d iters %d, Laplace - quadrature %.2e" % (u0[0], r["u"][0], r["status"], r["iters"], d))
        assert r["status"] == 1
        assert abs(d) <= 1e-5, (u0, d)
    # without the prior, from the centre: the uniform evidence (a seeded start finds a second mode 4.6 nats down)
    r = mp.map_ref(c["ev"], c["prior"], np.zeros(1), [False], False)
    d = r["laplace"] - math.log(2.0) - q_uniform
    print("i1 uniform: u %.5f, Laplace - quadrature %.4f" % (r["u"][0], d))
    assert r["status"] == 1 and r["lnp"] == 0.0
    assert abs(d) <= 0.05, d


def test_reference_with_a_held_column_matches_quadrature_i2():
    c = held_case()
    r = c["run"]
    d = r["laplace"] - c["quad"]
    print("i2, column 1 held: u %s status %d, Laplace - midpoint rule %.2e" % (r["u"], r["status"], d))
    assert r["status"] == 1 and r["d_free"] == 1
    assert abs(d) <= 1e-3, d
    # the held coordinate is the float32 value, bit for bit, and its row and column of the precision the identity's
    assert np.float32(r["u"][1]).tobytes() == np.float32(HELD_U).tobytes() and r["u"][1] == float(np.float32(HELD_U))
    assert np.array_equal(r["prec_u"][1], [0.0, 1.0]) and np.array_equal(r["prec_u"][:, 1], [0.0, 1.0])
    # its prior is never read: ln p is that of column 0 alone
    kind, mu, sd = c["prior"]
    assert r["lnp"] == pytest.approx(-0.5 * ((r["u"][0] - mu[0]) / sd[0]) ** 2, rel=1e-14)


def test_posterior_gradient_vanishes_at_the_reference_points():
    c, h = i1_runs(), held_case()
    cases = [(c["p"], c["ev"], c["prior"], np.array([False]), r) for r in c["runs"]]
    cases.append((h["p"], h["ev"], h["prior"], h["hold"], h["run"]))
    p2 = ic.problem("i2")
    cases.append((p2, mp.single(p2["ev"]), ic.evidence_prior("i2"), np.array([False, False]),
                  mp.map_ref(mp.single(p2["ev"]), ic.evidence_prior("i2"), np.zeros(2), [False, False], True)))
    checked = 0
    for p, ev, prior, hold, r in cases:
        if r["status"] != 1 or np.any(np.abs(r["u"][~hold]) >= 1.0):
            continue
        g, scale = mp.posterior_gradient(ev, prior, r["u"], hold, True, lik_terms(p, r["u"]))
        print("d = %d, %d held: |grad| %.2e of %.2e" % (hold.size, hold.sum(), np.max(np.abs(g)), scale))
        assert np.max(np.abs(g)) <= 1e-6 * scale, (g, scale)
        checked += 1
    assert checked == len(cases)


def test_controls_fail_the_bounds():
    """each wrong variant of the Laplace value misses the bounds above: they discriminate"""
    c, h = i1_runs(), held_case()
    q_prior = ic.evidence_quadrature("i1")[0]
    shifts = {}
    for name in ("no_prior_in_det", "d_free_plus_one"):
        r = mp.map_ref(c["ev"], c["prior"], np.zeros(1), [False], True, control=name)
        shifts[name] = r["laplace"] - c["norm"] - q_prior
        assert abs(shifts[name]) > 1e-5, (name, shifts[name])
    assert shifts["d_free_plus_one"] == pytest.approx(0.5 * math.log(2.0 * math.pi), abs=1e-5)
    for name in mp.CONTROLS:
        r = mp.map_ref(h["ev"], h["prior"], h["u0"], h["hold"], True, control=name)
        shifts["held " + name] = r["laplace"] - h["quad"]
        assert abs(shifts["held " + name]) > 1e-3, (name, shifts["held " + name])
    print("control shifts:", {k: round(v, 4) for k, v in shifts.items()})
    # (tests/test_map_gpu.py: the device's Laplace bound must stay below a quarter of the smallest of these)
    assert min(abs(v) for v in shifts.values()) > 0.8


def test_hold_and_information_rules_of_the_reference():
    p = ic.problem("i2")
    ev, prior = mp.single(p["ev"]), ic.evidence_prior("i2")
    # every column held: the clamped start, status 1, no iteration
    r = mp.map_ref(ev, prior, np.array([0.3, 1.7]), [True, True], True)
    assert r["status"] == 1 and r["iters"] == 0 and r["d_free"] == 0 and r["lnp"] == 0.0
    assert np.array_equal(r["u"], np.array([np.float32(0.3), 1.0], np.float64))
    assert r["laplace"] == r["lnl"]
    # a flat likelihood: without a prior no information; under a normal column the prior's mode, clamped into the box
    flat = lambda u: (0.0, np.zeros(2), np.zeros((2, 2)))
    assert mp.map_ref(flat, prior, np.zeros(2), [False, False], False)["status"] == 3
    assert mp.map_ref(flat, prior, np.zeros(2), [False, True], False)["status"] == 3
    mixed = ic.mixed_prior(2)  # (column 1: mu = -1.4, outside the box)
    r = mp.map_ref(flat, mixed, np.zeros(2), [False, False], True)
    assert r["status"] == 1
    np.testing.assert_allclose(r["u"], np.clip(mixed[1], -1.0, 1.0), atol=1e-6, rtol=0)


def test_surface_is_declared_and_bound():
    nat = pkg("_native")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "v21.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in nat.SIGNATURES, name
    types = open(os.path.join(ROOT, "include", "v21_types.h")).read()
    assert "v21_map_opts" in types and "v21_map_out" in types
    assert C.sizeof(nat.MapOpts) == 36     # int, int[8]
    assert C.sizeof(nat.MapOut) == 24      # three pointers
    assert C.sizeof(nat.FitOpts) == 32     # (unchanged)
    assert [f[0] for f in nat.MapOut._fields_] == list(nat.MAP_OUTPUTS) == ["lnp", "laplace", "prec_u"]
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("library not built")
    lib = nat.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    # null handles are refused before any device work
    assert lib.v21_mlp_fit_map(None, None, 0, 1, None, 0, None, None, None, None, None, None, None, None, 0, 0) == -1
    assert lib.v21_mlp_fit_map_dev(None, None, 7, 1, None, 0, None, None, None, None, None, None, None, None, 0, 0) == -1


def _hostless_stack(dims):
    """a Stack object without a device handle: argument checks that run before the library is called"""
    nat = pkg("_native")
    st = nat.Stack.__new__(nat.Stack)
    st.dims, st.act = list(dims), [1] * (len(dims) - 2) + [0]
    st.lib, st.ctx, st.h = None, None, None
    return st


def test_stack_fit_map_validates_arguments():
    st = _hostless_stack([7, 16, 451])
    x = np.zeros((6, 7))
    with pytest.raises(ValueError):
        st.fit_map(np.zeros((6, 5)))                        # wrong parameter count
    with pytest.raises(ValueError):
        st.fit_map(x, data=np.zeros((4, 451)))              # 6 rows over 4 spectra
    with pytest.raises(ValueError):
        st.fit_map(x, hold=[0, 1, 0])                       # one entry per column
    with pytest.raises(ValueError, match=r"hold\[3\]"):
        st.fit_map(x, hold=[0, 0, 0, 2, 0, 0, 0])           # 0 or 1
    with pytest.raises(ValueError, match="use_prior"):
        st.fit_map(x, use_prior=2)
    with pytest.raises(ValueError, match="unknown output"):
        st.fit_map(x, outputs=("lnp", "cov"))
    with pytest.raises(ValueError):
        _hostless_stack([9, 16, 451]).fit_map(np.zeros((2, 9)))  # at most 8 parameters
    o = st.map_opts(True, [1, 0, 0, 0, 0, 0, 1], 7)
    assert o.use_prior == 1 and list(o.hold) == [1, 0, 0, 0, 0, 0, 1, 0]
    o = st.map_opts()
    assert o.use_prior == 0 and not any(o.hold)


def test_fit_parameters_validates_fixed_before_any_device_work():
    emu = pkg("emulator")
    synth = pkg("synth")
    e = emu.Emulator.__new__(emu.Emulator)
    e.par_train = synth.make_params(500, seed=2, corners=True)
    e.par_labels = list(pkg("priors").PAR_LABELS)
    with pytest.raises(ValueError, match="taus"):
        e._fixed_columns({"taus": 0.05})
    hi = float(e.par_train[:, 3].max())
    with pytest.raises(ValueError, match="tau"):
        e._fixed_columns({"tau": 2.0 * hi + 1.0})
    with pytest.raises(ValueError, match="Vc"):
        e._fixed_columns({"Vc": -1.0})                      # (a log column: no logarithm)
    hold, val = e._fixed_columns({"tau": hi, "fx": 0.0})   # (the box's end, and fx = 0: its zero floor)
    assert list(np.flatnonzero(hold)) == [2, 3] and val[3] == hi and val[2] == 0.0 and np.all(np.isnan(val[~hold]))
    hold, _ = e._fixed_columns(None)
    assert not hold.any()


def test_prior_log_integral_matches_the_reference():
    priors, synth = pkg("priors"), pkg("synth")
    pt = synth.make_params(500, seed=2, corners=True)
    lo, hi = pt[:, 3].min(), pt[:, 3].max()
    P = priors.Prior({"tau": ("normal", lo + 0.9 * (hi - lo), 0.2 * (hi - lo)), "fstar": ("lognormal", -1.5, 0.3)}, pt)
    ref = pr.as_prior(*P.to_u())
    d = len(P.labels)
    assert P.log_integral_u() == pytest.approx(pr.log_norm(ref) + d * math.log(2.0), rel=1e-13)
    # over a subset: the held columns drop out, a uniform column counts ln 2
    free = np.ones(d, bool)
    free[[3, 5]] = False
    kind, mu, sd = ref
    sub = pr.as_prior(np.where(free, kind, 0), mu, sd)
    assert P.log_integral_u(free) == pytest.approx(pr.log_norm(sub) + (d - 2) * math.log(2.0), rel=1e-13)
    assert priors.Prior(None, pt).log_integral_u() == pytest.approx(d * math.log(2.0), rel=1e-15)
    # and it normalises log_density_u: ln p_unnormalised - log_integral + d ln 2
    u = np.random.default_rng(0).uniform(-1, 1, size=(5, d))
    np.testing.assert_allclose(P.log_density_u(u), pr.log_prior(ref, u) - P.log_integral_u() + d * math.log(2.0), rtol=0, atol=1e-12)


def test_free_block_inverse():
    """fit_parameters' cov_u: the inverse of the precision on the free block, zeros on held rows and columns, NaN for a
    matrix that is no usable precision"""
    inv = pkg("emulator")._free_block_inverse
    free = np.array([True, False, True])
    A = np.array([[4.0, 0.0, 2.0], [0.0, 1.0, 0.0], [2.0, 0.0, 9.0]], np.float32)  # (the held row and column: the identity's)
    want = np.zeros((3, 3))
    want[np.ix_([0, 2], [0, 2])] = np.array([[9.0, -2.0], [-2.0, 4.0]]) / 32.0
    np.testing.assert_allclose(inv(A, free), want, rtol=1e-15, atol=0)
    # columns in very different units are no ill conditioning: the guard looks at the matrix scaled to a unit diagonal
    S = np.diag([1e6, 1.0, 1e-6])
    np.testing.assert_allclose(inv(S @ A.astype(np.float64) @ S, free), np.diag([1e-6, 0.0, 1e6]) @ want @ np.diag([1e-6, 0.0, 1e6]), rtol=1e-12)
    # batched, with what has no inverse: a NaN entry, a diagonal entry that is not positive, an exactly and a nearly
    # singular free block (correlation 1 - 1e-9: beyond float32 data)
    nan, neg, sing, near = (A.astype(np.float64).copy() for _ in range(4))
    nan[0, 2] = nan[2, 0] = np.nan
    neg[2, 2] = -9.0
    sing[0, 2] = sing[2, 0] = 6.0
    near[0, 2] = near[2, 0] = 6.0 * (1.0 - 1e-9)
    out = inv(np.stack([A, nan, neg, sing, near]).reshape(1, 5, 3, 3), free)
    assert out.shape == (1, 5, 3, 3)
    np.testing.assert_allclose(out[0, 0], want, rtol=1e-15, atol=0)
    for k in range(1, 5):
        assert np.all(np.isnan(out[0, k][np.ix_([0, 2], [0, 2])])), k
        assert np.all(out[0, k][1] == 0) and np.all(out[0, k][:, 1] == 0), k
    # nothing free: all zeros
    assert np.all(inv(A, np.zeros(3, bool)) == 0)
