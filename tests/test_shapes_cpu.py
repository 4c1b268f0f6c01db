"""The float64 references at the shapes of tests/shape_cases.py (no GPU needed): jacobian_ref against central differences
of the oracle forward on every stack, marg_ref's whitening and invariance on every basis, sample_ref's draws and one
rebuilt transition at every in_dim, fit_ref.lm_ref from the starts tests/test_shapes_gpu.py uses -- and every condition
the GPU tests state as a cap, evaluated on the references alone."""
import numpy as np
import pytest

import fit_ref as fr
import jacobian_ref as jr
import marg_ref as mr
import sample_ref as sr
import shape_cases as sc
from infer_support import alpha_bound, alpha_of

IDS = [c.name for c in sc.CASES]
FIT_CASES = [c for c in sc.CASES if c.fit]


def test_table_covers_the_axes():
    ins, outs = {c.dims[0] for c in sc.CASES}, {c.dims[-1] for c in sc.CASES}
    assert {1, 2, 4, 5, 8, 9, 14, 15, 16, 17} <= ins and {1, 3, 63, 64, 65, 130, 451} <= outs
    assert 20 <= len(sc.CASES) + 2 <= 25 and len(set(IDS)) == len(IDS)
    pairs = {(c.dims[0], c.dims[-1]) for c in sc.CASES}
    assert {(15, 65), (1, 1), (8, 64), (8, 451)} <= pairs  # the corners together
    assert any(len(c.dims) == 2 and c.act == [0] for c in sc.CASES) and any(len(c.dims) == 2 and c.act == [1] for c in sc.CASES)
    assert any(max(c.dims) == c.dims[0] for c in sc.CASES) and any(max(c.dims) == c.dims[-1] for c in sc.CASES)
    assert any(max(c.dims) < 32 for c in sc.CASES) and any(sc.GAUSS in c.act and c.dims[0] != 7 for c in sc.CASES)
    for c in sc.CASES:  # hidden widths stay at or below 64 outside the two wide cases
        assert all(h <= 64 for h in c.dims[1:-1]) or c.name in ("i2w300", "i7w3000"), c.name
        assert {c.dims[0] for c in FIT_CASES} == {1, 4, 5, 8} and all(sc.has_tin(c.dims) for c in FIT_CASES)
        for K in c.modes:
            assert np.count_nonzero(sc.weights(c.dims[-1], 1, K)) >= K + 1
    # the LDS arithmetic of jac_run (csrc/api_jacobian.hip) the comments of the table quote
    def tc_of(dims):
        tc, maxw = min(dims[0], 7), max(dims)
        while tc > 1 and 2 * (tc + 1) * maxw * 4 > 160 * 1024:
            tc -= 1
        return tc, 2 * (tc + 1) * maxw * 4
    assert tc_of([7, 3000, 5])[0] == 5 and tc_of(sc.TOO_WIDE[0]) == (1, 163856) and tc_of([2, 10240, 1]) == (1, 160 * 1024)
    assert all(tc_of(c.dims)[1] < 256 * 4 for c in sc.CASES if c.name in ("i1o1", "i2o1"))
    assert sc.SPLIT_ROWS > 65535 + 1


def smooth_rows(st, tin, want=24, draw=600):
    """raw rows (none on the zero floor) with no ReLU unit of any layer, the output layer included, near its kink: 1e-3 of
    the layer's largest |z| as in test_jacobian_cpu; 1e-4 for the 3000-wide layer, of whose units some lie within 1e-3
    in every row (the steps below move a pre-activation by about 1e-6 of that scale)"""
    dims = st["dims"]
    u = sc.rows_u(dims, draw, 77)
    x = fr.untransform(u, tin[0], tin[2], tin[3]) if tin is not None else u
    xt = jr.transform(x, *tin)[0] if tin is not None else x
    _, _, zs = jr.jvp(st["Ws"], st["bs"], st["act"], xt)
    rel = np.full(draw, np.inf)
    for z, a in zip(zs, st["act"]):
        if a == jr.RELU:
            rel = np.minimum(rel, np.min(np.abs(z), axis=1) / np.max(np.abs(z), axis=1))
    return x[rel >= (1e-3 if max(dims) <= 512 else 1e-4)][:want]


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_reference_jacobian_matches_finite_differences(case):
    """as test_jacobian_cpu.test_reference_jacobian_matches_finite_differences (rows away from every kink, 1e-6), with and
    without the transforms.  Worst of the table: 6.8e-8, and 8.3e-7 on the 3000-wide stack (whose rows keep 1e-4, not
    1e-3, from the nearest kink)."""
    st = sc.make_stack(case.dims, case.act)
    Ws, bs, act = st["Ws"], st["bs"], st["act"]
    worst = 0.0
    for tin, tout in ((st["tin"], st["tout"]), (None, None)):
        x = smooth_rows(st, tin)
        assert x.shape[0] >= 8, "too few rows away from every kink"
        y, J = jr.jacobian(Ws, bs, act, x, tin, tout)
        np.testing.assert_allclose(y, jr.oracle_outputs(Ws, bs, act, x, tin, tout), rtol=0, atol=0)
        lm = np.asarray(tin[0], bool) if tin is not None else np.zeros(case.dims[0], bool)
        steps = 1e-6 * np.where(lm, np.abs(x), np.maximum(np.abs(x), 0.05))  # (a linear column crosses zero)
        std = 1.0 if tout is None else tout[0]
        rng = np.random.default_rng(1)
        data = y[0] + rng.normal(size=case.dims[-1]) * 0.1 * std
        w = sc.weights(case.dims[-1], 1).astype(np.float64)
        lnl, g = jr.loglike(y, J, data, w)
        fd, gfd = np.empty_like(J), np.empty_like(g)
        for j in range(x.shape[1]):
            h = steps[:, j]
            xp, xm = x.copy(), x.copy()
            xp[:, j] += h
            xm[:, j] -= h
            yp, ym = jr.oracle_outputs(Ws, bs, act, xp, tin, tout), jr.oracle_outputs(Ws, bs, act, xm, tin, tout)
            fd[:, j, :] = (yp - ym) / (2 * h)[:, None]
            gfd[:, j] = (jr.loglike(yp, J, data, w)[0] - jr.loglike(ym, J, data, w)[0]) / (2 * h)
        err = jr.rel_frobenius(J, fd)
        assert err.max() <= 1e-6, err.max()
        assert jr.rel_frobenius(g, gfd).max() <= 1e-6
        worst = max(worst, err.max(), jr.rel_frobenius(g, gfd).max())
    print("%s: worst %.2e" % (case.name, worst))


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.modes], ids=[c.name for c in sc.CASES if c.modes])
def test_whitening_and_invariance(case):
    """Q W Q^T = I, a well-conditioned basis (cond(R) of the table at most 17), and marg unchanged by any combination of
    the modes added to the data -- relative to the sums of its terms' magnitudes, at foreground scale too"""
    st = sc.make_stack(case.dims, case.act)
    dout = case.dims[-1]
    x = sc.rows(case.dims, 5, 3)
    y, J = jr.jacobian(st["Ws"], st["bs"], st["act"], x, st["tin"], st["tout"])
    data, _ = sc.data_for(st, 1)
    for K in case.modes:
        w = sc.weights(dout, 1, K).astype(np.float64)
        A = sc.basis(dout, K)
        Q, R = mr.whiten(A, w)
        np.testing.assert_allclose((Q * w) @ Q.T, np.eye(K), atol=1e-12)
        assert np.all(Q[:, w == 0] == 0)
        assert sc.basis_condition(dout, K, w) < 100, (case.name, K, sc.basis_condition(dout, K, w))
        m0 = mr.marg(y, J, data, w, A)
        for amp in (3.0, 1e6 * sc.OUT_STD):
            a = amp * np.random.default_rng(K).normal(size=K)
            m1 = mr.marg(y, J, data.astype(np.float64) + a @ A, w, A)
            rel = 1e-9 * max(1.0, amp / sc.OUT_STD)  # (float64 rounding of data carrying amp)
            assert np.all(np.abs(m1["lnl"] - m0["lnl"]) <= rel * m0["lnl_scale"])
            assert np.all(np.abs(m1["grad"] - m0["grad"]) <= rel * m0["grad_scale"])
            np.testing.assert_array_equal(m1["F"], m0["F"])


def test_refused_bases():
    """the table's refusals: fewer than K + 1 live bins"""
    assert np.count_nonzero(sc.weights(1, 1)) == 1 and np.count_nonzero(sc.weights(3, 1)) == 2
    with pytest.raises(AssertionError):
        sc.weights(3, 1, 4)


def evaluations(case, prob, u):
    """(ln L, gradient, Fisher) of the first spectrum at u in float64, rounded to the float32 the device hands over"""
    st = sc.make_stack(case.dims, case.act)
    ev = sr.evaluator_batch(st["Ws"], st["bs"], st["act"], prob["data"][0], prob["w"], st["tout"])
    return tuple(a.astype(np.float32).astype(np.float64) for a in ev(u))


@pytest.mark.parametrize("din", sorted({c.dims[0] for c in sc.CASES if c.dims[0] <= 8}))
def test_normals_at_every_in_dim(din):
    chains = sc.CHAIN0 + np.arange(64)
    xi = sr.normals(sc.SEED, chains, sc.STEP0, din)
    assert xi.shape == (64, din) and np.all(np.isfinite(xi))
    full = sr.normals(sc.SEED, chains, sc.STEP0, 8)
    np.testing.assert_array_equal(xi, full[:, :din])  # a column does not depend on how many are asked for ...
    np.testing.assert_array_equal(sr.normals(sc.SEED, chains, sc.STEP0, 4), sr.normals(sc.SEED, chains, sc.STEP0, 5)[:, :4])
    if din > 4:  # ... and block 1 is another draw than block 0
        assert not np.array_equal(full[:, 4:8], full[:, 0:4])


@pytest.mark.parametrize("case", FIT_CASES, ids=[c.name for c in FIT_CASES])
def test_one_transition_is_self_consistent_and_inside_the_caps(case):
    """the transition test_shapes_gpu rebuilds, on float64 evaluations rounded to float32: log q of the proposal is the
    density of the normals that drew it, the reverse move's log alpha is the negative of the forward's, and the share of
    accept decisions the first-order bound (infer_support.alpha_bound) excuses stays under its cap of 0.5 % --
    reference figures: 0 of 384 at in_dim 1, 4, 5 and 8; every proposal inside the box; 0.97, 0.87, 0.84, 0.78 accepted."""
    prob = sc.fit_problem(case)
    din = case.dims[0]
    tin = sc.make_stack(case.dims, case.act)["tin"]
    x0 = sc.chain_starts(case, prob)
    u0 = jr.transform(x0, *tin)[0].astype(np.float32).astype(np.float64)
    n = u0.shape[0]
    chains, eps = sc.CHAIN0 + np.arange(n), np.full(n, sc.EPS0)
    e0 = evaluations(case, prob, u0)
    xi = sr.normals(sc.SEED, chains, sc.STEP0, din)
    prop, lq, inside = sr.propose(u0, e0[1], e0[2], eps, xi, sc.RIDGE)
    L0, ok0 = sr.factor(e0[2], sc.RIDGE)
    assert ok0.all() and inside.mean() >= 0.9, inside.mean()
    ld = np.sum(np.log(np.diagonal(L0, axis1=1, axis2=2)), axis=1)
    lq_xi = -0.5 * np.sum(xi * xi, axis=1) + ld - 0.5 * din * np.log(2 * np.pi * sc.EPS0 ** 2)
    # (prop is rounded to float32: |d log q| <= |xi| |L^T d prop| / eps)
    slack = np.sqrt(np.sum(xi * xi, axis=1)) * np.linalg.norm(L0, axis=(1, 2)) * 2.0 ** -24 * np.sqrt(din) / sc.EPS0 + 1e-9
    assert np.all(np.abs(lq - lq_xi) <= slack + 0.5 * slack ** 2)
    e1 = evaluations(case, prob, prop)
    la = alpha_of(u0, e0, prop, e1, eps, sc.RIDGE)
    back = alpha_of(prop, e1, u0, e0, eps, sc.RIDGE)
    fin = np.isfinite(la)
    assert np.array_equal(fin, inside) and np.allclose(la[fin], -back[fin], rtol=0, atol=1e-9 * (1 + np.abs(la[fin])))
    bound = alpha_bound(u0, e0, prop, e1, eps, sc.RIDGE, la)
    logu = np.log(sr.accept_uniform(sc.SEED, chains, sc.STEP0))
    excused = np.abs(logu - la) <= bound
    print("%s: inside %.3f, accepted %.3f, excused %d of %d" % (case.name, inside.mean(), (logu < la).mean(), excused.sum(), n))
    assert excused.sum() == 0  # with room: the cap allows one


@pytest.mark.parametrize("case", FIT_CASES, ids=[c.name for c in FIT_CASES])
def test_lm_ref_converges_from_the_starts(case):
    """from every start test_shapes_gpu fits: status 1 inside the box, cond(F) at the optimum under the 1e6 gate of the
    comparison (reference figures, worst cond per stack: i1o63 1, i4o65 7.3, i5o130 5.2, i8o64 41; at most 4
    proposals), and the same
    optimum from a start moved by 1e-6 (what float32 evaluations do to the path must not change where it ends)"""
    st = sc.make_stack(case.dims, case.act)
    prob = sc.fit_problem(case)
    worst = 0.0
    for i, u0 in enumerate(prob["u0"]):
        ev = fr.evaluator(st["Ws"], st["bs"], st["act"], prob["data"][i // sc.FIT_STARTS], prob["w"], st["tout"])
        ref = fr.lm_ref(ev, u0, max_iter=40)
        cond = np.linalg.cond(ev(ref["u"])[2])
        worst = max(worst, cond)
        assert ref["status"] == 1 and np.all(np.abs(ref["u"]) < 1 - 1e-3) and cond < 1e5, (case.name, i, ref["status"], ref["u"], cond)
        assert ref["lnl"] >= ref["lnl0"]
        moved = fr.lm_ref(ev, u0 + 1e-6, max_iter=40)
        np.testing.assert_allclose(moved["u"], ref["u"], atol=1e-5)
        assert abs(moved["lnl"] - ref["lnl"]) <= 1e-5 * max(1.0, abs(ref["lnl"]))
    print("%s: worst cond(F) %.2e" % (case.name, worst))


def test_kink_share_of_the_rows_the_gpu_tests_use():
    """check_rows explains rows beyond 1e-5 by units within 1e-5 max|z| of their kink and caps them at 0.5 % (at least one
    row) per call: on the reference no row of any call of the table has such a unit -- 0 of 22 rows per stack"""
    for case in sc.CASES:
        st = sc.make_stack(case.dims, case.act)
        for n, tin_on, _, x in sc.jac_inputs(case):
            xt = jr.transform(x, *st["tin"])[0] if tin_on else x.astype(np.float64)
            kinks = jr.near_kinks(st["Ws"], st["bs"], st["act"], xt)
            near = np.zeros(n, bool)
            for k in kinks:
                if k is not None:
                    near |= k.any(axis=1)
            assert near.sum() == 0, (case.name, n, near.sum())
