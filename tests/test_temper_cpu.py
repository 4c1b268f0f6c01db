"""CPU: the parallel-tempered sampler's reference (tests/temper_ref.py) against grid quadrature -- the independent check of
the algorithm that include/v21.h states for v21_mlp_sample_tempered -- and the host-only pieces of its Python surface.
The problems, their constants and the quadrature live in tests/infer_cases.py, which tests/test_temper_gpu.py shares."""
import numpy as np
import pytest

import sample_ref as sr
import shape_cases as sc
import temper_ref as tr
from conftest import pkg
from infer_cases import (BETAS, LADDERS, N_SE, RUN, RUNGS, SWAP_CASES, SWAP_EVERY, SWAP_SEED, ladder_check, problem, quadrature, scattered_u,
                         swap_betas)


@pytest.mark.parametrize("name", ["i1", "i2"])
def test_reference_against_quadrature(name):
    """temper_ref, 64 ladders of 8 rungs on the float64 oracle, against E_beta[ln L] by the midpoint rule on the box:
    every rung within 5 standard errors, and the trapezoid of the rungs within 5 of its own.  Halving the grid's spacing
    moves no value by a tenth of the sampler's standard error (it moves them by less than 1e-3 of it).  Worst |z| over the
    rungs 1.25 (1 input) and 1.37 (2 inputs), of ln Z 0.40 and 0.99.
    The same run WITHOUT swaps from starts far from the mode (the truth mirrored to the other side of the box, 0.9 from
    the centre) does NOT miss on these two problems: their posteriors have one mode, which the Langevin drift finds
    within the warm-up (worst |z| 3.1 and 2.5), so the two problems check the estimator, not the rescue of a stuck chain."""
    p = problem(name)
    q, q_coarse = quadrature(name)
    r = tr.temper_ref(p["ev"], p["starts_u"], BETAS, swap_every=SWAP_EVERY, **RUN)
    z, z_lz, se = ladder_check(r["mean_lnl"], name)
    print("%s: z per rung %s, z of ln Z %.2f, grid change / se %.1e, swaps %d" % (name, z.round(2), z_lz, np.max(np.abs(q - q_coarse) / se), r["swaps"]))
    assert np.all(np.abs(q - q_coarse) < 0.1 * se)
    assert r["swaps"] > 0 and np.all(np.isfinite(r["mean_lnl"]))
    assert np.all(np.abs(z) < N_SE), z
    assert abs(z_lz) < N_SE, z_lz
    # the swap rates belong to the lower row of a pair; the last rung never is one
    sw = r["swap_accept"].reshape(LADDERS, RUNGS)
    assert np.all(sw[:, -1] == 0) and np.all(sw[:, :-1].mean(axis=0) > 0.2)


@pytest.mark.parametrize("T,ladders", SWAP_CASES)
def test_swap_cases_on_the_reference(T, ladders):
    """the cases of test_temper_gpu.test_swaps_are_the_stated_permutation on the float64 oracle: after one transition from
    the scattered starts no pair of either event lies within the margin that test excuses (|log U - rhs| <= 1e-9 max(1,
    |rhs|)), at least 10 % of the pairs swap and at least 10 % refuse, and temper_ref's own run with swap_every = 1 is the
    run without swaps permuted by that decision"""
    case = sc.BY_NAME["i4o65"]
    st, prob = sc.make_stack(case.dims, case.act), sc.fit_problem(case)
    ev = sr.evaluator_batch(st["Ws"], st["bs"], st["act"], prob["data"][0], prob["w"], st["tout"])
    n, betas = T * ladders, swap_betas(T)
    u0 = scattered_u(4, n, SWAP_SEED)
    opts = dict(n_warmup=0, n_steps=1, seed=sc.SEED, chain0=sc.CHAIN0, eps0=0.5)
    for step0 in (0, 1):
        A = tr.temper_ref(ev, u0, betas, swap_every=0, step0=step0, **opts)
        B = tr.temper_ref(ev, u0, betas, swap_every=1, step0=step0, **opts)
        perm, lower, swapped, logu, rhs = tr.swap_event(A["lnl"], betas, step0, sc.SEED, sc.CHAIN0, step0)
        assert np.all(lower % T % 2 == step0 % 2) and np.all(lower % T + 1 < T) and lower.size == ladders * ((T - step0) // 2)
        assert not np.any(np.abs(logu - rhs) <= 1e-9 * np.maximum(1.0, np.abs(rhs)))
        if lower.size:  # (T = 2 has no odd pair: event 1 proposes nothing there)
            assert swapped.mean() >= 0.1 and (~swapped).mean() >= 0.1, swapped.mean()
        assert (lower.size == 0) == (T == 2 and step0 == 1)
        assert np.array_equal(B["u"], A["u"][perm]) and np.array_equal(B["lnl"], A["lnl"][perm]) and B["swaps"] == swapped.sum()
        assert np.array_equal(B["mean_lnl"], B["lnl"]) and np.array_equal(B["eps"], A["eps"])
        dec = np.zeros(n)
        dec[lower] = swapped
        assert np.array_equal(B["swap_accept"], dec)
    assert tr.temper_ref(ev, u0, betas, swap_every=2, step0=0, **opts)["swaps"] == 0


def test_signatures_hold_the_new_entries():
    nat = pkg("_native")
    for sym in ("v21_mlp_sample_tempered", "v21_mlp_sample_tempered_dev"):
        assert sym in nat.SIGNATURES, sym
        assert len(nat.SIGNATURES[sym][1]) == 13
    assert [f for f, _ in nat.TemperOpts._fields_] == ["n_temps", "betas", "swap_every"]
    assert [f for f, _ in nat.TemperOut._fields_] == ["mean_lnl", "var_lnl", "swap_accept"]


def test_temper_opts_refuses_what_the_library_refuses():
    nat = pkg("_native")
    t = nat.Stack.temper_opts(3, [1.0, 0.5, 0.0], 2, n=12, n_data=2)
    assert t.n_temps == 3 and list(t.betas)[:3] == [1.0, 0.5, 0.0] and t.swap_every == 2
    assert nat.Stack.temper_opts().n_temps == 1 and nat.Stack.temper_opts().betas[0] == 1.0
    bad = [dict(n_temps=0, betas=[]), dict(n_temps=33, betas=np.linspace(1, 0, 33)), dict(n_temps=2, betas=[1.0]),
           dict(n_temps=2, betas=[1.5, 0.5]), dict(n_temps=2, betas=[0.5, -0.1]), dict(n_temps=2, betas=[0.5, 0.5]),
           dict(n_temps=2, betas=[0.2, 0.7]), dict(n_temps=2, betas=[1.0, np.nan]), dict(n_temps=2, betas=[1.0, 0.0], swap_every=-1),
           dict(n_temps=3, betas=[1.0, 0.5, 0.0], n=10),             # no whole ladders
           dict(n_temps=3, betas=[1.0, 0.5, 0.0], n=12, n_data=3)]   # 4 rows per spectrum: a ladder would straddle two
    for kw in bad:
        with pytest.raises(ValueError):
            nat.Stack.temper_opts(**kw)


def test_default_betas_and_log_evidence():
    em = pkg("emulator")
    assert np.array_equal(em.default_betas(1), [1.0])
    b = em.default_betas(8)
    np.testing.assert_allclose(b, [1.0, (6 / 7) ** 5, (5 / 7) ** 5, (4 / 7) ** 5, (3 / 7) ** 5, (2 / 7) ** 5, (1 / 7) ** 5, 0.0], rtol=1e-15)
    assert b[0] == 1.0 and b[-1] == 0.0 and np.all(np.diff(b) < 0)
    np.testing.assert_allclose(b, BETAS, rtol=0, atol=0)
    # by hand: (1 - 0.5) (-2 - 4) / 2 + (0.5 - 0) (-4 - 10) / 2 = -1.5 - 3.5
    assert em.log_evidence([1.0, 0.5, 0.0], [-2.0, -4.0, -10.0]) == -5.0
    E = np.array([[[-2.0, -4.0, -10.0], [0.0, 0.0, 0.0]]])
    assert np.array_equal(em.log_evidence([1.0, 0.5, 0.0], E), [[-5.0, 0.0]])
    assert em.log_evidence([1.0], [-3.0]) == 0.0
    assert em.TemperedSamples._fields[:7] == em.PosteriorSamples._fields
    assert em.TemperedSamples._fields[7:] == ("betas", "mean_lnl", "swap_rate", "log_evidence", "log_evidence_err")
