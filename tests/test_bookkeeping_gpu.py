"""The bookkeeping the three samplers share (csrc/rowmath.h: Moments, raw_row): the moments of the kept transitions, the
thinned store, the last state and the acceptance count, for MALA, its tempered form and the stretch-move ensemble on the
generic route at in_dim 1, 4 and 8 (tests/shape_cases.py) -- the ensemble and the tempered rows run nowhere else away
from 7 inputs.  Host forms, float64 starts, 3 warm-up and 12 kept transitions."""
import numpy as np
import pytest

import jacobian_ref as jr
import shape_cases as sc
from conftest import pkg
from infer_support import device_stack, flags_of, same

pytestmark = pytest.mark.gpu

N_WARMUP, N_STEPS = 3, 12
BETAS = (1.0, 0.25, 0.0)
SAMPLERS = ("mala", "tempered", "ensemble")
CASES = ("i1o63", "i4o65", "i8o64")


def rows_of(sampler, din):
    """5 chains; 2 ladders of 3 rungs; 2 ensembles of max(4, 2 (din + 1)) walkers"""
    return {"mala": 5, "tempered": 2 * len(BETAS), "ensemble": 2 * max(4, 2 * (din + 1))}[sampler]


def run(st, sampler, x0, flags, thin):
    opts = dict(n_steps=N_STEPS, n_warmup=N_WARMUP, thin=thin, seed=sc.SEED, chain0=sc.CHAIN0, step0=sc.STEP0)
    if sampler == "mala":
        return st.sample(x0, "f32", flags, eps0=sc.EPS0, ridge=sc.RIDGE, **opts)
    if sampler == "tempered":
        return st.sample_tempered(x0, len(BETAS), BETAS, 1, "f32", flags, eps0=sc.EPS0, ridge=sc.RIDGE, **opts)
    return st.sample_ensemble(x0, x0.shape[0] // 2, "f32", flags, **opts)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_kept_transitions(ctx, sampler, name):
    """thin = 1: mean_u and cov_u equal the float64 recomputation from the call's own samples mapped back to u (atol 1e-13
    for the Langevin samplers, 1e-12 for the ensemble, as test_sample_gpu / test_ensemble_gpu hold this identity; with
    swaps after every transition for every rung of the tempered call); x_last / lnl_last are the last sample bit for bit;
    accept_rate * 12 is an integer (to the rounding of one division) and, without swaps, lies between c and c + 1 for c
    changes of state between consecutive samples.  thin = 4 and 5 store the states [thin - 1::thin][:12 // thin] of the
    thin = 1 run bit for bit, thin = 0 stores none, and all four runs agree bit for bit in everything else."""
    nat = pkg("_native")
    case = sc.BY_NAME[name]
    st, rec = device_stack(ctx, case.dims, case.act)
    tin, flags, din = rec["tin"], flags_of(nat, rec["tin"] is not None), case.dims[0]
    prob = sc.fit_problem(case)
    st.set_likelihood(prob["data"][0], prob["w"])
    n = rows_of(sampler, din)
    x0 = np.ascontiguousarray(sc.chain_starts(case, prob)[:n])
    assert x0.dtype == np.float64
    full = run(st, sampler, x0, flags, 1)
    smp, sl = full["samples"], full["samples_lnl"]
    assert smp.shape == (n, N_STEPS, din) and smp.dtype == np.float64 and sl.shape == (n, N_STEPS)
    # moments against the samples
    us = jr.transform(smp.reshape(-1, din), *tin)[0].reshape(n, N_STEPS, din)
    atol = 1e-12 if sampler == "ensemble" else 1e-13
    mean = us.mean(axis=1)
    cov = np.einsum("nki,nkj->nij", us, us) / N_STEPS - np.einsum("ni,nj->nij", mean, mean)
    print("%s %s: |mean_u - ref| %.2e, |cov_u - ref| %.2e (atol %.0e), accept %.3f"
          % (sampler, name, np.abs(full["mean_u"] - mean).max(), np.abs(full["cov_u"] - cov).max(), atol, full["accept_rate"].mean()))
    np.testing.assert_allclose(full["mean_u"], mean, rtol=0, atol=atol)
    np.testing.assert_allclose(full["cov_u"], cov, rtol=0, atol=atol)
    # the last state
    assert same(full["x_last"], smp[:, -1]) and same(full["lnl_last"], sl[:, -1])
    # the acceptance count
    k = full["accept_rate"] * N_STEPS
    assert np.all(np.abs(k - np.rint(k)) <= 1e-12), k
    if sampler != "tempered":
        c = np.any(smp[:, 1:] != smp[:, :-1], axis=2).sum(axis=1)
        assert np.all((np.rint(k) >= c) & (np.rint(k) <= c + 1)), (k, c)
        assert 0 < c.sum() < n * (N_STEPS - 1)  # (both outcomes occur: the count is not trivially right)
    # thinning
    for thin in (4, 5, 0):
        r = run(st, sampler, x0, flags, thin)
        if thin == 0:
            assert "samples" not in r and "samples_lnl" not in r
        else:
            keep = N_STEPS // thin
            assert r["samples"].shape == (n, keep, din)
            assert same(r["samples"], smp[:, thin - 1::thin][:, :keep]) and same(r["samples_lnl"], sl[:, thin - 1::thin][:, :keep])
        for key in ("mean_u", "cov_u", "accept_rate", "x_last", "lnl_last"):
            assert same(r[key], full[key]), (thin, key)
    st.set_likelihood(None, None)
