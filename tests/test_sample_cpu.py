"""Posterior sampling, host side: Philox4x32-10 and the draw mapping of include/v21.h, the float64 reference sampler
(tests/sample_ref.py) on targets whose law is known -- a Gaussian posterior (a stack without hidden layers) and the uniform
law on the box (all weights zero), with a control that a clamping sampler fails the latter -- the new ABI symbols, r_hat
from moments, and the argument checks of the Python surface that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_ref as sr
from conftest import ROOT, pkg

NEW_SYMBOLS = ("v21_mlp_sample", "v21_mlp_sample_dev")
N_SE = 5.0


def test_philox_known_answers():
    kats = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
            ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
            ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, out in kats:
        assert [int(v) for v in sr.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))] == out
    # batched over counters, and the counter / key layout of a draw block: (chain low, chain high, step, block), (seed low, seed high)
    both = sr.philox4x32_10(np.array([k[0] for k in kats], np.uint64), np.array([k[1] for k in kats], np.uint64))
    assert [[int(v) for v in row] for row in both] == [k[2] for k in kats]
    seed, chain = 0x299f31d0a4093822, 0x85a308d3243f6a88
    assert [int(v) for v in sr.block(seed, np.array([chain], np.uint64), 0x13198a2e, 0x03707344)[0]] == kats[2][2]


def test_draw_mapping():
    chains = np.arange(5, 5 + 4096)
    seed, step = 77, 9
    w0, w1, w2 = (sr.block(seed, chains, step, b) for b in range(3))
    # uniforms: (word + 0.5) 2^-32, inside (0, 1) at both ends of the word range
    assert sr.uniform(np.uint32(0)) == 2.0 ** -33 and sr.uniform(np.uint32(0xFFFFFFFF)) == 1 - 2.0 ** -33
    np.testing.assert_array_equal(sr.accept_uniform(seed, chains, step), (w2[:, 0].astype(np.float64) + 0.5) / 2.0 ** 32)
    # normals: Box-Muller in float64 on the word pairs of blocks 0 and 1
    xi = sr.normals(seed, chains, step, 7)
    assert xi.shape == (4096, 7)
    for b, w in ((0, w0), (1, w1)):
        for h in range(2):
            r = np.sqrt(-2 * np.log((w[:, 2 * h] + 0.5) / 2.0 ** 32))
            th = 2 * np.pi * (w[:, 2 * h + 1] + 0.5) / 2.0 ** 32
            j = 4 * b + 2 * h
            np.testing.assert_array_equal(xi[:, j], r * np.cos(th))
            if j + 1 < 7:
                np.testing.assert_array_equal(xi[:, j + 1], r * np.sin(th))
    # fewer parameters read the same draws; a draw depends on (seed, chain, step, block) only
    np.testing.assert_array_equal(sr.normals(seed, chains, step, 3), xi[:, :3])
    np.testing.assert_array_equal(sr.normals(seed, chains[100:110], step, 7), xi[100:110])
    assert not np.array_equal(sr.normals(seed + 1, chains, step, 7), xi) and not np.array_equal(sr.normals(seed, chains, step + 1, 7), xi)
    # standard normal: 28,672 draws, mean within 5 / sqrt(N), variance within 5 sqrt(2 / N)
    N = xi.size
    assert abs(xi.mean()) < 5 / np.sqrt(N) and abs(xi.var() - 1) < 5 * np.sqrt(2.0 / N)


def test_reference_sampler_on_a_gaussian_posterior():
    """A stack without a hidden layer: y = u W + b, so the posterior is N(u_hat, F^-1) with a constant F, once sigma is
    small enough that the box holds all but a negligible part of it.  256 chains of 100 + 400 transitions (1.5 s): the
    pooled mean and covariance within 5 standard errors taken from the between-chain spread; on the development machine
    the largest deviation is 1.4 standard errors."""
    rng = np.random.default_rng(1)
    d, dout, sigma = 4, 24, 0.2
    W, b = rng.normal(size=(d, dout)), rng.normal(size=dout) * 0.1
    u_hat = rng.uniform(-0.3, 0.3, size=d)
    data, w = u_hat @ W + b, np.full(dout, 1 / sigma ** 2)
    cov = np.linalg.inv((W * w) @ W.T)
    assert np.all(np.abs(u_hat) + 6 * np.sqrt(np.diag(cov)) < 1)
    ev = sr.evaluator_batch([W], [b], [0], data, w)
    r = sr.sample_ref(ev, np.tile(u_hat, (256, 1)), n_steps=400, n_warmup=100, seed=3)
    assert abs(r["accept_rate"].mean() - 0.574) < 0.15, r["accept_rate"].mean()
    _, z = sr.pooled_check(r["mean_u"], u_hat)
    assert np.all(z < N_SE), z
    # per-chain second moments about the known mean: each an unbiased estimate of the covariance
    dm = r["mean_u"] - u_hat
    _, zc = sr.pooled_check(r["cov_u"] + dm[:, :, None] * dm[:, None, :], cov)
    assert np.all(zc < N_SE), zc
    print("Gaussian target: accept %.3f, eps %.3f, max z mean %.2f cov %.2f" % (r["accept_rate"].mean(), r["eps"].mean(), z.max(), zc.max()))


def uniform_target(d=3, dout=8, seed=2):
    W = np.random.default_rng(seed).normal(size=(d, dout))
    return sr.evaluator_batch([W], [np.zeros(dout)], [0], np.zeros(dout), np.zeros(dout))


def uniform_z(r):
    """|pooled mean| and |pooled second moment - 1/3| per coordinate, in standard errors from the between-chain spread"""
    m2 = np.diagonal(r["cov_u"], axis1=1, axis2=2) + r["mean_u"] ** 2
    return sr.pooled_check(r["mean_u"], 0.0)[1], sr.pooled_check(m2, 1.0 / 3.0)[1]


def test_reference_sampler_on_the_uniform_target_and_clamping_control():
    """All weights zero: G = ridge I, a random walk whose stationary law is uniform on the box -- mean 0, variance 1/3 per
    coordinate -- PROVIDED a proposal outside the box is rejected.  The control clips it onto the box instead: mass piles
    up on the faces and the second moment leaves 1/3 by thousands of standard errors."""
    ev = uniform_target()
    u0 = np.random.default_rng(4).uniform(-1, 1, size=(512, 3))
    r = sr.sample_ref(ev, u0, n_steps=500, n_warmup=100, seed=5)
    zm, zv = uniform_z(r)
    assert np.all(zm < N_SE) and np.all(zv < N_SE), (zm, zv)
    assert 0 < r["accept_rate"].mean() < 1 and np.all(np.abs(r["u"]) <= 1)
    bad = sr.sample_ref(ev, u0, n_steps=500, n_warmup=100, seed=5, clamp=True)
    zm_b, zv_b = uniform_z(bad)
    assert np.any(zv_b > 10 * N_SE), zv_b
    print("uniform target: z mean %s var %s; clamping control var %s" % (zm, zv, zv_b))


def test_reference_sampler_bookkeeping():
    ev = uniform_target()
    u0 = np.random.default_rng(6).uniform(-1.5, 1.5, size=(16, 3))
    # thin that does not divide n_steps: n_steps // thin samples, the transitions beyond still enter the moments
    r = sr.sample_ref(ev, u0, n_steps=10, n_warmup=3, thin=4, seed=1)
    full = sr.sample_ref(ev, u0, n_steps=10, n_warmup=3, thin=1, seed=1)
    assert r["samples_u"].shape == (16, 2, 3)
    np.testing.assert_array_equal(r["samples_u"], full["samples_u"][:, [3, 7]])
    np.testing.assert_array_equal(r["mean_u"], full["mean_u"])
    np.testing.assert_allclose(full["mean_u"], full["samples_u"].mean(axis=1), atol=1e-15)
    # n_steps = 0: the clamped start; resumed runs continue the chain
    z = sr.sample_ref(ev, u0, n_steps=0, n_warmup=0)
    np.testing.assert_array_equal(z["u"], np.clip(u0, -1, 1).astype(np.float32))
    a = sr.sample_ref(ev, u0, n_steps=6, n_warmup=0, seed=1)
    b = sr.sample_ref(ev, a["u"], n_steps=6, n_warmup=0, seed=1, step0=6, eps_start=a["eps"])
    c = sr.sample_ref(ev, u0, n_steps=12, n_warmup=0, seed=1)
    np.testing.assert_array_equal(np.concatenate([a["samples_u"], b["samples_u"]], axis=1), c["samples_u"])
    # chains do not depend on the others of the call
    part = sr.sample_ref(ev, u0[5:9], n_steps=10, n_warmup=3, seed=1, chain0=5)
    np.testing.assert_array_equal(part["samples_u"], full["samples_u"][5:9])


def test_r_hat_from_moments_equals_r_hat_from_samples():
    em = pkg("emulator")
    rng = np.random.default_rng(8)
    s = rng.normal(size=(2, 12, 300, 5)) * rng.uniform(0.1, 2, size=5) + rng.normal(size=(2, 12, 1, 5)) * 0.3
    mean_c = s.mean(axis=2)
    cov_c = np.einsum("mcki,mckj->mcij", s - mean_c[:, :, None], s - mean_c[:, :, None]) / 300
    rh = em.r_hat_from_moments(mean_c, cov_c, 300)
    assert rh.shape == (2, 5)
    for m in range(2):
        np.testing.assert_allclose(rh[m], sr.r_hat_from_samples(s[m]), rtol=1e-12)
    assert np.all(rh > 1.0)
    mean, cov = em.pooled_moments(mean_c, cov_c)
    flat = s.reshape(2, 12 * 300, 5)
    np.testing.assert_allclose(mean, flat.mean(axis=1), atol=1e-13)
    for m in range(2):
        np.testing.assert_allclose(cov[m], np.cov(flat[m].T, bias=True), atol=1e-12)
    assert np.all(np.isnan(em.r_hat_from_moments(mean_c[:, :1], cov_c[:, :1], 300)))  # one chain: undefined


def test_new_symbols_declared_and_bound():
    nat = pkg("_native")
    src = open(os.path.join(ROOT, "include", "v21.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in nat.SIGNATURES, name
    types = open(os.path.join(ROOT, "include", "v21_types.h")).read()
    assert "v21_sample_opts" in types and "v21_sample_out" in types
    # the C layout: three ints (+ 4 bytes of padding), three doubles, three 64-bit integers; ten pointers
    assert C.sizeof(nat.SampleOpts) == 64 and nat.SampleOpts.eps0.offset == 16 and nat.SampleOpts.seed.offset == 40
    assert C.sizeof(nat.SampleOut) == 10 * C.sizeof(C.c_void_p)
    for name in nat.SAMPLE_OUTPUTS:
        assert re.search(r"\b%s;" % name, types), name
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("library not built")
    lib = nat.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    # null arguments are refused before any device work
    assert lib.v21_mlp_sample(None, None, 0, 1, None, 0, None, None, None, 0, 0) == -1
    assert lib.v21_mlp_sample_dev(None, None, 7, 1, None, 0, None, None, None, 0, 0) == -1


def _hostless_stack(dims):
    nat = pkg("_native")
    st = nat.Stack.__new__(nat.Stack)
    st.dims, st.act = list(dims), [1] * (len(dims) - 2) + [0]
    st.lib, st.ctx, st.h = None, None, None
    return st


def test_python_surface_validates_arguments():
    nat = pkg("_native")
    st = _hostless_stack([7, 16, 451])
    x = np.zeros((6, 7))
    bad_calls = [dict(x0=np.zeros((6, 5))),                          # wrong parameter count
                 dict(x0=x, data=np.zeros((4, 451))),                # 6 chains over 4 spectra
                 dict(x0=x, data=np.zeros((3, 450))),                # wrong bin count
                 dict(x0=x, eps_start=np.ones(5)),                   # one step size per chain
                 dict(x0=x, eps_start=np.zeros(6)),
                 dict(x0=x, n_steps=-1), dict(x0=x, n_warmup=-1), dict(x0=x, thin=-1), dict(x0=x, n_steps=2.5),
                 dict(x0=x, eps0=0.0), dict(x0=x, eps0=-1.0), dict(x0=x, eps0=np.inf), dict(x0=x, ridge=0.0), dict(x0=x, ridge=-2.0),
                 dict(x0=x, target_accept=0.0), dict(x0=x, target_accept=1.0),
                 dict(x0=x, chain0=-1), dict(x0=x, step0=-1), dict(x0=x, seed=-1), dict(x0=x, step0=2 ** 32 - 1000)]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            st.sample(**kw)
    with pytest.raises(ValueError):
        _hostless_stack([9, 16, 451]).sample(np.zeros((2, 9)))      # at most 8 parameters
    o = nat.Stack.sample_opts(n_steps=3, seed=2 ** 63 + 5)
    assert (o.n_steps, o.n_warmup, o.thin, o.eps0, o.ridge, o.target_accept, o.seed, o.chain0, o.step0) == \
        (3, 200, 1, 1.0, 1.0, 0.574, 2 ** 63 + 5, 0, 0)
