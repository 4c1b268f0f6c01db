"""Parameter Jacobian and Gaussian log-likelihood on the GPU (include/v21.h: v21_mlp_jacobian[_dev], v21_mlp_loglike[_dev]):
fused_jac<Arch, Prec> on the stacks of archs.h and the generic kernel on every other, against the float64 reference of
tests/jacobian_ref.py.  Per-row relative Frobenius error: f32 <= 1e-5 (rows off by more must be explained by ReLU units
at their kink: the reference with every unit of |z| <= 1e-5 max|z| in float64 flipped, at most 0.5 % of the rows), f16 p99 <= 1e-2 / max <= 3e-2, bf16 p99 <=
5e-2 / max <= 1e-1 against the float64 Jacobian taken with the ReLU decisions of the 16-bit primal (jacobian_ref.masks16).  The primal is bit-identical to the forward's fused route."""
import numpy as np
import pytest

import jacobian_ref as jr
from conftest import pkg
from helpers import init_weights
from infer_cases import transforms
from infer_support import check_rows, rows_for, stack_of

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 4, 5, 31, 33, 4099, 65536]
CMP_ROWS = 2048


def subset(n):
    return np.arange(n) if n <= CMP_ROWS else np.unique(np.r_[0, n - 1, np.random.default_rng(n).choice(n, CMP_ROWS - 2, replace=False)])


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "DE", "S3", "S4"])
def test_fused_parity_and_primal_bit_identity(ctx, name, prec):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout = stack_of(ctx, name)
    for k, n in enumerate(ROWS):
        tin_on = dims[0] == 7 and k % 2 == 0
        dtype = np.float64 if k % 4 < 2 else np.float32
        flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | (nat.FWD_OUT_TRANSFORM if k % 3 else 0)
        x = rows_for(dims, n, 10 + k, dtype)
        if dims[0] == 7 and not tin_on:  # without the input transform: rows in the network's own domain [-1, 1]
            x = jr.transform(x, *tin)[0].astype(dtype)
        tag = "%s %s n=%d %s flags=%d" % (name, prec, n, dtype.__name__, flags)
        y, jac = st.jacobian(x, prec, flags, return_outputs=True)
        assert st.last_jac_route()[0] == "fused", tag
        assert jac.shape == (n, dims[0], dims[-1]) and np.all(np.isfinite(jac)) and np.all(np.isfinite(y)), tag
        yf = st.forward(x, prec, flags | nat.FWD_NO_SMALL)
        assert np.array_equal(y.view(np.uint32), yf.view(np.uint32)), tag
        idx = subset(n)
        to = tout if flags & nat.FWD_OUT_TRANSFORM else None
        xs = x[idx]
        yr, Jr = jr.jacobian(Ws, bs, act, xs, tin if tin_on else None, to)
        xt = jr.transform(xs, *tin)[0] if tin_on else xs.astype(np.float64)
        check_rows(tag, prec, jac[idx], Jr, Ws, bs, act, xt, tin_on, xs, tin, to)


def test_guard_region_and_device_entry_points(ctx):
    """v21_mlp_jacobian_dev / v21_mlp_loglike_dev on tile, wave and workgroup edges: the bytes past row n stay as they were"""
    nat = pkg("_native")
    for name, prec in (("D1", "f16"), ("S4", "f32"), ("S3", "bf16"), ("NB", "f32")):
        st, dims, act, *_ = stack_of(ctx, name)
        din, dout = dims[0], dims[-1]
        st.set_likelihood(np.zeros(dout, np.float32), np.ones(dout, np.float32))
        for n in (3, 33, 4099):
            x = rows_for(dims, n, 3, np.float32)
            g = 64
            dx, dy, dj = ctx.malloc(x.nbytes), ctx.malloc((n + g) * dout * 4), ctx.malloc((n + g) * din * dout * 4)
            dl, dg = ctx.malloc((n + g) * 4), ctx.malloc((n + g) * din * 4)
            try:
                ctx.h2d(dx, x)
                for p, nb in ((dy, (n + g) * dout * 4), (dj, (n + g) * din * dout * 4), (dl, (n + g) * 4), (dg, (n + g) * din * 4)):
                    ctx.memset(p, 0x7F, nb)
                st.jacobian_dev(dx, din, n, dy, dout, dj, prec, 0)
                st.loglike_dev(dx, din, n, dl, dg, prec, 0)
                ctx.sync()
                y = np.empty((n + g, dout), np.float32); ctx.d2h(y, dy)
                j = np.empty((n + g, din, dout), np.float32); ctx.d2h(j, dj)
                lnl = np.empty(n + g, np.float32); ctx.d2h(lnl, dl)
                gr = np.empty((n + g, din), np.float32); ctx.d2h(gr, dg)
                poison = np.frombuffer(b"\x7f\x7f\x7f\x7f", np.uint32)[0]
                for a in (y, j, lnl, gr):
                    assert np.all(a[n:].view(np.uint32) == poison), (name, prec, n)
                    assert np.all(np.isfinite(a[:n])), (name, prec, n)
                yh, jh = st.jacobian(x, prec, 0, return_outputs=True)
                assert np.array_equal(yh, y[:n]) and np.array_equal(jh, j[:n]), (name, prec, n)
            finally:
                for p in (dx, dy, dj, dl, dg):
                    ctx.free(p)
        st.set_likelihood(None, None)


@pytest.mark.parametrize("n", [8193, 16385])
@pytest.mark.parametrize("name,prec", [("D1", "f16"), ("NB", "f32")])
def test_host_and_device_entry_points_agree(ctx, name, prec, n):
    """each host form (chunks of 8,192 rows) equals its _dev form (rows of pitch in_dim + 3, one call) bit for bit across
    a host chunk and a 16,384-row workspace slice, on a fused and a generic stack; every call counts its route once and
    the bytes past row n of the _dev outputs stay as they were"""
    nat = pkg("_native")
    st, dims, act, *_ = stack_of(ctx, name)
    din, dout = dims[0], dims[-1]
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    route = "fused" if name == "D1" else "generic"
    rng = np.random.default_rng(7)
    st.set_likelihood(rng.normal(size=dout).astype(np.float32), np.where(rng.uniform(size=dout) < 0.2, 0, 4.0).astype(np.float32))
    x = rows_for(dims, n, 11, np.float32)
    xp = np.zeros((n, din + 3), np.float32)
    xp[:, :din] = x
    g = 64
    sizes = {"x": xp.nbytes, "y": (n + g) * dout, "jac": (n + g) * din * dout, "lnl": n + g, "grad": (n + g) * din,
             "F": (n + g) * din * din, "xh": (n + g) * din, "lnl0": n + g, "status": n + g}
    d = {}
    counts = lambda: st.last_jac_route()[1].get(route, 0)

    def out(key, shape, dtype=np.float32):
        a = np.empty(shape, dtype)
        ctx.d2h(a, d[key])
        return a

    def poisoned(a):
        return np.all(a[n:].view(np.uint32) == np.frombuffer(b"\x7f\x7f\x7f\x7f", np.uint32)[0])

    try:
        for k, v in sizes.items():
            d[k] = ctx.malloc(v if k == "x" else v * 4)
            if k != "x":
                ctx.memset(d[k], 0x7F, v * 4)
        ctx.h2d(d["x"], xp)
        c0 = counts()
        st.jacobian_dev(d["x"], din + 3, n, d["y"], dout, d["jac"], prec, flags)
        st.loglike_dev(d["x"], din + 3, n, d["lnl"], d["grad"], prec, flags)
        ctx.sync()
        assert counts() - c0 == 2
        y, j = out("y", (n + g, dout)), out("jac", (n + g, din, dout))
        lnl, gr = out("lnl", n + g), out("grad", (n + g, din))
        for a in (y, j, lnl, gr):
            assert poisoned(a)
        c0 = counts()
        yh, jh = st.jacobian(x, prec, flags, return_outputs=True)
        assert np.array_equal(yh, y[:n]) and np.array_equal(jh, j[:n])
        lh, gh = st.loglike(x, prec, flags)
        assert np.array_equal(lh, lnl[:n]) and np.array_equal(gh, gr[:n])
        assert counts() - c0 == 2
        for k in ("lnl", "grad"):
            ctx.memset(d[k], 0x7F, sizes[k] * 4)
        c0 = counts()
        st.fisher_dev(d["x"], din + 3, n, d["F"], d["lnl"], d["grad"], prec, flags)
        ctx.sync()
        assert counts() - c0 == 1
        F, lnl, gr = out("F", (n + g, din, din)), out("lnl", n + g), out("grad", (n + g, din))
        for a in (F, lnl, gr):
            assert poisoned(a)
        c0 = counts()
        Fh, lh, gh = st.fisher(x, prec, flags, lnl=True, grad=True)
        assert counts() - c0 == 1
        assert np.array_equal(Fh, F[:n]) and np.array_equal(lh, lnl[:n]) and np.array_equal(gh, gr[:n])
        for k in ("F", "lnl"):
            ctx.memset(d[k], 0x7F, sizes[k] * 4)
        c0 = counts()
        st.fit_dev(d["x"], din + 3, n, None, 0, d["xh"], d["lnl"], d["lnl0"], d["F"], d["status"], prec, flags, max_iter=5,
                   check_every=2)
        ctx.sync()
        assert counts() - c0 == 2
        xh, lnl, l0 = out("xh", (n + g, din)), out("lnl", n + g), out("lnl0", n + g)
        F, ss = out("F", (n + g, din, din)), out("status", n + g, np.int32)
        for a in (xh, lnl, l0, F, ss):
            assert poisoned(a)
        c0 = counts()
        r = st.fit(x, prec, flags, max_iter=5, check_every=2, fisher=True)
        assert counts() - c0 == 2
        for key, a in (("x_hat", xh), ("lnl", lnl), ("lnl_start", l0), ("fisher", F), ("status", ss)):
            assert np.array_equal(r[key].view(np.uint8), a[:n].view(np.uint8)), key
        assert np.all(np.isfinite(r["lnl"])) and np.all(r["lnl"] >= r["lnl_start"])
    finally:
        for p in d.values():
            ctx.free(p)
        st.set_likelihood(None, None)


@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["D1", "S3", "S4", "NB"])
def test_loglike(ctx, name, prec):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout = stack_of(ctx, name)
    dout = dims[-1]
    tin_on = dims[0] == 7
    flags = (nat.FWD_IN_TRANSFORM if tin_on else 0) | nat.FWD_OUT_TRANSFORM
    to = tout
    x = rows_for(dims, 4099, 21, np.float64)
    rng = np.random.default_rng(2)
    data = (jr.jacobian(Ws, bs, act, x[:1], tin if tin_on else None, to)[0][0] + rng.normal(size=dout) * 0.05 * tout[0]).astype(np.float32)
    w = np.where(rng.uniform(size=dout) < 0.25, 0.0, 1.0 / (0.05 * tout[0]) ** 2).astype(np.float32)
    st.set_likelihood(data, w)
    lnl, g = st.loglike(x, prec, flags)
    assert lnl.shape == (4099,) and g.shape == (4099, dims[0])
    # the fused reduction alone: the device's own y and jac, reduced in float64
    y, jac = st.jacobian(x, prec, flags, return_outputs=True)
    l64, g64 = jr.loglike(y, jac, data, w)
    np.testing.assert_allclose(lnl, l64, rtol=1e-5, atol=0)
    # (a sum with cancellation: relative to the sum of the terms' magnitudes)
    scale = np.einsum("nk,njk->nj", np.abs(w * (data - y.astype(np.float64))), np.abs(jac.astype(np.float64)))
    assert np.all(np.abs(g - g64) <= 1e-5 * scale), np.max(np.abs(g - g64) / scale)
    # against float64
    idx = subset(4099)
    yr, Jr = jr.jacobian(Ws, bs, act, x[idx], tin if tin_on else None, to)
    lr, gr = jr.loglike(yr, Jr, data, w)
    tol = {"f32": 1e-4, "f16": 3e-2, "bf16": 1e-1}[prec]
    assert np.median(np.abs(lnl[idx] - lr) / np.abs(lr)) <= tol
    assert np.median(jr.rel_frobenius(g[idx], gr)) <= tol
    # data in bins with w == 0 do not enter
    data2 = data.copy()
    data2[w == 0] = 1e30
    st.set_likelihood(data2, w)
    lnl2, g2 = st.loglike(x, prec, flags)
    assert np.array_equal(lnl2.view(np.uint32), lnl.view(np.uint32)) and np.array_equal(g2.view(np.uint32), g.view(np.uint32))
    st.set_likelihood(None, None)


@pytest.mark.parametrize("K", [0, 5])
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_loglike_is_fisher_without_F(ctx, prec, K):
    """on the fused route loglike and fisher(lnl, grad) are one reduction (jac_reduce_kernel) that differs only in whether
    F is formed: ln L and its gradient agree bit for bit, without a nuisance record and with K = 5 modes (5 rows: one
    full workgroup of the reduction and one row)"""
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout = stack_of(ctx, "D1")
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    x = rows_for(dims, 5, 23, np.float32)
    rng = np.random.default_rng(4)
    data = (jr.jacobian(Ws, bs, act, x[:1], tin, tout)[0][0] + rng.normal(size=dims[-1]) * 0.05 * tout[0]).astype(np.float32)
    w = np.where(rng.uniform(size=dims[-1]) < 0.25, 0.0, 1.0 / (0.05 * tout[0]) ** 2).astype(np.float32)
    st.set_likelihood(data, w)
    try:
        if K:
            st.set_nuisance(pkg("foregrounds").linlog_basis(np.linspace(50.0, 200.0, dims[-1]), K))
        lnl, g = st.loglike(x, prec, flags)
        assert st.last_jac_route()[0] == "fused"
        _, lnl_f, g_f = st.fisher(x, prec, flags, lnl=True, grad=True)
        assert np.all(np.isfinite(lnl)) and np.all(np.isfinite(g))
        assert np.array_equal(lnl.view(np.uint32), lnl_f.view(np.uint32))
        assert np.array_equal(g.view(np.uint32), g_f.view(np.uint32))
    finally:
        st.set_likelihood(None, None)


@pytest.mark.parametrize("name", ["NB", "W6", "VG"])
def test_generic_route_parity(ctx, name):
    nat = pkg("_native")
    st, dims, act, Ws, bs, tin, tout = stack_of(ctx, name)
    for n, prec in ((1, "f16"), (33, "f32"), (1500, "f32")):
        x = rows_for(dims, n, 7, np.float32)
        flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
        y, jac = st.jacobian(x, prec, flags, return_outputs=True)
        assert st.last_jac_route()[0] == "generic"
        yr, Jr = jr.jacobian(Ws, bs, act, x, tin, (tout[0], tout[1]))
        xt = jr.transform(x, *tin)[0]
        check_rows("%s generic n=%d" % (name, n), "f32", jac, Jr, Ws, bs, act, xt, True, x, tin, (tout[0], tout[1]))
        np.testing.assert_allclose(y, yr, rtol=1e-5, atol=2e-5 * tout[0])
    _, counts = st.last_jac_route()
    assert set(counts) == {"generic"}


def test_generic_route_of_a_stack_ending_in_relu(ctx):
    """a stack whose output layer is a ReLU (the engine's Dense accepts it; predict evaluates it): y is the forward's, the
    Jacobian and ln L gradient carry the output layer's mask"""
    nat = pkg("_native")
    dims, act = [7, 64, 128, 451], [1, 1, 1]
    Ws, bs, _ = init_weights(dims, 4)
    st = nat.Stack(ctx, dims, act)
    st.set_weights(jr.ora.flatten_params(Ws, bs))
    tin, tout, _ = transforms(5)
    st.set_input_transform(*tin)
    st.set_output_transform(tout[0], tout[1].astype(np.float32))
    flags = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    assert nat.route_jacobian(dims, act, "f32", 100, flags) == "generic"
    x = rows_for(dims, 300, 9, np.float64)
    y, jac = st.jacobian(x, "f32", flags, return_outputs=True)
    assert st.last_jac_route()[0] == "generic"
    yr, Jr = jr.jacobian(Ws, bs, act, x, tin, tout)
    off = jr.forward(Ws, bs, act, jr.transform(x, *tin)[0]) <= 0
    assert off.any(axis=1).all()  # every row has output bins the ReLU switches off
    np.testing.assert_allclose(y, yr, rtol=1e-5, atol=2e-5 * tout[0])
    np.testing.assert_allclose(y, st.forward(x, "f32", flags), rtol=1e-5, atol=2e-5 * tout[0])
    check_rows("relu output", "f32", jac, Jr, Ws, bs, act, jr.transform(x, *tin)[0], True, x, tin, tout)
    data = yr[0].astype(np.float32)
    w = np.full(451, 1.0 / (0.05 * tout[0]) ** 2, np.float32)
    st.set_likelihood(data, w)
    lnl, g = st.loglike(x, "f32", flags)
    lr, gr = jr.loglike(yr, Jr, data, w)
    np.testing.assert_allclose(lnl, lr, rtol=1e-4, atol=1e-3)
    scale = np.einsum("nk,njk->nj", np.abs(w * (data - yr)), np.abs(Jr))
    assert np.all(np.abs(g - gr) <= 1e-4 * scale + 1e-6 * np.abs(gr).max())


def test_emulator_class_surface(shipped):
    emulator, synth = pkg("emulator"), pkg("synth")
    data = synth.make_dataset(n_train=3000, n_val=50, n_test=200, seed=11)
    ps = pkg("preprocess").ParamStats(data["par_train"])
    tin = (ps.log_mask, ps.zero_floor, ps.lo, ps.hi)
    tout = (float(np.std(data["signal_train"])), np.mean(data["signal_train"], axis=0))
    # DirectEmulator (untrained: the default stack, initial weights)
    de = emulator.DirectEmulator(**data)
    pars = data["par_test"][:40].copy()
    pars[3, 2] = 0.0  # fx == 0: the derivative at the floor
    J1 = de.jacobian(pars[0])
    assert J1.shape == (451, 7)
    sig, J = de.jacobian(pars, return_signal=True)
    assert J.shape == (40, 451, 7) and sig.shape == (40, 451)
    np.testing.assert_allclose(sig, de.predict(pars), rtol=1e-5, atol=2e-5 * tout[0])
    st = de.emulator._ensure_stack()
    Ws, bs = jr.ora.unflatten_params(st.get_weights(), st.dims)
    _, Jr = jr.jacobian(Ws, bs, st.act, pars, tin, tout)
    xt = jr.transform(pars, *tin)[0]
    check_rows("DirectEmulator", "f32", J.transpose(0, 2, 1), Jr, Ws, bs, st.act, xt, True, pars, tin, tout)
    assert np.abs(J[3, :, 2]).max() > 0
    # AutoEncoderEmulator on the reference's trained weights
    ae = emulator.AutoEncoderEmulator(**data)
    ae.load_model()
    em, dec = shipped["ae_emulator"], shipped["decoder"]
    Ws, bs = list(em[0]) + list(dec[0]), list(em[1]) + list(dec[1])
    act = [1, 1, 1, 1, 0, 1, 1, 0]
    Ja = ae.jacobian(pars)
    _, Jr = jr.jacobian(Ws, bs, act, pars, tin, tout)
    check_rows("AutoEncoderEmulator", "f32", Ja.transpose(0, 2, 1), Jr, Ws, bs, act, xt, True, pars, tin, tout)
    # log_likelihood over a band, with its gradient
    d = data["signal_test"][0]
    sigma = np.full(451, 0.02) + 0.01 * np.arange(451) / 451
    flow, fhigh = 60.0, 160.0
    lnl, g = ae.log_likelihood(pars, d, sigma, flow=flow, fhigh=fhigh, grad=True)
    nu = np.asarray(ae.frequencies)
    w = np.where((nu >= flow) & (nu <= fhigh), 1.0 / sigma ** 2, 0.0)
    yr, Jr = jr.jacobian(Ws, bs, act, pars, tin, tout)
    lr, gr = jr.loglike(yr, Jr, d, w)
    np.testing.assert_allclose(lnl, lr, rtol=1e-4)
    scale = np.einsum("nk,njk->nj", np.abs(w * (d - yr)), np.abs(Jr))
    assert np.all(np.abs(g - gr) <= 1e-4 * scale), np.max(np.abs(g - gr) / scale)
    l0 = ae.log_likelihood(pars[0], d, 0.05)
    assert np.ndim(l0) == 0
