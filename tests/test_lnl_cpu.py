"""Forward-only log-likelihood, host side (no GPU): the route decision (csrc/routes.h: decide_loglike_fwd through
v21_route_loglike_fwd), the argument errors that need no device, ``LogPosterior`` on a numpy stub of ``Stack.loglike_fwd``
and the mutation catalogue of tests/lnl_ref.py against the documented parity bound."""
import types

import numpy as np
import pytest

import lnl_ref as lr
import shape_cases as sc
from conftest import pkg
from helpers import STACKS
from infer_cases import ARCHS, VG


def test_route_table():
    nat = pkg("_native")
    F = nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM
    arch, other = ARCHS["S1"], STACKS["NB"]
    relu_end = sc.BY_NAME["i8relu"]
    table = [
        # stack, n, n_data, K, flags -> route
        (arch, 65536, 0, 0, F, "fused"),            # the record
        (arch, 1, 0, 0, 0, "fused"),                # any n: there is no few-row route
        (arch, 384, 3, 0, F, "fused"),              # 128 rows per spectrum: one data row per workgroup
        (arch, 390, 3, 0, F, "two_launch"),         # 130 rows per spectrum
        (arch, 65536, 0, 4, F, "two_launch"),       # a nuisance record
        (arch, 384, 3, 4, F, "two_launch"),
        (arch, 65536, 0, 0, F | nat.FWD_FORCE_GENERIC, "two_launch"),
        (arch, 65536, 0, 0, F | nat.FWD_FORCE_CHAIN, "two_launch"),
        (ARCHS["S4"], 129, 0, 0, nat.FWD_OUT_TRANSFORM, "fused"),
        (ARCHS["S3"], 256, 2, 0, F, "fused"),
        (ARCHS["S2"], 4099, 0, 0, F, "fused"),
        (other, 65536, 0, 0, F, "two_launch"),      # outside archs.h
        (other, 384, 3, 0, F, "two_launch"),
        (other, 65536, 0, 4, F, "two_launch"),
        ((relu_end.dims, relu_end.act), 9, 0, 0, 0, "two_launch"),  # ends in a ReLU
        (VG, 4099, 0, 0, F, "two_launch"),          # V21_ACT_GAUSS
    ]
    for (dims, act), n, nd, K, flags, want in table:
        for prec in ("f32", "f16", "bf16"):
            assert nat.route_loglike_fwd(dims, act, prec, n, nd, K, flags) == want, (dims, n, nd, K, flags, prec)
    assert nat.LNL_ROUTES == {1: "fused", 2: "two_launch"}


def test_argument_errors():
    """the argument errors that need no device.  "No record set" (V21_ERR_STATE) needs a handle, and a handle needs a
    GPU: that case is in tests/test_lnl_gpu.py::test_state_errors_and_empty_calls, deliberately not here."""
    nat = pkg("_native")
    dims, act = ARCHS["S1"]
    with pytest.raises(nat.EngineError, match="n_data"):
        nat.route_loglike_fwd(dims, act, "f32", 385, 3)             # n % n_data != 0
    with pytest.raises(nat.EngineError):
        nat.route_loglike_fwd(dims, act, "f32", 384, 3, n_modes=9)
    with pytest.raises(ValueError):
        nat.route_loglike_fwd(dims, act, "f64", 384)
    # the binding refuses rows that are no whole spectra before the library sees them
    st = object.__new__(nat.Stack)
    st.dims = list(dims)
    with pytest.raises(ValueError, match="multiple"):
        st.loglike_fwd(np.zeros((5, 7), np.float32), data=np.zeros((2, 451), np.float32))
    with pytest.raises(ValueError, match="data must be"):
        st.loglike_fwd(np.zeros((4, 7), np.float32), data=np.zeros((2, 450), np.float32))
    # forward_only computes no gradient
    em = object.__new__(pkg("emulator")._EmulatorBase)
    with pytest.raises(ValueError, match="forward_only"):
        em.log_likelihood(np.zeros(7), np.zeros(451), 1.0, grad=True, forward_only=True)
    # a data matrix of the wrong width is refused before anything else is looked at
    em.signal_train, em.par_labels = np.zeros((2, 451)), list(range(7))
    with pytest.raises(ValueError, match="data must be"):
        em.log_likelihood(np.zeros((4, 7)), np.zeros((2, 450)), 1.0, forward_only=True)
    with pytest.raises(ValueError, match="need data of shape"):
        em.log_likelihood(np.zeros((2, 2, 7)), np.zeros(451), 1.0, forward_only=True)


class _StubStack:
    """what LogPosterior and log_likelihood(forward_only=True) touch of a Stack, with Stack's own use_* record logic"""

    def __init__(self, nat):
        self.dims = [7, 451]
        self.lk_record = self.nu_record = None
        self.uploads, self.calls, self.rows_seen = 0, 0, []
        self.use_likelihood = types.MethodType(nat.Stack.use_likelihood, self)
        self.use_nuisance = types.MethodType(nat.Stack.use_nuisance, self)

    def set_likelihood(self, d, w):
        self.uploads += 1

    def set_nuisance(self, basis):
        raise AssertionError("no foreground in this test")

    def nuisance_modes(self):
        return 0

    def loglike_fwd(self, x, precision="f32", flags=0, data=None):
        self.calls += 1
        self.rows_seen.append(np.array(x))
        base = -np.sum(np.asarray(x, np.float64) ** 2, axis=1)
        if data is not None:
            R = x.shape[0] // data.shape[0]
            base = base + np.repeat(np.asarray(data, np.float64)[:, 0], R)
        return base.astype(np.float32)


def _stub_emulator():
    nat, emu, synth = pkg("_native"), pkg("emulator"), pkg("synth")
    em = object.__new__(emu._EmulatorBase)
    em.par_labels = list(emu._EmulatorBase.par_labels)
    em.par_train = synth.make_params(2000, seed=5, corners=True)
    em.frequencies = None
    em.signal_train = np.zeros((2, 451), np.float32)
    st = _StubStack(nat)
    model = types.SimpleNamespace(precision="f16")
    em._diff_stack = lambda params: (model, st, 3, np.array(params, np.float64, ndmin=2))
    return em, st


def test_log_posterior_on_a_stub():
    pp = pkg("preprocess")
    em, st = _stub_emulator()
    lp = em.log_posterior(np.zeros(451, np.float32), 0.5)
    assert st.uploads == 1 and st.calls == 0
    centre = lp.prior_transform(0.5 * np.ones(7))
    assert centre.shape == (7,) and np.allclose(pp.par_transform(centre, em.par_train), 0.0, atol=1e-12)
    assert np.array_equal(centre, pp.par_untransform(np.zeros(7), em.par_train)[0])
    cube = np.random.default_rng(1).uniform(size=(64, 7))
    theta = lp.prior_transform(cube)
    assert theta.shape == (64, 7) and theta.dtype == np.float64
    assert np.allclose(pp.par_transform(theta, em.par_train), 2 * cube - 1, atol=1e-9)  # uniform in u
    # one vector -> a float, rows -> (n,) float64
    v = lp(centre)
    assert isinstance(v, float) and v == float(np.float32(-np.sum(centre ** 2)))
    out = lp(theta)
    assert out.shape == (64,) and out.dtype == np.float64 and np.all(np.isfinite(out))
    # rows outside the box: -inf, and never handed to the stack
    bad = theta[:6].copy()
    u = pp.par_transform(bad, em.par_train)
    lo, hi = pp.par_untransform(-1.05 * np.ones(7), em.par_train)[0], pp.par_untransform(1.05 * np.ones(7), em.par_train)[0]
    bad[0, 3] = hi[3]; bad[1, 0] = lo[0]; bad[2, 5] = np.nan; bad[3, 1] = -1.0  # (a negative value in a log10 column)
    calls = st.calls
    got = lp(bad)
    assert np.all(got[:4] == -np.inf) and np.all(np.isfinite(got[4:])) and st.calls == calls + 1
    assert st.rows_seen[-1].shape == (2, 7) and np.array_equal(st.rows_seen[-1], bad[4:])
    calls = st.calls
    assert lp(bad[0]) == -np.inf and np.all(lp(bad[:4]) == -np.inf) and st.calls == calls  # no device call at all
    assert np.all(np.abs(u[4:]) <= 1)
    with pytest.raises(ValueError):
        lp(np.zeros((3, 6)))
    # the record is uploaded once, however often the object is called -- and again only after another call replaced it
    assert st.uploads == 1
    em.log_likelihood(centre, np.ones(451, np.float32), 0.5, forward_only=True)
    assert st.uploads == 2
    lp(centre)
    assert st.uploads == 3
    lp(centre)
    assert st.uploads == 3


def test_forward_only_shapes_on_a_stub():
    em, st = _stub_emulator()
    x = em.log_posterior(np.zeros(451), 1.0).prior_transform(np.random.default_rng(2).uniform(size=(6, 7)))
    one = em.log_likelihood(x[0], np.zeros(451), 1.0, forward_only=True)
    assert np.ndim(one) == 0
    assert em.log_likelihood(x, np.zeros(451), 1.0, forward_only=True).shape == (6,)
    data = np.zeros((3, 451), np.float32)
    data[:, 0] = (100.0, 200.0, 300.0)
    b = em.log_likelihood(x, data, 1.0, forward_only=True)  # (R, 7) scored against every spectrum
    assert b.shape == (3, 6)
    assert np.allclose(b - b[:1], np.array([[0.0], [100.0], [200.0]]), atol=1e-3)
    p = em.log_likelihood(x.reshape(3, 2, 7), data, 1.0, forward_only=True)  # block m against spectrum m
    assert p.shape == (3, 2)
    assert np.allclose(p[:, 0], b[[0, 1, 2], [0, 2, 4]])
    # 2-D params always broadcast, also when their row count is a multiple of the spectra
    assert em.log_likelihood(x[:3], data, 1.0, forward_only=True).shape == (3, 3)
    with pytest.raises(ValueError):
        em.log_likelihood(x.reshape(2, 3, 7), data, 1.0, forward_only=True)


def test_mutation_catalogue_bites():
    """every mutation of lnl_ref.MUTATIONS moves the float64 ln L of a numpy y by more than 16x the documented bound
    (4x what the GPU test asks of it at 4x the bound) at 33 and at 4,099 rows, so the parity test sees each of them"""
    rng = np.random.default_rng(11)
    k = np.arange(451)
    mean = -60.0 + 40.0 * np.sin(0.02 * k)
    std = 55.0
    for n in (33, 4099):
        amp = rng.uniform(0.2, 2.0, size=(n, 1))
        y = mean + std * amp * np.sin(0.013 * k * rng.uniform(0.5, 2.0, size=(n, 1)) + rng.uniform(0, 6.28, size=(n, 1)))
        for zero_tail in (False, True):
            d, w = lr.record(y[0], std, 3, zero_tail)
            ref = lr.lnl64(y, d, w)
            assert np.all(ref < 0) and np.all(np.isfinite(ref))
            # the reference itself skips what carries no weight
            d2 = d.copy()
            d2[np.flatnonzero(w == 0)[:3]] = np.inf
            assert np.array_equal(lr.lnl64(y, d2, w), ref)
            eff = lr.mutation_effects(y, d, w, mean)
            assert set(eff) == {"drop_bin", "pad_bins", "half_swap", "tile_twice", "neighbour_w"}
            for name, e in eff.items():
                assert e > 16 * lr.LNL_FWD_TOL, (name, n, zero_tail, e)


def _llvm_bin():
    import os
    import shutil
    cands = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        cands.append(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin"))
    for c in cands:
        if all(os.path.exists(os.path.join(c, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")):
            return c
    return None


@pytest.mark.parametrize("obj", ["lnl_S1_F16x2spLnl", "lnl_S3_F16x2spLnl"])
def test_data_loads_sit_at_one_seam_of_the_built_kernel(obj, tmp_path):
    """The ln L variant keeps its d / w loads out of the ring's counted waits by WHERE they are: issued together right
    before the output layer, and waited for by the compiler before any later ring rendezvous (csrc/fused_fwd.h: lnl_load
    / lnl_pin).  A compiler that moved them would break that silently, so the built object is
    read: inside the MFMA stream every plain global load lies in one group of 15 (one per output tile), every wait the
    compiler placed (a vmcnt wait that no barrier follows) lies between that group and the next ring rendezvous (a vmcnt
    wait followed by s_barrier), and nothing goes through scratch memory."""
    import os
    import subprocess
    from conftest import ROOT
    path = os.path.join(ROOT, "21cmvae_amd", "csrc", "build", obj + ".o")
    tools = _llvm_bin()
    if tools is None or not os.path.exists(path):
        pytest.skip("no LLVM binutils or no built object to read")
    fb, co = str(tmp_path / "fb"), str(tmp_path / "dev.co")
    subprocess.run([os.path.join(tools, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, path], check=True)
    subprocess.run([os.path.join(tools, "clang-offload-bundler"), "--unbundle", "--type=o",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co], check=True)
    text = subprocess.run([os.path.join(tools, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    ins = [l.split("//")[0].split() for l in text.splitlines() if l.startswith("\t")]
    ins = [i for i in ins if i]
    mfma = [k for k, i in enumerate(ins) if i[0].startswith("v_mfma")]
    assert len(mfma) > 100
    body = ins[mfma[0]:mfma[-1] + 1]
    assert not any(i[0].startswith("scratch_") for i in ins), "the kernel spills"
    loads = [k for k, i in enumerate(body) if i[0].startswith("global_load_dword") and "lds" not in i[0]]
    assert len(loads) == 15, len(loads)  # one register per output tile: 451 bins = 15 tiles of 32
    assert loads[-1] - loads[0] < 64, "the d / w loads are no longer issued together"
    vm = [k for k, i in enumerate(body) if i[0] == "s_waitcnt" and any(a.startswith("vmcnt") for a in i[1:])]
    ring = [k for k in vm if body[k + 1][0] == "s_barrier"]
    own = [k for k in vm if body[k + 1][0] != "s_barrier"]
    assert len(ring) >= 4 and own, (len(ring), len(own))
    next_ring = min(k for k in ring if k > loads[-1])
    assert all(loads[-1] < k < next_ring for k in own), "a wait of the compiler's outside the seam"
    assert any("vmcnt(0)" in body[k] for k in own), "the loads are not drained before the next rendezvous"
