"""The ln L variant of fused_fwd<ArchRT, Prec> instantiated at run time (csrc/jit.hip: kJitLnl) where no GPU
is needed: the route table with and without a handle that asked (csrc/routes.h: decide_loglike_fwd / decide_ensemble
through the route queries), who may have the kernel and why not (jit_lnl_eligible through v21_jit_prebuild), that every
case of tests/lnlrt_cases.py compiles through the child compiler without scratch memory and keeps its d / w loads where
K12's accounting needs them, that the other three kinds' cached objects keep their names, the new symbols, and the
mutation catalogue at these shapes."""
import ctypes.util
import os
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lnl_ref as lr
import lnlrt_cases as lc
from conftest import ROOT, pkg

HAVE_HIPRTC = os.path.exists("/opt/rocm/lib/libhiprtc.so") or ctypes.util.find_library("hiprtc") is not None
S1 = ([7, 352, 352, 352, 224, 451], [1, 1, 1, 1, 0])
S4 = ([9, 32, 352, 451], [1, 1, 0])
NINE = ([9, 40, 37], [3, 0])   # a 9-input stack outside archs.h, beside S4
FORM = {"f32": "PrecF32Lnl", "f16": "PrecF16x2spLnl", "bf16": "PrecBF16x2spLnl"}


# ---- the route table
def _old_rule(compiled, in_dim, n_modes, rpd, n, flags, nat):
    """decide_loglike_fwd as it stood before route 3"""
    forced = flags & (nat.FWD_FORCE_GENERIC | nat.FWD_FORCE_CHAIN | nat.FWD_FORCE_JIT)
    tin_ok = not (flags & nat.FWD_IN_TRANSFORM) or in_dim <= 8
    uniform = rpd == 0 or rpd % 128 == 0
    return "fused" if compiled and not forced and tin_ok and n_modes == 0 and uniform and n // 128 < 2 ** 31 else "two_launch"


def test_route_table_with_and_without_a_handle_that_asked():
    nat = pkg("_native")
    assert nat.LNL_ROUTES_RT == {1: "fused", 2: "two_launch", 3: "fused_rt"} and 3 not in nat.LNL_ROUTES
    flag_sets = (0, nat.FWD_IN_TRANSFORM, nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM, nat.FWD_FORCE_GENERIC, nat.FWD_FORCE_CHAIN,
                 nat.FWD_FORCE_JIT, nat.FWD_NO_SMALL)
    seen = set()
    for (compiled, custom) in ((S1, lc.NB), (S4, NINE)):
        for modes in (0, 3):
            for n, n_data in ((1, 0), (257, 0), (384, 3), (390, 3), (128 * 2 ** 31, 0), (256, 2), (256, 4)):
                for flags in flag_sets:
                    args = (n, n_data, modes, flags)
                    rpd = n // n_data if n_data else 0
                    base_c = nat.route_loglike_fwd(*compiled, "f16", *args)
                    base_u = nat.route_loglike_fwd(*custom, "f32", *args)
                    # without rt_ready: what the rule always gave
                    assert base_c == _old_rule(True, compiled[0][0], modes, rpd, n, flags, nat), (compiled[0], args)
                    assert base_u == "two_launch", (custom[0], args)
                    # with it: 3 exactly where a compiled stack says 1; a compiled stack keeps its kernel
                    assert nat.route_loglike_fwd_rt(*custom, "f32", *args) == ("fused_rt" if base_c == "fused" else "two_launch"), (custom[0], args)
                    assert nat.route_loglike_fwd_rt(*compiled, "f16", *args) == base_c, (compiled[0], args)
                    seen.add(base_c)
    assert seen == {"fused", "two_launch"}
    # the samplers: the same through decide_ensemble, chunk arithmetic included (S1 against NB: 7 inputs both)
    for modes in (0, 2):
        for n, W, n_data in ((8208, 16, 0), (512, 256, 2), (520, 260, 2), (16384, 16, 2), (48 * 400, 48, 400), (1024, 512, 0)):
            for host_form in (False, True):
                for flags in (0, nat.FWD_OUT_TRANSFORM, nat.FWD_FORCE_JIT, nat.FWD_FORCE_GENERIC):
                    args = (n, W, n_data, modes, flags, host_form)
                    c = nat.route_ensemble(*S1, "f16", *args)
                    assert nat.route_ensemble(*lc.NB, "f16", *args)[0] == "two_launch", args
                    assert nat.route_ensemble_rt(*S1, "f16", *args) == c, args
                    got = nat.route_ensemble_rt(*lc.NB, "f16", *args)
                    assert got == (("fused_rt" if c[0] == "fused" else "two_launch"), c[1]), (args, c, got)
                    # (the nested sampler's query is the same function with n_live for n_walkers)
                    assert nat.route_nested(*S1, "f16", n, W, n_data, modes, flags, host_form) == c, args
    # a stack the kernel cannot express never gets route 3
    for name, (dims, act, _) in lc.REFUSALS.items():
        assert nat.route_loglike_fwd_rt(dims, act, "f32", 256) == "two_launch", name


def test_refusals_carry_the_reason(tmp_path):
    nat = pkg("_native")
    for name, (dims, act, why) in lc.REFUSALS.items():
        with pytest.raises(nat.EngineError, match=why):
            nat.jit_prebuild_loglike(dims, act, "f16", str(tmp_path))
    # a kernel argument with two kind bits, or a kind over a precision it has not
    for kernel in (64 | 32, 64 | 16 | 1, 64 | 3, 128):
        with pytest.raises(nat.EngineError):
            nat._prebuild(*lc.CASES["R0"], kernel, str(tmp_path))
    assert os.listdir(str(tmp_path)) == []


# ---- compilation through the child compiler (hiprtc, no GPU)
def _child(call):
    code = ("import importlib, sys; sys.path.insert(0, %r); n = importlib.import_module('21cmvae_amd._native'); n.%s"
            % (ROOT, call))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, V21_JIT_TOOLCHAIN="70200000"))
    assert r.returncode == 0, (call, r.stderr[-800:])


def _msgpack_uint(blob, key):
    """the unsigned integer that follows the string `key` in a code object's msgpack metadata note"""
    at = blob.index(key.encode()) + len(key)
    t = blob[at]
    if t < 0x80:
        return t
    size = {0xCC: 1, 0xCD: 2, 0xCE: 4, 0xCF: 8}[t]
    return int.from_bytes(blob[at + 1:at + 1 + size], "big")


def _code_object(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"V21KOBJ1"
    n = struct.unpack("<I", blob[8:12])[0]
    return blob[12 + n:]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not HAVE_HIPRTC:
        pytest.skip("libhiprtc is not installed here")
    d = str(tmp_path_factory.mktemp("lnlrt_kc"))
    jobs = [(name, prec) for name in lc.CASES for prec in lc.PRECS]

    def one(job):
        dims, act = lc.CASES[job[0]]
        _child("jit_prebuild_loglike(%r, %r, %r, %r)" % (list(dims), list(act), job[1], d))
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(one, jobs))
    return d, jobs


def _object_of(d, name, prec):
    dims, act = lc.CASES[name]
    spec = "fused_lnl_%s_a%s_%s_" % ("x".join(map(str, dims)), "".join(str(a) for a in act), FORM[prec])
    mine = [f for f in os.listdir(d) if f.startswith(spec) and f.endswith(".v21k")]
    assert len(mine) == 1, (spec, os.listdir(d))
    return os.path.join(d, mine[0])


def test_every_case_compiles_without_scratch(compiled):
    d, jobs = compiled
    files = sorted(f for f in os.listdir(d) if f.endswith(".v21k"))
    assert len(files) == len(jobs) and all(f.startswith("fused_lnl_") for f in files), files
    print("LNLRT resources: kernel, VGPRs, AGPRs, scratch bytes")
    for name, prec in jobs:
        code = _code_object(_object_of(d, name, prec))
        res = {k: _msgpack_uint(code, "." + k) for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
        print("LNLRT %-3s %-5s: %d %d %d" % (name, prec, res["vgpr_count"], res["agpr_count"], res["private_segment_fixed_size"]))
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, prec, res)
        assert 0 < res["vgpr_count"] <= (512 if prec == "f32" else 256), (name, prec, res)   # 16 bits: two workgroups per CU


def _llvm_objdump():
    import shutil
    cands = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        cands.append(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin"))
    for c in cands:
        if os.path.exists(os.path.join(c, "llvm-objdump")):
            return os.path.join(c, "llvm-objdump")
    return None


def test_data_loads_keep_their_place_in_every_compiled_object(compiled, tmp_path):
    """The condition K12's accounting rests on (csrc/fused_fwd.h: lnl_load / lnl_pin), read off every run-time object: from the
    start of the weight ring to the last MFMA the plain (non-LDS) global loads form ONE group of ceil(out_dim / 32); after that group no ring
    rendezvous (s_waitcnt vmcnt(N), s_barrier) with N > 0 comes before a vmcnt(0); nothing touches scratch.  (That every
    wait of the compiler's lies at that one seam, as tests/test_lnl_cpu.py asserts of S1 and S3, does not hold in
    general: 7-64-128-451 in f32 waits twice for its input rows after the first MFMA.)"""
    objdump = _llvm_objdump()
    if objdump is None:
        pytest.skip("no llvm-objdump")
    d, jobs = compiled
    for name, prec in jobs:
        co = str(tmp_path / ("%s_%s.co" % (name, prec)))
        open(co, "wb").write(_code_object(_object_of(d, name, prec)))
        text = subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout
        ins = [l.split("//")[0].split() for l in text.splitlines() if l.startswith("\t")]
        ins = [i for i in ins if i]
        tag = (name, prec)
        assert not any(i[0].startswith("scratch_") for i in ins), tag
        mfma = [k for k, i in enumerate(ins) if i[0].startswith("v_mfma")]
        assert mfma, tag
        # (from the ring's first LDS-direct load on: a one-layer stack issues its d / w load between the ring's only
        #  rendezvous and its first MFMA -- the region is a superset of the MFMA stream, and the count below shows that no
        #  other plain load lies in it)
        ring0 = min(k for k, i in enumerate(ins) if i[0].startswith("global_load_lds"))
        assert ring0 < mfma[0], tag
        body = ins[ring0:mfma[-1] + 1]
        loads = [k for k, i in enumerate(body) if i[0].startswith("global_load") and "lds" not in i[0]]
        tiles = (lc.CASES[name][0][-1] + 31) // 32
        assert len(loads) == tiles, (tag, len(loads), tiles)
        assert loads[-1] - loads[0] < 64, (tag, "the d / w loads are no longer issued together")
        assert not any(i[0] == "s_barrier" for i in body[loads[0]:loads[-1] + 1]), (tag, "a rendezvous inside the group")
        vm = [k for k, i in enumerate(body) if k > loads[-1] and i[0] == "s_waitcnt" and any(a.startswith("vmcnt") for a in i[1:])]
        zero = [k for k in vm if any(a.startswith("vmcnt(0)") for a in body[k][1:])]
        counted = [k for k in vm if k + 1 < len(body) and body[k + 1][0] == "s_barrier" and k not in zero]
        assert not counted or (zero and zero[0] < counted[0]), (tag, "a counted ring rendezvous before the loads are drained")
        print("LNLRT seam %-3s %-5s: %d loads, %d waits after them, %d counted rendezvous" % (name, prec, len(loads), len(vm), len(counted)))


# ---- cache names
def _fnv1a(data, h=1469598103934665603):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.skipif(not HAVE_HIPRTC, reason="libhiprtc is not installed here")
def test_other_kinds_keep_their_cache_names(tmp_path):
    """R1's f16 forward, training (7-64-128-451: R1 has no fused training kernel worth a name) and Jacobian objects get the
    same file names whether or not an ln L object is built beside them; the ln L object's name is its own, under the
    prefix "fused_lnl_", and -- same source blob, same options -- differs from the forward's only through the spec."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    dims, act = lc.CASES["R1"]
    others = ["jit_prebuild(%r, %r, 'f16', %%r)" % (list(dims), list(act)), "jit_prebuild_jacobian(%r, %r, 'f16', %%r)" % (list(dims), list(act)),
              "jit_prebuild_train(%r, %r, 'f16', %%r)" % lc.NB]
    for call in others:
        _child(call % a)
    _child("jit_prebuild_loglike(%r, %r, 'f16', %r)" % (list(dims), list(act), b))
    for call in others:
        _child(call % b)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    lnl = [f for f in fb if f.startswith("fused_lnl_")]
    assert len(fa) == 3 and len(lnl) == 1 and sorted(fa + lnl) == fb, (fa, fb)
    assert lnl[0].startswith("fused_lnl_5x40x72x37_a110_PrecF16x2spLnl_")
    for f in fa:   # and the bytes: an object is a function of its own kind's sources alone
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


def test_new_symbols_are_exported_and_declared():
    import re
    native = pkg("_native")
    lib = native.load_library()
    header = open(os.path.join(ROOT, "include", "v21.h")).read()
    for sym in ("v21_mlp_jit_loglike", "v21_route_loglike_fwd_rt", "v21_route_ensemble_rt"):
        assert getattr(lib, sym) is not None and re.search(r"\bint %s\(" % sym, header), sym
    assert hasattr(native.Stack, "jit_loglike") and hasattr(native, "jit_prebuild_loglike") and hasattr(native, "route_loglike_fwd_rt")
    assert hasattr(pkg("emulator")._EmulatorBase, "compile_likelihood")


# ---- the mutation catalogue at these shapes
@pytest.mark.parametrize("name", list(lc.CASES))
def test_mutation_catalogue_bites_at_these_shapes(name):
    """every mutation of lnlrt_cases.MUTATIONS (lnl_ref's, restated for any width) moves the float64 ln L of the float64
    forward by more than 4x the bound at 33 and at 257 rows, with the record the GPU parity test uses (R1: its last tile
    dead) and, for R1, with its five-bin last tile live"""
    rec = lc.stack(name)
    dims = rec["dims"]
    for n in (33, 257):
        for tout_on in (False, True):
            x = lc.sc.rows_u(dims, n, 50 + n)
            y = lc.forward64(rec, x, False, tout_on)
            std = float(rec["tout"][0]) if tout_on else 1.0
            mean = rec["tout"][1] if tout_on else np.ones(dims[-1])
            truth = lc.forward64(rec, lc.sc.rows_u(dims, 1, 900), False, tout_on)[0]
            for dead_tile in ((True, False) if name == "R1" else (True,)):
                d, w = lc.record(name, truth, std, 3, dead_tile)
                ref = lr.lnl64(y, d, w)
                assert np.all(ref < 0) and np.all(np.isfinite(ref))
                d2 = d.copy()
                d2[np.flatnonzero(w == 0)[:3]] = np.inf
                if np.any(w == 0):
                    assert np.array_equal(lr.lnl64(y, d2, w), ref)
                eff = lc.mutation_effects(y, d, w, mean)
                print("LNLRT mutations %s n=%d tout=%d dead=%d: %s" % (name, n, tout_on, dead_tile, {k: "%.1e" % e for k, e in eff.items()}))
                for mut, e in eff.items():
                    assert e > 4 * lr.LNL_FWD_TOL, (name, n, tout_on, dead_tile, mut, e)
