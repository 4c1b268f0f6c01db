"""fused_jac<ArchRT, Prec> instantiated at run time (csrc/jit.hip: kJitJac) where no GPU is needed: who may
have the kernel and why not (jit_jac_eligible through v21_route_jacobian_rt and v21_jit_prebuild), that every case of
tests/jacrt_cases.py compiles through the child compiler without scratch memory, that the forward kernels' cached
objects keep their names, the new symbols, the kink rule's cap on the REFERENCE, and the float64 restatement of the
16-bit kernel on smooth stacks against act_ref.jacobian."""
import ctypes.util
import os
import re
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import act_ref as ar
import half_ref as hr
import jacrt_cases as jc
import jacobian_ref as jr
from conftest import ROOT, pkg

HAVE_HIPRTC = os.path.exists("/opt/rocm/lib/libhiprtc.so") or ctypes.util.find_library("hiprtc") is not None
needs_hiprtc = pytest.mark.skipif(not HAVE_HIPRTC, reason="libhiprtc is not installed here")
ARCHS = {"S1": [7, 352, 352, 352, 224, 451], "S2": [7, 288, 352, 288, 224, 451], "S3": [7, 352, 352, 352, 224, 9, 32, 352, 451],
         "S4": [9, 32, 352, 451]}
ARCH_ACT = {"S1": [1, 1, 1, 1, 0], "S2": [1, 1, 1, 1, 0], "S3": [1, 1, 1, 1, 0, 1, 1, 0], "S4": [1, 1, 0]}


# ---- eligibility and routes
def test_routes_and_refusals(tmp_path):
    native = pkg("_native")
    assert native.JAC_ROUTES == {1: "fused", 2: "generic", 3: "fused_rt"}
    for name, (dims, act) in jc.CASES.items():
        for prec in jc.PRECS:
            assert native.route_jacobian_rt(dims, act, prec) == "fused_rt", (name, prec)
            assert native.route_jacobian_rt(dims, act, prec, native.FWD_FORCE_GENERIC) == "generic", (name, prec)
            for n in (1, 130, 65537):
                assert native.route_jacobian(dims, act, prec, n) == "generic", (name, prec, n)
    for name, dims in ARCHS.items():
        for prec in jc.PRECS:
            assert native.route_jacobian(dims, ARCH_ACT[name], prec, 130) == "fused", name
            assert native.route_jacobian_rt(dims, ARCH_ACT[name], prec) == "fused", name   # compiled in: forced only
            assert native.route_jacobian_rt(dims, ARCH_ACT[name], prec, native.FWD_FORCE_JIT) == "fused_rt", name
    for name, (dims, act, why) in jc.REFUSALS.items():
        assert native.route_jacobian_rt(dims, act, "f32") == "generic", name
        assert native.route_jacobian(dims, act, "f32", 130) == "generic", name
        with pytest.raises(native.EngineError, match=why):
            native.jit_prebuild_jacobian(dims, act, "f16", str(tmp_path))
    assert os.listdir(str(tmp_path)) == []


# ---- compilation through the child compiler (hiprtc, no GPU)
def _child(call, d):
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


def _resources(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"V21KOBJ1"
    n = struct.unpack("<I", blob[8:12])[0]
    code = blob[12 + n:]
    return {k: _msgpack_uint(code, "." + k) for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count")}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not HAVE_HIPRTC:
        pytest.skip("libhiprtc is not installed here")
    d = str(tmp_path_factory.mktemp("jacrt_kc"))
    jobs = [(name, prec) for name in jc.CASES for prec in jc.PRECS] + [("S4", "f16")]

    def one(job):
        rec = jc.stack(job[0])
        _child("jit_prebuild_jacobian(%r, %r, %r, %r)" % (rec["dims"], rec["act"], job[1], d), d)
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(one, jobs))
    return d, jobs


def test_every_case_compiles_without_scratch(compiled):
    d, jobs = compiled
    files = sorted(f for f in os.listdir(d) if f.endswith(".v21k"))
    assert len(files) == len(jobs) and all(f.startswith("fused_jac_") for f in files), files
    form = {"f32": "PrecF32", "f16": "PrecF16x2sp", "bf16": "PrecBF16x2sp"}
    print("JACRT resources: kernel, VGPRs, AGPRs, scratch bytes")
    for name, prec in jobs:
        rec = jc.stack(name)
        spec = "fused_jac_%s_a%s_%s_" % ("x".join(map(str, rec["dims"])), "".join(str(a) for a in rec["act"]), form[prec])
        mine = [f for f in files if f.startswith(spec)]
        assert len(mine) == 1, (spec, files)
        res = _resources(os.path.join(d, mine[0]))
        print("JACRT %-3s %-5s %s: %d %d %d" % (name, prec, spec, res["vgpr_count"], res["agpr_count"], res["private_segment_fixed_size"]))
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, prec, res)
        assert 0 < res["vgpr_count"] <= 256, (name, prec, res)   # two workgroups per CU in 16 bits


def _fnv1a(data, h=1469598103934665603):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _hip_version():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        p = os.path.join(root or "", "include", "hip", "hip_version.h")
        if root and os.path.exists(p):
            t = open(p).read()
            v = [int(re.search(r"#define\s+HIP_VERSION_%s\s+(\d+)" % k, t).group(1)) for k in ("MAJOR", "MINOR", "PATCH")]
            return v[0] * 10000000 + v[1] * 100000 + v[2]
    return None


@needs_hiprtc
def test_forward_object_keeps_its_cache_name(tmp_path):
    """R1's f16 FORWARD object is named by the rule this library had before the Jacobian kind: "fused_<spec>_<hash>.v21k",
    the hash FNV-1a over the forward's embedded sources (include/v21_types.h, par_transform.h, act.h, fused_fwd.h with
    their own #include "..." lines and #pragma once removed, and the array's closing 0), the compiler options, the spec
    and (cache format 2, the runtime version the child is told, HIP_VERSION).  fused_jac.h is in none of it: the
    Jacobian kind hashes a blob of its own, and the two names differ."""
    hipv = _hip_version()
    if hipv is None:
        pytest.skip("no hip_version.h to read HIP_VERSION from")
    d = str(tmp_path)
    dims, act = jc.CASES["R1"]
    _child("jit_prebuild(%r, %r, 'f16', %r)" % (dims, act, d), d)
    _child("jit_prebuild_jacobian(%r, %r, 'f16', %r)" % (dims, act, d), d)
    csrc = os.path.join(ROOT, "21cmvae_amd", "csrc")
    blob = b""
    for f in (os.path.join(ROOT, "include", "v21_types.h"), os.path.join(csrc, "par_transform.h"), os.path.join(csrc, "act.h"),
              os.path.join(csrc, "fused_fwd.h")):
        for line in open(f, "rb").read().splitlines(keepends=True):
            if not line.startswith(b'#include "') and not line.startswith(b"#pragma once"):
                blob += line
    h = _fnv1a(blob + b"\0")
    for o in ("--offload-arch=gfx950", "-std=c++20", "-O3", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form=1"):
        h = _fnv1a(o.encode(), h)
    spec = "5x40x72x37_a110_PrecF16x2sp"
    h = _fnv1a(spec.encode(), h)
    h = _fnv1a(struct.pack("<3i", 2, 70200000, hipv), h)
    files = sorted(os.listdir(d))
    assert "fused_%s_%016x.v21k" % (spec, h) in files, files
    jac = [f for f in files if f.startswith("fused_jac_" + spec)]
    assert len(jac) == 1 and not jac[0].endswith("%016x.v21k" % h), files


def test_new_symbols_are_exported_and_declared():
    native = pkg("_native")
    lib = native.load_library()
    header = open(os.path.join(ROOT, "include", "v21.h")).read()
    for sym in ("v21_mlp_jit_jacobian", "v21_route_jacobian_rt"):
        assert getattr(lib, sym) is not None and re.search(r"\bint %s\(" % sym, header), sym
    assert hasattr(native.Stack, "jit_jacobian") and hasattr(native, "jit_prebuild_jacobian")
    assert hasattr(pkg("emulator")._EmulatorBase, "compile_derivatives")


# ---- the f32 check's kink rule, on the reference alone
def test_kink_exclusion_stays_below_its_cap():
    """rows excluded from the f32 GPU check (a float64 pre-activation of a hidden ReLU unit within 1e-5 of its layer's
    largest): at most 1 % of the rows of a case and never a whole call.  A seed that exceeds that is changed (jacrt_cases.SEED),
    not the cap."""
    for name in jc.RELU_CASES:
        rec = jc.stack(name)
        rows = excluded = 0
        for n, tin_on, _, x in jc.calls(name):
            k = jc.kink_rows(rec, jc.transformed(rec, x, tin_on))
            assert k.sum() < n, (name, n, "a whole call excluded")
            rows, excluded = rows + n, excluded + int(k.sum())
        print("JACRT kink rows %s: %d of %d" % (name, excluded, rows))
        assert excluded <= 0.01 * rows, (name, excluded, rows)
    for name in jc.SMOOTH_CASES:   # smooth stacks have no kinks
        rec = jc.stack(name)
        assert not any(jc.kink_rows(rec, jc.transformed(rec, x, t)).any() for _, t, _, x in jc.calls(name))


# ---- the 16-bit restatement for smooth stacks
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(jc.SMOOTH_CASES))
def test_smooth_restatement_against_float64(name, prec):
    """loose: the 16-bit rounding of weights, activations and tangents dominates (f16 2^-11, bf16 2^-8 per operand).  With
    the rounding switched off it IS act_ref.jacobian."""
    rec = jc.stack(name)
    x = sc_rows(rec, 40)
    J64 = ar.jacobian(rec["Ws"], rec["bs"], rec["act"], x.astype(np.float64))
    orig = hr.round16
    try:
        hr.round16 = lambda a, p: np.asarray(a, np.float64)
        J0 = jc.jvp16_smooth(rec["Ws"], rec["bs"], rec["act"], x, prec)[1]
    finally:
        hr.round16 = orig
    assert jr.rel_frobenius(J0, J64).max() <= 1e-12
    J16 = jc.jvp16_smooth(rec["Ws"], rec["bs"], rec["act"], x, prec)[1]
    e = jr.rel_frobenius(J16, J64)
    print("JACRT restatement %s %s: rel Frobenius median %.2e max %.2e" % (name, prec, np.median(e), e.max()))
    assert np.isfinite(J16).all() and e.max() <= (1e-2 if prec == "f16" else 8e-2), (name, prec, e.max())
    # every mutation moves the statistic the GPU test bounds, on the restatement itself
    for mut in jc.SMOOTH_MUTATIONS:
        Jm = jc.jvp16_smooth(rec["Ws"], rec["bs"], rec["act"], x, prec, mut=mut)[1]
        v = hr.jac_worst_cell_median(Jm, J16)
        print("JACRT restatement %s %s: %s moves the worst-cell median to %.3e" % (name, prec, mut, v))
        assert v > 0, (name, prec, mut)


def sc_rows(rec, n):
    import shape_cases as sc
    return sc.rows_u(rec["dims"], n, 77).astype(np.float32)
