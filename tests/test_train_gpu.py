"""GPU parity of the training path (K2 loss/grad, K3 backward GEMMs, K4 Adam, K5 batch
gather + Keras-shaped epoch loop) against the CPU oracle, through the C ABI.

Tolerances: the device sums in a different order from numpy (and in f32), so f32 mode
is compared with the float64 oracle at rtol 2e-4 on gradients / 1e-4 on weights after a
few steps (relative to the tensor's scale); f16/bf16 operand modes are checked on the
gradient direction (cosine) and on the loss trajectory."""
import os

import numpy as np
import pytest
import torch   # before the engine's first call, also when this module runs alone: one HIP runtime per process

import half_ref as hr
from conftest import pkg
from helpers import (HALF_STEP_TOL, STACKS, assert_step_matches_oracle, half_step_check, oracle_step, per_layer_gradient_check,
                     stack_data, twin_steps)
from oracle import ref_numpy as ora
from train_support import close as _close, cos as _cos, forward64, loss64, new_trainer, signal_rows, vae_weights

pytestmark = pytest.mark.gpu


def _make(ctx, dims, act=None, seed=0, prec="f32", max_batch=256, lr=None):
    act = act or [1] * (len(dims) - 2) + [0]
    Ws, bs = ora.init_mlp(dims, seed=seed)
    rng = np.random.default_rng(seed + 1)
    bs = [rng.normal(scale=0.05, size=b.shape).astype(np.float32) for b in bs]
    st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, max_batch, lr=lr)
    return st, tr, Ws, bs


def test_single_step_grad_adam_state(ctx):
    dims = [7, 32, 16, 5]
    st, tr, Ws, bs = _make(ctx, dims, seed=3, lr=1e-2)
    rng = np.random.default_rng(0)
    n = 64
    x = rng.normal(size=(n, 7)).astype(np.float32)
    y = rng.normal(size=(n, 5)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=n).astype(np.float32)
    tr.set_data(0, x, y, w)
    loss = tr.run_epoch(None, n)  # one step, rows in order
    # oracle, float64
    W64 = [W.astype(np.float64) for W in Ws]; b64 = [b.astype(np.float64) for b in bs]
    sto = ora.AdamState(st.num_params, dtype=np.float64, lr=1e-2)
    W2, b2, loss_o, g_o = ora.train_step(W64, b64, sto, x.astype(np.float64), y.astype(np.float64), w.astype(np.float64), np.float64)
    assert abs(loss - loss_o) / loss_o < 1e-5
    _close(tr.get_grad(), g_o, 2e-4, "gradient")
    it, m, v = tr.get_state()
    assert it == 1
    _close(m, sto.m, 2e-4, "adam m")
    _close(v, sto.v, 4e-4, "adam v")
    _close(st.get_weights(), ora.flatten_params(W2, b2), 1e-5, "weights after 1 step")
    # the forward of the updated weights is served by the fused/generic predict path too
    np.testing.assert_allclose(st.forward(x, "f32"), ora.mlp_forward(W2, b2, x), atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("n,batch", [(100, 32), (96, 32), (50, 64)])
def test_epochs_match_oracle_fit(ctx, n, batch):
    """Keras bookkeeping: shuffled order, partial last batch kept, sample-weighted epoch
    loss, validation pass after the epoch."""
    dims = [7, 24, 12, 9]
    st, tr, Ws, bs = _make(ctx, dims, seed=5, max_batch=64, lr=3e-3)
    rng = np.random.default_rng(1)
    x = rng.normal(size=(n, 7)).astype(np.float32); y = rng.normal(size=(n, 9)).astype(np.float32)
    xv = rng.normal(size=(40, 7)).astype(np.float32); yv = rng.normal(size=(40, 9)).astype(np.float32)
    w = ora.mse_row_weight(y).astype(np.float32); wv = ora.mse_row_weight(yv).astype(np.float32)
    tr.set_data(0, x, y, w); tr.set_data(1, xv, yv, wv)
    sto = ora.AdamState(st.num_params, dtype=np.float64, lr=3e-3)
    W, b = [a.astype(np.float64) for a in Ws], [a.astype(np.float64) for a in bs]
    for ep in range(3):
        perm = ora.epoch_permutation(n, 7, ep)
        loss = tr.run_epoch(perm, batch)
        vloss = tr.evaluate(1, batch)
        W, b, hist = ora.fit(W, b, sto, x.astype(np.float64), y.astype(np.float64), w.astype(np.float64), 1, batch, seed=7,
                             val=(xv.astype(np.float64), yv.astype(np.float64), wv.astype(np.float64)),
                             dtype=np.float64, start_epoch=ep)
        assert abs(loss - hist["loss"][0]) / hist["loss"][0] < 2e-5, (ep, loss, hist["loss"][0])
        assert abs(vloss - hist["val_loss"][0]) / hist["val_loss"][0] < 2e-5
    it, _, _ = tr.get_state()
    assert it == sto.t == 3 * ((n + batch - 1) // batch)
    _close(st.get_weights(), ora.flatten_params(W, b), 2e-4, "weights after 3 epochs")


def test_autoencoder_fit_y_is_x_relative_mse(ctx):
    """AutoEncoderEmulator phase 1 (emulator.py:739-747): x -> x with relative_mse_loss,
    linear latent layer in the middle of the stack."""
    dims = [451, 48, 9, 16, 451]
    act = [1, 0, 1, 0]
    st, tr, Ws, bs = _make(ctx, dims, act=act, seed=8, max_batch=128, lr=1e-3)
    y, w = signal_rows(200, seed=3)
    tr.set_data(0, y, None, w)
    perm = ora.epoch_permutation(200, 1, 0)
    loss = tr.run_epoch(perm, 128)
    # oracle with the same activations
    W = [a.astype(np.float64) for a in Ws]; b = [a.astype(np.float64) for a in bs]
    sto = ora.AdamState(st.num_params, dtype=np.float64, lr=1e-3)
    tot = 0.0
    for s in range(0, 200, 128):
        idx = perm[s:s + 128]
        l, g = oracle_step(W, b, act, y[idx], y[idx], w[idx])
        tot += l * len(idx)
        flat = ora.adam_step(ora.flatten_params(W, b), g, sto)
        W, b = ora.unflatten_params(flat, dims)
    assert abs(loss - tot / 200) / (tot / 200) < 2e-5
    _close(st.get_weights(), ora.flatten_params(W, b), 2e-4, "AE weights after 1 epoch")


def test_reference_architecture_step_all_precisions(ctx):
    """DirectEmulator default stack (emulator.py:196), batch 256 as emulator.py:372."""
    dims = [7, 288, 352, 288, 224, 451]
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, size=(256, 7)).astype(np.float32)
    y, w = signal_rows(256, seed=4)
    ref = None
    for prec, cos_min in (("f32", 0.999999), ("f16", 0.9995), ("bf16", 0.99)):
        st, tr, Ws, bs = _make(ctx, dims, seed=6, prec=prec, lr=1e-3)
        tr.set_data(0, x, y, w)
        loss = tr.run_epoch(None, 256)
        g = tr.get_grad()
        if ref is None:
            W64 = [W.astype(np.float64) for W in Ws]; b64 = [b.astype(np.float64) for b in bs]
            sto = ora.AdamState(st.num_params, dtype=np.float64, lr=1e-3)
            _, _, loss_o, g_o = ora.train_step(W64, b64, sto, x.astype(np.float64), y.astype(np.float64),
                                               w.astype(np.float64), np.float64)
            ref = (loss_o, g_o)
            _close(g, g_o, 5e-4, "f32 gradient of the reference stack")
        cos = _cos(g, ref[1])
        print("%s: loss rel err %.2e, grad cosine %.7f" % (prec, abs(loss - ref[0]) / ref[0], cos))
        assert cos > cos_min
        assert abs(loss - ref[0]) / ref[0] < (1e-5 if prec == "f32" else 2e-2)
        # (r5: layer by layer -- the cosine of the whole arena cannot see a small layer)
        model = None
        if prec != "f32":   # the 16-bit branch: the rounding reference of the route's model (tests/half_ref.py)
            model = hr.route_model(tr.last_route()[0][0])
        ok, note = per_layer_gradient_check(dims, [1, 1, 1, 1, 0], Ws, bs, x, g, ref[1], prec, tgt=y, w=w, loss=loss, model=model)
        assert ok, (prec, note)


def test_loss_decreases_and_state_roundtrip(ctx):
    dims = [7, 64, 64, 20]
    st, tr, Ws, bs = _make(ctx, dims, seed=9, max_batch=128, lr=3e-3)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, size=(1000, 7)).astype(np.float32)
    y = np.tanh(x @ rng.normal(size=(7, 20))).astype(np.float32)
    w = ora.mse_row_weight(y).astype(np.float32)
    tr.set_data(0, x, y, w)
    losses = [tr.run_epoch(ora.epoch_permutation(1000, 0, ep), 128) for ep in range(8)]
    assert losses[-1] < 0.5 * losses[0], losses
    assert abs(tr.evaluate(0, 128) - tr.evaluate(0, 100)) < 1e-6 * losses[-1] + 1e-9
    it, m, v = tr.get_state()
    tr.set_state(it, m, v)
    it2, m2, v2 = tr.get_state()
    assert it2 == it and np.array_equal(m, m2) and np.array_equal(v, v2)
    tr.set_lr(1e-4)
    assert tr.get_lr() == float(np.float32(1e-4))


def test_trainer_argument_errors(ctx):
    native = pkg("_native")
    st, tr, _, _ = _make(ctx, [7, 8, 3], max_batch=16)
    with pytest.raises(native.EngineError):
        tr.run_epoch(None, 8)  # no data yet
    x = np.zeros((20, 7), np.float32); y = np.zeros((20, 3), np.float32); w = np.ones(20, np.float32)
    tr.set_data(0, x, y, w)
    with pytest.raises(native.EngineError):
        tr.run_epoch(None, 64)  # exceeds max_batch
    with pytest.raises(native.EngineError):
        tr.set_data(0, x, None, w)  # y = x needs in_dim == out_dim
    for prec in ("f32", "f16"):  # an output non-linearity would not be differentiated: refused, not mis-trained
        with pytest.raises(native.EngineError, match="output layer"):
            native.Trainer(native.Stack(ctx, [7, 8, 3], [1, 1]), prec, 16)
    # the epoch's row table: one entry per row of the training set, every entry a row of it -- a short table would be read
    # past its end and a wrong entry is a GPU memory fault in the gather (r4: checked by the binding AND by the library)
    with pytest.raises(ValueError, match="row table"):
        tr.run_epoch(np.arange(8, dtype=np.int32), 8)
    import ctypes as C
    bad = np.arange(20, dtype=np.int32); bad[7] = 20
    loss = C.c_double(0)
    rc = tr.lib.v21_trainer_run_epoch(tr.h, bad.ctypes.data_as(C.POINTER(C.c_int32)), 8, C.byref(loss))
    assert rc != 0 and b"entry 7 = 20" in tr.lib.v21_last_error()
    bad[7] = -1
    assert tr.lib.v21_trainer_run_epoch(tr.h, bad.ctypes.data_as(C.POINTER(C.c_int32)), 8, C.byref(loss)) != 0
    assert np.isfinite(tr.run_epoch(np.arange(20, dtype=np.int32)[::-1].copy(), 8))


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_layers_wider_than_512_train_on_the_per_layer_path(ctx, prec):
    """`hidden_dims` is free in the reference (emulator.py:12-48).  Stacks with a layer wider than 512 have no chain kernel
    and step through the per-layer NT kernels (csrc/gemm_nt.h); until r4 its launcher REFUSED a contraction over more than
    512 features (V21_ERR_UNSUPPORTED: such a stack could predict but not train) although the kernel walks any range in
    rounds.  First-step loss and full gradient against the float64 oracle, then the loss falls."""
    dims, act = [7, 600, 520, 33], [1, 1, 0]
    n = 300
    rng = np.random.default_rng(3)
    Ws, bs = ora.init_mlp(dims, seed=8)
    bs = [rng.normal(scale=0.05, size=b.shape).astype(np.float32) for b in bs]
    x = rng.uniform(-1, 1, size=(n, 7)).astype(np.float32)
    y = rng.normal(size=(n, 33)).astype(np.float32)
    w = ora.mse_row_weight(y).astype(np.float32)
    st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, n, lr=1e-3)
    tr.set_data(0, x, y, w)
    l1 = tr.run_epoch(None, n); g = tr.get_grad()
    lo, go = oracle_step(Ws, bs, act, x, y, w)
    tol = 2e-5 if prec == "f32" else 3e-3
    assert abs(l1 - lo) <= tol * lo, (l1, lo)
    if prec == "f32":
        _close(g, go, 2e-5, "gradient of a 600-wide stack")
    else:
        assert _cos(g, go) > 0.9995
    losses = [tr.run_epoch(None, 100) for _ in range(10)]
    assert losses[-1] < 0.9 * l1, (l1, losses)


def test_rccl_single_rank_communicator_is_identity():
    """K6 plumbing on one GPU: a 1-rank RCCL communicator must not change an epoch."""
    native = pkg("_native")
    c2 = native.Context(0)
    res = []
    for use_comm in (False, True):
        st, tr, Ws, bs = _make(c2, [7, 24, 9], seed=2, max_batch=64)
        rng = np.random.default_rng(4)
        x = rng.normal(size=(90, 7)).astype(np.float32); y = rng.normal(size=(90, 9)).astype(np.float32)
        w = ora.mse_row_weight(y).astype(np.float32)
        tr.set_data(0, x, y, w)
        if use_comm:
            c2.comm_init(1, 0, c2.comm_unique_id())
        loss = tr.run_epoch(ora.epoch_permutation(90, 1, 0), 32)
        res.append((loss, st.get_weights()))
    c2.comm_destroy()
    assert res[0][0] == res[1][0]
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_large_batch_step_uses_big_tiles_and_split_k(ctx):
    """Per-GPU batch 4096 (BASELINE configs[3]): 64x64 workgroup tiles, the batch contraction of
    the weight gradient split into slabs; same gradient as the oracle."""
    dims, act = STACKS["AE"]
    n = 4096
    st, tr, Ws, bs = _make(ctx, dims, act=act, seed=12, max_batch=n, lr=1e-3)
    y, w = signal_rows(n, seed=9)
    tr.set_data(0, y, None, w)
    loss = tr.run_epoch(None, n)
    g = tr.get_grad()
    # float64 oracle gradient of the same stack
    l, ref = oracle_step(Ws, bs, act, y, y, w)
    assert abs(loss - l) / l < 2e-5
    _close(g, ref, 5e-4, "gradient at batch 4096")


FUSED_TRAIN_STACKS = [   # csrc/archs.h: the stacks with a compiled fused training kernel (csrc/fused_train.h); (name, dims, act, y = x)
    ("T1 autoencoder",) + STACKS["AE"] + (True,),
    ("T2 latent emulator",) + STACKS["LE"] + (False,),
    ("T3 direct emulator (reference default)",) + STACKS["DE"] + (False,),
    ("T4 direct emulator (configs[1])",) + STACKS["D1"] + (False,),
]


@pytest.mark.parametrize("rows_per_wave", [32, 16])
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", range(len(FUSED_TRAIN_STACKS)), ids=[c[0].split()[0] for c in FUSED_TRAIN_STACKS])
def test_fused_training_kernel_matches_chain_route_and_oracle(ctx, case, prec, rows_per_wave, monkeypatch):
    """BOTH fused training kernels: csrc/fused_train.h (32 rows per wave, 128-row workgroups: trainers of >= 24,576 rows per
    step) and csrc/fused_train16.h (16 rows per wave on the 16 x 16 x 32 MFMA, 64-row workgroups, two per CU: smaller trainers,
    from 8,193 rows per step) -- which one a trainer takes is fixed at its creation (V21_FUSED_TRAIN16 overrides).
    Large steps of f16 / bf16 trainers take csrc/fused_train.h: 128 rows per workgroup,
    weights through an LDS ring shared by four waves, activations, ReLU masks and the activation gradients in registers,
    forward pass + loss + activation-gradient chain as ONE unrolled virtual stack.  Forced here onto a ragged step of
    777 rows (6 workgroups of 128 + one of 9; 48.6 groups of 16; the last 128-row block reaches past max_batch rounded up
    to 32 rows -- the operand buffers are sized for whole blocks since that case overwrote another tile's rows in r4) of
    every stack it is compiled for: loss and
    FULL gradient against the 32-row chain route (the same 16-bit arithmetic in another order) and the float64 oracle, a
    second step (the packed stream is rebuilt from the arena Adam moved), targets = inputs and separate targets."""
    monkeypatch.setenv("V21_FUSED_TRAIN16", "1" if rows_per_wave == 16 else "0")
    name, dims, act, ae = FUSED_TRAIN_STACKS[case]
    n = 777
    rng = np.random.default_rng(40 + case)
    Ws, bs = ora.init_mlp(dims, seed=30 + case)
    bs = [rng.normal(scale=0.05, size=b.shape).astype(np.float32) for b in bs]
    flat = ora.flatten_params(Ws, bs)
    if ae:
        (x, w), y = signal_rows(n, seed=9), None
    else:
        x = rng.uniform(-1, 1, size=(n, dims[0])).astype(np.float32)
        if dims[-1] == 451:
            y, w = signal_rows(n, seed=10)
        else:
            y = rng.normal(size=(n, dims[-1])).astype(np.float32)
            w = ora.mse_row_weight(y).astype(np.float32)
    res = {}
    for route, rows_env in (("chain", "1000000"), ("fused", "1")):
        monkeypatch.setenv("V21_FUSED_TRAIN_ROWS", rows_env)
        st, tr = new_trainer(ctx, dims, act, flat, prec, n, lr=1e-3)
        tr.set_data(0, x, y, w)
        l1 = tr.run_epoch(None, n)
        g1 = tr.get_grad()
        kind = tr.last_route()[0][0]
        w_mid = st.get_weights()                                 # the arena Adam moved: what the second step's stream is packed from
        l2 = tr.run_epoch(ora.epoch_permutation(n, 3, 0), n)     # gathered through an index table, weights moved by Adam
        res[route] = (l1, g1, l2, st.get_weights(), kind, w_mid)
        rc = tr.route_counters()   # "the routes agree" must not pass with both taking the same kernel
        assert (rc["chain"], rc["fused"]) == ((2, 0) if route == "chain" else (0, 2)), (route, rc)
        if route == "fused":       # the first step packs the stream, the second finds it written by the first's Adam pass
            assert rc["stream_packs"] == 1 and rc["stream_adam"] == 2, rc
    # float64 oracle: loss and gradient of the first step
    tgt = (x if y is None else y).astype(np.float64)
    lo, go = oracle_step(Ws, bs, act, x, tgt, w)
    tol_l, tol_c = (3e-3, 0.9995) if prec == "f16" else (3e-2, 0.995)
    perm2 = ora.epoch_permutation(n, 3, 0)
    for route in ("chain", "fused"):
        l1, g1, l2, _, kind, w_mid = res[route]
        assert kind == ("chain16" if route == "chain" else ("fused64" if rows_per_wave == 16 else "fused128")), (route, kind)
        assert abs(l1 - lo) / lo < tol_l, (name, route, l1, lo)
        cos = _cos(g1, go)
        assert cos > tol_c and abs(np.linalg.norm(g1) / np.linalg.norm(go) - 1) < 10 * tol_l, (name, route, cos)
        # ... and against the rounding reference of the route's model (tests/half_ref.py), every mutation refused
        ok, note = per_layer_gradient_check(dims, act, Ws, bs, x, g1, go, prec, tgt=tgt, w=w, loss=l1, model=hr.route_model(kind))
        assert ok, (name, route, note)
        # the second step runs on weights Adam repacked: its loss against the rounding reference of the device's OWN arena
        # weights before it (a stale or misplaced packed fragment shows at ~1e-6 here, not at the float64 bound of 3e-3)
        Wm, bm = ora.unflatten_params(np.asarray(w_mid, np.float32), dims)
        l2r, _ = hr.step(Wm, bm, act, x[perm2], tgt[perm2], w[perm2], prec, mask=hr.route_model(kind))
        e2 = abs(l2 - l2r) / l2r
        print("HALFREF second step %s %s %s loss %.1e" % (name, prec, kind, e2))
        assert e2 <= HALF_STEP_TOL[prec]["loss"], (name, route, "second step loss vs rounding reference", e2)
    (lc, gc, lc2, wc, _, _), (lf, gf, lf2, wf, _, _) = res["chain"], res["fused"]
    # the two routes round the same operands to 16 bits and sum in fp32: they agree far better than either meets float64
    assert abs(lf - lc) / lc < 1e-5 and abs(lf2 - lc2) / lc2 < 1e-3, (name, lf, lc, lf2, lc2)
    cos = _cos(gc, gf)
    assert cos > 0.99999 and np.abs(gc - gf).max() <= 2e-3 * np.abs(gc).max(), (name, cos, np.abs(gc - gf).max(), np.abs(gc).max())
    dc, df = wc - flat, wf - flat
    assert _cos(dc, df) > 0.999


@pytest.mark.parametrize("rows_per_wave", [32, 16])
@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_fused_training_stream_written_by_adam_equals_the_packed_one(ctx, prec, rows_per_wave, monkeypatch):
    """From its second consecutive step on, the fused training kernel reads a weight stream that the previous step's Adam
    pass scattered element by element (csrc/train_kernels.h: adam_repack_element, AdamArgs::ts) instead of one rebuilt
    by pack_stream_kernel.  After three fused steps: the fourth step's loss and FULL gradient equal those of a fresh
    trainer handed the same weights (whose first step packs the stream from the arena) bit for bit, on a
    ragged autoencoder step and on the direct emulator; then set_weights between fused steps invalidates the stream
    (the next step packs again and reproduces the very first loss)."""
    monkeypatch.setenv("V21_FUSED_TRAIN_ROWS", "1")
    monkeypatch.setenv("V21_FUSED_TRAIN16", "1" if rows_per_wave == 16 else "0")
    for name, dims, act, ae in (FUSED_TRAIN_STACKS[0], FUSED_TRAIN_STACKS[3]):
        n = 777
        rng = np.random.default_rng(5)
        Ws, bs = ora.init_mlp(dims, seed=77)
        bs = [rng.normal(scale=0.05, size=b.shape).astype(np.float32) for b in bs]
        flat = ora.flatten_params(Ws, bs)
        tgt, w = signal_rows(n, seed=11)
        x, y = (tgt, None) if ae else (rng.uniform(-1, 1, size=(n, dims[0])).astype(np.float32), tgt)
        st, tr = new_trainer(ctx, dims, act, flat, prec, n, lr=1e-3)
        tr.set_data(0, x, y, w)
        l1 = tr.run_epoch(None, n)
        for _ in range(2):
            tr.run_epoch(None, n)
        w3 = st.get_weights()
        assert np.abs(w3 - flat).max() > 1e-3          # Adam moved the weights: a stale stream would show
        l4 = tr.run_epoch(None, n); g4 = tr.get_grad()
        rc = tr.route_counters()
        assert rc["fused"] == 4 and rc["stream_packs"] == 1 and rc["chain"] == 0, rc
        st2, tr2 = new_trainer(ctx, dims, act, w3, prec, n, lr=1e-3)
        tr2.set_data(0, x, y, w)
        l4p = tr2.run_epoch(None, n); g4p = tr2.get_grad()
        assert tr2.route_counters()["stream_packs"] == 1
        # the same bits in the stream, the same kernels in the same order: identical results
        assert l4 == l4p and np.array_equal(g4, g4p), (name, l4, l4p, np.abs(g4 - g4p).max(), np.abs(g4p).max())
        st.set_weights(flat)
        l5 = tr.run_epoch(None, n)
        assert tr.route_counters()["stream_packs"] == 2
        assert l5 == l1, (name, l5, l1)


# ---- A13: variational latent layer (V21_ACT_GAUSS) -- build-side extension ----------------
def _make_vae(ctx, dims, gl, seed=0, max_batch=256, prec="f32", env=None):
    """train_support.vae_weights: layer `gl` is the (z_mean | z_log_var) head"""
    act, Ws, bs = vae_weights(dims, gl, seed)
    st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, max_batch, env=env)
    assert st.num_params == sum(W.size + b.size for W, b in zip(Ws, bs))
    return st, tr, Ws, bs


def test_vae_step_matches_oracle(ctx):
    """Sampled step: loss (reconstruction + kl_weight KL) and the full gradient against the
    float64 oracle fed the same counter-based noise; then Adam moved the weights."""
    dims = [451, 64, 9, 32, 451]
    st, tr, Ws, bs = _make_vae(ctx, dims, gl=1, seed=21, max_batch=160)
    n = 150
    y, w = signal_rows(n, seed=4)
    kl_weight, seed = 2e-3, 0xDEADBEEF12345
    tr.set_vae(kl_weight, sample=True, seed=seed)
    tr.set_adam(lr=1e-3)
    tr.set_state(5)  # the noise stream is keyed on the step counter
    tr.set_data(0, y, None, w)
    loss = tr.run_epoch(None, n)
    eps = ora.gauss_eps(seed, 5, n, 9)
    W = [a.astype(np.float64) for a in Ws]; b = [a.astype(np.float64) for a in bs]
    lo, g = ora.vae_loss_and_grads(W, b, 1, y.astype(np.float64), y.astype(np.float64), w.astype(np.float64), eps, kl_weight)
    assert abs(loss - lo) / lo < 2e-5, (loss, lo)
    _close(tr.get_grad(), g, 3e-4, "VAE gradient")
    assert tr.get_state()[0] == 6
    # validation pass: eps = 0, KL term included
    tr.set_data(1, y, None, w)
    lv = tr.evaluate(1, 64)
    flat, o, Wn, bn = st.get_weights().astype(np.float64), 0, [], []
    for W_, b_ in zip(Ws, bs):
        Wn.append(flat[o:o + W_.size].reshape(W_.shape)); o += W_.size
        bn.append(flat[o:o + b_.size]); o += b_.size
    le, _ = ora.vae_loss_and_grads(Wn, bn, 1, y.astype(np.float64), y.astype(np.float64), w.astype(np.float64),
                                   np.zeros((n, 9)), kl_weight)
    assert abs(lv - le) / le < 2e-5
    # deterministic forward (predict): z = z_mean
    acts, mu, _ = ora.vae_forward(Wn, bn, 1, y[:20].astype(np.float64), np.zeros((20, 9)))
    np.testing.assert_allclose(st.forward(y[:20], "f32"), acts[-1], atol=2e-4, rtol=1e-4)


def test_chain_job_table_is_validated_against_the_packed_streams(ctx):
    """The small-batch f32 chain kernel follows a host-built job table into the packed weight streams without range
    checks (csrc/train_chain32s.h; the r3 abort: a request past the end of a stream).  The host validates every address
    a row names when the trainer is created; here the same check is handed a deliberately TRUNCATED stream and must
    answer with an error instead of a launch -- for the stack of the aborted test and for the reference's autoencoder."""
    native = pkg("_native")
    for dims, act in (([451, 64, 9, 32, 451], [1, native.ACT_GAUSS, 1, 0]), ([451, 352, 9, 32, 352, 451], [1, 0, 1, 1, 0])):
        st = native.Stack(ctx, dims, act)
        tr = native.Trainer(st, "f32", 256)
        tr.check_chain_jobs()                                     # the real streams: every row inside
        with pytest.raises(native.EngineError, match="chain job table"):
            tr.check_chain_jobs(bw_bytes=4096)                    # a backward stream cut to one chunk
        with pytest.raises(native.EngineError, match="chain job table"):
            tr.check_chain_jobs(fw_bytes=8192)
    # the last 4-KiB chunk of the forward stream missing: only the rows of the last forward layer's last tile notice
    st = native.Stack(ctx, [451, 352, 9, 32, 352, 451], [1, 0, 1, 1, 0])
    tr = native.Trainer(st, "f32", 256)
    frags = lambda d: ((d + 3) // 4 + 3) // 4 * 4                 # chain32s_frags
    fw_bytes = sum(-(-n // 64) * frags(k) * 1024 for k, n in zip([451, 352, 9, 32, 352], [352, 9, 32, 352, 451]))
    tr.check_chain_jobs(fw_bytes=fw_bytes)
    with pytest.raises(native.EngineError, match="within the stream"):
        tr.check_chain_jobs(fw_bytes=fw_bytes - 4096)
    tr16 = native.Trainer(st, "f16", 256)
    with pytest.raises(native.EngineError, match="no job table"):
        tr16.check_chain_jobs()


def test_vae_without_noise_and_kl_equals_plain_autoencoder(ctx):
    """kl_weight = 0 and eps = 0 must give the deterministic autoencoder of emulator.py:517:
    same loss and same gradients as the plain stack holding the z_mean columns."""
    dims = [451, 48, 9, 16, 451]
    st, tr, Ws, bs = _make_vae(ctx, dims, gl=1, seed=5, max_batch=128)
    n = 100
    y, w = signal_rows(n, seed=6)
    tr.set_vae(0.0, sample=False, seed=1)
    tr.set_adam(lr=1e-3); tr.set_data(0, y, None, w)
    loss = tr.run_epoch(None, n)
    g = tr.get_grad()
    Wp = [Ws[0], np.ascontiguousarray(Ws[1][:, :9]), Ws[2], Ws[3]]
    bp = [bs[0], bs[1][:9].copy(), bs[2], bs[3]]
    st2, tr2 = new_trainer(ctx, dims, [1, 0, 1, 0], ora.flatten_params(Wp, bp), "f32", 128, lr=1e-3)
    tr2.set_data(0, y, None, w)
    loss2 = tr2.run_epoch(None, n)
    g2 = tr2.get_grad()
    assert loss == loss2
    # split both gradients per layer and compare the shared parts
    o = o2 = 0
    for l, (W_, b_) in enumerate(zip(Ws, bs)):
        gw = g[o:o + W_.size].reshape(W_.shape); o += W_.size
        gb = g[o:o + b_.size]; o += b_.size
        gw2 = g2[o2:o2 + Wp[l].size].reshape(Wp[l].shape); o2 += Wp[l].size
        gb2 = g2[o2:o2 + bp[l].size]; o2 += bp[l].size
        if l == 1:
            np.testing.assert_array_equal(gw[:, 9:], 0); np.testing.assert_array_equal(gb[9:], 0)
            gw, gb = gw[:, :9], gb[:9]
        np.testing.assert_allclose(gw, gw2, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(gb, gb2, rtol=1e-6, atol=1e-9)


def test_vae_trainer_argument_errors(ctx):
    native = pkg("_native")
    st = native.Stack(ctx, [8, 4, 8], [1, 0])
    tr = native.Trainer(st, "f32", 16)
    with pytest.raises(native.EngineError):
        tr.set_vae(1.0)  # no variational layer in the stack
    with pytest.raises(native.EngineError):
        native.Stack(ctx, [8, 4, 4, 8], [2, 2, 0])  # at most one
    enc = native.Stack(ctx, [8, 6, 3], [1, 2])  # an encoder alone: forward gives z_mean ...
    assert enc.num_params == 8 * 6 + 6 + 6 * 6 + 6
    assert enc.forward(np.zeros((2, 8), np.float32), "f32").shape == (2, 3)
    with pytest.raises(native.EngineError):
        native.Trainer(enc, "f32", 16)  # ... but cannot be trained without a decoder


# ---- one-kernel forward + activation-gradient chain (csrc/train_chain.h) --------------------
def _half_ref_check(tag, dims, act, Ws, bs, x, tgt, w, loss, g, prec, route, brows=None):
    """the 16-bit branch of the step checks (helpers.half_step_check): loss and FULL gradient against the float64 reference
    that rounds where the kernels round, in the ReLU model of the route taken (tests/half_ref.py); every mutation of the
    catalogue applied to the device's own result refused"""
    dims = [np.shape(Ws[0])[0]] + [np.shape(W)[1] for W in Ws]
    ok, note, _ = half_step_check(dims, act, Ws, bs, x, tgt, w, loss, g, prec, hr.route_model(route), brows=brows)
    assert ok, (tag, route, note)


def _chain_env(chain):
    """the path is chosen when the trainer is created"""
    return {"V21_TRAIN_CHAIN": "1" if chain else "0"}


def _one_step(ctx, dims, act, prec, x, y, w, perm, batch, chain, route=None):
    Ws, bs = ora.init_mlp(dims, seed=31)
    st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, batch, lr=1e-3, env=_chain_env(chain))
    tr.set_data(0, x, y, w)
    loss = tr.run_epoch(perm, batch)
    if route is not None:   # (a list: the forward route the step took is appended)
        route.append(tr.last_route()[0][0])
    return loss, tr.get_grad().astype(np.float64), st.get_weights(), (Ws, bs)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["autoencoder_tail", "direct_7_to_451", "batch_4096"])
def test_chain_kernel_matches_per_layer_path_and_oracle(ctx, prec, case):
    """The chain kernel (gather + all forward layers + loss + all activation gradients in one
    launch) against the per-layer NT path in the same precision, and both against the float64
    oracle.  Cases: a batch that is not a multiple of 32 drawn through a permutation (y = x);
    separate targets with a 7-wide input; a batch whose weight gradient is split into slabs."""
    synth = pkg("synth")
    if case == "direct_7_to_451":
        (dims, act), n = STACKS["DE"], 300
        par = synth.make_params(n, seed=3)
        x = ora.par_transform(par, par).astype(np.float32)
        sig = synth.signals_from_params(par)
        y = ora.preproc(sig, sig)
        w = ora.relative_mse_row_weight(y, sig).astype(np.float32)
        batch = 300
    else:
        dims, act = STACKS["AE"]
        n = 4096 if case == "batch_4096" else 200
        (x, w), y = signal_rows(n, seed=13), None
        batch = n
    perm = np.random.default_rng(2).permutation(n).astype(np.int32)
    routes = []
    lc, gc, wc, (Ws, bs) = _one_step(ctx, dims, act, prec, x, y, w, perm, batch, chain=True, route=routes)
    ln, gn, wn, _ = _one_step(ctx, dims, act, prec, x, y, w, perm, batch, chain=False, route=routes)
    assert routes == ["chain16", "per_layer"], routes
    tgt = x if y is None else y
    for (l_, g_), r_ in zip(((lc, gc), (ln, gn)), routes):   # both routes against the rounding reference
        _half_ref_check(case, dims, act, Ws, bs, x[perm], tgt[perm], w[perm], l_, g_, prec, r_)
    # float64 oracle of the same step
    lo, go = oracle_step(Ws, bs, act, x[perm], tgt[perm], w[perm])
    tol = 2e-3 if prec == "f16" else 2e-2
    assert abs(lc - lo) / lo < tol and abs(lc - ln) / ln < tol, (lc, ln, lo)
    assert _cos(gc, go) > (0.9995 if prec == "f16" else 0.995), _cos(gc, go)
    assert _cos(gc, gn) > (0.9995 if prec == "f16" else 0.995), _cos(gc, gn)
    assert abs(np.linalg.norm(gc) / np.linalg.norm(go) - 1) < (5e-3 if prec == "f16" else 3e-2)
    # Adam moved the weights the same way (first step: w -= lr * sign-like update; compare the update)
    uc, un = wc - ora.flatten_params(Ws, bs), wn - ora.flatten_params(Ws, bs)
    assert _cos(uc.astype(np.float64), un.astype(np.float64)) > 0.98


def test_chain_kernel_trains_and_validates(ctx):
    """Several epochs through the chain path: the loss falls, the validation pass (per-layer
    forward on the refreshed weight copies) agrees with the training loss level, and predict()
    sees the trained weights."""
    dims, act = [451, 64, 9, 32, 451], [1, 0, 1, 0]
    Ws, bs = ora.init_mlp(dims, seed=4)
    st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), "f16", 256, lr=2e-3)
    y, w = signal_rows(1000, seed=21)
    tr.set_data(0, y, None, w); tr.set_data(1, y[:300], None, w[:300])
    losses = [tr.run_epoch(ora.epoch_permutation(1000, 3, ep), 256) for ep in range(12)]
    assert losses[-1] < 0.5 * losses[0], losses
    v = tr.evaluate(1, 256)
    assert 0.3 * losses[-1] < v < 3 * losses[-1]
    Wt, bt = ora.unflatten_params(st.get_weights().astype(np.float64), dims)
    np.testing.assert_allclose(st.forward(y[:50], "f32"), forward64(Wt, bt, act, y[:50]), atol=5e-4, rtol=1e-3)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_validation_pass_is_one_forward_only_chain_launch(ctx, prec):
    """v21_trainer_eval on the chain path: one forward-only launch over ALL rows of the split (more than max_batch,
    not a multiple of 32), against the float64 oracle's loss of the same weights; training state is left alone (the
    next epoch's loss and weights are those of a trainer that never validated)."""
    dims, act = [451, 64, 9, 32, 451], [1, 0, 1, 0]
    Ws, bs = ora.init_mlp(dims, seed=9)
    y, w = signal_rows(1500, seed=5)
    res = []
    for validate in (True, False):
        st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, 128, lr=1e-3)
        tr.set_data(0, y[:500], None, w[:500]); tr.set_data(1, y[500:1477], None, w[500:1477])
        tr.run_epoch(None, 128)
        if validate:
            v = tr.evaluate(1, 128)
            W, b = ora.unflatten_params(st.get_weights().astype(np.float64), dims)
            expect = loss64(W, b, act, y[500:1477], y[500:1477], w[500:1477])
            assert abs(v - expect) / expect < (3e-3 if prec == "f16" else 3e-2), (v, expect)
            assert abs(tr.evaluate(1, 64) - v) == 0.0  # the batch argument no longer cuts the pass: same launch, same sum
        res.append((tr.run_epoch(None, 128), st.get_weights()))
    assert res[0][0] == res[1][0]
    np.testing.assert_array_equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dims,act,n", [
    ([451, 451], [0], 70),                         # one layer: the loss epilogue is also the first layer
    ([33, 500, 512, 17], [1, 1, 0], 45),           # widths that are not multiples of 16/32, the 512 limit
    ([7, 64, 3], [1, 0], 1),                       # a single row
    ([20, 40, 8, 40, 20], [1, 0, 1, 0], 257),      # linear layer inside, batch one past a block boundary
])
def test_chain_kernel_odd_shapes(ctx, dims, act, n):
    """Edge shapes of the chain path against the float64 oracle: gradient direction and norm, loss."""
    rng = np.random.default_rng(5)
    x = rng.normal(size=(n, dims[0])).astype(np.float32)
    y = None if dims[0] == dims[-1] and len(dims) > 2 else rng.normal(size=(n, dims[-1])).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=n).astype(np.float32) / dims[-1]
    perm = rng.permutation(n).astype(np.int32)
    routes = []
    lc, gc, _, (Ws, bs) = _one_step(ctx, dims, act, "f16", x, y, w, perm, max(n, 2), chain=True, route=routes)
    assert routes == ["chain16"], routes
    tgt = x if y is None else y
    _half_ref_check(dims, dims, act, Ws, bs, x[perm], tgt[perm], w[perm], lc, gc, "f16", routes[0])
    lo, go = oracle_step(Ws, bs, act, x[perm], tgt[perm], w[perm])
    assert abs(lc - lo) / lo < 3e-3, (lc, lo)
    assert _cos(gc, go) > 0.9995, _cos(gc, go)
    assert abs(np.linalg.norm(gc) / np.linalg.norm(go) - 1) < 5e-3


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("dims,act,n", [
    ([64, 32, 96, 64], [1, 1, 0], 48),      # K = 64: exactly ceil(K/16) k-steps, the bias row opens a tile of its own
    ([128, 9, 40, 128], [0, 1, 0], 33),     # a 9-wide latent: one partly filled n-tile, 16-row batch step + 1
    ([33, 500, 17], [1, 0], 130),           # nothing is a multiple of 16
])
def test_one_launch_gradient_adam_kernel_state_and_packed_copies(ctx, prec, dims, act, n):
    """csrc/dw_adam.h (single-rank chain steps): after each of three steps (m, v, w) follow the float64 oracle's
    Adam driven by the DEVICE's own gradient, and the loss the NEXT step reports -- computed by the chain kernel from
    the packed 16-bit weight copies this kernel rebuilt -- is the float64 forward loss of the arena weights.  A stale,
    misplaced or missing fragment of the packed copies shows up as a loss that is off by far more than the
    precision's tolerance."""
    rng = np.random.default_rng(11)
    x = rng.normal(size=(n, dims[0])).astype(np.float32)
    y = None if dims[0] == dims[-1] else rng.normal(size=(n, dims[-1])).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=n).astype(np.float32) / dims[-1]
    tgt = x if y is None else y
    Ws, bs = ora.init_mlp(dims, seed=7)
    st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, n, lr=5e-3)
    tr.set_data(0, x, y, w)
    ostate = ora.AdamState(st.num_params, dtype=np.float64, lr=5e-3)
    flat = ora.flatten_params(Ws, bs).astype(np.float64)
    tol = 3e-3 if prec == "f16" else 3e-2
    for step in range(3):
        Wb, bb = ora.unflatten_params(st.get_weights(), dims)   # the arena before the step
        expect = loss64(Wb, bb, act, x, tgt, w)
        loss = tr.run_epoch(None, n)
        assert abs(loss - expect) / expect < tol, (step, loss, expect)
        g = tr.get_grad().astype(np.float64)
        # ... and against the rounding reference of the arena weights before the step: steps 2 and 3 run on the packed
        # copies this kernel rebuilt, where a stale or misplaced fragment shows at ~1e-6 instead of the float64 bound
        _half_ref_check((dims, step), dims, act, Wb, bb, x, tgt, w, loss, g, prec, tr.last_route()[0][0])
        flat = ora.adam_step(flat, g, ostate)
        it, m, v = tr.get_state()
        assert it == step + 1
        np.testing.assert_allclose(m, ostate.m, rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(v, ostate.v, rtol=1e-4, atol=1e-12)
        np.testing.assert_allclose(st.get_weights(), flat, rtol=1e-4, atol=2e-6)
        flat = st.get_weights().astype(np.float64)  # (keep following the device: differences must not accumulate)
        ostate.m[:] = m; ostate.v[:] = v


@pytest.mark.parametrize("rows", ["rows16", "rows8", "rows4"])
@pytest.mark.parametrize("case", ["autoencoder_ragged", "direct_7_to_451", "latent_emulator", "batch_4096", "single_row"])
def test_f32_chain_kernel_matches_per_layer_path_and_oracle(ctx, case, rows, monkeypatch):
    """csrc/train_chain32.h (the fp32 chain: 16-row blocks on the 16 x 16 x 4 MFMA, weight gradients in one grouped NT
    launch, Adam) and csrc/train_chain32s.h (8-row blocks on the 4 x 4 x 1 MFMA, its own packed-stream format; the
    default for trainers of <= 2,048 rows -- both kernels are forced here on every case) against the per-layer f32 path
    (V21_TRAIN_CHAIN=0) and the float64 oracle at the stated f32 tolerance: loss 2e-5, gradient 2e-4 of its scale,
    weights after the step, Adam moments; then two more epochs with a partial last batch and the forward-only
    validation launch."""
    monkeypatch.setenv("V21_CHAIN32S", "0" if rows == "rows16" else "1")
    monkeypatch.setenv("V21_C32S_ROWS", "4" if rows == "rows4" else "8")
    synth = pkg("synth")
    if case == "direct_7_to_451":
        (dims, act), n = STACKS["DE"], 300
        par = synth.make_params(n, seed=3)
        x = ora.par_transform(par, par).astype(np.float32)
        sig = synth.signals_from_params(par)
        y = ora.preproc(sig, sig)
        w = ora.relative_mse_row_weight(y, sig).astype(np.float32)
    elif case == "latent_emulator":
        (dims, act), n = STACKS["LE"], 257
        rng = np.random.default_rng(3)
        x = rng.uniform(-1, 1, size=(n, 7)).astype(np.float32)
        y = rng.normal(size=(n, 9)).astype(np.float32)
        w = ora.mse_row_weight(y).astype(np.float32)
    else:
        dims, act = STACKS["AE"]
        n = {"autoencoder_ragged": 203, "batch_4096": 4096, "single_row": 1}[case]
        (x, w), y = signal_rows(n, seed=13, stats_from=max(n, 64)), None   # (statistics over >= 64 signals: one row alone pre-processes to zeros)
    perm = np.random.default_rng(2).permutation(n).astype(np.int32)
    batch = max(n, 2)
    res = {}
    for chain in (True, False):
        Ws, bs = ora.init_mlp(dims, seed=31)
        st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), "f32", batch, lr=1e-3, env=_chain_env(chain))
        tr.set_data(0, x, y, w)
        tr.set_data(1, x[: max(1, n // 3)], None if y is None else y[: max(1, n // 3)], w[: max(1, n // 3)])
        loss = tr.run_epoch(perm, batch)
        g = tr.get_grad().astype(np.float64)
        w1 = st.get_weights()
        it, m1, v1 = tr.get_state()
        more = [tr.run_epoch(ora.epoch_permutation(n, 5, ep), max(2, (n + 2) // 3)) for ep in range(2)]
        val = tr.evaluate(1, batch)
        res[chain] = (loss, g, w1, m1, v1, np.array(more + [val]), st.get_weights(), tr.get_state()[0])
    # float64 oracle of the first step
    sto = ora.AdamState(st.num_params, dtype=np.float64, lr=1e-3)
    lo, go = oracle_step(Ws, bs, act, x[perm], (x if y is None else y)[perm], w[perm])
    W2, b2 = ora.unflatten_params(ora.adam_step(ora.flatten_params(Ws, bs).astype(np.float64), go, sto), dims)
    lc, gc, wc, mc, vc, morec, wend, itc = res[True]
    ln, gn, wn, mn, vn, moren, wendn, itn = res[False]
    assert abs(lc - lo) / lo < 2e-5 and abs(lc - ln) / ln < 2e-5, (lc, ln, lo)

    def near(a_, b_, what):
        # A hidden unit whose pre-activation is within rounding of zero takes the other side of the ReLU kink in another
        # summation order (or in float64): its whole column of the weight gradient moves, legitimately.  Hence: the
        # direction to 1e-4, 99 % of the elements to 5e-4 of the tensor's scale (without such a flip every element is
        # within 2e-4, which `single_row` and the small stacks of the other f32 tests still assert).
        a_, b_ = np.asarray(a_, np.float64), np.asarray(b_, np.float64)
        assert 1.0 - _cos(a_, b_) < 1e-4, (what, 1.0 - _cos(a_, b_))
        err = np.abs(a_ - b_) / (np.abs(b_).max() + 1e-30)
        assert np.quantile(err, 0.99) < 5e-4, (what, np.quantile(err, 0.99))
    near(gc, go, "gradient vs oracle")
    near(gc, gn, "gradient vs per-layer path")
    near(mc, sto.m, "adam m")
    w0 = ora.flatten_params(Ws, bs).astype(np.float64)
    assert _cos(wc - w0, ora.flatten_params(W2, b2) - w0) > 0.99       # Adam's first step is ~lr * sign(g): compare the movement
    np.testing.assert_allclose(morec, moren, rtol=2e-3)  # later epochs + validation: the two paths stay together
    assert itc == itn
    d1, d2 = wend - ora.flatten_params(Ws, bs), wendn - ora.flatten_params(Ws, bs)
    assert _cos(d1.astype(np.float64), d2.astype(np.float64)) > 0.99


def test_chain_path_is_actually_used(ctx):
    """Trainers of stacks up to 512 wide run a chain kernel (its stamps exist): f16 / bf16 (variational heads up to 32
    latent dimensions) and, from r3 on, f32 (train_chain32.h; a variational head only on the small-batch kernel of
    train_chain32s.h); wider stacks, wider latents and variational f32 trainers of more than 2,048 rows per step take the
    per-layer path."""
    native = pkg("_native")
    st = native.Stack(ctx, [16, 32, 16], [1, 0])
    x = np.zeros((8, 16), np.float32); w = np.ones(8, np.float32)
    tr = native.Trainer(st, "f16", 8); tr.set_data(0, x, None, w)
    with pytest.raises(native.EngineError):
        tr.chain_stamps(6)          # off until asked for (they cost 2-3 us per step)
    tr.enable_stamps(); tr.run_epoch(None, 8)
    s = tr.chain_stamps(6)
    assert s[0] > 0 and np.all(np.diff(s.astype(np.int64)[:5]) > 0)
    t32 = native.Trainer(st, "f32", 8); t32.set_data(0, x, None, w); t32.enable_stamps(); t32.run_epoch(None, 8)
    s32 = t32.chain_stamps(6)
    assert s32[0] > 0 and np.all(np.diff(s32.astype(np.int64)[:5]) > 0)
    for stack, prec in ((native.Stack(ctx, [16, 600, 16], [1, 0]), "f32"), (native.Stack(ctx, [16, 600, 16], [1, 0]), "f16"),
                        (native.Stack(ctx, [16, 40, 16], [2, 0]), "bf16"), (native.Stack(ctx, [16, 40, 16], [2, 0]), "f32"),
                        (native.Stack(ctx, [16, 8, 16], [2, 0]), "f32_max_batch_4096")):
        t2 = native.Trainer(stack, prec[:3] if prec.startswith("f32") else prec, 4096 if prec.endswith("4096") else 8)
        with pytest.raises(native.EngineError):
            t2.enable_stamps()
    # a variational f32 stack of up to 32 latent dimensions and 2,048 rows per step: the small-batch f32 chain (train_chain32s.h)
    tv = native.Trainer(native.Stack(ctx, [16, 8, 16], [2, 0]), "f32", 8)
    tv.set_vae(1e-3, sample=True, seed=3); tv.set_data(0, x, None, w); tv.enable_stamps(); tv.run_epoch(None, 8)
    assert tv.chain_stamps(6)[0] > 0


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_data_parallel_arithmetic_without_a_communicator(ctx, prec):
    """What two ranks would feed the all-reduce: each takes its slice of the global batch with
    global_rows = B in the loss scale; the SUM of the two gradient arenas (and of the two loss slots)
    must be the single-process full-batch gradient (per-layer path in f32, chain kernel in f16)."""
    dims, act = [451, 96, 9, 32, 451], [1, 0, 1, 0]
    n, cut = 200, 77  # uneven split, neither part a multiple of 32
    y, w = signal_rows(n, seed=17)
    Ws, bs = ora.init_mlp(dims, seed=2)
    flat = ora.flatten_params(Ws, bs)

    def grad_of(rows, global_rows):
        st, tr = new_trainer(ctx, dims, act, flat, prec, 256, lr=0.0)
        d_x, d_w = ctx.malloc(y[rows].nbytes), ctx.malloc(w[rows].nbytes)
        ctx.h2d(d_x, np.ascontiguousarray(y[rows])); ctx.h2d(d_w, np.ascontiguousarray(w[rows]))
        tr.step_dev(d_x, None, d_w, len(y[rows]), global_rows)
        g, l = tr.get_grad().astype(np.float64), tr.last_step_loss()
        if prec != "f32":   # each slice against the rounding reference with the GLOBAL row count (loss scale and gs); the
            # loss slot holds sum_i w_i sum_j (p - y)^2 of the slice, not yet divided by the global rows (api_trainer.hip:1653)
            _half_ref_check((rows, global_rows), dims, act, Ws, bs, y[rows], y[rows], w[rows], l / global_rows, g, prec,
                            tr.last_route()[0][0], brows=global_rows)
        ctx.free(d_x); ctx.free(d_w)
        return g, l
    g_all, l_all = grad_of(slice(0, n), n)
    g_a, l_a = grad_of(slice(0, cut), n)
    g_b, l_b = grad_of(slice(cut, n), n)
    tol = 1e-5 if prec == "f32" else 2e-3
    assert abs((l_a + l_b) - l_all) / l_all < tol
    err = np.abs(g_a + g_b - g_all).max() / np.abs(g_all).max()
    assert err < tol, err


@pytest.mark.parametrize("prec", ["f16", "bf16", "f32", "f32_rows8"])
def test_variational_stack_on_the_chain_kernel(ctx, prec, monkeypatch):
    """A13 on the one-launch path: sampled latent + KL inside train_chain_kernel (f32: train_chain32s_kernel, both row
    heights), against the float64 oracle fed the same counter-based noise, and against the per-layer path in the same
    precision."""
    if prec.startswith("f32"):
        monkeypatch.setenv("V21_C32S_ROWS", "8" if prec == "f32_rows8" else "4")
        prec = "f32"
    dims = [451, 96, 9, 32, 451]
    n = 150
    y, w = signal_rows(n, seed=4)
    kl_weight, seed = 5e-3, 0x1234ABCD
    res = {}
    for chain in (True, False):
        st, tr, Ws, bs = _make_vae(ctx, dims, gl=1, seed=21, max_batch=160, prec=prec, env=_chain_env(chain))
        tr.set_vae(kl_weight, sample=True, seed=seed)
        tr.set_adam(lr=1e-3)
        tr.set_state(7)
        tr.set_data(0, y, None, w)
        if chain:
            tr.enable_stamps()
        loss = tr.run_epoch(None, n)
        res[chain] = (loss, tr.get_grad().astype(np.float64))
        if chain:
            assert tr.chain_stamps(4)[0] > 0  # really the chain kernel
    eps = ora.gauss_eps(seed, 7, n, 9)
    W = [a.astype(np.float64) for a in Ws]; b = [a.astype(np.float64) for a in bs]
    lo, go = ora.vae_loss_and_grads(W, b, 1, y.astype(np.float64), y.astype(np.float64), w.astype(np.float64), eps, kl_weight)
    (lc, gc), (ln, gn) = res[True], res[False]
    ltol, ctol = {"f16": (3e-3, 0.9995), "bf16": (3e-2, 0.995), "f32": (2e-5, 0.999999)}[prec]
    assert abs(lc - lo) / lo < ltol and abs(lc - ln) / ln < ltol, (lc, ln, lo)
    assert _cos(gc, go) > ctol and _cos(gc, gn) > ctol, (_cos(gc, go), _cos(gc, gn))
    # the KL term's own gradient reaches the z_log_var columns (they get nothing from the decoder when eps = 0)
    o = Ws[0].size + bs[0].size
    g_lv = gc[o:o + Ws[1].size].reshape(Ws[1].shape)[:, 9:]
    assert np.abs(g_lv).max() > 0


# ---- captured steps (hipGraph): SURVEY 7.1 step 6 -------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_replayed_steps_equal_eager_steps_bit_for_bit(ctx, prec):
    """A captured step replays the very kernels an eager step launches (first row / Adam step size / loss slot
    come from a device table instead of the kernel arguments): weights, Adam state and epoch losses must be
    IDENTICAL, over epochs with a partial last batch, a learning-rate change between epochs, and on the
    step_dev path."""
    dims, act = [451, 40, 9, 24, 451], [1, 0, 1, 0]
    y, w = signal_rows(300, seed=9)
    res = {}
    for graph in (True, False):
        Ws, bs = ora.init_mlp(dims, seed=21)
        st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, 128)
        tr.use_graph(graph)  # (off by default)
        tr.set_adam(lr=2e-3)
        tr.set_data(0, y, None, w)
        losses = []
        for ep in range(3):
            if ep == 2:
                tr.set_lr(5e-4)
            losses.append(tr.run_epoch(ora.epoch_permutation(300, 4, ep), 128))  # 128 + 128 + 44 rows
        d_x, d_w = ctx.malloc(y[:96].nbytes), ctx.malloc(w[:96].nbytes)
        ctx.h2d(d_x, np.ascontiguousarray(y[:96])); ctx.h2d(d_w, np.ascontiguousarray(w[:96]))
        for _ in range(5):
            tr.step_dev(d_x, None, d_w, 96, 96)
        losses.append(tr.last_step_loss())
        it, mm, vv = tr.get_state()
        res[graph] = (np.array(losses), st.get_weights(), mm, vv, it)
        ctx.free(d_x); ctx.free(d_w)
    assert res[True][4] == res[False][4] == 3 * 3 + 5
    for a, b in zip(res[True][:4], res[False][:4]):
        np.testing.assert_array_equal(a, b)


def test_replayed_steps_follow_data_and_state_changes(ctx):
    """What a captured step bakes in must be re-captured when it changes: new training data (pointers), new
    Adam betas, a restored optimizer state; and a variational stack refuses capture."""
    native = pkg("_native")
    dims, act = [7, 32, 16, 9], [1, 1, 0]
    rng = np.random.default_rng(3)

    def run(graph):
        Ws, bs = ora.init_mlp(dims, seed=4)
        st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), "f32", 64)
        tr.use_graph(graph)
        out = []
        for k in range(3):
            r = np.random.default_rng(10 + k)
            x = r.normal(size=(150 + 10 * k, 7)).astype(np.float32); yy = r.normal(size=(150 + 10 * k, 9)).astype(np.float32)
            tr.set_data(0, x, yy, ora.mse_row_weight(yy).astype(np.float32))   # new buffers every time
            tr.set_adam(lr=1e-3, beta1=0.9 - 0.1 * k)                           # betas live in kernel arguments
            out.append(tr.run_epoch(None, 64))
            if k == 1:
                it, mm, vv = tr.get_state()
                tr.set_state(it + 7, mm * 0.5, vv)                              # resumed optimizer state
        return np.array(out), st.get_weights()
    a, b = run(True), run(False)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    stv = native.Stack(ctx, [451, 32, 4, 16, 451], [1, native.ACT_GAUSS, 1, 0])
    trv = native.Trainer(stv, "f16", 32)
    with pytest.raises(native.EngineError):
        trv.use_graph(True)
    trv.use_graph(False)


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_replayed_steps_see_weights_set_between_replays(ctx, prec):
    """the lazy refresh of the packed weight copies is not part of a captured step.  An epoch
    with captured steps, then Stack.set_weights(new), then another epoch: the replayed steps must run on the NEW
    weights -- identical, bit for bit, to the same sequence executed eagerly."""
    dims, act = [451, 40, 9, 24, 451], [1, 0, 1, 0]
    y, w = signal_rows(256, seed=19)
    W2, b2 = ora.init_mlp(dims, seed=77)
    res = {}
    for graph in (True, False):
        Ws, bs = ora.init_mlp(dims, seed=21)
        st, tr = new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, 128)
        tr.use_graph(graph)
        tr.set_adam(lr=2e-3)
        tr.set_data(0, y, None, w)
        losses = [tr.run_epoch(None, 128)]
        st.set_weights(ora.flatten_params(W2, b2))      # the arena is rewritten behind the captured steps
        losses.append(tr.run_epoch(None, 128))
        res[graph] = (np.array(losses), st.get_weights())
    np.testing.assert_array_equal(res[True][0], res[False][0])
    np.testing.assert_array_equal(res[True][1], res[False][1])
    # and the second epoch really started from the new weights: its first-batch loss level is the new model's
    l0 = loss64(W2, b2, act, y[:128], y[:128], w[:128])
    assert abs(res[True][0][1] - l0) / l0 < 0.2, (res[True][0][1], l0)   # (epoch mean of two nearby batches vs batch 1)


# ---- BASELINE configs[2]: latent emulator at full width, and the joint enc + dec + emulator step ----------------
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_latent_emulator_full_width_mse_matches_oracle(ctx, prec):
    """The reference's second phase at its real size (emulator.py:657-663, :756-764): 7 -> [352, 352, 352, 224]
    -> 9 trained with mean_squared_error, batch 256 with a partial last batch, against the float64 oracle.
    f32: per-layer path at the stated f32 tolerance; f16: chain kernel, operand-rounding tolerance."""
    dims = STACKS["LE"][0]
    st, tr, Ws, bs = _make(ctx, dims, seed=12, prec=prec, max_batch=256, lr=1e-3)
    rng = np.random.default_rng(3)
    n, batch = 600, 256   # 256 + 256 + 88
    x = rng.uniform(-1, 1, size=(n, 7)).astype(np.float32)
    z = rng.normal(size=(n, 9)).astype(np.float32)
    w = ora.mse_row_weight(z).astype(np.float32)
    tr.set_data(0, x, z, w)
    sto = ora.AdamState(st.num_params, dtype=np.float64, lr=1e-3)
    W, b = [a.astype(np.float64) for a in Ws], [a.astype(np.float64) for a in bs]
    tol_l, tol_w = (2e-5, 2e-4) if prec == "f32" else (3e-3, 3e-2)
    for ep in range(2):
        loss = tr.run_epoch(ora.epoch_permutation(n, 5, ep), batch)
        W, b, hist = ora.fit(W, b, sto, x.astype(np.float64), z.astype(np.float64), w.astype(np.float64), 1, batch, seed=5,
                             dtype=np.float64, start_epoch=ep)
        assert abs(loss - hist["loss"][0]) / hist["loss"][0] < tol_l, (ep, loss, hist["loss"][0])
    # Adam's first steps move every weight by ~lr whatever the gradient's size: compare the MOVEMENT
    w0 = ora.flatten_params(Ws, bs).astype(np.float64)
    d_dev, d_ora = st.get_weights().astype(np.float64) - w0, ora.flatten_params(W, b) - w0
    if prec == "f32":
        _close(d_dev, d_ora, 5e-3, "weight movement after 2 epochs (f32)")
    else:
        cos = _cos(d_dev, d_ora)
        assert cos > 0.99 and abs(np.linalg.norm(d_dev) / np.linalg.norm(d_ora) - 1) < tol_w, (cos,)
    assert tr.get_state()[0] == 6


@pytest.mark.parametrize("prec,batch", [("f16", 128), ("f32", 128), ("f32", 300)])
def test_joint_step_is_phase_two_when_the_encoder_is_frozen(ctx, prec, batch):
    """v21_joint_*: with the autoencoder's learning rate at 0 a joint epoch must be the reference's second phase
    (emulator.py:753-764): the emulator trained on encoder(x) of exactly its batch rows.  Checked against (a) the
    float64 oracle's fit on the oracle's latents, (b) a separate device trainer fed those latents; the
    autoencoder must not move and must report the loss it reports alone."""
    native = pkg("_native")
    n = 300   # (batch 300, f32: one step per epoch, more rows than the one-launch gradient kernel of dw_adam32.h takes)
    y, wa = signal_rows(n, seed=5)
    par = np.random.default_rng(8).uniform(-1, 1, size=(n, 7)).astype(np.float32)
    ae_dims, ae_act = [451, 48, 9, 24, 451], [1, 0, 1, 0]
    em_dims, em_act = [7, 40, 9], [1, 0]
    Wa, ba = ora.init_mlp(ae_dims, seed=31)
    We, be = ora.init_mlp(em_dims, seed=32)
    z = forward64(Wa, ba, ae_act, y, layers=2)    # oracle latents: encoder = the autoencoder's first two layers
    wz = ora.mse_row_weight(z.astype(np.float32)).astype(np.float32)

    def trainer(dims, act, Ws, bs, lr):
        return new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, batch, lr=lr)
    sta, tra = trainer(ae_dims, ae_act, Wa, ba, 0.0)        # frozen autoencoder
    ste, tre = trainer(em_dims, em_act, We, be, 2e-3)
    tra.set_data(0, y, None, wa)
    tre.set_data(0, par, np.zeros((n, 9), np.float32), wz)
    joint = native.Joint(tra, tre, latent_layer=1)
    stx, trx = trainer(em_dims, em_act, We, be, 2e-3)        # (b) the same emulator on precomputed latents
    trx.set_data(0, par, z.astype(np.float32), wz)
    sto = ora.AdamState(ste.num_params, dtype=np.float64, lr=2e-3)
    W, b = [a.astype(np.float64) for a in We], [a.astype(np.float64) for a in be]
    sta2, tra2 = trainer(ae_dims, ae_act, Wa, ba, 0.0)
    tra2.set_data(0, y, None, wa)
    for ep in range(2):
        perm = ora.epoch_permutation(n, 9, ep)
        la, le = joint.run_epoch(perm, batch)
        lx = trx.run_epoch(perm, batch)
        W, b, hist = ora.fit(W, b, sto, par.astype(np.float64), z, wz.astype(np.float64), 1, batch, seed=9, dtype=np.float64,
                             start_epoch=ep)
        assert la == tra2.run_epoch(perm, batch)                      # the autoencoder half is the plain chain step
        assert abs(le - hist["loss"][0]) / hist["loss"][0] < (5e-3 if prec == "f16" else 5e-5), (ep, le, hist["loss"][0])
        assert abs(le - lx) / lx < (2e-3 if prec == "f16" else 2e-5), (ep, le, lx)   # latents from f16 operands vs fp64: tiny shift
    np.testing.assert_array_equal(sta.get_weights(), ora.flatten_params(Wa, ba))   # lr = 0: untouched
    w0 = ora.flatten_params(We, be).astype(np.float64)
    dj, dx, do = (ste.get_weights() - w0), (stx.get_weights() - w0), (ora.flatten_params(W, b) - w0)
    for d, what in ((dx, "separate trainer"), (do, "oracle")):
        cos = _cos(dj, d)
        assert cos > (0.995 if prec == "f16" else 0.9999) and abs(np.linalg.norm(dj) / np.linalg.norm(d) - 1) < (2e-2 if prec == "f16" else 2e-3), (what, cos)
    assert tra.get_state()[0] == tre.get_state()[0] == 2 * -(-n // batch)
    # argument checks
    with pytest.raises(native.EngineError):
        native.Joint(tra, tre, latent_layer=0)      # a ReLU layer, and 48 wide: not the emulator's output
    st32 = native.Stack(ctx, em_dims, em_act)
    with pytest.raises(native.EngineError):      # the two trainers must share a precision
        native.Joint(tra, native.Trainer(st32, "f32" if prec == "f16" else "f16", batch), latent_layer=1)


@pytest.mark.parametrize("prec", ["f16", "bf16", "f32"])
def test_joint_step_full_width_against_the_oracle(ctx, prec):
    """BASELINE configs[2] at its real widths: autoencoder 451 -> 352 -> 9 -> 32 -> 352 -> 451 + latent emulator
    7 -> [352, 352, 352, 224] -> 9, batch 256 with a partial last batch (600 rows = 256 + 256 + 88).
    (a) encoder frozen (lr 0): the emulator's epochs are the reference's second phase (emulator.py:753-764) --
        against the float64 oracle's fit on the oracle's latents, and the autoencoder must not move;
    (b) both models training: the autoencoder's half is bit-identical to the autoencoder trained alone (the two
        families of row blocks share nothing), and the emulator's first-step loss is its float64 loss against the
        encoder's latents of that step.
    f32 (the reference's arithmetic; csrc/train_chain32s.h: train_chain32s_joint_kernel): the same at the f32 tolerances."""
    native = pkg("_native")
    n, batch = 600, 256
    y, wa = signal_rows(n, seed=5)
    par = np.random.default_rng(8).uniform(-1, 1, size=(n, 7)).astype(np.float32)
    (ae_dims, ae_act), (em_dims, em_act) = STACKS["AE"], STACKS["LE"]
    Wa, ba = ora.init_mlp(ae_dims, seed=31)
    We, be = ora.init_mlp(em_dims, seed=32)
    z = forward64(Wa, ba, ae_act, y, layers=2)                # the oracle's latents of the initial encoder
    wz = ora.mse_row_weight(z.astype(np.float32)).astype(np.float32)
    tol_l, tol_n = {"f16": (5e-3, 3e-2), "bf16": (4e-2, 1e-1), "f32": (5e-5, 2e-3)}[prec]

    def trainer(dims, act, Ws, bs, lr):
        return new_trainer(ctx, dims, act, ora.flatten_params(Ws, bs), prec, batch, lr=lr)
    # ---- (a) frozen encoder
    sta, tra = trainer(ae_dims, ae_act, Wa, ba, 0.0)
    ste, tre = trainer(em_dims, em_act, We, be, 1e-3)
    tra.set_data(0, y, None, wa)
    tre.set_data(0, par, np.zeros((n, 9), np.float32), wz)
    joint = native.Joint(tra, tre, latent_layer=1)
    sto = ora.AdamState(ste.num_params, dtype=np.float64, lr=1e-3)
    W, b = [a.astype(np.float64) for a in We], [a.astype(np.float64) for a in be]
    for ep in range(2):
        perm = ora.epoch_permutation(n, 9, ep)
        la, le = joint.run_epoch(perm, batch)
        W, b, hist = ora.fit(W, b, sto, par.astype(np.float64), z, wz.astype(np.float64), 1, batch, seed=9, dtype=np.float64,
                             start_epoch=ep)
        assert abs(le - hist["loss"][0]) / hist["loss"][0] < tol_l, (ep, le, hist["loss"][0])
    np.testing.assert_array_equal(sta.get_weights(), ora.flatten_params(Wa, ba))   # lr = 0: untouched
    w0 = ora.flatten_params(We, be).astype(np.float64)
    dj, do = ste.get_weights() - w0, ora.flatten_params(W, b) - w0
    cos = _cos(dj, do)
    assert cos > {"f16": 0.99, "bf16": 0.9, "f32": 0.9999}[prec] and abs(np.linalg.norm(dj) / np.linalg.norm(do) - 1) < tol_n, cos
    assert tra.get_state()[0] == tre.get_state()[0] == 6
    # the one-launch validation of both models (v21_joint_eval): the autoencoder's is its own forward-only pass, bit for
    # bit; the emulator's is its loss against the (frozen) encoder's latents of the validation signals
    nv = 150
    tra.set_data(1, y[:nv], None, wa[:nv]); tre.set_data(1, par[:nv], np.zeros((nv, 9), np.float32), wz[:nv])
    va, ve = joint.evaluate()
    assert va == tra.evaluate(1, batch)
    tre.set_data(1, par[:nv], z[:nv].astype(np.float32), wz[:nv])
    vx = tre.evaluate(1, batch)
    assert abs(ve - vx) / vx < {"f16": 3e-3, "bf16": 3e-2, "f32": 2e-5}[prec], (ve, vx)
    # ---- (b) both models training
    sta, tra = trainer(ae_dims, ae_act, Wa, ba, 1e-3)
    ste, tre = trainer(em_dims, em_act, We, be, 1e-3)
    sts, trs = trainer(ae_dims, ae_act, Wa, ba, 1e-3)        # the autoencoder alone
    tra.set_data(0, y, None, wa); trs.set_data(0, y, None, wa)
    tre.set_data(0, par, np.zeros((n, 9), np.float32), wz)
    joint = native.Joint(tra, tre, latent_layer=1)
    perm = ora.epoch_permutation(n, 9, 0)
    la, le = joint.run_epoch(perm, batch)
    ls = trs.run_epoch(perm, batch)
    assert la == ls
    np.testing.assert_array_equal(sta.get_weights(), sts.get_weights())
    assert np.isfinite(le) and le > 0


@pytest.mark.parametrize("prec", ["f16", "f32"])
def test_joint_step_with_a_variational_autoencoder(ctx, prec):
    """The joint step with a (z_mean | z_log_var) head in the autoencoder (f16: train_chain.h; f32: train_chain32s.h): the emulator's targets are z_mean of the
    encoder of that step (what encoder.predict returns).  With the autoencoder frozen the emulator's epoch equals a
    separate trainer fed the float64 z_mean; with kl_weight = 0 and no sampling the autoencoder's half equals the
    deterministic autoencoder's."""
    native = pkg("_native")
    n, batch = 200, 128
    y, wa = signal_rows(n, seed=6)
    par = np.random.default_rng(9).uniform(-1, 1, size=(n, 7)).astype(np.float32)
    ae_dims, ae_act = [451, 64, 9, 32, 451], [1, native.ACT_GAUSS, 1, 0]
    em_dims, em_act = [7, 48, 9], [1, 0]
    sta = native.Stack(ctx, ae_dims, ae_act)   # (the arena's size is the stack's to tell)
    flat = (np.random.default_rng(3).normal(size=sta.num_params) * 0.05).astype(np.float32)
    sta.set_weights(flat)
    tra = native.Trainer(sta, prec, batch); tra.set_adam(lr=0.0); tra.set_vae(1e-3, sample=True, seed=5)
    We, be = ora.init_mlp(em_dims, seed=12)
    ste, tre = new_trainer(ctx, em_dims, em_act, ora.flatten_params(We, be), prec, batch, lr=2e-3)
    # float64 z_mean of the (frozen) encoder: Dense 451 -> 64 (ReLU), Dense 64 -> 18, first 9 columns
    o = 0
    W0 = flat[o:o + 451 * 64].reshape(451, 64).astype(np.float64); o += 451 * 64
    b0 = flat[o:o + 64].astype(np.float64); o += 64
    W1 = flat[o:o + 64 * 18].reshape(64, 18).astype(np.float64); o += 64 * 18
    b1 = flat[o:o + 18].astype(np.float64)
    zm = (np.maximum(y.astype(np.float64) @ W0 + b0, 0) @ W1 + b1)[:, :9]
    wz = ora.mse_row_weight(zm.astype(np.float32)).astype(np.float32)
    tra.set_data(0, y, None, wa)
    tre.set_data(0, par, np.zeros((n, 9), np.float32), wz)
    joint = native.Joint(tra, tre, latent_layer=1)
    stx, trx = new_trainer(ctx, em_dims, em_act, ora.flatten_params(We, be), prec, batch, lr=2e-3)
    trx.set_data(0, par, zm.astype(np.float32), wz)
    for ep in range(2):
        perm = ora.epoch_permutation(n, 4, ep)
        la, le = joint.run_epoch(perm, batch)
        lx = trx.run_epoch(perm, batch)
        assert np.isfinite(la) and abs(le - lx) / lx < (3e-3 if prec == "f16" else 2e-5), (ep, le, lx)
    np.testing.assert_array_equal(sta.get_weights(), flat)
    d1, d2 = ste.get_weights() - ora.flatten_params(We, be), stx.get_weights() - ora.flatten_params(We, be)
    assert _cos(d1, d2) > (0.995 if prec == "f16" else 0.99999)


@pytest.mark.parametrize("prec", ["f16", "f32"])
def test_joint_step_trains_a_sampling_variational_autoencoder_like_the_autoencoder_alone(ctx, prec):
    """Joint step, variational autoencoder at lr > 0 WITH sampling, several steps per epoch and two epochs: the
    autoencoder's half must be, bit for bit, the autoencoder trained alone on the same permutations -- which holds only
    if every optimizer step of the joint epoch keys its noise on its own step number (ChainStep::step_off; ADVICE r3:
    the f32 branch of v21_joint_run_epoch drew the same eps in every step of an epoch)."""
    native = pkg("_native")
    n, batch = 300, 128                                   # 3 steps per epoch, the last one partial
    y, wa = signal_rows(n, seed=16)
    par = np.random.default_rng(19).uniform(-1, 1, size=(n, 7)).astype(np.float32)
    ae_dims, ae_act = [451, 64, 9, 32, 451], [1, native.ACT_GAUSS, 1, 0]
    em_dims, em_act = [7, 48, 9], [1, 0]
    flat = (np.random.default_rng(13).normal(size=native.Stack(ctx, ae_dims, ae_act).num_params) * 0.05).astype(np.float32)
    We, be = ora.init_mlp(em_dims, seed=12)

    def ae_trainer():
        st, tr = new_trainer(ctx, ae_dims, ae_act, flat, prec, batch, lr=1e-3)
        tr.set_vae(1e-2, sample=True, seed=77)
        tr.set_data(0, y, None, wa)
        return st, tr
    sta, tra = ae_trainer()
    sts, trs = ae_trainer()                               # the autoencoder alone
    ste, tre = new_trainer(ctx, em_dims, em_act, ora.flatten_params(We, be), prec, batch, lr=2e-3)
    tre.set_data(0, par, np.zeros((n, 9), np.float32), np.full(n, 1 / 9, np.float32))
    joint = native.Joint(tra, tre, latent_layer=1)
    for ep in range(2):
        perm = ora.epoch_permutation(n, 21, ep)
        la, le = joint.run_epoch(perm, batch)
        ls = trs.run_epoch(perm, batch)
        assert la == ls, (ep, la, ls)
        np.testing.assert_array_equal(sta.get_weights(), sts.get_weights())
        assert np.isfinite(le) and le > 0
    # and the noise really differs from step to step: with the same draw in every step the epoch would equal one
    # trained with the key frozen at the epoch's first step, which the stand-alone trainer above is not
    assert tra.get_state()[0] == trs.get_state()[0] == 6


@pytest.mark.parametrize("prec", ["f16", "f32"])
def test_autoencoder_emulator_joint_training_through_the_class_surface(ctx, prec):
    """AutoEncoderEmulator.train(joint=True): both histories fill, the models learn, early stopping of the
    autoencoder freezes it and the emulator goes on (the reference's phase 2), predict works afterwards.  f16 and the
    reference's arithmetic (f32: train_chain32s_joint_kernel)."""
    synth, emu, optm, cbm = pkg("synth"), pkg("emulator"), pkg("optimizers"), pkg("callbacks")
    data = synth.make_dataset(1200, 200, 100)
    pkg("engine").set_random_seed(3)
    ae = emu.AutoEncoderEmulator(precision=prec, enc_hidden_dims=[64], dec_hidden_dims=[32, 64], em_hidden_dims=[64, 64], **data)
    ae.autoencoder.compile(optimizer=optm.Adam(2e-3), loss=emu.relative_mse_loss(ae.signal_train))
    ae.emulator.compile(optimizer=optm.Adam(2e-3), loss=emu.mean_squared_error)

    class StopAt:
        def __init__(self, k): self.k = k
        def set_model(self, m): self.model = m
        def on_epoch_end(self, epoch, logs=None):
            if epoch + 1 >= self.k: self.model.stop_training = True
    out = ae.train(epochs=6, ae_callbacks=[StopAt(3)], em_callbacks=[], verbose=0, joint=True)
    ae_loss, ae_val, em_loss, em_val = out
    assert len(ae_loss) == len(ae_val) == 3 and len(em_loss) == len(em_val) == 6
    assert ae_loss[-1] < ae_loss[0]
    assert em_loss[5] < em_loss[3]  # (while the encoder still moves its latents the target moves too; once frozen, phase 2)
    assert all(np.isfinite(v) for v in ae_val + em_val)
    p = ae.predict(data["par_test"][:5])
    assert p.shape == (5, 451) and np.isfinite(p).all()
    with pytest.raises(ValueError):   # the emulator's loss must not depend on the targets
        ae.emulator.compile(optimizer=optm.Adam(1e-3), loss=emu.relative_mse_loss(ae.signal_train))
        ae.train(epochs=1, verbose=0, joint=True)


def test_a_script_that_ends_with_live_joint_sweep_and_trainers_exits_cleanly(tmp_path):
    """Objects left in a script's namespace are finalized in arbitrary order at interpreter exit (r4: a Trainer freed before
    the Joint built on it crashed the process AFTER its last line).  A fresh interpreter builds trainers, a joint object and
    a sweep at module level next to a function (the cycle through the module namespace), steps them, and must leave with
    status 0."""
    import subprocess, sys, textwrap
    script = tmp_path / "leave_objects_behind.py"
    script.write_text(textwrap.dedent('''
        import importlib, os, sys
        import numpy as np
        sys.path.insert(0, %r)
        native = importlib.import_module("21cmvae_amd._native")
        ctx = native.Context.default()
        def make(dims, act, n=64):
            st = native.Stack(ctx, dims, act)
            st.set_weights((np.random.default_rng(0).normal(size=st.num_params) * 0.05).astype(np.float32))
            tr = native.Trainer(st, "f16", n); tr.set_adam(lr=1e-3)
            return st, tr
        x = np.random.default_rng(1).uniform(-1, 1, size=(64, 33)).astype(np.float32)
        p = np.random.default_rng(2).uniform(-1, 1, size=(64, 7)).astype(np.float32)
        w = np.full(64, 1.0 / 33, np.float32)
        sa, ta = make([33, 16, 4, 16, 33], [1, 0, 1, 0]); se, te = make([7, 16, 4], [1, 0])
        ta.set_data(0, x, None, w); te.set_data(0, p, np.zeros((64, 4), np.float32), np.full(64, 0.25, np.float32))
        joint = native.Joint(ta, te, latent_layer=1)
        print(joint.run_epoch(None, 32))
        members = [make([33, 8 + k, 33], [1, 0]) for k in range(3)]
        members[0][1].set_data(0, x, None, w)
        sweep = native.Sweep([m[1] for m in members])
        print(sweep.run_epoch(None, 32))
        keep = [joint, sweep, members, sa, se]       # and a cycle of our own
        keep.append(keep)
    ''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    for _ in range(3):   # (the order depends on addresses: a few tries)
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])


def test_created_and_destroyed_handles_give_their_device_memory_back(ctx):
    """Every device buffer of a stack and a trainer is owned by a member whose destructor frees it (csrc/api_internal.h:
    Dev).  One warm-up round, then 200 rounds of stack + trainer (f16, and f32 with a variational head) + set_data + one
    step + destroy: the device's free memory may fall by what the allocator keeps, but by less than ONE round holds while
    alive -- a single trainer buffer forgotten per round would show as 200 of them."""
    import gc
    native = pkg("_native")
    n = 256
    x = np.random.default_rng(0).uniform(-1, 1, size=(n, 451)).astype(np.float32)
    w = np.full(n, 1.0 / 451, np.float32)

    def build():
        objs = []
        for act, prec in (([1, 0, 1, 1, 0], "f16"), ([1, 2, 1, 1, 0], "f32")):
            st = native.Stack(ctx, [451, 352, 9, 32, 352, 451], act)
            st.set_weights((np.random.default_rng(1).normal(size=st.num_params) * 0.03).astype(np.float32))
            tr = native.Trainer(st, prec, n)
            tr.set_adam(lr=1e-4)
            tr.set_data(0, x, None, w)
            tr.set_data(1, x[:100], None, w[:100])
            assert np.isfinite(tr.run_epoch(None, n))
            objs += [tr, st]
        return objs

    def free_bytes():
        gc.collect()
        ctx.sync()
        return torch.cuda.mem_get_info()[0]

    del build()[:]
    before = free_bytes()
    alive = build()
    held = before - free_bytes()
    del alive[:]
    for _ in range(200):
        del build()[:]
    fall = before - free_bytes()
    print("one round holds %d bytes while alive; free memory fell by %d bytes over 200 rounds" % (held, fall))
    assert held > 0
    assert fall < held, (fall, held)


@pytest.mark.parametrize("rows_per_wave", [32, 16])
def test_fused_training_gathers_the_resident_16_bit_copy_with_identical_results(ctx, rows_per_wave, monkeypatch):
    """v21_trainer_set_data keeps the training inputs of a trainer with a fused training kernel as 16-bit rows as well
    (ChainStep::x16); a fused step that reads rows of the RESIDENT set gathers those instead of the fp32 rows (half the bytes of
    the step's largest read).  The same step on a caller's own device copy of the same rows gathers fp32 and rounds in the
    kernel: the operands are the same 16-bit values, so loss, gradient and weights must be identical bit for bit -- whole set,
    and a slice of the resident set stepped through its device pointers (v21_trainer_get_data_dev)."""
    monkeypatch.setenv("V21_FUSED_TRAIN_ROWS", "1")
    monkeypatch.setenv("V21_FUSED_TRAIN16", "1" if rows_per_wave == 16 else "0")
    name, dims, act, ae = FUSED_TRAIN_STACKS[0]
    n = 500
    x, w = signal_rows(n, seed=12)
    Ws, bs = ora.init_mlp(dims, seed=5)
    flat = ora.flatten_params(Ws, bs)
    res = []
    for resident in (True, False):
        st, tr = new_trainer(ctx, dims, act, flat, "f16", n, lr=1e-3)
        tr.set_data(0, x, None, w)
        if resident:
            d_x, d_y, d_rw, rows = tr.data_dev(0)
            assert rows == n and d_y == d_x
        else:
            d_x, d_rw = ctx.malloc(x.nbytes), ctx.malloc(w.nbytes)
            ctx.h2d(d_x, x); ctx.h2d(d_rw, w)
        out = []
        for first, cnt in ((0, n), (123, 300)):      # the whole set, then rows 123 .. 422
            tr.step_dev(d_x + 4 * 451 * first, None, d_rw + 4 * first, cnt, cnt)
            out.append((tr.last_step_loss(), tr.get_grad()))
        res.append((out, st.get_weights(), tr.route_counters()))
        if not resident:
            ctx.free(d_x); ctx.free(d_rw)
    (oa, wa, ca), (ob, wb, cb) = res
    assert ca["fused"] == cb["fused"] == 2
    for (la, ga), (lb, gb) in zip(oa, ob):
        assert la == lb and np.array_equal(ga, gb)
    assert np.array_equal(wa, wb)


@pytest.mark.parametrize("name,dims,act,prec,rows,use_perm,max_batch", [
    ("AE", None, None, "f16", 16384, True, 16384),       # fused_train16, two rounds of workgroups
    ("AE", None, None, "bf16", 16389, False, 16400),     # ragged, no row table
    ("D1", None, None, "f16", 8197, True, 16384),        # input width 7: one feature tile that also holds the bias feature
    ("AE", None, None, "f16", 24581, True, 32768),       # the 32-rows-per-wave kernel
    ("X64", [64, 96, 64], [1, 0], "f16", 9000, True, 16384),  # run-time kernel; input width a multiple of 32: the bias feature's tile lies past the row pitch
])
def test_layer0_gradient_operand_gathered_from_resident_rows_is_bit_identical(ctx, monkeypatch, name, dims, act, prec, rows, use_perm, max_batch):
    """r5: a fused large step on rows of the resident training set no longer flushes a duplicate of its
    input rows as the layer-0 weight-gradient operand; gemm_dw16_lds_kernel's loader waves gather the set's 16-bit rows through
    the step's row table and the compute waves read them through the hardware transpose (train_chain.h: DwXRows).  The operand
    values and the order of every sum are those of the flushed form (V21_DW_XROWS=0): loss, FULL gradient and weights after two
    more epochs must be identical bit for bit -- and match the float64 oracle."""
    if dims is None:
        dims, act = STACKS[name]
    n = rows   # the first epoch is ONE step of all rows (through the row table when there is one); the later epochs take steps of
    x, y, w = stack_data(dims, n, seed=31)   # 9,000 / 8,200 rows out of the set and a partial last step
    rng = np.random.default_rng(9)
    perm = rng.permutation(n).astype(np.int32) if use_perm else None
    more = ((perm, 9000), (None, 8200))
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("V21_DW_XROWS", flag)
        twins, weights = twin_steps(ctx, dims, act, prec, max_batch, x, y, w, perm, rows, more=more, wait_jit=name == "X64")
        assert twins[0][3][0] in ("fused64", "fused128") and twins[0][3][1] == "dw16_splitk", twins[0][3]
        assert_step_matches_oracle((name, prec, rows, flag), twins, weights, act, x, y, w, perm, rows, prec)
        res[flag] = twins[0]
    (l1, g1, w1, _, _), (l0, g0, w0, _, _) = res["1"], res["0"]
    assert l1 == l0
    assert np.array_equal(g1, g0), "gradient differs: max %.3e" % np.abs(g1 - g0).max()
    assert np.array_equal(w1, w0)
