"""The f32 training kernels at the shapes of tests/train32_cases.py, on the device: train_chain32.h and train_chain32s.h
(forward, activation gradients, validation), dw_adam32.h and gemm_nt_dwadam_kernel<1 | 2> (weight gradients, Adam, packed
streams), adam_repack_kernel (the element-wise packer and Adam) and the per-layer path, under ten arms: three forward
routes x three update routes, and V21_TRAIN_CHAIN=0.

Per (case, forward route), for every rows entry and update arm, at lr = 1e-2 (Adam moves every weight by percents of its
size per step: a stale packed copy cannot hide):
1. the route the launch sites recorded is the literal table's (a switch the library did not read would pass all the rest);
2. three steps over the whole split: the loss against the float64 forward loss of the arena weights before the step, the
   FULL gradient against the float64 gradient at those weights by the strict check (every layer's block 2e-6, cosine
   0.999999, norm ratio 2e-4 -- no kink excuse: test_train32_cpu holds the kink candidates of these inputs at zero), and
   (m, v, w) against float64 Adam driven by the device's own gradient and previous state, within 4 x the float32 model's
   worst error;
3. a fresh Stack and Trainer handed the weights and the state take step 4 to the same bits: its streams come from the
   element-wise packer reading the arena, the old trainer's were scattered by three one-launch epilogues;
4. the validation pass on rows // 2 + 1 other rows against its float64 loss;
5. tile-32 cases up to 256 rows: register operands (V21_DW32_LDS=0) and LDS operands agree bit for bit;
6. once per case, the chain's FORWARD mode at these widths;
7. a shorter step after a longer one on the same trainer, both at lr = 0 (the weights stay the start weights, where no ReLU
   is near its kink): the shorter step's loss and gradient meet the strict check, so nothing of the longer step's rows that
   is left in the padding of the gradient operands enters the contraction.

Recorded on the MI355X (worst over every arm, rows entry and step of the case; bounds: loss 2e-5, layer 2e-6, 1 - cos 1e-6,
norm ratio 2e-4, Adam m 6.0e-7 / v 8.4e-7 / w 1.1e-5, validation 2e-5, forward 2e-5; "short": the layer error of item 7):
  case    loss     layer    1 - cos  ratio    adam m   adam v   adam w   val      short    forward (table)
  o1      2.2e-07  1.1e-07  3.6e-16  1.1e-07  4.5e-08  8.0e-08  5.1e-08  1.2e-07  4.7e-08  5.3e-08
  i1h3    9.1e-08  1.9e-07  1.3e-14  1.2e-07  5.8e-08  7.2e-08  9.1e-08  6.9e-08  1.1e-07  5.3e-08
  tails   1.6e-07  3.0e-07  1.9e-14  7.9e-08  1.5e-07  1.7e-07  4.1e-07  1.1e-07  1.7e-07  1.3e-07
  full64  8.4e-08  3.9e-07  5.1e-14  3.2e-08  1.3e-07  1.8e-07  3.2e-07  1.4e-07  2.1e-07  2.4e-07
  latent  1.0e-07  4.8e-07  5.9e-14  1.4e-07  1.4e-07  1.9e-07  6.0e-07  1.6e-07  2.1e-07  1.6e-07
  k16     8.3e-08  2.6e-07  2.5e-14  7.5e-08  1.4e-07  1.9e-07  3.1e-07  4.7e-08  1.7e-07  1.9e-07
  big64   3.4e-08  5.3e-07  1.0e-13  4.4e-08  1.5e-07  2.2e-07  2.7e-06  2.8e-08  5.3e-07  7.2e-07
  slabs   6.7e-08  2.3e-07  2.6e-14  8.1e-08  1.4e-07  1.8e-07  5.9e-07  5.4e-08  1.9e-07  2.3e-07
Every (case, rows, arm) ran and passed, the whole module in under four seconds: every pair of {chain32, chain32s_8,
chain32s_4} x {dwadam32, nt_dwadam, nt_sliced} and the per-layer path, big64's default arm on the 64-tile
gemm_nt_dwadam_kernel<2>.  Three deliberate breaks of the kernels, each in a scratch build, make the module fail: the
scalar tail of the format-4 stream store of dw_adam32.h skipping the last weight row (items 2 and 3 on o1, i1h3, tails,
latent under both chain32s routes), the `kk + e >= K` select of dw_adam32.h removed (item 7 under chain32s_4 on seven of
the eight cases; items 1 - 6 cannot see it: rows past the batch are zeros in the operands a step of the same length left),
and the last of the 16 chunks of the NT == 1 contraction split of train_chain32.h left out of the sum (items 2 and 6 on latent).
"""
import numpy as np
import pytest

import train32_cases as tc
from conftest import pkg

pytestmark = pytest.mark.gpu

FWDS = ("chain32", "chain32s_8", "chain32s_4", "per_layer")


def _trainer(native, ctx, case, d, flat):
    st = native.Stack(ctx, case.dims, case.act)
    st.set_weights(flat)
    tr = native.Trainer(st, "f32", d["max_batch"])
    tr.set_adam(lr=tc.LR, beta1=tc.BETA1, beta2=tc.BETA2, eps=tc.EPS)
    tr.set_data(0, d["x"], d["y"], d["w"])
    tr.set_data(1, d["xv"], d["yv"], d["wv"])
    return st, tr


def _short_step(native, ctx, case, k, tag, worst):
    """item 7 for one (rows entry, arm)"""
    d = tc.data(case, k)
    r2 = tc.short_rows(d["rows"])
    if not r2:
        return
    x, tgt, w = tc.step_rows(d)
    flat = tc.start_weights(case)[2]
    st, tr = _trainer(native, ctx, case, d, flat)
    tr.set_lr(0.0)
    tr.run_epoch(d["perm"], d["rows"])
    tr.set_data(0, x[:r2], None if case.y_is_x else tgt[:r2], w[:r2])
    loss = tr.run_epoch(None, r2)
    lo, go = tc.oracle(case, flat, x[:r2], tgt[:r2], w[:r2])
    e = tc.strict_errors(case.dims, loss, tr.get_grad(), lo, go)
    worst["short"] = max(worst.get("short", 0.0), e["layer"])
    assert tc.strict_ok(e), (tag, "%d rows after %d" % (r2, d["rows"]), e)
    assert np.array_equal(st.get_weights(), flat), (tag, "lr = 0 moved the weights")


def _run_entry(native, ctx, case, k, fwd, upd, worst):
    """items 1 - 4 for one (rows entry, arm) -> what item 5 compares: [(loss, gradient, w, m, v)] of the three steps"""
    d = tc.data(case, k)
    rows, tag = d["rows"], (case.name, d["rows"], fwd, upd)
    x, tgt, w = tc.step_rows(d)
    _short_step(native, ctx, case, k, tag, worst)
    st, tr = _trainer(native, ctx, case, d, tc.start_weights(case)[2])
    if fwd.startswith("chain32s"):
        tr.check_chain_jobs()
    flat0 = st.get_weights()
    trace = []
    for t in range(1, tc.STEPS + 1):
        before = st.get_weights()
        it, pm, pv = tr.get_state()
        assert it == t - 1, tag
        loss = tr.run_epoch(d["perm"], rows)
        if t == 1:
            assert tr.last_route()[0] == tc.expected_route(case, k, fwd, upd), (tag, tr.last_route()[0])
        g = tr.get_grad()
        lo, go = tc.oracle(case, before, x, tgt, w)
        e = tc.strict_errors(case.dims, loss, g, lo, go)
        for q, v_ in e.items():
            worst[q] = max(worst.get(q, 0.0), v_)
        assert tc.strict_ok(e), (tag, "step %d" % t, e)
        it, m, v = tr.get_state()
        after = st.get_weights()
        assert it == t, tag
        ea = tc.adam_errors(before, pm, pv, g, t, m, v, after)
        for q, v_ in zip("mvw", ea):
            worst["adam_" + q] = max(worst.get("adam_" + q, 0.0), v_)
            assert v_ <= tc.ADAM_TOL[q], (tag, "step %d" % t, "adam " + q, v_, tc.ADAM_TOL[q])
        trace.append((loss, g, after, m, v))
    # 4. the forward-only instantiations at these widths
    val = tr.evaluate(1, rows)
    vo = tc.val_loss64(case, st.get_weights(), d)
    worst["val"] = max(worst.get("val", 0.0), abs(val - vo) / vo)
    assert abs(val - vo) <= tc.TOL_LOSS * vo, (tag, "validation", val, vo)
    # 3. the weights moved, layer by layer, so a stale stream would show ...
    offs = np.cumsum([0] + [a * b + b for a, b in zip(case.dims[:-1], case.dims[1:])])
    now = st.get_weights()
    for l in range(len(case.act)):
        a, b = now[offs[l]:offs[l + 1]].astype(np.float64), flat0[offs[l]:offs[l + 1]].astype(np.float64)
        assert np.linalg.norm(a - b) > 1e-2 * np.linalg.norm(b), (tag, "layer %d did not move" % l)
    # ... and a fresh trainer, whose streams the element-wise packer writes from the arena, takes step 4 to the same bits
    it, m, v = tr.get_state()
    st2, tr2 = _trainer(native, ctx, case, d, now)
    tr2.set_state(it, m, v)
    l_a, l_b = tr.run_epoch(d["perm"], rows), tr2.run_epoch(d["perm"], rows)
    assert tr2.last_route()[0] == tr.last_route()[0] == tc.expected_route(case, k, fwd, upd), tag
    g_a, g_b = tr.get_grad(), tr2.get_grad()
    (it_a, m_a, v_a), (it_b, m_b, v_b) = tr.get_state(), tr2.get_state()
    w_a, w_b = st.get_weights(), st2.get_weights()
    assert it_a == it_b == tc.STEPS + 1, tag
    assert l_a == l_b and np.array_equal(g_a, g_b) and np.array_equal(w_a, w_b) and np.array_equal(m_a, m_b) and np.array_equal(v_a, v_b), (
        tag, "step 4 of a freshly packed trainer differs: loss %r %r, gradient max diff %.2e in %d elements, weights %.2e, m %.2e, v %.2e" % (
            l_a, l_b, np.abs(g_a - g_b).max(), int((g_a != g_b).sum()), np.abs(w_a - w_b).max(), np.abs(m_a - m_b).max(), np.abs(v_a - v_b).max()))
    return trace


@pytest.mark.parametrize("fwd", FWDS)
@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_f32_step_at_odd_shapes(ctx, case, fwd, monkeypatch):
    native = pkg("_native")
    worst, traces = {}, {}
    for k in range(len(case.rows)):
        for upd in tc.upd_arms_of(fwd):
            tc.set_arm(monkeypatch, fwd, upd)
            traces[(k, upd)] = _run_entry(native, ctx, case, k, fwd, upd, worst)
    # 5. register operands against LDS operands: the same split of the batch over the waves, the same MFMA order, the same
    # epilogue (tests/test_variants_gpu.py promises it on the autoencoder stack).  Item 1 showed that the switch took effect.
    n5 = 0
    for k, rows in enumerate(case.rows):
        if fwd == "per_layer" or rows > 256 or tc.UPD_ROUTES[case.name]["default"] != "dwadam32":
            continue
        for t, (a, b) in enumerate(zip(traces[(k, "default")], traces[(k, "lds0")])):
            assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:])), (
                case.name, rows, fwd, "step %d: dwadam32 and nt_dwadam differ: loss %r %r, gradient max diff %.2e, weights %.2e" % (
                    t + 1, a[0], b[0], np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max()))
        n5 += 1
    assert n5 == (0 if fwd == "per_layer" or case.name == "big64" else sum(r <= 256 for r in case.rows))
    print("TRAIN32 %-7s %-10s loss %.1e layer %.1e 1-cos %.1e ratio %.1e | adam m %.1e v %.1e w %.1e | val %.1e | short %.1e | %d entries x %d arms" % (
        case.name, fwd, worst["loss"], worst["layer"], worst["cos1"], worst["ratio"], worst["adam_m"], worst["adam_v"], worst["adam_w"],
        worst["val"], worst.get("short", 0.0), len(case.rows), len(tc.upd_arms_of(fwd))))


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_f32_chain_forward_mode_at_odd_shapes(ctx, case):
    """6. train_chain32.h in FORWARD mode (the table route) on the largest rows entry, at 2e-5 of the output's largest magnitude"""
    native = pkg("_native")
    k = len(case.rows) - 1
    d = tc.data(case, k)
    flat = tc.start_weights(case)[2]
    assert native.route_forward(case.dims, case.act, "f32", d["rows"], flags=native.FWD_FORCE_CHAIN) == "table"
    st = native.Stack(ctx, case.dims, case.act)
    st.set_weights(flat)
    out = st.forward(d["x"], "f32", native.FWD_FORCE_CHAIN)
    assert st.last_route()[0] == "table"
    ref = tc.forward64(case, flat, d["x"])
    err = float(np.abs(out - ref).max() / np.abs(ref).max())
    print("TRAIN32 %-7s forward (table) rows %d: max |error| / max |y| %.1e" % (case.name, d["rows"], err))
    assert err < 2e-5, (case.name, err)
