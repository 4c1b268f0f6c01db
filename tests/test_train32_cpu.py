"""The table of tests/train32_cases.py on the host: what tests/test_train32_gpu.py relies on, shown without a GPU.

* no (case, rows) entry has a ReLU pre-activation within 1e-5 of its kink at the weights of any of its three steps, so the
  strict gradient check needs no excuse for a ReLU taken the other way;
* the reference alone stays inside the strict bounds: the same step in numpy float32 passes against float64;
* every entry of the mutation catalogue is refused by more than 4 x a bound wherever it applies;
* the Adam bounds are 4 x the worst error of a numpy float32 evaluation of adam_update_element's expressions on the
  table's own gradients, and four wrong variants of the formula exceed them by more than 4 x;
* the literal route table equals the library's decision under every arm's environment, reaches every pair of forward and
  update route, and sends big64 through the 64-tile one-launch update."""
import numpy as np
import pytest

import train32_cases as tc
from conftest import pkg

ENTRIES = [(c, k) for c in tc.CASES for k in range(len(c.rows))]


@pytest.fixture(scope="module")
def model():
    """model_steps of every entry, computed once: {(case name, k): [step tuples]}"""
    return {(c.name, k): list(tc.model_steps(c, k)) for c, k in ENTRIES}


def test_the_table_is_well_formed():
    assert len({c.name for c in tc.CASES}) == len(tc.CASES) and len(tc.ARMS) == 10
    for c in tc.CASES:
        assert len(c.dims) == len(c.act) + 1 and c.act[-1] == tc.LINEAR and max(c.dims) <= 512
        assert not c.y_is_x or c.dims[0] == c.dims[-1]
        for u in tc.UPD_ROUTES[c.name].values():
            assert isinstance(u, str) or len(u) == len(c.rows)
    assert all(BY in tc.BY_NAME and r in tc.BY_NAME[BY].rows for BY, r in tc.DATA_SEED)
    assert [tc.short_rows(r) for r in (1, 2, 5, 9, 16, 257, 300, 2048)] == [0, 1, 4, 4, 12, 252, 299, 2044]


def test_no_relu_pre_activation_is_a_kink_candidate(model):
    total = 0
    for c, k in ENTRIES:
        if tc.RELU not in c.act:
            continue
        counts = [tc.kink_candidates(c, s[1], s[4]) for s in model[(c.name, k)]]
        print("TRAIN32 kinks %-7s rows %-4d seed %-5d candidates per step %s" % (c.name, c.rows[k], tc.DATA_SEED.get((c.name, c.rows[k]), 100), counts))
        assert counts == [0] * tc.STEPS, (c.name, c.rows[k], counts)
        total += 1
    assert total >= 20


def test_float32_numpy_step_passes_the_strict_check(model):
    worst = {}
    for c, k in ENTRIES:
        for (t, flat, pm, pv, x, tgt, w, lo, go, _) in model[(c.name, k)]:
            l32, g32 = tc.step32(c, flat, x, tgt, w)
            e = tc.strict_errors(c.dims, l32, g32, lo, go)
            assert tc.strict_ok(e), (c.name, c.rows[k], t, e)
            for q, v in e.items():
                worst[q] = max(worst.get(q, 0.0), v)
            r2 = tc.short_rows(c.rows[k])
            if t == 1 and r2:   # the shorter step at the start weights (test_train32_gpu, item 7)
                lo2, go2 = tc.oracle(c, flat, x[:r2], tgt[:r2], w[:r2])
                e = tc.strict_errors(c.dims, *tc.step32(c, flat, x[:r2], tgt[:r2], w[:r2]), lo2, go2)
                assert tc.strict_ok(e) and tc.kink_candidates(c, flat, x[:r2]) == 0, (c.name, c.rows[k], r2, e)
    print("TRAIN32 float32 numpy against float64, worst: loss %.1e (tol %.0e) layer %.1e (tol %.0e) 1 - cos %.1e (tol %.0e) norm ratio %.1e (tol %.0e)" % (
        worst["loss"], tc.TOL_LOSS, worst["layer"], tc.TOL_LAYER, worst["cos1"], 1 - tc.TOL_COS, worst["ratio"], tc.TOL_RATIO))


def test_every_mutation_is_refused_by_four_times_a_bound(model):
    smallest, applied = {}, {}
    for c, k in ENTRIES:
        t, flat, pm, pv, x, tgt, w, lo, go, _ = model[(c.name, k)][0]
        for name, fn in tc.mutations(c):
            r = fn(c, flat, x, tgt, w, lo, go)
            if r is None:
                continue
            e = tc.strict_errors(c.dims, r[0], r[1], lo, go)
            over = max(v for v in tc.strict_excess(e).values() if np.isfinite(v)) if np.any(r[1]) else np.inf
            kind = name.rsplit("_l", 1)[0]
            applied.setdefault(kind, set()).add(c.name)
            if over < smallest.get(kind, (np.inf,))[0]:
                smallest[kind] = (over, c.name, c.rows[k], name)
            assert over > 4.0 and not tc.strict_ok(e), (c.name, c.rows[k], name, e)
    for kind, (over, cname, rows, name) in sorted(smallest.items()):
        print("TRAIN32 mutation %-14s smallest effect %.1e x its bound (%s rows %d, %s); applied on %s" % (kind, over, cname, rows, name, sorted(applied[kind])))
    assert set(smallest) == {"last_row", "rows_from_256", "bias_row", "last_element", "relu_mask", "tile"}
    # where they apply: the two row mutations and the bias row everywhere (rows_from_256: above 256 rows), a ReLU mask on
    # every case with a ReLU, a neighbouring tile wherever a block has two tiles
    assert applied["last_row"] == applied["bias_row"] == set(tc.BY_NAME)
    assert applied["rows_from_256"] == {c.name for c in tc.CASES if max(c.rows) > 256}
    assert applied["relu_mask"] == {c.name for c in tc.CASES if tc.RELU in c.act}
    assert applied["tile"] == {c.name for c in tc.CASES if max(c.dims) >= 63}


def test_adam_bounds_are_four_times_the_float32_model(model):
    worst = {"m": 0.0, "v": 0.0, "w": 0.0}
    over = {}   # (variant, case name): the most any step of the case's entries exceeds a bound by
    for c, k in ENTRIES:
        for (t, flat, pm, pv, x, tgt, w, lo, go, (m, v, wn)) in model[(c.name, k)]:
            g = go.astype(np.float32)
            for q, e in zip("mvw", tc.adam_errors(flat, pm, pv, g, t, m, v, wn)):
                worst[q] = max(worst[q], e)
            for variant in tc.ADAM_CONTROLS:   # a wrong formula, evaluated exactly, against the bounds
                e = tc.adam_errors(flat, pm, pv, g, t, *tc.adam_eval(flat, pm, pv, g, t, np.float64, variant))
                o = max(x_ / tc.ADAM_TOL[q] for q, x_ in zip("mvw", e))
                if variant != "eps_in_sqrt":   # these three move every element of every step
                    assert o > 4.0, (variant, c.name, c.rows[k], t, o)
                over[(variant, c.name)] = max(over.get((variant, c.name), 0.0), o)
    print("TRAIN32 adam float32 model, worst: m %.3e v %.3e w %.3e; bounds m %.1e v %.1e w %.1e" % (
        worst["m"], worst["v"], worst["w"], tc.ADAM_TOL["m"], tc.ADAM_TOL["v"], tc.ADAM_TOL["w"]))
    for variant in tc.ADAM_CONTROLS:
        o, cname = min((over[(variant, c.name)], c.name) for c in tc.CASES)
        print("TRAIN32 adam control %-13s least %.1e x its bound (%s)" % (variant, o, cname))
    # pinned: the constants in train32_cases.py are these measurements, rounded up in the third digit (the window: another
    # host's float64 matrix product may sum in another order and move a float32 gradient element by an ulp)
    for q in "mvw":
        assert tc.ADAM_MODEL_WORST[q] / 1.5 <= worst[q] <= 1.5 * tc.ADAM_MODEL_WORST[q], (q, worst[q], tc.ADAM_MODEL_WORST[q])
        assert tc.ADAM_TOL[q] == 4 * tc.ADAM_MODEL_WORST[q]
    # eps inside the square root differs from eps outside only where sqrt(v) is not far above eps = 1e-7: the one-layer
    # case o1 has two gradient elements, both of order 1, and cannot tell the two apart; every other case has such elements
    for c in tc.CASES:
        assert over[("eps_in_sqrt", c.name)] > 4.0 or c.name == "o1", (c.name, over[("eps_in_sqrt", c.name)])


@pytest.fixture
def arm(monkeypatch):
    return lambda fwd, upd: tc.set_arm(monkeypatch, fwd, upd)


def test_route_table_equals_the_decision_under_every_arm(arm):
    native = pkg("_native")
    reached = set()
    for fwd, upd in tc.ARMS:
        arm(fwd, upd)
        for c, k in ENTRIES:
            d = tc.data(c, k)
            got = native.route_train(c.dims, c.act, "f32", d["max_batch"], c.rows[k])
            assert got == tc.expected_route(c, k, fwd, upd), (c.name, c.rows[k], fwd, upd, got)
            reached.add(got)
    assert reached >= {(f, u) for f in ("chain32", "chain32s_4", "chain32s_8") for u in ("dwadam32", "nt_dwadam", "nt_sliced")}
    assert ("per_layer", "per_layer") in reached
    # one rank, V21_DW32_LDS unset, not dwadam32: plan_update32 took nt_dwadam because dw32_tile is 64
    big = tc.BY_NAME["big64"]
    for fwd in ("chain32", "chain32s_8", "chain32s_4"):
        assert tc.expected_route(big, 0, fwd, "default") == (fwd, "nt_dwadam")
    assert sum(((a + 1 + 63) // 64) * ((b + 63) // 64) for a, b in zip(big.dims[:-1], big.dims[1:])) >= 192
