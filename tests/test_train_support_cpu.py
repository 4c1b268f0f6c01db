"""tests/train_support.py against oracle/ref_numpy.py: the shared float64 forward and the step oracle are the oracle's own
arithmetic on an all-ReLU stack, the partial forward and the loss agree with the full pass on a stack with a linear layer
inside, and forced_env puts back exactly what it found."""
import os

import numpy as np
import pytest

from helpers import init_weights, oracle_step
from oracle import ref_numpy as ora
from train_support import forced_env, forward64, layers64, loss64

DIMS, ROWS = [7, 12, 5, 3], 4
VAR = "TRAIN_SUPPORT_TEST_VARIABLE"


def _data():
    Ws, bs, _ = init_weights(DIMS, 3)
    rng = np.random.default_rng(4)
    x = rng.normal(size=(ROWS, DIMS[0])).astype(np.float32)
    y = rng.normal(size=(ROWS, DIMS[-1])).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=ROWS).astype(np.float32)
    return Ws, bs, x, y, w


def test_forward_and_step_oracle_are_the_numpy_oracle_on_a_relu_stack():
    Ws, bs, x, y, w = _data()
    act = [1, 1, 0]
    np.testing.assert_array_equal(forward64(Ws, bs, act, x), ora.mlp_forward(Ws, bs, x, dtype=np.float64))
    W64 = [W.astype(np.float64) for W in Ws]
    acts = ora.mlp_forward(Ws, bs, x, dtype=np.float64, keep=True)
    lo_ref, dout = ora.batch_loss_and_grad(acts[-1], y.astype(np.float64), w.astype(np.float64))
    lo, go = oracle_step(Ws, bs, act, x, y, w)
    assert lo == lo_ref
    np.testing.assert_array_equal(go, ora.flatten_params(*ora.mlp_backward(W64, acts, dout)[:2]))


def test_partial_forward_and_loss_on_a_stack_with_a_linear_hidden_layer():
    Ws, bs, x, y, w = _data()
    act = [1, 0, 0]
    full = [h for _, h in layers64(Ws, bs, act, x)]
    assert len(full) == 3 and (full[1] < 0).any()   # the second layer really is linear
    np.testing.assert_array_equal(forward64(Ws, bs, act, x, layers=2), full[1])
    np.testing.assert_array_equal(forward64(Ws, bs, act, x), full[2])
    z1 = np.maximum(x.astype(np.float64) @ Ws[0].astype(np.float64) + bs[0].astype(np.float64), 0)
    np.testing.assert_array_equal(full[1], z1 @ Ws[1].astype(np.float64) + bs[1].astype(np.float64))
    assert loss64(Ws, bs, act, x, y, w) == oracle_step(Ws, bs, act, x, y, w)[0]


@pytest.mark.parametrize("before", [None, "old value"])
@pytest.mark.parametrize("raises", [False, True])
def test_forced_env_restores_what_was_there(monkeypatch, before, raises):
    if before is None:
        monkeypatch.delenv(VAR, raising=False)
    else:
        monkeypatch.setenv(VAR, before)
    try:
        with forced_env(**{VAR: "forced"}):
            assert os.environ[VAR] == "forced"
            if raises:
                raise KeyError("from the body")
    except KeyError:
        assert raises
    else:
        assert not raises
    assert os.environ.get(VAR) == before
