"""The checks the ctypes front end's callers share (_native.py: _data_rows, _count_opts): each refuses the same values
under every caller, with the caller's name in the message, before the library is reached."""
import numpy as np
import pytest

from conftest import pkg

DIN, DOUT = 7, 451


def callers(st):
    """the four callers of _data_rows as (entry name, call(rows, data))"""
    return [("loglike_fwd", lambda n, data: st.loglike_fwd(np.zeros((n, DIN)), data=data)),
            ("fit", lambda n, data: st.fit(np.zeros((n, DIN)), data=data)),
            ("sample", lambda n, data: st.sample(np.zeros((n, DIN)), data=data)),
            ("sample_ensemble", lambda n, data: st.sample_ensemble(np.zeros((n, DIN)), 16, data=data))]


def test_data_rows():
    nat = pkg("_native")
    assert nat._data_rows("fit", None, 5, DOUT) == (None, 0)
    dp, nd = nat._data_rows("fit", np.zeros(DOUT), 5, DOUT)  # (one spectrum as a vector)
    assert dp.shape == (1, DOUT) and dp.dtype == np.float32 and dp.flags.c_contiguous and nd == 1
    dp, nd = nat._data_rows("fit", np.zeros((4, DOUT), np.float64)[::2], 32, DOUT)
    assert dp.shape == (2, DOUT) and dp.dtype == np.float32 and dp.flags.c_contiguous and nd == 2
    st = object.__new__(nat.Stack)  # (no handle: every refusal below comes before the library is called)
    st.dims = [DIN, DOUT]
    for name, call in callers(st):
        for data in (np.zeros((2, DOUT - 1), np.float32), np.zeros(DOUT + 1, np.float32), np.zeros((0, DOUT), np.float32),
                     np.zeros((2, 1, DOUT), np.float32)):
            with pytest.raises(ValueError, match=r"^%s: data must be \(n_data, %d\)" % (name, DOUT)):
                call(32, data)
        with pytest.raises(ValueError, match=r"^%s: 32 rows are not a multiple of 3 data rows" % name):
            call(32, np.zeros((3, DOUT), np.float32))


def test_count_opts():
    nat = pkg("_native")
    bad = [dict(n_steps=-1), dict(n_warmup=-1), dict(thin=-1), dict(chain0=-1), dict(step0=-1), dict(seed=-1), dict(n_steps=1.5),
           dict(thin=0.5), dict(n_steps=2 ** 31), dict(n_warmup=2 ** 31), dict(thin=2 ** 31), dict(seed=2 ** 64),
           dict(step0=2 ** 32 - 10, n_steps=10, n_warmup=0), dict(step0=2 ** 32 - 10, n_steps=0, n_warmup=10)]
    good = [dict(n_steps=0, n_warmup=0, thin=0), dict(seed=2 ** 64 - 1), dict(step0=2 ** 32 - 11, n_steps=10, n_warmup=0),
            dict(n_steps=2 ** 31 - 1, n_warmup=0, thin=2 ** 31 - 1)]
    for name, make in (("sample", nat.Stack.sample_opts), ("sample_ensemble", nat.Stack.ensemble_opts)):
        for kw in bad:
            with pytest.raises(ValueError, match="^%s: " % name):
                make(**kw)
        for kw in good:
            o = make(**kw)
            assert all(getattr(o, k) == v for k, v in kw.items())
    # (the ensemble's own count goes through the same check)
    with pytest.raises(ValueError, match="^sample_ensemble: n_walkers = 16.5"):
        nat.Stack.ensemble_opts(n_walkers=16.5)
