"""User-facing emulator classes: the reference's ``VeryAccurateEmulator.emulator`` surface
(``DirectEmulator`` emulator.py:207-442, ``AutoEncoder`` :445-518, ``AutoEncoderEmulator``
:528-842, ``_gen_model`` :12-48, ``relative_mse_loss`` :51-83, ``error`` :129-192 and the
redshift/frequency helpers) on top of the MI355X engine instead of TensorFlow.

Same names, arguments, return values and error behaviour; the differences a user can
observe are listed in INTEGRATION.md (no dataset download, ``precision=`` option,
training-set statistics cached, AE predict evaluated as one fused device stack).
"""
import os
from collections import namedtuple

import numpy as np

from . import _native as nat, engine, foregrounds as fg, preprocess as pp
from .callbacks import TqdmCallback
from .engine import ChainedModel, Dense, GaussianLatent, Input, Model, Sequential, sequential_from_arrays
from .losses import mean_squared_error, relative_mse_loss  # noqa: F401  (public, as in the reference)
from .priors import Prior

PATH = os.path.dirname(os.path.abspath(__file__)) + "/"


def _with_tqdm(verbose, *callback_lists):
    """``verbose="tqdm"``: a progress bar on (a copy of) every callback list and no printing.  -> (verbose, *lists)"""
    lists = [list(c) for c in callback_lists]  # (copies: the reference appends to its default-argument lists)
    if verbose == "tqdm":
        for c in lists:
            c.append(TqdmCallback())
        verbose = 0
    return (verbose, *lists)


def _gen_model(in_dim, hidden_dims, out_dim, activation_func, name=None, variational=False):
    """Generate a new model: Dense(h, activation) per hidden dim, then a linear
    Dense(out_dim).  ``activation_func``: "relu", "linear", "tanh", "sigmoid", "elu" or "softplus" (Keras'
    definitions; a callable is taken by its ``__name__``), as the reference's "str or instance of tf.keras.activations".  ``in_dim`` None defers weight creation until ``build``/first call
    (a decoder that follows another model).  ``variational`` (not in the reference
    snapshot) makes the last layer a ``GaussianLatent`` (z_mean | z_log_var) head."""
    layers = []
    if in_dim is not None:
        layers.append(Input(shape=(in_dim,)))
    for dim in hidden_dims or []:
        layers.append(Dense(dim, activation=activation_func))
    layers.append(GaussianLatent(out_dim, name="z_mean_log_var") if variational else Dense(out_dim))
    return Sequential(layers, name=name)


NU_0 = 1420405751.7667  # Hz, rest frequency of the 21-cm line

# Three places where this module deliberately does NOT reproduce an accident of the reference
# (INTEGRATION.md section 6).  ``set_strict_reference(True)`` switches all three back to the
# reference's observable behaviour, for callers that depend on it:
#   * ``error(..., flow=x)`` or ``error(..., fhigh=x)`` with ONE bound returns shape (N, 1), because the
#     reference indexes with an (k, 1) argwhere result (emulator.py:179-184); both bounds give (N,)
#   * ``freq2redshift`` multiplies an ndarray argument by 1e6 IN PLACE (emulator.py:124), so a
#     ``frequencies=`` array passed to a constructor is left in Hz (emulator.py:314-317)
#   * the latent emulator's model name keeps the reference's spelling "ae_emualtor" (emulator.py:662)
strict_reference = False


def set_strict_reference(on=True):
    """Reproduce the reference's three accidental behaviours listed above (default: off)."""
    global strict_reference
    strict_reference = bool(on)


def redshift2freq(z):
    """Redshift -> frequency in MHz."""
    nu = NU_0 / (1 + z)
    nu /= 1e6
    return nu


def freq2redshift(nu):
    """Frequency in MHz -> redshift.  The argument is left untouched unless
    ``strict_reference`` is set (the reference converts an ndarray to Hz in place,
    emulator.py:124)."""
    if strict_reference:
        nu *= 1e6  # to Hz -- in place for ndarrays, exactly as the reference does
        return NU_0 / nu - 1
    return NU_0 / (np.asarray(nu, dtype=float) * 1e6) - 1 if np.ndim(nu) else NU_0 / (nu * 1e6) - 1


def error(true_signal, pred_signal, relative=True, nu_arr=None, flow=None, fhigh=None):
    """Eq. 1 of Bye et al. (2022): rms over bins, optionally as % of the signal amplitude
    and restricted to a frequency band (emulator.py:129-192)."""
    if (flow or fhigh) and nu_arr is None:
        raise ValueError("No frequency array is given, cannot compute error in specified frequency band.")
    pred_signal, true_signal = np.asarray(pred_signal), np.asarray(true_signal)
    if pred_signal.ndim == 1:
        pred_signal = pred_signal[None, :]
        true_signal = true_signal[None, :]
    if flow or fhigh:
        sel = np.ones(len(nu_arr), bool)
        if flow:
            sel &= nu_arr >= flow
        if fhigh:
            sel &= nu_arr <= fhigh
        f = np.flatnonzero(sel)
        if strict_reference and not (flow and fhigh):
            f = f[:, None]  # the reference's (k, 1) index -> (N, k, 1) selection -> (N, 1) result
        pred_signal, true_signal = pred_signal[:, f], true_signal[:, f]
    err = np.sqrt(np.mean((pred_signal - true_signal) ** 2, axis=1))
    if relative:
        err = err / np.max(np.abs(true_signal), axis=1) * 100
    return err


# ---- default data (emulator.py:196-204) ---------------------------------------------
hidden_dims = [288, 352, 288, 224]
redshifts = np.linspace(5, 50, 451)
_DATASET_KEYS = ("par_train", "par_val", "par_test", "signal_train", "signal_val", "signal_test")
_dataset = None


def load_dataset(path=None):
    """The six arrays of ``dataset_21cmVAE.h5``.  The reference reads that file at import and
    downloads it when missing; this package NEVER downloads: the file is looked for at
    ``path``, ``$V21_DATASET`` or next to this module, and otherwise the constructors
    require the arrays to be passed explicitly.

    The arrays are shared by every emulator built without explicit data and are READ-ONLY
    (the reference's module-level arrays are writable; an in-place edit here raises numpy's
    "assignment destination is read-only" -- pass an edited copy to the constructor instead).
    That is what lets a default-constructed emulator skip the per-call checksum of the
    training set: nobody holds a writable handle on these buffers, so the cached statistics
    (``preprocess._cached``) are exact on identity alone."""
    global _dataset
    if _dataset is not None and path is None:
        return _dataset
    cands = [path, os.environ.get("V21_DATASET"), PATH + "dataset_21cmVAE.h5"]
    for c in cands:
        if c and os.path.exists(c):
            from . import h5lite
            with h5lite.File(c) as hf:
                _dataset = {k: pp.freeze(hf[k][:]) for k in _DATASET_KEYS}
            return _dataset
    return None


def _resolve_data(given):
    if all(v is not None for v in given.values()):
        return given
    ds = load_dataset()
    if ds is None:
        missing = [k for k, v in given.items() if v is None]
        raise ValueError("dataset_21cmVAE.h5 was not found (this package does not download it): pass %s, or "
                         "set V21_DATASET" % ", ".join(missing))
    return {k: (v if v is not None else ds[k]) for k, v in given.items()}


def _grid(redshifts_, frequencies):
    if frequencies is None:
        if redshifts_ is not None:
            frequencies = redshift2freq(redshifts_)
    elif redshifts_ is None:
        redshifts_ = freq2redshift(frequencies)
    return redshifts_, frequencies


# fit_parameters' result (fisher: None unless asked for; log_prior: None without prior / fixed / return_evidence;
# log_evidence, cov_u: None unless return_evidence)
FitResult = namedtuple("FitResult", ["params", "lnl", "status", "fisher", "log_prior", "log_evidence", "cov_u"],
                       defaults=(None, None, None))


def _free_block_inverse(prec_u, free):
    """(..., d, d) posterior precisions (float32 data) -> covariances: the inverse on the rows and columns of ``free`` (a
    boolean mask), zeros on the others.  NaN on the free block of a matrix that is no usable precision: an entry not
    finite, a diagonal entry not positive, or -- scaled to a unit diagonal, so that the columns' units do not count -- a
    condition number above 1 / float32 epsilon (2^23), beyond which the inverse of float32 data carries no digit."""
    A = np.asarray(prec_u, np.float64)
    idx = np.flatnonzero(free)
    out = np.zeros_like(A)
    if idx.size:
        blk = A[..., idx[:, None], idx[None, :]]
        diag = np.diagonal(blk, axis1=-2, axis2=-1)
        with np.errstate(all="ignore"):
            ok = np.isfinite(blk).all(axis=(-1, -2)) & (diag > 0).all(axis=-1)
            s = 1.0 / np.sqrt(np.where(ok[..., None], diag, 1.0))
            C = np.where(ok[..., None, None], blk * s[..., :, None] * s[..., None, :], np.eye(idx.size))
            ok &= np.linalg.cond(C) <= 2.0 ** 23
        inv = np.full_like(blk, np.nan)
        inv[ok] = np.linalg.inv(C[ok]) * s[ok][:, :, None] * s[ok][:, None, :]
        out[..., idx[:, None], idx[None, :]] = inv
    return out


# sample_posterior's result.  params / lnl: None with thin = 0; mean_u, cov_u: pooled over the chains of a spectrum, in
# par_transform's coordinates u, from the device's per-chain moments (as r_hat is: none of the three needs the samples)
PosteriorSamples = namedtuple("PosteriorSamples", ["params", "lnl", "accept_rate", "step_size", "r_hat", "mean_u", "cov_u"])


# sample_tempered's result: the fields of PosteriorSamples from the beta = 1 rows (one chain per ladder), then the ladder,
# the per-rung means of ln L, the swap rates pooled over ladders and the evidence with its ladder-to-ladder error
TemperedSamples = namedtuple("TemperedSamples", PosteriorSamples._fields + ("betas", "mean_lnl", "swap_rate", "log_evidence",
                                                                           "log_evidence_err"))


def default_betas(n_temps):
    """The default ladder of ``sample_tempered``: beta_k = ((T - 1 - k) / (T - 1))^5, k = 0 .. T - 1 ([1.0] for T = 1) -- a
    power law that crowds the rungs toward beta = 0, where E_beta[ln L] changes fastest; the first rung is the posterior,
    the last exactly the prior."""
    T = int(n_temps)
    if T < 1:
        raise ValueError("n_temps must be >= 1")
    if T == 1:
        return np.ones(1)
    return ((T - 1.0 - np.arange(T)) / (T - 1.0)) ** 5


def log_evidence(betas, mean_lnl):
    """Thermodynamic integration by the trapezoid rule: sum_k (beta_k - beta_k+1) (E_k + E_k+1) / 2 over the trailing
    axis of mean_lnl (..., T), E_k = E_beta_k[ln L] at the decreasing inverse temperatures betas (T,).  With betas from 1
    to 0 this is ln Z up to the rule's discretisation error; 0 for a single rung."""
    b, E = np.asarray(betas, np.float64), np.asarray(mean_lnl, np.float64)
    return np.sum((b[:-1] - b[1:]) * (E[..., :-1] + E[..., 1:]) / 2.0, axis=-1)


# nested_sample's result, per spectrum.  params / lnl / log_weights: (n_runs, P, ..) with P = n_iter n_live / 2 dead points
# (iteration-major, ascending ln L within an iteration) followed by the n_live live points; the weights are normalised
# over the POOLED runs.  log_evidence_err: the formula's for one run, the runs' scatter / sqrt(n_runs) for several.
# stopped: "dlogz" or "max_iter".  mean_u, cov_u: the weighted moments in par_transform's coordinates u
NestedSamples = namedtuple("NestedSamples", ["params", "lnl", "log_weights", "log_evidence", "log_evidence_err", "information", "n_iter",
                                             "n_evals", "accept_rate", "mean_u", "cov_u", "stopped"])


def nested_evidence(dead_lnl, live_lnl, n_live):
    """The evidence from a nested run's record, in float64.  dead_lnl (..., T, k): ln L of the k = n_live / 2 points each of
    T iterations deleted, ascending within an iteration; live_lnl (..., n_live): the live points left; leading axes are
    independent runs.  Deleting the k lowest of N = n_live points one after the other shrinks the prior volume X by
    E[-ln t] = 1 / (N - i) at the i-th, so with s_k = sum_{i<k} 1 / (N - i) the volume after the death of rank r of
    iteration t is ln X_{t,r} = -t s_k - sum_{i<=r} 1 / (N - i); that dead point weighs L_{t,r} (X_prev - X_{t,r}) (X = 1
    before the first death) and the live points X_T mean(L_live).
    -> (log_evidence (...), log_evidence_err, information, log_weights (..., T k + n_live)): ln Z; its error
    sqrt(H v_k / s_k), v_k = sum_{i<k} 1 / (N - i)^2 -- ln X spreads by v_k per iteration of s_k nats, 1.44 / N per nat at
    k = N / 2 against 1 / N for one death at a time --; H = sum w ln L - ln Z, the information; and the normalised log
    weights, dead points iteration-major first, then the live points."""
    dl, ll = np.asarray(dead_lnl, np.float64), np.asarray(live_lnl, np.float64)
    N = int(n_live)
    T, k = dl.shape[-2:]
    if ll.shape[-1] != N or 2 * k != N or dl.shape[:-2] != ll.shape[:-1]:
        raise ValueError("nested_evidence: dead_lnl (..., T, %d) and live_lnl (..., %d) expected, got %r and %r" % (N // 2, N, dl.shape, ll.shape))
    step = 1.0 / (N - np.arange(k))
    cum = np.cumsum(step)
    s_k, v_k = cum[-1], np.sum(step ** 2)
    before = -np.arange(T)[:, None] * s_k - np.concatenate([[0.0], cum[:-1]])  # ln X_prev (T, k)
    lw_dead = dl + before + np.log(-np.expm1(-step))
    lw = np.concatenate([lw_dead.reshape(dl.shape[:-2] + (T * k,)), ll - T * s_k - np.log(N)], axis=-1)
    both = np.concatenate([dl.reshape(dl.shape[:-2] + (T * k,)), ll], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(lw, axis=-1, keepdims=True)
        lz = m + np.log(np.sum(np.exp(lw - m), axis=-1, keepdims=True))
        lw = lw - lz
        w = np.exp(lw)
        H = np.sum(np.where(w > 0, w * np.where(w > 0, both, 0.0), 0.0), axis=-1) - lz[..., 0]
    return lz[..., 0], np.sqrt(np.maximum(H, 0.0) * v_k / s_k), H, lw


def pooled_moments(mean_c, cov_c):
    """Mean and covariance of the pooled samples of equally long chains from their per-chain means (..., C, d) and
    covariances (..., C, d, d) (both divided by the chain length): the mean of the means, and the mean within-chain
    covariance plus the covariance of the means."""
    mean_c, cov_c = np.asarray(mean_c, np.float64), np.asarray(cov_c, np.float64)
    mean = mean_c.mean(axis=-2)
    dm = mean_c - mean[..., None, :]
    return mean, cov_c.mean(axis=-3) + np.einsum("...ci,...cj->...ij", dm, dm) / mean_c.shape[-2]


def r_hat_from_moments(mean_c, cov_c, n):
    """Gelman-Rubin potential scale reduction per coordinate from per-chain means (..., C, d) and covariances (..., C, d, d)
    of chains of n samples each (covariances divided by n, as the device returns them): W = the mean unbiased within-chain
    variance, B / n = the unbiased variance of the chain means, R = sqrt(((n - 1) / n W + B / n) / W).  NaN where it is
    undefined (one chain, one sample, or W = 0)."""
    mean_c = np.asarray(mean_c, np.float64)
    var_c = np.diagonal(np.asarray(cov_c, np.float64), axis1=-2, axis2=-1)
    C = mean_c.shape[-2]
    if C < 2 or n < 2:
        return np.full(mean_c.shape[:-2] + mean_c.shape[-1:], np.nan)
    W = var_c.mean(axis=-2) * n / (n - 1.0)
    B_over_n = mean_c.var(axis=-2, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(((n - 1.0) / n * W + B_over_n) / W)


def foreground_basis(frequencies, nb, foreground, flow, fhigh):
    """The (K, nb) float64 nuisance basis ``foreground=`` stands for: None -> None (no marginalisation); an int -> that many
    LinLog terms (foregrounds.linlog_basis) over the bins of the band [flow, fhigh], zero outside; a (K, nb) array -> itself."""
    if foreground is None:
        return None
    if isinstance(foreground, (int, np.integer)) and not isinstance(foreground, bool):
        if frequencies is None:
            raise ValueError("No frequency array is given, cannot select a frequency band.")
        if not 1 <= int(foreground) <= 8:
            raise ValueError("foreground: %d terms (1 .. 8)" % int(foreground))
        return fg.band_basis(frequencies, int(foreground), flow, fhigh)
    A = np.array(foreground, np.float64, ndmin=2)
    if A.ndim != 2 or A.shape[1] != nb or not 1 <= A.shape[0] <= 8:
        raise ValueError("foreground must be None, a number of LinLog terms or a (K, %d) basis with K <= 8, got %r" % (nb, np.shape(foreground)))
    return A


class LogPosterior:
    """ln L of one observed signal under the uniform prior on the training box, for an outside sampler (made by
    ``log_posterior``).  The box is [-1, 1]^7 in par_transform's coordinates u: uniform in the linear columns, log-uniform
    in the log10 columns.  The prior's constant is left out, as ln L's is: inside the box the value is ln L.
    With ``prior`` (a ``priors.Prior`` or its dict) the value is ln L + ``Prior.log_density_u``, the prior's density
    normalised on the box relative to the uniform one, and ``prior_transform`` goes through ``Prior.ppf_u``.
    ``lp(theta)``: theta (7,) or (n, 7) raw parameters -> a float or (n,) float64; -inf for every row with a coordinate
    outside the box (or not finite), and such rows are never sent to the device.
    ``lp.prior_transform(cube)``: (7,) or (n, 7) points of the unit cube -> raw parameters, uniform in u
    (``preprocess.par_untransform``) -- the form nested samplers ask for.
    With ``fixed`` (``{label: raw value}``, as ``fit_parameters`` takes it) those columns are no parameters: ``ndim`` is
    the number of free columns d_free, theta and cube are (d_free,) or (n, d_free) -- the free columns in label order --,
    the held columns take their values, and their prior is not read.
    The data / sigma record is uploaded when the object is made and again only if another call replaced it."""

    def __init__(self, em, data, sigma, flow=None, fhigh=None, foreground=None, prior=None, fixed=None):
        self.em = em
        self.prior = Prior.of(prior, em.par_train)
        self.hold, self.held = em._fixed_columns(fixed)
        if self.hold.all():
            raise ValueError("fixed: every parameter is fixed (nothing to sample)")
        if self.prior is not None and self.hold.any():
            labels = list(em.par_labels)
            self.prior = Prior({k: v for k, v in self.prior.spec.items() if not self.hold[labels.index(k)]}, em.par_train, self.prior.labels)
        self.ndim = int(np.count_nonzero(~self.hold))
        model, st, flags, _ = em._diff_stack(np.zeros((1, len(em.par_labels))))
        nb = st.dims[-1]
        self._d = np.ascontiguousarray(np.broadcast_to(np.asarray(data, np.float32), (nb,)))
        self._w = em._band_weights(nb, sigma, flow, fhigh)
        self._fg, self._band = foreground, (flow, fhigh)
        self._record(st)

    def _record(self, st):
        self.em._use_record(st, self._d, self._w, self._fg, *self._band)

    def _full(self, free):
        """(n, ndim) rows of the free columns -> (n, din) with the held columns at their values (a copy)"""
        f = np.array(free, np.float64, ndmin=2)
        if not self.hold.any():
            return f
        x = np.empty((f.shape[0], self.hold.size))
        x[:, ~self.hold] = f
        x[:, self.hold] = self.held[self.hold]
        return x

    def inside(self, theta):
        """(n,) bool: the rows of raw parameters inside the training box"""
        x = self._full(theta)
        with np.errstate(invalid="ignore", divide="ignore"):
            u = pp.par_transform(x, self.em.par_train)
        return np.all(np.isfinite(u) & (np.abs(u) <= 1.0), axis=1)

    def __call__(self, theta):
        x = np.array(theta, np.float64, ndmin=2)
        if x.ndim != 2 or x.shape[1] != self.ndim:
            raise ValueError("expected parameters of shape (%d,) or (n, %d), got %r" % (self.ndim, self.ndim, np.shape(theta)))
        ok = self.inside(x)
        x = self._full(x)
        out = np.full(x.shape[0], -np.inf, np.float64)
        if ok.any():
            model, st, flags, rows = self.em._diff_stack(x[ok])
            self._record(st)
            out[ok] = st.loglike_fwd(rows, model.precision, flags)
            if self.prior is not None:
                out[ok] += self.prior.log_density_u(pp.par_transform(x[ok], self.em.par_train), self.em.par_train)
        return float(out[0]) if np.ndim(theta) == 1 else out

    def prior_transform(self, cube):
        c = np.array(cube, np.float64, ndmin=2)
        if self.hold.any():
            if c.ndim != 2 or c.shape[1] != self.ndim:
                raise ValueError("expected a cube of shape (%d,) or (n, %d), got %r" % (self.ndim, self.ndim, np.shape(cube)))
            full = np.full((c.shape[0], self.hold.size), 0.5)
            full[:, ~self.hold] = c
            c = full
        u = 2.0 * c - 1.0 if self.prior is None else self.prior.ppf_u(c, self.em.par_train)
        x = pp.par_untransform(u, self.em.par_train)[:, ~self.hold]
        return x[0] if np.ndim(cube) == 1 else x


class _EmulatorBase:
    par_labels = ["fstar", "Vc", "fx", "tau", "alpha", "nu_min", "Rmfp"]

    def _set_data(self, par_train, par_val, par_test, signal_train, signal_val, signal_test, freeze_data="auto"):
        """``freeze_data`` (not in the reference) says how ``self.par_train`` / ``self.signal_train`` -- the two arrays
        whose statistics every ``predict`` needs -- are held.  The reference keeps the caller's arrays and recomputes mean /
        std / min / max of the ~44 MB training set on every call (preprocess.py:22-23, 44-45, 89-101); caching those
        numbers is exact only while the buffer cannot change.

        ``"auto"`` (default since r5): THE CALLER'S OWN ARRAYS, as in the reference -- ``em.signal_train is
        signal_train``, nothing is held twice -- with their ``writeable`` flag switched off when they own their buffer:
        nobody can then edit them in place (numpy raises "assignment destination is read-only" instead of the edit being
        silently ignored), so the statistics are cached on identity alone and a call costs no checksum (~70 us for one
        parameter vector).  To change the training set, ASSIGN a new array (``em.signal_train = new``) -- or switch the
        flag back on (``arr.setflags(write=True)``): a writable array is re-hashed on every call, see ``False``.  Arrays that
        do not own their buffer (views: the base could still be written) are treated as ``False``.
        ``True`` (r4's default): private read-only COPIES; the caller's arrays are not touched, the training set is held twice.
        ``False``: the reference's semantics to the letter -- the caller's writable arrays, edits in place honoured -- at
        the price of a whole-buffer hash per call (``preprocess._cached``: ~1.2 ms on the 44 MB set)."""
        d = _resolve_data(dict(par_train=par_train, par_val=par_val, par_test=par_test,
                               signal_train=signal_train, signal_val=signal_val, signal_test=signal_test))
        for k, v in d.items():
            if k in ("par_train", "signal_train") and not pp._is_frozen(v):
                if freeze_data is True:
                    v = pp.freeze(v)
                elif freeze_data == "auto" and isinstance(v, np.ndarray) and v.base is None and v.flags.owndata:
                    v.flags.writeable = False   # (the caller's object, locked: pp._is_frozen(v) holds from here on)
            setattr(self, k, v)
        self.par_labels = list(_EmulatorBase.par_labels)

    def _stack_rows(self, model, params, host_fallback):
        """(stack, flags, rows) for evaluating ``model`` on raw parameters with both transforms inside the library (include/
        v21.h: v21_affine_in; the un-preprocessing rides in the last layer's epilogue): float32 and float64 rows are handed
        over RAW and take the reference's branch for their dtype there, integer rows as float64 (documented deviation: the
        reference truncates the fx floor in integer arrays).  What the library's input transform does not take -- another
        float dtype, more than 8 columns -- goes through ``preprocess.par_transform`` on the host with ``host_fallback``,
        and is cast to float64 without."""
        x = np.asarray(params)
        if x.ndim == 1:
            x = x[None, :]
        if not np.issubdtype(x.dtype, np.floating) or not host_fallback and x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        st = model._ensure_stack()
        st.use_output_stats(pp.SignalStats.of(self.signal_train))  # a new record whenever the training set changed (even in place)
        if host_fallback and not (x.dtype in (np.float32, np.float64) and x.shape[-1] <= 8):
            return st, nat.FWD_OUT_TRANSFORM, pp.par_transform(x, self.par_train)
        st.use_input_stats(pp.ParamStats.of(self.par_train))
        return st, nat.FWD_IN_TRANSFORM | nat.FWD_OUT_TRANSFORM, x

    def _predict_stack(self, model, params, devices=None):
        """par_transform -> device stack -> unpreproc, squeezing a single row (emulator.py:401-407 / :788-795).  Few rows are
        transformed on the host while they are padded, many in float64 on the device, so a 65,536-row call is bound by the
        118 MB of results over PCIe and not by a 4-ms numpy transform."""
        _, flags, x = self._stack_rows(model, params, host_fallback=True)
        pred = model.predict(x, devices=devices, flags=flags)
        return pred[0, :] if pred.shape[0] == 1 else pred

    def _diff_stack(self, params):
        """(model, stack, flags, rows) of the model ``predict`` evaluates, with both transforms set, for the derivatives
        below (the library differentiates par_transform for the rows' dtype)."""
        model = self._predict_chain() if hasattr(self, "_predict_chain") else self.emulator
        out = (model,) + self._stack_rows(model, params, host_fallback=False)
        # compile_derivatives: a stack REBUILT since then (new weights of another shape, another precision) asks again,
        # without waiting; the stack that was asked is not asked twice
        if getattr(self, "_derivatives_rt", None) not in (None, (out[1], model.precision)):
            self._ask_derivatives(out[1], model.precision, 0)
            self._derivatives_rt = (out[1], model.precision)
        # compile_likelihood: the same rule for the forward-only ln L kernel
        if getattr(self, "_likelihood_rt", None) not in (None, (out[1], model.precision)):
            self._ask_likelihood(out[1], model.precision, 0)
            self._likelihood_rt = (out[1], model.precision)
        return out

    @staticmethod
    def _ask_derivatives(st, precision, wait_ms):
        """Stack.jit_jacobian; "unsupported" for a stack the kernel cannot express (the library's "no fused Jacobian kernel
        for this stack").  Every other failure -- run-time compilation switched off with nothing cached, a compiler
        error, a kernel too wide for the registers -- is raised as it is: it is not the stack's shape that is in the way."""
        try:
            return st.jit_jacobian(precision, wait_ms)
        except nat.EngineError as e:
            if "no fused Jacobian kernel for this stack" in str(e):
                return "unsupported"
            raise

    def compile_derivatives(self, wait=True):
        """Opt in to the fused Jacobian kernel instantiated for THIS emulator's stack at run time (include/v21.h:
        v21_mlp_jit_jacobian): afterwards ``jacobian``, ``log_likelihood(grad=True)``, ``fisher``, ``fit_parameters``,
        ``sample_posterior`` and ``sample_tempered`` take the "fused_rt" route in the model's precision instead of the
        generic kernel -- for any ``hidden_dims``, with ReLU or a smooth ``activation_func``.  wait=True waits for the
        compilation (seconds, once per stack: the code object is cached on disk).  -> "ready", "compiling", or
        "unsupported" for a stack the kernel cannot express (a variational head, a non-linear output layer, more than 15
        parameters): such an emulator computes as before.  Never raises for an ineligible stack; an eligible stack whose
        kernel cannot be had (V21_JIT=0 with nothing cached, a compiler failure) raises EngineError with the reason."""
        model, st, _, _ = self._diff_stack(np.zeros((1, len(self.par_labels))))
        state = self._ask_derivatives(st, model.precision, -1 if wait else 0)
        self._derivatives_rt = None if state == "unsupported" else (st, model.precision)
        return state

    @staticmethod
    def _ask_likelihood(st, precision, wait_ms):
        """Stack.jit_loglike; "unsupported" for a stack the kernel cannot express (the library's "no fused ln L kernel for
        this stack"); every other failure is raised as it is (_ask_derivatives says why)."""
        try:
            return st.jit_loglike(precision, wait_ms)
        except nat.EngineError as e:
            if "no fused ln L kernel for this stack" in str(e):
                return "unsupported"
            raise

    def compile_likelihood(self, wait=True):
        """Opt in to the fused forward-only ln L kernel instantiated for THIS emulator's stack at run time (include/v21.h:
        v21_mlp_jit_loglike): afterwards ``log_likelihood(forward_only=True)``, ``log_posterior``, ``sample_ensemble``
        and ``nested_sample`` take the "fused_rt" route in the model's precision -- chi-square reduced inside the forward
        kernel, 4 bytes per row -- instead of the two-launch route, for any ``hidden_dims``, with ReLU or a smooth
        ``activation_func``, wherever the compiled stacks take "fused" (no ``foreground``; data uniform per 128 rows).
        wait=True waits for the compilation (seconds, once per stack: the code object is cached on disk).  -> "ready",
        "compiling", or "unsupported" for a stack the kernel cannot express (a variational head, a non-linear output
        layer): such an emulator computes as before.  Never raises for an ineligible stack; an eligible stack whose kernel
        cannot be had (V21_JIT=0 with nothing cached, a compiler failure) raises EngineError with the reason.  A stack
        rebuilt later (new weights of another shape, another precision) asks again by itself, without waiting."""
        model, st, _, _ = self._diff_stack(np.zeros((1, len(self.par_labels))))
        state = self._ask_likelihood(st, model.precision, -1 if wait else 0)
        self._likelihood_rt = None if state == "unsupported" else (st, model.precision)
        return state

    def jacobian(self, params, return_signal=False):
        """d signal / d params in mK per raw parameter unit (not in the reference: there, tf.GradientTape around
        ``emulator.emulator``): (451, 7) for one parameter vector, (N, 451, 7) for an (N, 7) array; the log10 columns
        are differentiated at the value after the fx zero floor.  return_signal: (signal, jacobian), the signal being
        what ``predict`` returns (bit for bit where ``predict`` takes the fused kernel: 16-bit precisions, or more than
        4,096 rows)."""
        model, st, flags, x = self._diff_stack(params)
        y, jac = st.jacobian(x, model.precision, flags, return_outputs=True)
        J = jac.transpose(0, 2, 1)
        if x.shape[0] == 1:
            y, J = y[0], J[0]
        return (y, J) if return_signal else J

    def log_likelihood(self, params, data, sigma, flow=None, fhigh=None, grad=False, foreground=None, forward_only=False):
        """Gaussian ln L = -1/2 sum_k (data_k - signal_k)^2 / sigma_k^2 over the bins of the band [flow, fhigh] of
        ``self.frequencies`` (as ``error`` selects them; bins outside get weight 0), and with grad=True its gradient
        with respect to the raw parameters -- both reduced on the device (not in the reference).  ``sigma``: a scalar or
        one value per bin, mK.  One value (and a (7,) gradient) for a parameter vector, (N,) (and (N, 7)) for N.  The
        data / sigma record is kept on the device per stack: a sampler's repeated call uploads only its parameters.
        ``foreground`` (here and in ``fisher``, ``fit_parameters``, ``sample_posterior``): None, or linear foreground modes
        whose amplitudes get a flat prior and are integrated out analytically on the device (include/v21.h:
        v21_mlp_set_nuisance) -- an int K for K LinLog terms (``foregrounds.linlog_basis``) over the selected band, or
        any (K, 451) basis, K <= 8.  ln L is then the profile likelihood over the amplitudes, unchanged by adding any
        combination of the modes to ``data``, which may carry the full foreground (10^6 mK and more) in float32.
        ``forward_only=True`` (only with grad=False): the same ln L from the forward-only entry (include/v21.h:
        v21_mlp_loglike_fwd) -- no Jacobian is formed; on the compiled stacks chi-square is reduced inside the forward
        kernel.  It agrees with the default to float32 rounding of the sums, not bit for bit.  With it ``data`` may also be
        (M, 451): 2-D params (R, 7) are then ALWAYS scored against every spectrum (also when R is a multiple of M); 3-D
        params (M, R, 7) block m against spectrum m -- reshape a flat (M R, 7) array to that; the result is (M, R).
        Without ``forward_only`` nothing changes."""
        if forward_only:
            if grad:
                raise ValueError("log_likelihood: forward_only computes no gradient (grad must be False)")
            return self._log_likelihood_fwd(params, data, sigma, flow, fhigh, foreground)
        model, st, flags, x = self._diff_stack(params)
        nb = st.dims[-1]
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(data, np.float32), (nb,)))
        w = self._band_weights(nb, sigma, flow, fhigh)
        self._use_record(st, d, w, foreground, flow, fhigh)
        out = st.loglike(x, model.precision, flags, grad=grad)
        if grad:
            lnl, g = out
            return (lnl[0], g[0]) if x.shape[0] == 1 else (lnl, g)
        return out[0] if x.shape[0] == 1 else out

    def _log_likelihood_fwd(self, params, data, sigma, flow, fhigh, foreground):
        """log_likelihood(forward_only=True): one spectrum as the default call, (M, 451) spectra -> (M, R)"""
        dat = np.asarray(data, np.float32)
        p = np.asarray(params)
        nb, din = int(np.shape(self.signal_train)[-1]), len(self.par_labels)
        if dat.ndim > 2 or (dat.ndim == 2 and (dat.shape[1] != nb or dat.shape[0] < 1)):
            raise ValueError("data must be (%d,) or (M, %d), got %r" % (nb, nb, np.shape(data)))
        if dat.ndim < 2:
            if p.ndim > 2:
                raise ValueError("log_likelihood: per-spectrum parameters (M, R, %d) need data of shape (M, %d)" % (din, nb))
            model, st, flags, x = self._diff_stack(p)
            d = np.ascontiguousarray(np.broadcast_to(dat, (nb,)))
            self._use_record(st, d, self._band_weights(nb, sigma, flow, fhigh), foreground, flow, fhigh)
            out = st.loglike_fwd(x, model.precision, flags)
            return out[0] if x.shape[0] == 1 else out
        M = dat.shape[0]
        if p.ndim == 3:
            if p.shape[0] != M:
                raise ValueError("log_likelihood: per-spectrum parameters must be (%d, R, %d), got %r" % (M, din, np.shape(params)))
            rows = p.reshape(M * p.shape[1], p.shape[2])
        elif p.ndim <= 2:
            rows = np.tile(p[None, :] if p.ndim == 1 else p, (M, 1))
        else:
            raise ValueError("log_likelihood: parameters must be (%d,), (R, %d) or (%d, R, %d), got %r" % (din, din, M, din, np.shape(params)))
        R = rows.shape[0] // M
        model, st, flags, x = self._diff_stack(rows)
        dat = np.ascontiguousarray(dat)
        self._use_record(st, dat[0], self._band_weights(nb, sigma, flow, fhigh), foreground, flow, fhigh)
        return st.loglike_fwd(x, model.precision, flags, data=dat).reshape(M, R)

    def log_posterior(self, data, sigma, flow=None, fhigh=None, foreground=None, prior=None, fixed=None):
        """The log-posterior of the parameters given one observed signal, as an object to hand to an outside sampler
        (nested, ensemble, importance; not in the reference): a ``LogPosterior``.  ``lp(theta)``: float64 ln L of
        ``log_likelihood(forward_only=True)`` under the uniform prior on the training box in par_transform's coordinates,
        -inf outside the box; ``lp.prior_transform(cube)``: the unit cube -> raw parameters, uniform in those coordinates.
        ``prior``: as in ``sample_posterior``; ``lp(theta)`` then adds ``Prior.log_density_u`` and ``prior_transform``
        draws from the prior.  ``fixed``: ``{label: raw value}`` as in ``sample_posterior``; ``lp.ndim`` is then the number
        of free columns, and theta / cube are those columns in label order."""
        return LogPosterior(self, data, sigma, flow, fhigh, foreground, prior, fixed)

    def _use_prior(self, st, prior):
        """the samplers' prior record on the stack -- ``prior``: None (the record is cleared: a prior of another call
        never leaks in), a ``priors.Prior`` or its dict -- set beside ``_use_record``; -> the Prior or None"""
        pr = Prior.of(prior, self.par_train)
        st.use_prior(None if pr is None else pr.to_u(self.par_train))
        return pr

    def _hold_u(self, fixed):
        """the samplers' ``fixed`` ({label: raw value}, None: nothing; ``_fixed_columns``' errors) -> (hold mask (din,) bool,
        raw values (din,), u (din,) float64: par_transform of the values, 0 where free)"""
        hold, val = self._fixed_columns(fixed)
        if hold.all():
            raise ValueError("fixed: every parameter is fixed (nothing to sample)")
        row = pp.par_untransform(np.zeros((1, hold.size)), self.par_train)
        row[0, hold] = val[hold]
        u = np.where(hold, np.clip(pp.par_transform(row, self.par_train)[0], -1.0, 1.0), 0.0)
        return hold, val, u

    @staticmethod
    def _held_results(hold, u, mean, cov, r_hat=None):
        """a sampler's pooled moments (..., din) / (..., din, din) with the held columns as the device reports them per
        row: the mean the float32 the column carries, its row and column of cov exact zeros; r_hat NaN there"""
        if hold.any():
            mean[..., hold] = u.astype(np.float32)[hold]
            cov[..., hold, :] = 0.0
            cov[..., :, hold] = 0.0
            if r_hat is not None:
                r_hat[..., hold] = np.nan
        return mean, cov, r_hat

    def _use_record(self, st, d, w, foreground, flow, fhigh):
        """the likelihood record (d, w) and the nuisance basis of ``foreground`` (None: none) on the stack"""
        A = foreground_basis(self.frequencies, st.dims[-1], foreground, flow, fhigh)
        if A is None or st.nu_record is None or not np.array_equal(st.nu_record, A):
            st.use_nuisance(None)  # (before the record: the new weights need not suit the basis the stack still holds)
        st.use_likelihood(d, w)
        st.use_nuisance(A)

    def foreground_amplitudes(self, params, data, sigma, foreground, flow=None, fhigh=None):
        """Best-fit amplitudes of the foreground modes for ``data`` at ``params`` (the maximum over the amplitudes that
        ``log_likelihood(..., foreground=)`` profiles out): ``(a_hat, foreground_model)`` in float64, a_hat (K,) and the
        model a_hat @ basis (451,) in mK for one parameter vector, (N, K) and (N, 451) for N."""
        model, st, flags, x = self._diff_stack(params)
        nb = st.dims[-1]
        A = foreground_basis(self.frequencies, nb, foreground, flow, fhigh)
        if A is None:
            raise ValueError("foreground_amplitudes needs a foreground")
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(data, np.float32), (nb,)))
        self._use_record(st, d, self._band_weights(nb, sigma, flow, fhigh), A, flow, fhigh)
        a = st.nuisance_coef(x, model.precision, flags)
        fgm = a @ A
        return (a[0], fgm[0]) if x.shape[0] == 1 else (a, fgm)

    def _band_weights(self, nb, sigma, flow, fhigh):
        """float32 1 / sigma^2 per bin, 0 outside the band [flow, fhigh] of ``self.frequencies`` (as ``error`` selects it)"""
        s = np.broadcast_to(np.asarray(sigma, np.float64), (nb,))
        w = (1.0 / s ** 2).astype(np.float32)
        if flow or fhigh:
            if self.frequencies is None:
                raise ValueError("No frequency array is given, cannot select a frequency band.")
            nu = np.asarray(self.frequencies)
            sel = np.ones(nb, bool)
            if flow:
                sel &= nu >= flow
            if fhigh:
                sel &= nu <= fhigh
            w = np.where(sel, w, np.float32(0))
        return w

    def fisher(self, params, sigma, flow=None, fhigh=None, foreground=None):
        """Fisher matrix F = J^T diag(1 / sigma^2) J of the signal at ``params`` in raw parameter units (not in the
        reference), over the bins of the band [flow, fhigh] as ``log_likelihood`` selects them; computed and reduced on
        the device.  (7, 7) for one parameter vector, (N, 7, 7) for N.  Its inverse is the Gaussian forecast covariance."""
        model, st, flags, x = self._diff_stack(params)
        nb = st.dims[-1]
        w = self._band_weights(nb, sigma, flow, fhigh)
        d = st.lk_record[0] if st.lk_record is not None else np.zeros(nb, np.float32)  # (the data are not read: keep the record's)
        self._use_record(st, d, w, foreground, flow, fhigh)
        F = st.fisher(x, model.precision, flags)
        return F[0] if x.shape[0] == 1 else F

    def _spectra(self, data):
        """(model, stack, flags) of ``_diff_stack`` and observed signal(s) (451,) or (M, 451) as contiguous float32 (M, 451),
        with whether there was one"""
        model, st, flags, _ = self._diff_stack(np.zeros((1, len(self.par_labels))))
        nb = st.dims[-1]
        dat = np.asarray(data, np.float32)
        one = dat.ndim == 1
        dat = np.ascontiguousarray(dat.reshape(1, -1) if one else dat)
        if dat.ndim != 2 or dat.shape[1] != nb:
            raise ValueError("data must be (%d,) or (M, %d), got %r" % (nb, nb, np.shape(data)))
        return model, st, flags, dat, one

    def _sampler_starts(self, st, dat, per, p0, sigma, flow, fhigh, seed, foreground, prior=None, fixed=None):
        """The samplers' raw start rows (M prod(per), din), ``per`` the shape of one spectrum's starts: ``p0`` ((din,) or
        (per[-1], din), the same for every spectrum) or the best ``fit_parameters`` start per spectrum -- under the call's
        ``prior`` its MAP fit, with ``fixed`` that fit with those columns held --, every row jittered (seeded, 0.02 in u,
        clipped into the box), the ``fixed`` columns then set to their values; then the call's likelihood record is set on
        the stack"""
        din, shape = st.dims[0], (dat.shape[0],) + tuple(per) + (st.dims[0],)
        if p0 is None:
            centre = np.array(self.fit_parameters(dat, sigma, flow=flow, fhigh=fhigh, seed=seed, foreground=foreground, prior=prior,
                                                  fixed=fixed).params, np.float64, ndmin=2)
            u0 = np.repeat(pp.par_transform(centre, self.par_train)[:, None, :], int(np.prod(per)), axis=1).reshape(shape)
        else:
            starts = np.array(p0, np.float64, ndmin=2)
            if starts.ndim != 2 or starts.shape[1] != din or starts.shape[0] not in (1, per[-1]):
                raise ValueError("p0 must be (%d,) or (%d, %d), got %r" % (din, per[-1], din, np.shape(p0)))
            u0 = np.broadcast_to(pp.par_transform(starts, self.par_train), shape)
        rng = np.random.default_rng(seed)
        u0 = np.clip(np.clip(u0, -1.0, 1.0) + 0.02 * rng.normal(size=shape), -1.0, 1.0)
        x0 = pp.par_untransform(u0.reshape(-1, din), self.par_train)
        if fixed is not None:
            hold, val = self._fixed_columns(fixed)
            x0[:, hold] = val[hold]
        self._use_record(st, dat[0], self._band_weights(st.dims[-1], sigma, flow, fhigh), foreground, flow, fhigh)
        return x0

    @staticmethod
    def _posterior_samples(r, view, n_kept, return_lnl, one, held=None):
        """``PosteriorSamples`` from a sampler's result arrays r; view: a per-row array (n, ...) -> (M, chains, ...), or
        (M, ensembles, walkers, ...) whose walkers are pooled before the ensembles are compared; n_kept: kept transitions;
        held: (hold mask, u) of a call with ``fixed`` (``_held_results``)"""
        K = r["samples"].shape[1] if "samples" in r else 0
        params = view(r["samples"]) if K else None
        lnl = view(r["samples_lnl"]) if K and return_lnl else None
        acc, step = view(r["accept_rate"]), (view(r["eps_last"]) if "eps_last" in r else None)
        mean_c, cov_c = view(r["mean_u"]), view(r["cov_u"])
        if mean_c.ndim == 4:
            n_kept *= mean_c.shape[2]
            mean_c, cov_c = pooled_moments(mean_c, cov_c)
        rh = r_hat_from_moments(mean_c, cov_c, n_kept)
        mean_p, cov_p = pooled_moments(mean_c, cov_c)
        if held is not None:
            mean_p, cov_p, rh = _EmulatorBase._held_results(held[0], held[1], np.array(mean_p), np.array(cov_p), np.array(rh))
        out = (params, lnl, acc, step, rh, mean_p, cov_p)
        return PosteriorSamples(*[a[0] if one and a is not None else a for a in out])

    def _fixed_columns(self, fixed):
        """``fit_parameters``' ``fixed`` ({label: raw value}, None: nothing) -> (hold mask (din,) bool, raw values (din,),
        NaN where free).  ValueError, naming the column: an unknown label, a value outside the training box"""
        labels = list(self.par_labels)
        hold, val = np.zeros(len(labels), bool), np.full(len(labels), np.nan)
        centre = pp.par_untransform(np.zeros((1, len(labels))), self.par_train)
        for name, v in dict(fixed or {}).items():
            if name not in labels:
                raise ValueError("fixed: unknown parameter %r (one of %s)" % (name, ", ".join(labels)))
            j = labels.index(name)
            row = centre.copy()
            row[0, j] = float(v)
            with np.errstate(all="ignore"):
                u = pp.par_transform(row, self.par_train)[0, j]
            if not -1.0 <= u <= 1.0:
                raise ValueError("fixed: %s = %r lies outside the training box" % (name, v))
            hold[j], val[j] = True, float(v)
        return hold, val

    def fit_parameters(self, data, sigma, p0=None, n_starts=8, max_iter=50, flow=None, fhigh=None, seed=0, return_all=False,
                       return_fisher=False, foreground=None, prior=None, fixed=None, return_evidence=False):
        """Maximum-likelihood or maximum-a-posteriori parameters of observed signal(s) (not in the reference): a projected
        Levenberg-Marquardt fit per (spectrum, start) on the device, inside the training box, of the Gaussian ln L of
        ``log_likelihood``.
        ``data``: (451,) or (M, 451) mK.  Starts: ``p0`` ((7,) or (S, 7) raw parameters, the same for every spectrum), or
        the box centre and ``n_starts - 1`` uniform points of the box (seeded; uniform in par_transform's coordinates).
        Returns a ``FitResult`` (params, lnl, status[, fisher]) of the best start per spectrum (the lowest start index
        among equals), or of every start with ``return_all`` ((M, S, ...); the M axis dropped for one spectrum).  status:
        1 converged, 2 no improving step, 3 no information (all weights zero), 0 ``max_iter`` reached.  ``fisher``: the
        Fisher matrix at the result in raw units (of the likelihood alone).  Bounds: a log column's lower bound comes back
        as 10^lo (the fx zero floor 1e-6, not 0).
        ``prior``: as in ``sample_posterior``; the fit then maximises ln L + ln p (include/v21.h: v21_mlp_fit_map), and the
        best start is the one with the highest ln L + ln p.  ``lnl`` stays ln L.
        ``fixed``: ``{label: raw value}``; that column of every start is set to the value and held there: it is no
        parameter of the fit, its prior is not read, and it comes back as the value to float32 rounding in u.
        ValueError, naming the column: an unknown label, a value outside the training box.
        With any of ``prior``, ``fixed``, ``return_evidence`` the result also has ``log_prior``: ln of the prior density
        at the result over the free columns, normalised as ``Prior.log_density_u`` (relative to the uniform prior: 0
        without a prior).  ``return_evidence`` adds ``log_evidence``, the Laplace approximation
        ln L + ln p + d_free / 2 ln 2 pi - 1/2 ln det(F + P) at the result, with respect to the normalised prior on the
        free columns (the definition ``sample_tempered`` and ``nested_sample`` use), and ``cov_u``, the inverse of F + P on
        the free columns in u (zeros on held rows and columns).
        THE LAPLACE VALUE assumes an interior mode and a smooth ln L.  At a mode on a face of the box it is not an
        evidence, and the ReLU kinks of the emulator near the mode bias it: on a 2-parameter test problem it was 0.14
        nats off the quadrature, on a 1-parameter one 4e-7.  NaN where F + P has no Cholesky factor.
        Without the three keywords the call is the maximum-likelihood fit it always was."""
        model, st, flags, dat, one = self._spectra(data)
        nb, din = st.dims[-1], st.dims[0]
        use_map = prior is not None or fixed is not None or bool(return_evidence)
        prior = Prior.of(prior, self.par_train)  # (argument errors before any device work)
        hold, held = self._fixed_columns(fixed)
        if p0 is None:
            if int(n_starts) < 1:
                raise ValueError("n_starts must be >= 1")
            rng = np.random.default_rng(seed)
            u = np.vstack([np.zeros((1, din)), rng.uniform(-1.0, 1.0, size=(int(n_starts) - 1, din))])
            starts = pp.par_untransform(u, self.par_train)
        else:
            starts = np.array(p0, np.float64, ndmin=2)
            if starts.ndim != 2 or starts.shape[1] != din:
                raise ValueError("p0 must be (%d,) or (S, %d), got %r" % (din, din, np.shape(p0)))
        starts[:, hold] = held[hold]
        M, S = dat.shape[0], starts.shape[0]
        w = self._band_weights(nb, sigma, flow, fhigh)
        self._use_record(st, dat[0], w, foreground, flow, fhigh)
        x0 = np.ascontiguousarray(np.tile(starts, (M, 1)))
        lnp = None
        if use_map:
            self._use_prior(st, prior)
            try:
                r = st.fit_map(x0, model.precision, flags, data=dat, max_iter=max_iter, fisher=return_fisher,
                               use_prior=prior is not None, hold=hold,
                               outputs=("lnp", "laplace", "prec_u") if return_evidence else ("lnp",))
            finally:
                st.use_prior(None)  # (never leaks into the next call)
            lnp = r["lnp"].reshape(M, S)
        else:
            r = st.fit(x0, model.precision, flags, data=dat, max_iter=max_iter, fisher=return_fisher)
        xh = r["x_hat"].reshape(M, S, din)
        lnl = r["lnl"].reshape(M, S)
        status = r["status"].reshape(M, S)
        F = r["fisher"].reshape(M, S, din, din) if return_fisher else None
        extra = []
        if use_map:
            # the device's ln p and Laplace value are those of the unnormalised density: its integral over the free columns
            norm = (prior or Prior(None, self.par_train, self.par_labels)).log_integral_u(~hold, self.par_train)
            extra = [lnp - norm + np.count_nonzero(~hold) * np.log(2.0), None, None]
            if return_evidence:
                extra[1] = r["laplace"].reshape(M, S) - norm
                extra[2] = _free_block_inverse(r["prec_u"].reshape(M, S, din, din), ~hold)
        if not return_all:
            obj = lnl if lnp is None else lnl.astype(np.float64) + lnp
            best = np.argmax(np.where(np.isnan(obj), -np.inf, obj), axis=1)  # (first maximum: the lowest start index)
            i = np.arange(M)
            xh, lnl, status = xh[i, best], lnl[i, best], status[i, best]
            F = F[i, best] if F is not None else None
            extra = [a[i, best] if a is not None else None for a in extra]
        if one:
            xh, lnl, status = xh[0], lnl[0], status[0]
            F = F[0] if F is not None else None
            extra = [a[0] if a is not None else None for a in extra]
        return FitResult(xh, lnl, status, F, *extra)

    def sample_posterior(self, data, sigma, n_chains=64, n_steps=1000, n_warmup=200, thin=1, p0=None, flow=None, fhigh=None, seed=0,
                         eps=None, return_lnl=False, foreground=None, prior=None, fixed=None):
        """Posterior samples of the parameters given observed signal(s) (not in the reference): ``n_chains`` independent
        Markov chains per spectrum, run entirely on the device -- a Metropolis-adjusted Langevin sampler preconditioned
        with the Fisher matrix at the current point (include/v21.h: v21_mlp_sample) -- of the Gaussian ln L of
        ``log_likelihood`` under a UNIFORM PRIOR ON THE TRAINING BOX in par_transform's coordinates u in [-1, 1]^7: uniform
        in the linear columns, log-uniform in the log10 columns, zero outside the box.
        ``prior`` (here and in ``sample_ensemble``, ``sample_tempered``, ``nested_sample``, ``log_posterior``): None, or a
        ``priors.Prior`` / its dict ``{label: spec}`` that puts a normal, truncated to the box, on chosen columns --
        ``("normal", mean, sd)`` in raw units on a linear column, ``("lognormal", mean_log10, sd_dex)`` on a log10 column;
        the others stay uniform.  The sampler then targets L times that prior on the device (include/v21.h:
        v21_mlp_set_prior); every returned ``lnl`` stays ln L.  The default starts are then MAP fits (``fit_parameters(prior=...)``).
        ``fixed`` (here and in ``sample_ensemble``, ``sample_tempered``, ``nested_sample``, ``log_posterior``): None, or
        ``{label: raw value}`` as ``fit_parameters`` takes it (ValueError naming the column: an unknown label, a value
        outside the training box; every column fixed).  Those columns are no parameters of the call: the sampler runs on
        the device over the d_free others with the fixed ones held at their values (include/v21.h: v21_mlp_set_hold), their
        prior is not read, the default starts are ``fit_parameters(..., prior=prior, fixed=fixed)`` and the fixed columns
        of ``p0`` are overwritten.  In the results a fixed column of ``params`` is the value to float32 rounding in u in
        every sample, ``mean_u`` is that float32, its row and column of ``cov_u`` are zeros and its ``r_hat`` is NaN (a
        constant has none): take ``np.nanmax(r_hat)`` for a convergence check.
        ``data``: (451,) or (M, 451) mK.  Starts: ``p0`` ((7,) or (n_chains, 7) raw parameters, the same for every
        spectrum), or by default the best ``fit_parameters`` start per spectrum; either way every chain is jittered
        (seeded, 0.02 in u, clipped into the box).  Each chain runs ``n_warmup`` transitions adapting its step size
        (initially ``eps``, default 1) to an acceptance rate of 0.574, then ``n_steps`` kept ones of which every
        ``thin``-th is stored (``thin = 0``: none, moments only).
        Returns ``PosteriorSamples``: params (M, n_chains, n_steps // thin, 7) raw, lnl (the same without the last axis;
        None unless ``return_lnl``), accept_rate and step_size (M, n_chains), r_hat (M, 7) -- the between / within-chain
        potential scale reduction in u -- and the pooled mean_u (M, 7) / cov_u (M, 7, 7), all three from the per-chain
        moments the device accumulates in float64; the M axis is dropped for one spectrum.  Bounds: a log column's lower
        bound comes back as 10^lo (the fx zero floor 1e-6, not 0)."""
        held = None if fixed is None else self._hold_u(fixed)  # (argument errors before any device work)
        model, st, flags, dat, one = self._spectra(data)
        prior = Prior.of(prior, self.par_train)  # (argument errors before any device work)
        M, C = dat.shape[0], int(n_chains)
        if C < 1:
            raise ValueError("n_chains must be >= 1")
        opts = dict(n_steps=n_steps, n_warmup=n_warmup, thin=thin, seed=seed, eps0=eps)
        nat.Stack.sample_opts(**opts)  # (argument errors before any device work)
        x0 = np.ascontiguousarray(self._sampler_starts(st, dat, (C,), p0, sigma, flow, fhigh, seed, foreground, prior, fixed))
        self._use_prior(st, prior)
        if held is None:
            r = st.sample(x0, model.precision, flags, data=dat, **opts)
        else:
            try:
                st.use_hold((held[0], held[2]))
                r = st.sample(x0, model.precision, flags, data=dat, **opts)
            finally:
                st.use_hold(None)  # (never leaks into the next call)
        return self._posterior_samples(r, lambda a: a.reshape((M, C) + a.shape[1:]), int(n_steps), return_lnl, one,
                                       held and (held[0], held[2]))

    def sample_ensemble(self, data, sigma, n_walkers=64, n_ensembles=4, n_steps=1000, n_warmup=500, thin=1, a=2.0, p0=None, flow=None,
                        fhigh=None, seed=0, return_lnl=False, foreground=None, prior=None, fixed=None):
        """Posterior samples from the affine-invariant ensemble sampler (not in the reference): ``n_ensembles`` independent
        ensembles of ``n_walkers`` walkers per spectrum, moved by Goodman & Weare's stretch move with scale ``a`` entirely
        on the device (include/v21.h: v21_mlp_sample_ensemble), on the forward-only ln L of ``log_likelihood`` under
        ``sample_posterior``'s prior -- uniform on the training box in par_transform's coordinates, or ``prior``.  It needs no gradient
        and no Fisher matrix, so it also serves posteriors on which ``sample_posterior``'s metric is singular or misleading.
        ``n_walkers``: even, 16 .. 512 for the 7 parameters.  Starts as ``sample_posterior`` chooses them: ``p0`` ((7,) or
        (n_walkers, 7) raw parameters, the same for every ensemble and spectrum) or the best ``fit_parameters`` start per
        spectrum, every walker jittered (seeded, 0.02 in u, clipped into the box).  ``n_warmup`` sweeps are burn-in
        (nothing is adapted), then ``n_steps`` kept ones of which every ``thin``-th is stored (``thin = 0``: none).
        Returns ``PosteriorSamples``: params (M, n_ensembles, n_walkers, n_steps // thin, 7) raw, lnl (the same without the
        last axis; None unless ``return_lnl``), accept_rate (M, n_ensembles, n_walkers), step_size None (the move has none),
        r_hat (M, 7) taken BETWEEN ENSEMBLES -- the walkers of one ensemble are not independent chains, so each ensemble's
        walkers are pooled (``pooled_moments``) and the ensembles compared (``r_hat_from_moments``; NaN for one ensemble) --
        and the pooled mean_u (M, 7) / cov_u (M, 7, 7); the M axis is dropped for one spectrum.
        ``fixed``: as in ``sample_posterior``.  The walker rule stays on the 7 columns."""
        held = None if fixed is None else self._hold_u(fixed)  # (argument errors before any device work)
        model, st, flags, dat, one = self._spectra(data)
        prior = Prior.of(prior, self.par_train)  # (argument errors before any device work)
        din = st.dims[0]
        M, E, W = dat.shape[0], int(n_ensembles), int(n_walkers)
        if E < 1:
            raise ValueError("n_ensembles must be >= 1")
        opts = dict(a=a, n_steps=n_steps, n_warmup=n_warmup, thin=thin, seed=seed)
        nat.Stack.ensemble_opts(W, in_dim=din, **opts)  # (argument errors before any device work)
        x0 = np.ascontiguousarray(self._sampler_starts(st, dat, (E, W), p0, sigma, flow, fhigh, seed, foreground, prior, fixed))
        self._use_prior(st, prior)
        if held is None:
            r = st.sample_ensemble(x0, W, model.precision, flags, data=dat, **opts)
        else:
            try:
                st.use_hold((held[0], held[2]))
                r = st.sample_ensemble(x0, W, model.precision, flags, data=dat, **opts)
            finally:
                st.use_hold(None)  # (never leaks into the next call)
        return self._posterior_samples(r, lambda a: a.reshape((M, E, W) + a.shape[1:]), int(n_steps), return_lnl, one,
                                       held and (held[0], held[2]))

    def sample_tempered(self, data, sigma, n_ladders=16, n_temps=8, betas=None, swap_every=5, n_steps=1000, n_warmup=200, thin=1,
                        p0=None, flow=None, fhigh=None, seed=0, eps=None, return_lnl=False, foreground=None, prior=None, fixed=None):
        """Parallel-tempered posterior samples and the Bayesian evidence (not in the reference): ``n_ladders`` ladders per
        spectrum, each of ``n_temps`` chains of ``sample_posterior``'s sampler at the inverse temperatures ``betas``
        (default ``default_betas(n_temps)``, from 1 down to 0), run entirely on the device (include/v21.h:
        v21_mlp_sample_tempered).  A chain at beta samples L^beta under the same uniform prior on the training box; every
        ``swap_every`` transitions neighbouring rungs of a ladder propose to exchange their states, so what the hot rungs
        find -- other modes, the far end of a degeneracy -- reaches the beta = 1 chain.  Starts as in ``sample_posterior``
        (``p0``: (7,) or (n_ladders, 7)), every rung of a ladder from the same jittered start.
        Returns ``TemperedSamples``: the seven fields of ``PosteriorSamples`` from the beta = 1 rows (``n_ladders`` chains
        per spectrum), then betas (T,), mean_lnl (M, n_ladders, T) -- the mean of ln L over the kept transitions of every
        rung --, swap_rate (M, T - 1) -- accepted / proposed swaps of each neighbouring pair, pooled over ladders --,
        log_evidence (M,) and log_evidence_err (M,); the M axis is dropped for one spectrum.
        THE EVIDENCE.  log_evidence estimates ln Z, Z = integral of L(u) du / 2^d over the training box (d = 7: the mean of
        L under the prior), L with the constants ``log_likelihood`` drops (ln L = -chi^2 / 2, without the Gaussian's
        normalisation).  It is the mean over ladders of each ladder's own trapezoid (``log_evidence``) of its rungs' mean
        ln L over beta; log_evidence_err is the scatter of those over ladders (std with ddof 1 / sqrt(n_ladders); nan for
        one ladder) -- the ladders are independent, so it needs no autocorrelation estimate -- and does NOT contain the
        trapezoid's discretisation bias, which only more rungs reduce.  ln Z is comparable between emulators, bands and
        noise levels at the same data and the same foreground basis (add the dropped -sum ln(sigma sqrt(2 pi)) over the
        band's bins where sigma or the band differ).  It is NOT comparable across different numbers of marginalised
        foreground modes: their flat prior is improper.  nan with ``n_temps = 1``.
        With ``prior`` a chain at beta samples L^beta times the prior, the beta = 0 rung the prior itself, mean_lnl stays the
        mean of ln L alone, and log_evidence is ln of the mean of L under the STATED, normalised prior.  It is comparable
        across priors only as a Bayes factor between models, not as a goodness of fit.
        ``fixed``: as in ``sample_posterior``.  log_evidence is then the CONDITIONAL evidence of the nested model: ln of the
        mean of L, at the fixed values, under the normalised prior on the FREE columns -- the definition
        ``FitResult.log_evidence`` uses with ``fixed``.  Its difference to the evidence of the call without ``fixed`` is
        not yet the Bayes factor "is this parameter needed?": that also takes the prior density of the fixed value."""
        held = None if fixed is None else self._hold_u(fixed)  # (argument errors before any device work)
        model, st, flags, dat, one = self._spectra(data)
        prior = Prior.of(prior, self.par_train)  # (argument errors before any device work)
        M, C, T = dat.shape[0], int(n_ladders), int(n_temps)
        if C < 1:
            raise ValueError("n_ladders must be >= 1")
        b = default_betas(T) if betas is None else np.asarray(betas, np.float64)
        opts = dict(n_steps=n_steps, n_warmup=n_warmup, thin=thin, seed=seed, eps0=eps)
        nat.Stack.sample_opts(**opts)  # (argument errors before any device work)
        nat.Stack.temper_opts(T, b, swap_every)
        x0 = self._sampler_starts(st, dat, (C,), p0, sigma, flow, fhigh, seed, foreground, prior, fixed)
        x0 = np.ascontiguousarray(np.repeat(x0, T, axis=0))  # (every rung of a ladder from its ladder's start)
        self._use_prior(st, prior)
        if held is None:
            r = st.sample_tempered(x0, T, b, swap_every, model.precision, flags, data=dat, **opts)
        else:
            try:
                st.use_hold((held[0], held[2]))
                r = st.sample_tempered(x0, T, b, swap_every, model.precision, flags, data=dat, **opts)
            finally:
                st.use_hold(None)  # (never leaks into the next call)
        # (the beta = 1 rows)
        ps = self._posterior_samples(r, lambda a: a.reshape((M, C, T) + a.shape[1:])[:, :, 0], int(n_steps), return_lnl, one,
                                     held and (held[0], held[2]))
        E = r["mean_lnl"].reshape(M, C, T)
        with np.errstate(invalid="ignore", divide="ignore"):
            # (pooled over ladders: every ladder proposes a pair equally often, so the mean of the ratios is the ratio)
            swap = r["swap_accept"].reshape(M, C, T)[:, :, :T - 1].mean(axis=1)
            lz_c = log_evidence(b, E)
            lz = lz_c.mean(axis=1) if T > 1 else np.full(M, np.nan)
            lz_err = lz_c.std(axis=1, ddof=1) / np.sqrt(C) if T > 1 and C > 1 else np.full(M, np.nan)
        if one:
            E, swap, lz, lz_err = E[0], swap[0], lz[0], lz_err[0]
        return TemperedSamples(*ps, b, E, swap, lz, lz_err)

    def nested_sample(self, data, sigma, n_live=256, n_runs=1, n_repeats=None, dlogz=0.01, max_iter=2000, flow=None, fhigh=None,
                      foreground=None, seed=0, return_lnl=True, prior=None, fixed=None):
        """Nested sampling of the posterior given observed signal(s) (not in the reference): the Bayesian evidence with its
        error and weighted posterior samples in one run, without a gradient, entirely on the device (include/v21.h:
        v21_mlp_sample_nested) on the forward-only ln L of ``log_likelihood`` under ``sample_posterior``'s prior -- uniform
        on the training box in par_transform's coordinates.  ``n_runs`` independent runs per spectrum of ``n_live`` live
        points each (even, 56 .. 512 for the 7 parameters), drawn uniform in the box from ``seed``.  An iteration deletes
        the lower half of the live points and replaces each by a copy of a survivor moved ``n_repeats`` times (default
        3 x 7) by the difference of two other survivors, inside the deleted points' highest ln L.  The library is called in
        blocks of 16 iterations until, in every run, what the live points could still add falls below ``dlogz`` --
        logaddexp(ln Z, ln X_T + max live ln L) - ln Z < dlogz -- or ``max_iter`` iterations are done; ``stopped`` says
        which ("dlogz" or "max_iter").  CHECK ``accept_rate``: the default ``n_repeats`` is measured on Gaussian-like
        posteriors, where a quarter of the moves is accepted; on the shipped model a tenth is, and ln Z at the default
        reads 0.4 (sigma = 1 mK) to 1.3 nats (0.05 mK) above the value it converges to at 3 to 9 times the moves (DESIGN §3
        K14).  Where the acceptance is near 0.1, run again with ``n_repeats`` tripled and compare.
        Returns ``NestedSamples``: params (M, n_runs, P, 7) raw -- the P = n_iter n_live / 2 dead points then the n_live
        live points of every run --, lnl and log_weights (M, n_runs, P) (lnl None unless ``return_lnl``; the weights
        normalised over the pooled runs, each run's by its own Z), log_evidence, log_evidence_err, information (M,), n_iter,
        n_evals (ln L evaluations per spectrum), accept_rate (M, n_runs), the weighted mean_u (M, 7) / cov_u (M, 7, 7) and
        stopped; the M axis is dropped for one spectrum.  With one run log_evidence_err is ``nested_evidence``'s
        sqrt(H v_k / s_k); with several, log_evidence is the mean of the runs' ln Z and log_evidence_err their scatter
        (std with ddof 1) / sqrt(n_runs), as ``sample_tempered`` reports its ladders.
        THE EVIDENCE.  log_evidence estimates ln Z, Z = integral of L(u) du / 2^d over the training box (d = 7: the mean of
        L under the prior), L with the constants ``log_likelihood`` drops (ln L = -chi^2 / 2, without the Gaussian's
        normalisation) -- the definition of ``sample_tempered``, so the two are directly comparable; this one has no
        discretisation bias in beta.  ln Z is comparable between emulators, bands and noise levels at the same data and
        the same foreground basis (add the dropped -sum ln(sigma sqrt(2 pi)) over the band's bins where sigma or the band
        differ).  It is NOT comparable across different numbers of marginalised foreground modes: their flat prior is
        improper.
        With ``prior`` the live points are drawn from it, a move is a Metropolis move on the prior inside the deleted
        points' highest ln L, ``lnl`` stays ln L, and log_evidence is ln of the mean of L under the STATED, normalised
        prior.  It is comparable across priors only as a Bayes factor between models, not as a goodness of fit.
        ``fixed``: as in ``sample_posterior``; every live and dead point carries the fixed columns' values.  The default
        ``n_repeats`` is then 3 x d_free (the ``n_live`` rule stays on the 7 columns), and log_evidence is the CONDITIONAL
        evidence of the nested model: ln of the mean of L, at the fixed values, under the normalised prior on the FREE
        columns -- the definition ``FitResult.log_evidence`` uses with ``fixed``, and ``sample_tempered``'s."""
        held = None if fixed is None else self._hold_u(fixed)  # (argument errors before any device work)
        model, st, flags, dat, one = self._spectra(data)
        prior = Prior.of(prior, self.par_train)  # (argument errors before any device work)
        din = st.dims[0]
        M, R, N = dat.shape[0], int(n_runs), int(n_live)
        if R < 1:
            raise ValueError("n_runs must be >= 1")
        if N < 8 * din:
            raise ValueError("n_live = %d: an evidence needs at least %d live points for %d parameters" % (N, 8 * din, din))
        if int(max_iter) < 1 or not float(dlogz) > 0.0:
            raise ValueError("max_iter must be >= 1 and dlogz positive")
        if held is not None and not n_repeats:
            n_repeats = 3 * int(np.count_nonzero(~held[0]))
        opts = dict(n_repeats=n_repeats, seed=seed)
        nat.Stack.nested_opts(N, n_iter=int(max_iter), in_dim=din, **opts)  # (argument errors before any device work)
        rep = int(n_repeats) if n_repeats else 3 * din
        self._use_record(st, dat[0], self._band_weights(st.dims[-1], sigma, flow, fhigh), foreground, flow, fhigh)
        self._use_prior(st, prior)
        if held is not None:
            st.use_hold((held[0], held[2]))
        try:
            return self._nested_blocks(model, st, flags, dat, one, M, R, N, int(max_iter), float(dlogz), opts, rep, return_lnl, held)
        finally:
            if held is not None:
                st.use_hold(None)  # (never leaks into the next call)

    def _nested_blocks(self, model, st, flags, dat, one, M, R, N, max_iter, dlogz, opts, rep, return_lnl, held):
        """``nested_sample``'s loop over blocks of iterations and its result, the records set on the stack"""
        din = st.dims[0]
        n, k, block = M * R * N, N // 2, 16
        s_k = np.sum(1.0 / (N - np.arange(k)))
        u, T, dead_u, dead_l, acc, stopped = None, 0, [], [], 0.0, "max_iter"
        while T < int(max_iter):
            it = min(block, int(max_iter) - T)
            r = st.sample_nested(u, n, N, model.precision, flags, data=dat, n_iter=it, iter0=T, **opts)
            u, T = r["live_u"], T + it
            dead_u.append(r["dead_u"])
            dead_l.append(r["dead_lnl"])
            acc = acc + it * r["accept_rate"].mean(axis=1)
            dl = np.concatenate(dead_l).reshape(T, M, R, k).transpose(1, 2, 0, 3)
            ll = r["live_lnl"].astype(np.float64).reshape(M, R, N)
            lz, err, H, lw = nested_evidence(dl, ll, N)
            if np.all(np.logaddexp(lz, -T * s_k + ll.max(axis=-1)) - lz < float(dlogz)):
                stopped = "dlogz"
                break
        du = np.concatenate(dead_u).reshape(T, M, R, k, din).transpose(1, 2, 0, 3, 4).reshape(M, R, T * k, din)
        pts = np.concatenate([du, u.reshape(M, R, N, din)], axis=2)
        lnl = np.concatenate([dl.reshape(M, R, T * k), ll], axis=2)
        m = lz.max(axis=1, keepdims=True)
        lw = lw + (lz - (m + np.log(np.sum(np.exp(lz - m), axis=1, keepdims=True))))[:, :, None]
        w = np.exp(lw).reshape(M, -1)
        flat = pts.reshape(M, -1, din)
        mean = np.einsum("mp,mpi->mi", w, flat)
        cen = flat - mean[:, None, :]
        cov = np.einsum("mp,mpi,mpj->mij", w, cen, cen)
        if held is not None:
            self._held_results(held[0], held[2], mean, cov)
        params = pp.par_untransform(pts.reshape(-1, din), self.par_train).reshape(pts.shape)
        lz_err = lz.std(axis=1, ddof=1) / np.sqrt(R) if R > 1 else err[:, 0]
        out = [params, lnl if return_lnl else None, lw, lz.mean(axis=1), lz_err, H.mean(axis=1), T, R * (N + k * T * rep),
               (acc / T).reshape(M, R), mean, cov, stopped]
        if one:
            out = [a[0] if isinstance(a, np.ndarray) else a for a in out]
        return NestedSamples(*out)

    def save(self):
        raise NotImplementedError("Not implemented yet.")


class DirectEmulator(_EmulatorBase):
    """The direct emulator (21cmVAE proper): 7 parameters -> 451-bin global signal."""

    def __init__(self, par_train=None, par_val=None, par_test=None, signal_train=None, signal_val=None,
                 signal_test=None, hidden_dims=hidden_dims, activation_func="relu", redshifts=redshifts,
                 frequencies=None, precision="f32", freeze_data="auto"):
        self._set_data(par_train, par_val, par_test, signal_train, signal_val, signal_test, freeze_data)
        self.emulator = _gen_model(self.par_train.shape[-1], hidden_dims, self.signal_train.shape[-1],
                                   activation_func, name="emulator")
        self.emulator.precision = precision
        self.redshifts, self.frequencies = _grid(redshifts, frequencies)

    def load_model(self, model_path=PATH + "models/emulator.h5"):
        """Load a saved model (Keras legacy .h5 or the engine's .npz).  Raises IOError if the
        path does not hold one (the reference's default file is not redistributed)."""
        from . import h5lite
        prec = self.emulator.precision
        self.emulator = h5lite.load_model(model_path)
        self.emulator.precision = prec

    def train(self, epochs, callbacks=[], verbose="tqdm", batch_size=256):
        """Train the emulator; returns (loss, val_loss) lists, one entry per epoch.
        ``batch_size`` (not in the reference, which hard-codes 256 at emulator.py:372): rows per optimizer
        step, e.g. 4,096 per GPU for BASELINE configs[3]; the default is the reference's."""
        X_train = pp.par_transform(self.par_train, self.par_train)
        X_val = pp.par_transform(self.par_val, self.par_train)
        y_train = pp.preproc(self.signal_train, self.signal_train)
        y_val = pp.preproc(self.signal_val, self.signal_train)
        verbose, callbacks = _with_tqdm(verbose, callbacks)
        hist = self.emulator.fit(x=X_train, y=y_train, batch_size=batch_size, epochs=epochs,
                                 validation_data=(X_val, y_val), validation_batch_size=batch_size,
                                 callbacks=callbacks, verbose=verbose)
        return hist.history["loss"], hist.history["val_loss"]

    def predict(self, params, devices=None):
        """Global signal(s) for one parameter vector (-> 1-D) or an (N, 7) array (-> (N, 451)).
        ``devices`` (not in the reference): GPU ordinals to spread the rows over."""
        return self._predict_stack(self.emulator, params, devices)

    def test_error(self, relative=True, flow=None, fhigh=None):
        return error(self.signal_test, self.predict(self.par_test), relative=relative,
                     nu_arr=self.frequencies, flow=flow, fhigh=fhigh)


class AutoEncoder(ChainedModel):
    """Encoder + decoder pair of the autoencoder-based emulator; ``call`` reconstructs."""

    def __init__(self, signal_train=None, enc_hidden_dims=[], dec_hidden_dims=[], latent_dim=9,
                 activation_func="relu", variational=False, kl_weight=0.0):
        """``variational`` / ``kl_weight`` (build-side): the encoder ends in a
        (z_mean | z_log_var) head, training samples z and adds kl_weight * KL to each row's
        loss; ``predict``/``encoder.predict`` use z = z_mean.  variational=False is the
        reference's deterministic autoencoder (emulator.py:445-518)."""
        if signal_train is None:
            signal_train = _resolve_data(dict(signal_train=None))["signal_train"]
        super().__init__([], name="auto_encoder")
        d = signal_train.shape[-1]
        self.encoder = _gen_model(d, enc_hidden_dims, latent_dim, activation_func, name="encoder",
                                  variational=variational)
        self.decoder = _gen_model(None, dec_hidden_dims, d, activation_func, name="decoder")
        self.kl_weight = float(kl_weight)

    def _chain(self):  # plain attribute assignment of .encoder/.decoder re-wires the chain
        return [self.encoder, self.decoder]

    def call(self, signals):
        return self.predict(signals)


# default parameters (emulator.py:522-525)
latent_dim = 9
enc_hidden_dims = [352]
dec_hidden_dims = [32, 352]
em_hidden_dims = [352, 352, 352, 224]


class AutoEncoderEmulator(_EmulatorBase):
    """The autoencoder-based emulator of Appendix A: parameters -> latent -> decoder."""

    AE_PATH = PATH + "models/autoencoder_based_emulator/"

    def __init__(self, par_train=None, par_val=None, par_test=None, signal_train=None, signal_val=None,
                 signal_test=None, latent_dim=latent_dim, enc_hidden_dims=enc_hidden_dims,
                 dec_hidden_dims=dec_hidden_dims, em_hidden_dims=em_hidden_dims, activation_func="relu",
                 redshifts=redshifts, frequencies=None, precision="f32", variational=False, kl_weight=0.0,
                 freeze_data="auto"):
        self._set_data(par_train, par_val, par_test, signal_train, signal_val, signal_test, freeze_data)
        self.redshifts, self.frequencies = _grid(redshifts, frequencies)
        autoencoder = AutoEncoder(self.signal_train, enc_hidden_dims, dec_hidden_dims, latent_dim, activation_func,
                                  variational=variational, kl_weight=kl_weight)
        autoencoder.build((None, self.signal_train.shape[-1]))
        autoencoder.precision = precision
        self.autoencoder = autoencoder
        self.emulator = _gen_model(self.par_train.shape[-1], em_hidden_dims, latent_dim, activation_func,
                                   name="ae_emualtor" if strict_reference else "ae_emulator")
        self.emulator.precision = precision
        self.precision = precision
        self._chain_model = None

    def load_model(self, emulator_path=AE_PATH + "ae_emulator.h5", encoder_path=AE_PATH + "encoder.h5",
                   decoder_path=AE_PATH + "decoder.h5"):
        from . import h5lite
        self.emulator = h5lite.load_model(emulator_path)
        encoder = h5lite.load_model(encoder_path)
        decoder = h5lite.load_model(decoder_path)
        autoencoder = AutoEncoder(signal_train=self.signal_train)
        autoencoder.encoder = encoder
        autoencoder.decoder = decoder
        for m in (self.emulator, autoencoder):
            m.precision = self.precision
        self.autoencoder = autoencoder
        self._chain_model = None

    def train(self, epochs, ae_callbacks=[], em_callbacks=[], verbose="tqdm", joint=False, batch_size=256):
        """Sequential two-phase recipe of the reference (emulator.py:701-768): fit the
        autoencoder x -> x, encode the signals with the frozen encoder, fit the emulator
        parameters -> latent.  Returns (ae_loss, ae_val_loss, loss, val_loss).

        ``joint=True`` (not in the reference; BASELINE configs[2]): both models take one optimizer step
        per batch on the SAME rows, the emulator's targets being the latents the encoder produces for those
        rows in that step -- see ``_train_joint``.
        ``batch_size`` (not in the reference, which hard-codes 256 at emulator.py:742,759): rows per optimizer step."""
        batch_size = int(batch_size)
        if joint:
            return self._train_joint(epochs, ae_callbacks, em_callbacks, verbose, batch_size)
        y_train = pp.preproc(self.signal_train, self.signal_train)
        y_val = pp.preproc(self.signal_val, self.signal_train)
        verbose, ae_callbacks, em_callbacks = _with_tqdm(verbose, ae_callbacks, em_callbacks)
        hist = self.autoencoder.fit(x=y_train, y=y_train, batch_size=batch_size, epochs=epochs,
                                    validation_data=(y_val, y_val), callbacks=ae_callbacks, verbose=verbose)
        ae_loss, ae_val_loss = hist.history["loss"], hist.history["val_loss"]
        X_train = pp.par_transform(self.par_train, self.par_train)
        X_val = pp.par_transform(self.par_val, self.par_train)
        z_train = self.autoencoder.encoder.predict(y_train)
        z_val = self.autoencoder.encoder.predict(y_val)
        hist = self.emulator.fit(x=X_train, y=z_train, batch_size=batch_size, epochs=epochs,
                                 validation_data=(X_val, z_val), callbacks=em_callbacks, verbose=verbose)
        self._chain_model = None
        return ae_loss, ae_val_loss, hist.history["loss"], hist.history["val_loss"]

    def _train_joint(self, epochs, ae_callbacks, em_callbacks, verbose, batch_size=256):
        """One pass over the data trains BOTH models (v21_joint_*): per batch, an autoencoder step (x -> x) and
        an emulator step (parameters -> the latents the encoder has just produced for these rows; no gradient
        into the encoder).  The reference's recipe waits for the autoencoder to finish first
        (emulator.py:739-764); here the emulator tracks the encoder while it still moves, and when the
        autoencoder's callbacks stop it, it is frozen (learning rate 0) and the remaining epochs ARE the
        reference's second phase.  Keras bookkeeping per model (History, callbacks, epoch losses, validation
        after every epoch -- the emulator's against the current encoder's latents of the validation set).
        Needs mean_squared_error on the emulator; any precision (f32: the reference's arithmetic, batches of up to
        2,048 rows).  A variational autoencoder (``AutoEncoder(variational=True)``) is fine: the emulator learns
        z_mean, what ``encoder.predict`` returns.
        With a data-parallel communicator on the context every rank trains on its share of every batch."""
        ae, em = self.autoencoder, self.emulator
        for m in (ae, em):
            engine._check_compiled(m)
        lat = em.layers[-1].units
        if not np.array_equal(em._row_weight(np.zeros((2, lat), np.float32)), em._row_weight(np.ones((2, lat), np.float32))):
            raise ValueError("joint training needs a target-independent emulator loss (mean_squared_error)")
        y_train = np.ascontiguousarray(pp.preproc(self.signal_train, self.signal_train), dtype=np.float32)
        y_val = np.ascontiguousarray(pp.preproc(self.signal_val, self.signal_train), dtype=np.float32)
        X_train = np.ascontiguousarray(pp.par_transform(self.par_train, self.par_train), dtype=np.float32)
        X_val = np.ascontiguousarray(pp.par_transform(self.par_val, self.par_train), dtype=np.float32)
        n = y_train.shape[0]
        verbose, ae_callbacks, em_callbacks = _with_tqdm(verbose, ae_callbacks, em_callbacks)
        tra, tre = ae._ensure_trainer(batch_size), em._ensure_trainer(batch_size)
        tra.set_data(0, y_train, None, ae._row_weight(y_train))
        tra.set_data(1, y_val, None, ae._row_weight(y_val))
        zdummy = np.zeros((n, lat), np.float32)
        tre.set_data(0, X_train, zdummy, em._row_weight(zdummy))
        zdv = np.zeros((X_val.shape[0], lat), np.float32)
        tre.set_data(1, X_val, zdv, em._row_weight(zdv))  # (targets: the encoder's latents of y_val, formed on the device)
        joint = nat.Joint(tra, tre, latent_layer=len(ae.encoder.layers) - 1)
        bcast = None
        if tra.ctx.nranks > 1:  # data parallel: the replicas must start equal and shuffle alike (as engine.Model.fit does)
            bcast = engine._broadcast_start(ae, tra)
            engine._broadcast_start(em, tre)
            if ae._vae_seed is not None:  # (this loop does not refresh the variational settings per epoch)
                tra.set_vae(ae.kl_weight, ae.sample_latent, ae._vae_seed)
        run_a = engine._Run(ae, tra, ae_callbacks, epochs, n, batch_size, verbose)
        run_e = engine._Run(em, tre, em_callbacks, epochs, n, batch_size, verbose)
        engine._Run.begin([run_a, run_e])
        ae_running = em_running = True
        for epoch in range(epochs):
            if not em_running and not ae_running:
                break
            if ae_running:
                run_a.cbs.on_epoch_begin(epoch)
            if em_running:
                run_e.cbs.on_epoch_begin(epoch)
            tra.set_lr(float(ae.optimizer.lr) if ae_running else 0.0)
            tre.set_lr(float(em.optimizer.lr))
            perm = engine._rng.permutation(n).astype(np.int32)
            if bcast is not None:
                perm = bcast(perm)
            if em_running:
                la, le = joint.run_epoch(perm, batch_size)
            else:  # the emulator has stopped: the autoencoder goes on alone
                la, le = tra.run_epoch(perm, batch_size), None
            ae._dirty_host = em._dirty_host = True
            # both validation passes in one launch; the emulator's against the current encoder's latents of the
            # validation signals (the reference's encoder.predict(signal_val), emulator.py:754, without leaving the device)
            va, ve = joint.evaluate() if em_running else (tra.evaluate(1, batch_size), None)
            if ae_running:
                run_a.cbs.on_epoch_end(epoch, {"loss": la, "val_loss": va})
                ae_running = not ae.stop_training  # once stopped, frozen from here on: the reference's phase 2
            if em_running:
                run_e.cbs.on_epoch_end(epoch, {"loss": le, "val_loss": ve})
                em_running = not em.stop_training
            if verbose in (1, 2):
                print("Epoch %d/%d - ae loss %.4e - emulator loss %s" % (epoch + 1, epochs, la, "%.4e" % le if le is not None else "-"))
        run_a.finish()
        run_e.finish()
        self._chain_model = None
        ha, he = run_a.history.history, run_e.history.history
        return ha["loss"], ha["val_loss"], he["loss"], he["val_loss"]

    def _predict_chain(self):
        blocks = [self.emulator, self.autoencoder.decoder]
        cm = self._chain_model
        if cm is None or cm._blocks[0] is not blocks[0] or cm._blocks[1] is not blocks[1]:
            cm = ChainedModel(blocks, name="ae_emulator_decoder")
            self._chain_model = cm
        cm.precision = self.emulator.precision
        return cm

    def predict(self, params, devices=None):
        """emulator.predict then decoder.predict then unpreproc (emulator.py:788-795),
        evaluated as ONE fused device stack 7 -> ... -> 9 -> 32 -> 352 -> 451."""
        return self._predict_stack(self._predict_chain(), params, devices)

    def test_error(self, use_autoencoder=False, relative=True, flow=None, fhigh=None):
        if use_autoencoder:
            pred = pp.unpreproc(self.autoencoder(pp.preproc(self.signal_test, self.signal_train)), self.signal_train)
        else:
            pred = self.predict(self.par_test)
        return error(self.signal_test, pred, relative=relative, nu_arr=self.frequencies, flow=flow, fhigh=fhigh)


# names used by BASELINE.json's north_star
Emulator = DirectEmulator
VAEEmulator = AutoEncoderEmulator
