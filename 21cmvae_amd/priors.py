"""Priors of the on-device samplers (include/v21.h: v21_mlp_set_prior; not in the reference): separable in
par_transform's coordinates u in [-1, 1]^7, every column uniform on the training box or a normal truncated to it.

    Prior({"tau": ("normal", 0.054, 0.007), "fstar": ("lognormal", -1.5, 0.3)})

``("normal", mean, sd)`` is in raw units and allowed on the linear columns only, ``("lognormal", mean_log10, sd_dex)`` on
the log10 columns only: both are normals in u, where the samplers work.  ``"uniform"`` (the default for a label left out)
is uniform in u: uniform in a linear column, log-uniform in a log10 column.
"""
import numpy as np
from scipy.special import ndtr, ndtri

from . import preprocess as pp

PAR_LABELS = ["fstar", "Vc", "fx", "tau", "alpha", "nu_min", "Rmfp"]


def tnorm_z(a, b, c):
    """The truncated standard normal's inverse CDF in float64: z with Phi(z) = Phi(a) + c (Phi(b) - Phi(a)), a < b the
    standardised ends, c in (0, 1).  Where the interval's middle lies above the mode (a + b > 0) the mirrored problem is
    solved, so that Phi is always taken in the tail nearer the mode -- the arithmetic of the nested sampler's drawn
    starts (csrc/nested_kernels.h: nest_tnorm_z)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    flip = a + b > 0.0
    lo, hi = np.where(flip, -a, a), np.where(flip, -b, b)
    pa, pb = ndtr(lo), ndtr(hi)
    # (pa - c (pa - pb) and pa + c (pb - pa), each as the device forms it)
    z = ndtri(np.where(flip, pa - c * (pa - pb), pa + c * (pb - pa)))
    return np.where(flip, -z, z)


def tnorm_log_mass(a, b):
    """ln(Phi(b) - Phi(a)), a < b, taken in the tail nearer the mode as ``tnorm_z`` takes it"""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    flip = a + b > 0.0
    lo, hi = np.where(flip, -b, a), np.where(flip, -a, b)
    return np.log(ndtr(hi) - ndtr(lo))


class Prior:
    """A separable prior from ``{label: spec}`` (above).  ValueError, naming the column: an unknown label, a normal on a
    log10 column, a lognormal on a linear one, a malformed spec, an sd that is not positive and finite.
    ``par_train``: the training parameters whose box defines u; given here, the methods below need none (one passed to
    a method takes precedence).
    ``to_u(par_train)`` -> (kind int32, mu, sd float64), each (7,), in u through par_transform's lo / span: what
    v21_mlp_set_prior takes (kind 0 uniform, 1 normal; mu = 0, sd = 1 where uniform).
    ``log_density_u(u)``: ln of the density normalised on the box RELATIVE TO THE UNIFORM PRIOR, ln[p(u) 2^d]
    -- 0 everywhere for an all-uniform prior, so an evidence keeps its definition as the mean of L under the prior.
    ``log_integral_u(free)``: ln of the unnormalised density's integral over the box, over the columns of ``free``.
    ``ppf_u(cube)``: the unit cube -> u, column by column the inverse CDF."""

    def __init__(self, spec=None, par_train=None, labels=None):
        self.labels = list(PAR_LABELS if labels is None else labels)
        self.par_train = par_train
        self.spec = {}
        for name, s in dict(spec or {}).items():
            if name not in self.labels:
                raise ValueError("prior: unknown parameter %r (one of %s)" % (name, ", ".join(self.labels)))
            j = self.labels.index(name)
            is_log = j in pp.LOG_COLUMNS
            if isinstance(s, str):
                if s != "uniform":
                    raise ValueError("prior on %r: %r (\"uniform\", (\"normal\", mean, sd) or (\"lognormal\", mean_log10, sd_dex))" % (name, s))
                continue
            try:
                kind, mean, sd = s
                mean, sd = float(mean), float(sd)
            except (TypeError, ValueError):
                raise ValueError("prior on %r: %r (\"uniform\", (\"normal\", mean, sd) or (\"lognormal\", mean_log10, sd_dex))" % (name, s)) from None
            if kind not in ("normal", "lognormal"):
                raise ValueError("prior on %r: kind %r (\"normal\" or \"lognormal\")" % (name, kind))
            if kind == "normal" and is_log:
                raise ValueError("prior on %r: a log10 column takes (\"lognormal\", mean_log10, sd_dex), not a normal" % name)
            if kind == "lognormal" and not is_log:
                raise ValueError("prior on %r: a linear column takes (\"normal\", mean, sd), not a lognormal" % name)
            if not (np.isfinite(mean) and np.isfinite(sd) and sd > 0.0):
                raise ValueError("prior on %r: mean %r, sd %r (finite, sd positive)" % (name, mean, sd))
            self.spec[name] = (kind, mean, sd)

    @classmethod
    def of(cls, prior, par_train=None):
        """None -> None; a Prior -> itself; a dict -> Prior(dict, par_train)"""
        if prior is None or isinstance(prior, cls):
            return prior
        return cls(prior, par_train)

    def _train(self, par_train):
        pt = self.par_train if par_train is None else par_train
        if pt is None:
            raise ValueError("prior: no training parameters to take the box from (pass par_train)")
        return pt

    def to_u(self, par_train=None):
        st = pp.ParamStats.of(self._train(par_train))
        d = len(self.labels)
        kind, mu, sd = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
        span = st.hi - st.lo
        for name, (_, mean, s) in self.spec.items():
            j = self.labels.index(name)
            kind[j] = 1
            mu[j] = 2.0 * (mean - st.lo[j]) / span[j] - 1.0
            sd[j] = 2.0 * s / span[j]
        return kind, mu, sd

    def log_density_u(self, u, par_train=None):
        kind, mu, sd = self.to_u(par_train)
        q = np.array(u, np.float64, ndmin=2)
        out = np.zeros(q.shape[0])
        for j in np.flatnonzero(kind):
            z = (q[:, j] - mu[j]) / sd[j]
            out += -0.5 * z * z - 0.5 * np.log(2.0 * np.pi) - np.log(sd[j]) - tnorm_log_mass((-1.0 - mu[j]) / sd[j], (1.0 - mu[j]) / sd[j]) + np.log(2.0)
        return out[0] if np.ndim(u) == 1 else out

    def log_integral_u(self, free=None, par_train=None):
        """ln of the integral over the box of exp(ln p), ln p = -1/2 sum ((u - mu) / sd)^2 the UNNORMALISED log density the
        device works with, over the columns of ``free`` (a boolean mask; None: all): ln(sqrt(2 pi) sd [Phi(b) - Phi(a)])
        per normal column, ln 2 per uniform one.  Subtracted from a Laplace value of the integral of L exp(ln p) it gives
        the evidence with respect to the normalised prior on those columns (``fit_parameters``)."""
        kind, mu, sd = self.to_u(par_train)
        free = np.ones(len(kind), bool) if free is None else np.asarray(free, bool)
        out = 0.0
        for j in np.flatnonzero(free):
            if kind[j]:
                out += 0.5 * np.log(2.0 * np.pi) + np.log(sd[j]) + float(tnorm_log_mass((-1.0 - mu[j]) / sd[j], (1.0 - mu[j]) / sd[j]))
            else:
                out += np.log(2.0)
        return float(out)

    def ppf_u(self, cube, par_train=None):
        kind, mu, sd = self.to_u(par_train)
        c = np.array(cube, np.float64, ndmin=2)
        q = 2.0 * c - 1.0
        for j in np.flatnonzero(kind):
            q[:, j] = np.clip(mu[j] + sd[j] * tnorm_z((-1.0 - mu[j]) / sd[j], (1.0 - mu[j]) / sd[j], c[:, j]), -1.0, 1.0)
        return q[0] if np.ndim(cube) == 1 else q
