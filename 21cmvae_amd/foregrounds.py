"""Linear foreground bases for the marginalised likelihood (include/v21.h: v21_mlp_set_nuisance; not in the reference).

A measured global-signal spectrum is a foreground of 10^3 - 10^4 K plus a signal of ~10^2 mK.  Every model that is linear
in its amplitudes, d = signal(theta) + A^T a + noise with a flat prior on a, is integrated out analytically by the
library: ``log_likelihood``, ``fisher``, ``fit_parameters`` and ``sample_posterior`` of the emulator classes take
``foreground=`` a number of LinLog terms or any (K, n_bins) basis A."""
import numpy as np


def linlog_basis(frequencies, n_terms, nu0=None, index=-2.5):
    """The "LinLog" foreground polynomial: rows (nu / nu0)^index ln(nu / nu0)^k, k = 0 .. n_terms - 1 -> (n_terms, len(nu))
    float64.  ``nu0`` defaults to the geometric centre sqrt(nu_min nu_max) of ``frequencies`` (the logarithms then change
    sign inside the band, which keeps the terms far from parallel)."""
    nu = np.asarray(frequencies, np.float64).ravel()
    n_terms = int(n_terms)
    if n_terms < 1:
        raise ValueError("linlog_basis: n_terms must be >= 1")
    if nu.size < 1 or not np.all(nu > 0):
        raise ValueError("linlog_basis: frequencies must be positive")
    if nu0 is None:
        nu0 = np.sqrt(nu.min() * nu.max())
    x = nu / float(nu0)
    lx = np.log(x)
    return np.stack([x ** float(index) * lx ** k for k in range(n_terms)])


def band_basis(frequencies, n_terms, flow=None, fhigh=None, index=-2.5):
    """``linlog_basis`` over the bins of the band [flow, fhigh] (selected as ``error`` selects them), zero outside:
    (n_terms, len(nu)), the form ``foreground=n_terms`` stands for."""
    nu = np.asarray(frequencies, np.float64).ravel()
    sel = np.ones(nu.size, bool)
    if flow:
        sel &= nu >= flow
    if fhigh:
        sel &= nu <= fhigh
    if not sel.any():
        raise ValueError("No frequency bin lies in the band [%r, %r]." % (flow, fhigh))
    A = np.zeros((int(n_terms), nu.size))
    A[:, sel] = linlog_basis(nu[sel], n_terms, index=index)
    return A


__all__ = ["linlog_basis", "band_basis"]
