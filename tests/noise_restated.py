"""Float64 NumPy / SciPy restatement of the noise estimator (the GPU form is
``unires_amd/csrc/noise.hip``): voxel selection, the 1024-bin histogram, the two-class Rice or
Gaussian EM and the Koay-Basser moment inversion, operation for operation in the kernel's order,
with ``scipy.special.i0e`` / ``i1e``."""
import math

import numpy as np
from scipy.special import i0e, i1e

BINS = 1024
EPS = np.finfo(np.float64).eps
RAYLEIGH_R = math.sqrt(math.pi / (4.0 - math.pi))  # mean / sd of a Rayleigh distribution


def select(dat, ct):
    """The voxels the histogram takes: finite, non-zero, and >= 0 unless CT (float32, flat)."""
    v = np.asarray(dat, dtype=np.float32).ravel()
    keep = np.isfinite(v) & (v != 0)
    if not ct:
        keep &= v >= 0
    return v[keep]


def histogram(dat, ct):
    """(counts (1024,) int64 or None, (mn, mx) float32): None when nothing is selected or mn == mx."""
    v = select(dat, ct)
    if v.size == 0:
        return None, (np.float32(np.inf), np.float32(-np.inf))
    mn, mx = v.min(), v.max()
    if not mx > mn:
        return None, (mn, mx)
    q = ((v.astype(np.float64) - np.float64(mn)) * float(BINS)) / (np.float64(mx) - np.float64(mn))
    idx = np.minimum(np.floor(q).astype(np.int64), BINS - 1)
    return np.bincount(idx, minlength=BINS), (mn, mx)


def koay_xi(th):
    t2 = th * th
    z = 0.25 * t2
    b = (2.0 + t2) * i0e(z) + t2 * i1e(z)
    return 2.0 + t2 - (math.pi / 8.0) * b * b


def koay_basser(mean, var):
    """Rice (nu, sigma) of the given mean and variance: the Koay-Basser fixed point started at
    theta = mean / sd, at most 256 steps, stopped at |d theta| < 1e-6; nu = 0 at or below the
    Rayleigh ratio."""
    r = mean / math.sqrt(var)
    if not r > RAYLEIGH_R:
        return 0.0, math.sqrt((mean * mean + var) / 2.0)
    th = r
    for _ in range(256):
        tn = math.sqrt(max(koay_xi(th) * (1.0 + r * r) - 2.0, 0.0))
        d = abs(tn - th)
        th = tn
        if d < 1e-6:
            break
    xi = koay_xi(th)
    sig = math.sqrt(var / xi)
    return math.sqrt(max(mean * mean + (xi - 2.0) * sig * sig, 0.0)), sig


def rice_mean(nu, sig):
    a = nu * nu / (2.0 * sig * sig)
    if a >= 20.0:
        return nu
    z = 0.5 * a
    return math.sqrt(math.pi * sig * sig / 2.0) * ((1.0 + 2.0 * z) * i0e(z) + 2.0 * z * i1e(z))


def rice_moments(nu, sig):
    """Exact (mean, variance) of Rice(nu, sigma) - no large-SNR shortcut - with E x^2 = nu^2 + 2 sigma^2."""
    z = nu * nu / (4.0 * sig * sig)
    m = math.sqrt(math.pi * sig * sig / 2.0) * ((1.0 + 2.0 * z) * i0e(z) + 2.0 * z * i1e(z))
    return m, nu * nu + 2.0 * sig * sig - m * m


def _pdf(gmm, x, loc, sig):
    s2 = sig * sig
    d = x - loc
    if gmm:
        return np.exp(-(d * d) / (2.0 * s2)) / np.sqrt(2.0 * math.pi * s2)
    return x / s2 * np.exp(-(d * d) / (2.0 * s2)) * i0e(x * loc / s2)


def fit(counts, mn, mx, max_iter=10000, stop=True):
    """Two-class EM on a histogram over linspace(mn, mx, 1024).  ``stop=False`` runs exactly
    ``max_iter`` M-steps (the GPU's count).  Returns a dict: mg, loc, sig, mean (2-vectors), ll (the
    last E-step's), iters (M-steps), sd, mu, gmm."""
    mn, mx = float(mn), float(mx)
    gmm = mn < 0
    h_all = np.asarray(counts, dtype=np.float64)
    x_all = np.linspace(mn, mx, BINS)
    nz = h_all > 0
    h, x = h_all[nz], x_all[nz]
    sumh = float(h_all.sum())
    tol = 1e-8 * sumh
    mg = [0.5, 0.5]
    if gmm:
        loc = [mn + 1.0 * (mx - mn) / 3.0, mn + 2.0 * (mx - mn) / 3.0]
        sig = [(mx - mn) / 20.0] * 2
    else:
        loc = [0.0, mx / 3.0]
        sig = [mx / 20.0] * 2
    ll, ll_prev, it = 0.0, -np.inf, 0
    while it < max_iter:
        p0 = mg[0] * _pdf(gmm, x, loc[0], sig[0]) + EPS
        p1 = mg[1] * _pdf(gmm, x, loc[1], sig[1]) + EPS
        s = p0 + p1
        r = [h * (p0 / s), h * (p1 / s)]
        ll = float(np.sum(h * np.log(s)))
        if stop and ll - ll_prev < tol:
            break
        tot = [(float(np.sum(rk)), float(np.sum(rk * x)), float(np.sum(rk * x * x))) for rk in r]
        m0s = tot[0][0] + tot[1][0]
        for k in range(2):
            m0, m1, m2 = tot[k]
            mg[k] = m0 / m0s
            mean = m1 / m0
            var = (m2 - m1 * m1 / m0 + 1e-6) / (m0 + 1e-6)
            if gmm:
                loc[k], sig[k] = mean, math.sqrt(var)
            else:
                loc[k], sig[k] = koay_basser(mean, var)
        ll_prev = ll
        it += 1
    mean = [loc[k] if gmm else rice_mean(loc[k], sig[k]) for k in range(2)]
    bg = 1 if mean[1] < mean[0] else 0
    return dict(mg=np.array(mg), loc=np.array(loc), sig=np.array(sig), mean=np.array(mean), ll=ll,
                iters=it, sd=sig[bg], mu=abs(mean[1 - bg] - mean[bg]), gmm=gmm)


def estimate(dat, ct=True, max_iter=10000):
    """The whole estimator on one volume (ValueError when nothing usable is left)."""
    counts, (mn, mx) = histogram(dat, ct)
    if counts is None:
        raise ValueError('no finite non-zero voxels, or all of them equal')
    return fit(counts, mn, mx, max_iter)


def init_lam(mus, cts, n_channels, super_resolution):
    """The reference's lambda (unires/_core.py:273-281) for one channel's repeats, in float32."""
    import torch
    mu_c = torch.zeros(len(mus), dtype=torch.float32)
    for n, (mu, ct) in enumerate(zip(mus, cts)):
        mu_c[n] = float(mu)
        if ct and super_resolution:
            mu_c[n] /= 4
    return math.sqrt(1 / n_channels) / torch.mean(mu_c)
