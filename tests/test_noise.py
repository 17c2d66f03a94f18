"""CPU checks of the noise / intensity hyper-parameter estimator: the float64
restatement (tests/noise_restated.py) recovers planted parameters, _init_lam follows the reference's
formula, and the library and package declare the new entry points."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import noise_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('snr', [0.0, 0.3, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 15.0, 40.0])
@pytest.mark.parametrize('sig', [1.0, 75.0])
def test_koay_basser_round_trip(snr, sig):
    nu = snr * sig
    mean, var = R.rice_moments(nu, sig)
    nu2, sig2 = R.koay_basser(mean, var)
    if snr == 0.0:
        # a Rayleigh distribution sits on the nu = 0 boundary: either branch by rounding; the fixed
        # point creeps towards theta = 0 there, and stops on its step rule with nu small but not 0
        assert nu2 < 0.2 * sig and sig2 == pytest.approx(sig, rel=5e-3)
    elif snr < 1.0:
        # low SNR: nu is poorly determined by two moments, sigma well
        assert sig2 == pytest.approx(sig, rel=2e-3) and abs(nu2 - nu) < 0.1 * sig
    else:
        assert sig2 == pytest.approx(sig, rel=1e-4) and nu2 == pytest.approx(nu, rel=1e-4)


def test_koay_basser_below_rayleigh_ratio_gives_nu_zero():
    mean, var = 1.0, 1.0  # r = 1 < sqrt(pi / (4 - pi))
    assert R.koay_basser(mean, var) == (0.0, math.sqrt((mean * mean + var) / 2.0))


def _rician(n, seed, frac_bg=0.6, nu=1000.0, sd=75.0):
    rng = np.random.default_rng(seed)
    loc = np.where(rng.random(n) < frac_bg, 0.0, nu)
    return np.abs(loc + sd * rng.standard_normal(n) + 1j * sd * rng.standard_normal(n)).astype(np.float32)


def _gaussian(n, seed, lo=-1000.0, hi=40.0, sd=20.0):
    rng = np.random.default_rng(seed)
    return (np.where(rng.random(n) < 0.5, lo, hi) + sd * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize('seed', [0, 1])
def test_restatement_recovers_rician_noise(seed):
    r = R.estimate(_rician(10 ** 6, seed), ct=False)
    assert not r['gmm']
    assert r['sd'] == pytest.approx(75.0, rel=0.02)
    # mu = |mean_fg - mean_bg|: the background class mean is the Rayleigh mean sd sqrt(pi / 2)
    assert r['mu'] == pytest.approx(1000.0 - 75.0 * math.sqrt(math.pi / 2), rel=0.02)


@pytest.mark.parametrize('seed', [0, 1])
def test_restatement_recovers_gaussian_noise(seed):
    r = R.estimate(_gaussian(10 ** 6, seed), ct=True)
    assert r['gmm']
    assert r['sd'] == pytest.approx(20.0, rel=0.02)
    assert r['mu'] == pytest.approx(1040.0, rel=0.02)


def test_restatement_selection_and_binning():
    v = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 1.0, 2.0, 5.0, 5.0], np.float32)
    assert sorted(R.select(v, ct=False).tolist()) == [1.0, 2.0, 5.0, 5.0]
    assert sorted(R.select(v, ct=True).tolist()) == [-3.0, 1.0, 2.0, 5.0, 5.0]
    counts, (mn, mx) = R.histogram(v, ct=False)
    assert (mn, mx) == (1.0, 5.0) and counts.sum() == 4
    assert counts[0] == 1 and counts[256] == 1 and counts[1023] == 2  # 2.0 on an edge; mx in the last bin
    assert R.histogram(np.zeros(8, np.float32), ct=False)[0] is None
    assert R.histogram(np.full(8, 3.0, np.float32), ct=False)[0] is None
    with pytest.raises(ValueError):
        R.estimate(np.full(8, -3.0, np.float32), ct=False)


@pytest.mark.parametrize('method', ['super-resolution', 'denoising'])
def test_init_lam_matches_reference_formula(method):
    import unires_amd as U
    sett = U.settings()
    sett.method = method
    mus = [[900.0, 1100.0], [400.0], [2000.0, 1500.0, 1000.0]]
    cts = [[False, False], [True], [False, True, False]]
    x = []
    for mc, cc in zip(mus, cts):
        xc = []
        for mu, ct in zip(mc, cc):
            xn = U._input()
            xn.mu, xn.ct = torch.tensor(mu, dtype=torch.float32), ct
            xc.append(xn)
        x.append(xc)
    y = [U._output() for _ in x]
    U._init_lam(x, y, sett)
    for c in range(3):
        want = R.init_lam(mus[c], cts[c], 3, method == 'super-resolution')
        assert float(y[c].lam0) == float(want) and float(y[c].lam) == float(want)
    # the CT repeat's mu counts a quarter in super-resolution only
    plain = math.sqrt(1 / 3) / 400.0
    assert float(y[1].lam0) == pytest.approx(plain * (4 if method == 'super-resolution' else 1), rel=1e-6)


def test_library_declares_the_noise_entry_points(lib):
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    declared = set(re.findall(r'\b(unires_[a-z0-9_]+)\s*\(', hdr))
    assert {'unires_noise_hist', 'unires_noise_fit'} <= declared
    assert lib.unires_noise_hist and lib.unires_noise_fit


def test_package_exports_the_estimator():
    import unires_amd as U
    for name in ('_estimate_hyperpar', '_init_lam', 'stats'):
        assert name in U.__all__ and hasattr(U, name)
    assert callable(U.stats.estimate_noise)
    with pytest.raises(NotImplementedError):
        U.stats.estimate_noise(torch.zeros(4), num_class=3)


def test_noise_entry_points_validate_arguments(lib):
    import ctypes as C
    ptrs = (C.c_void_p * 1)(None)
    sizes = (C.c_int64 * 1)(8)
    ct = (C.c_int32 * 1)(0)
    buf = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    assert lib.unires_noise_hist(1, ptrs, sizes, ct, buf, buf, None) == 1  # null observation
    assert lib.unires_noise_hist(0, ptrs, sizes, ct, buf, buf, None) == 3
    ptrs[0] = 16
    sizes[0] = 0
    assert lib.unires_noise_hist(1, ptrs, sizes, ct, buf, buf, None) == 2
    assert lib.unires_noise_fit(1, None, buf, 10, buf, None) == 1
    assert lib.unires_noise_fit(0, buf, buf, 10, buf, None) == 3
    assert lib.unires_noise_fit(1, buf, buf, -1, buf, None) == 3
