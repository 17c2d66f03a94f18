"""Exact medians, without a GPU: the restatement tests/median64.py checked against itself - the key
order, the three-pass digit select against the sort, the Haar detail - the estimator on a background-free phantom against
the planted noise and against the mixture rule, the new setting names, and the C-ABI surface.

Recorded on the phantom (48 x 48 x 40, zero outside a ball, 32 798 complete cells): the restated 'mad' sd is 5.441 for a
planted 5 and 21.716 for a planted 20 (both + 9 %: the curved edges of the piecewise-constant classes put a few per cent
of large details above the median); the mixture rule's sd is 64.3 and 71.5 - the spread of a tissue class."""
import os
import re

import numpy as np
import pytest

from tests import median64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('unires_median_absres', 'unires_median_hh', 'unires_voxel_huber_dev')


def value_sets(n, seed=0):
    """The magnitudes' value sets of the bit-for-bit cases, as float32 arrays of n values (signs mixed): all equal; two
    values one ulp apart straddling the rank (the last pass decides); one value per binary exponent (the first pass
    decides); subnormals and exact zeros; random normal."""
    rng = np.random.RandomState(seed + n)
    sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0).astype(np.float32)
    lo = np.float32(1.2345678)
    hi = np.nextafter(lo, np.float32(2.0))
    # (n >= 3: the rank-th smallest is the first `hi`; n == 2: one of each)
    ulp = np.where(np.arange(n) < max((n + 1) // 2 - 1, min(n - 1, 1)), lo, hi).astype(np.float32)
    rng.shuffle(ulp)
    expo = np.ldexp(np.float32(1.0), (np.arange(n) % 253) - 126).astype(np.float32)  # 2^-126 .. 2^126
    rng.shuffle(expo)
    sub = (rng.randint(0, 4, n) * rng.randint(0, 1 << 23, n)).astype(np.uint32).view(np.float32)  # 0 and subnormals
    return {'equal': np.full(n, 3.25, np.float32) * sign, 'ulp': ulp * sign, 'exponents': expo * sign, 'subnormal': sub * sign,
            'normal': (rng.standard_normal(n) * 7.0).astype(np.float32)}


SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1027, 40003)


def test_key_order_is_value_order():
    rng = np.random.RandomState(1)
    v = np.concatenate([rng.standard_normal(4000).astype(np.float32) * 1e3, value_sets(600)['subnormal'],
                        np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38], np.float32)])
    a, k = np.abs(v), M.key(v)
    order = np.argsort(k, kind='stable')
    assert (a[order][1:] >= a[order][:-1]).all()  # sorted by key is sorted by magnitude (inf included)
    assert ((a[:, None] < a[None, :200]) == (k[:, None] < k[None, :200])).all()
    assert M.key(np.float32(-0.0)) == M.key(np.float32(0.0)) == 0
    assert M.key(np.float32(-2.5)) == M.key(np.float32(2.5))


@pytest.mark.parametrize('n', SIZES)
def test_digit_select_equals_the_sort(n):
    for name, v in value_sets(n).items():
        got, want = M.digit_select(np.abs(v)), M.lower_median(np.abs(v))
        assert got[1] == want[1] == n
        assert np.float32(got[0]).view(np.uint32) == np.float32(want[0]).view(np.uint32), (name, n, got, want)
    assert M.digit_select(np.zeros(0, np.float32)) == (0.0, 0) and M.lower_median([]) == (0.0, 0)
    v = value_sets(n)['ulp']
    if n > 1:  # the two values differ in the last key bit only, and (n >= 3) the median is the upper one
        assert len(set(M.key(v).tolist())) == 2 and (n == 2 or M.lower_median(np.abs(v))[0] == np.abs(v).max())


def test_lower_median_convention():
    assert M.lower_median([4.0, 1.0, 3.0, 2.0]) == (2.0, 4)  # torch.median's: the lower of the two middle values
    assert M.lower_median([5.0, 1.0, 3.0]) == (3.0, 3)


def test_eligibility_of_the_residuals():
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0, np.nan, 5.0], np.float32)
    ay = np.array([9.0, 1.0, np.inf, 1.0, np.nan, 1.0, 5.5], np.float32)
    pr = np.array([1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.5], np.float32)
    assert M.absres(x, ay).tolist() == [0.0, 2.0, 0.5]       # x == 0, inf, nan and a nan x are out; x == ay counts as 0
    assert M.absres(x, ay, pr).tolist() == [0.0, 0.5]        # ... and so is prior == 0
    assert M.median_absres(x, ay, np.zeros(7)) == (0.0, 0)


def test_haar_detail_of_a_ramp_is_zero_and_counts_cells():
    i, j, k = np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing='ij')
    ramp = (8.0 + 2.0 * i + 3.0 * j + 5.0 * k).astype(np.float32)
    for axis in range(3):
        t = M.hh(ramp, axis)
        cells = np.prod([s - (a != axis) for a, s in enumerate(ramp.shape)])
        assert t.size == cells and (t == 0).all()
    assert M.hh(ramp[:1], 2).size == 0 and M.hh(ramp[:, :1], 0).size == 0  # no complete cell
    z = ramp.copy()
    z[2, 2, 1] = 0.0  # one zero removes the four cells of its plane that touch it
    assert M.hh(z, 2).size == 5 * 4 * 4 - 4
    neg = -ramp
    assert M.hh(neg, 2).size == 0 and M.hh(neg, 2, ct=True).size == 5 * 4 * 4
    d = np.zeros((2, 2, 1), np.float32)
    d[0, 0, 0], d[1, 0, 0], d[0, 1, 0], d[1, 1, 0] = 10.0, 1.0, 2.0, 4.0
    assert M.hh(d, 2).tolist() == [11.0]  # ((a - b) - c) + d


@pytest.mark.parametrize('sd', [5.0, 20.0])
def test_mad_estimate_on_a_background_free_phantom(sd):
    """The restated sd within 15 % of the planted one; the mixture rule (tests/noise_restated.py) off by more than a
    factor of 2 on the same volume: it has no noise class to find."""
    from tests import noise_restated as NR
    v = M.phantom(sd)
    assert (v == 0).mean() > 0.5 and (v[v != 0] > 100).all()
    med, N = M.median_hh(v, 2)
    got = float(M.sd_of(med))
    mix = float(NR.estimate(v, ct=False)['sd'])
    print('planted sd %g: mad %.3f (%d cells), mixture %.3f; mu %.3f' % (sd, got, N, mix, M.mu_of(v)), flush=True)
    assert N > 30000
    assert abs(got - sd) <= 0.15 * sd
    assert mix > 2.0 * sd or mix < 0.5 * sd


def test_float32_chains():
    med = np.float32(7.3399963)
    assert M.sd_of(med) == np.float32(np.float32(np.float32(1.4826) * med) * np.float32(0.5))
    assert M.mult_of(3.0) == np.float32(np.float32(3.0) * np.float32(1.4826))
    assert M.threshold(med, 3.0) == np.float32(M.mult_of(3.0) * med)
    import torch
    sd = torch.tensor(float(M.sd_of(med)), dtype=torch.float32)
    assert float(1 / sd ** 2) == float(M.tau_of(M.sd_of(med)))


def test_setting_names_and_defaults():
    import unires_amd as U
    from unires_amd._core import _noise_est
    from unires_amd._update import _voxel_scale
    from unires_amd.run import fit, init
    s = U.settings()
    assert s.noise_est == 'mixture' and s.voxel_scale == 'noise'
    assert _noise_est(s) == 'mixture' and _voxel_scale(s) == 'noise'
    s.noise_est, s.voxel_scale = 'mad', 'mad'
    assert _noise_est(s) == 'mad' and _voxel_scale(s) == 'mad'
    s.noise_est = 'median'
    with pytest.raises(ValueError, match='noise_est'):
        _noise_est(s)
    with pytest.raises(ValueError, match='noise_est'):
        init([], s)  # refused before anything is read
    s.voxel_scale = 'sigma'
    with pytest.raises(ValueError, match='voxel_scale'):
        _voxel_scale(s)
    import torch
    from unires_amd.struct import _input, _output
    x = [[_input(torch.zeros(2, 2, 2), torch.eye(4, dtype=torch.float64))]]
    y = [_output(torch.zeros(2, 2, 2), torch.eye(4, dtype=torch.float64), 1.0)]
    with pytest.raises(ValueError, match='voxel_scale'):
        fit(x, y, s)  # refused before any device work, robust or not


def test_new_symbols_are_declared_and_bound():
    from unires_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    declared = set(re.findall(r'\b(unires_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['unires_median_absres'][1]) == 7
    assert len(_lib.SIGNATURES['unires_median_hh'][1]) == 8
    assert len(_lib.SIGNATURES['unires_voxel_huber_dev'][1]) == 8
    m = re.search(r'#define UNIRES_MEDIAN_WORK_BYTES (\d+)', hdr)
    assert m and int(m.group(1)) == _lib.UNIRES_MEDIAN_WORK_BYTES == 4 * (3 * 2048 + 4)
