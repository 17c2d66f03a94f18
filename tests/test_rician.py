"""The Rician data term without a GPU (sett.noise_model = 'rician'): the majoriser, the accuracy of the
kernel's float32 forms (tests/rician64.py emulates their operation sequence in numpy), the fixed point on flat regions,
the settings and fit()'s refusals, and the new symbol.

Measured here: R to 1.10e-6 relative (cap 2e-6), c to 1.4e-7 (1 + |c|) (cap 1e-6); the fixed point 0.98 / 1.99 for a true
1 / 2 sigma where the plain mean is 1.54 / 2.27."""
import os

import numpy as np
import pytest
import torch

from tests import rician64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (1) the majoriser ------------------------------------------------------------------------------------------------
def test_the_surrogate_majorises_the_likelihood_and_touches_it():
    """Seeded (x, mu0, mu), mu and mu0 of either sign, x = 0 among them, three precisions: surrogate - nll >= -1e-12
    everywhere, 0 at mu = mu0, and the two have the same derivative there (central differences in float64)."""
    rng = np.random.default_rng(5)
    n = 20000
    for tau in (0.04, 1.0, 25.0):
        sd = tau ** -0.5
        x = np.abs(rng.normal(0.0, 3.0 * sd, n))
        x[:500] = 0.0
        mu0, mu = rng.normal(0.0, 3.0 * sd, n), rng.normal(0.0, 3.0 * sd, n)
        mu0[500:600] = 0.0
        slack = rician64.surrogate64(x, mu0, mu, tau) - rician64.nll64(x, mu, tau)
        assert slack.min() >= -1e-12, (tau, slack.min())
        assert slack.max() > 1e-3  # (it is not the likelihood itself)
        touch = rician64.surrogate64(x, mu0, mu0, tau) - rician64.nll64(x, mu0, tau)
        assert np.abs(touch).max() <= 1e-12, (tau, np.abs(touch).max())
        h = 1e-5 * sd
        dn = (rician64.nll64(x, mu0 + h, tau) - rician64.nll64(x, mu0 - h, tau)) / (2 * h)
        ds = (rician64.surrogate64(x, mu0, mu0 + h, tau) - rician64.surrogate64(x, mu0, mu0 - h, tau)) / (2 * h)
        scale = tau * (np.abs(x) + np.abs(mu0)) + 1.0 / sd
        assert (np.abs(dn - ds) <= 1e-6 * scale).all(), (tau, float((np.abs(dn - ds) / scale).max()))


# ---- (2) the float32 forms --------------------------------------------------------------------------------------------
def _grid():
    return np.concatenate([[0.0], np.logspace(-30, 30, 6001), np.linspace(3.5, 4.0, 20001),
                           np.linspace(0.0, 30.0, 30001)]).astype(np.float32)


def test_the_float32_forms_meet_the_accuracy_conditions():
    z = _grid()
    z64 = z.astype(np.float64)
    assert ((z > 3.7499) & (z <= rician64.BRANCH)).any() and ((z > rician64.BRANCH) & (z < 3.7501)).any()
    r32, r64 = rician64.ratio32(z).astype(np.float64), rician64.ratio64(z64)
    c32, c64 = rician64.c32(z).astype(np.float64), rician64.c64(z64)
    assert not np.isnan(r32).any() and not np.isnan(c32).any()
    rel = np.abs(r32 - r64) / np.where(r64 == 0, 1.0, r64)
    cer = np.abs(c32 - c64) / (1.0 + np.abs(c64))
    print('R: worst relative error %.3g at z = %g; c: worst |c32 - c64| / (1 + |c64|) %.3g at z = %g'
          % (rel.max(), z[rel.argmax()], cer.max(), z[cer.argmax()]), flush=True)
    assert (np.abs(r32 - r64) <= 2e-6 * r64).all(), (rel.max(), z[rel.argmax()])
    assert (np.abs(c32 - c64) <= 1e-6 * (1.0 + np.abs(c64))).all(), (cer.max(), z[cer.argmax()])
    assert r32[0] == 0.0 and c32[0] == 0.0  # exactly
    assert (r32 >= 0).all() and (r32 <= 1).all()
    # odd, and c on the negative side is the likelihood's there too
    assert np.array_equal(rician64.ratio32(-z), -rician64.ratio32(z))
    cn32, cn64 = rician64.c32(-z).astype(np.float64), rician64.c64(-z64)
    assert (np.abs(cn32 - cn64) <= 1e-6 * (1.0 + np.abs(cn64))).all()
    ends = np.array([np.inf, -np.inf], np.float32)
    assert rician64.ratio32(ends).tolist() == [1.0, -1.0]
    assert rician64.c32(ends).tolist() == [np.inf, -np.inf]
    assert float(rician64.ratio64(np.inf)) == 1.0


def test_terms32_follows_the_float64_statement():
    """The voxel terms on seeded inputs with gains: xt within (2e-6 + 4 2^-24) |xt64| + 2^-120 and exactly +0 where
    x == 0 - the bound the GPU test holds the kernel to."""
    gen = torch.Generator().manual_seed(3)
    shape, axis, tau = (9, 11, 13), 1, 0.04
    x = rician64.rice(torch.rand(shape, generator=gen, dtype=torch.float64) * 40.0, 5.0, shape, gen).float()
    x[torch.rand(shape, generator=gen) < 0.2] = 0.0
    ay = (torch.randn(shape, generator=gen) * 20.0 + 10.0).float()
    e = (0.5 + 1.5 * torch.rand(shape[axis], generator=gen)).float()
    xt, c = rician64.terms32(x.numpy(), ay.numpy(), e.numpy(), tau, axis)
    xt64, c64 = rician64.terms64(x.numpy(), ay.numpy(), e.numpy(), tau, axis)
    assert (np.abs(xt - xt64) <= (2e-6 + 4 * 2.0 ** -24) * np.abs(xt64) + 2.0 ** -120).all()
    assert (xt[x.numpy() == 0] == 0).all() and not np.signbit(xt[x.numpy() == 0]).any()
    assert (ay.numpy() < 0).any() and (xt < 0).any()  # (R is odd: a negative prediction gives a negative x~)


# ---- (3) the fixed point ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('snr', [1.0, 2.0])
def test_the_fixed_point_removes_the_bias_of_the_mean(snr):
    """4 096 seeded Rician samples with sigma = 1: the MM fixed point from the plain mean lies within 0.1 sigma of the
    signal, the plain mean more than 0.2 sigma above it."""
    gen = torch.Generator().manual_seed(17)
    x = rician64.rice(snr, 1.0, (4096,), gen).numpy()
    mu, mean = rician64.fixed_point64(x, 1.0, n_steps=8)
    print('true %.1f: mean %.3f, fixed point %.3f' % (snr, mean, mu), flush=True)
    assert abs(mu - snr) < 0.1
    assert mean - snr > 0.2


# ---- (4) settings and refusals --------------------------------------------------------------------------------------------
def _cpu_structs():
    from unires_amd.struct import _input, _output, _proj_op, settings
    xn = _input(dat=torch.ones(4, 5, 6), mat=torch.eye(4, dtype=torch.float64))
    xn.po = _proj_op()
    xn.po.dim_thick = 1
    xn.po.rigid = torch.eye(4, dtype=torch.float64)
    y = _output(dat=torch.zeros(4, 5, 6), mat=torch.eye(4, dtype=torch.float64), lam=1.0)
    sett = settings()
    sett.max_iter = 0
    sett.clean_fov = False
    return xn, y, sett


def test_the_default_is_gaussian():
    from unires_amd.struct import settings
    from unires_amd._update import NOISE_MODELS, _noise_model, _obs
    assert settings().noise_model == 'gaussian'
    assert NOISE_MODELS == ('gaussian', 'rician')
    assert _noise_model(object()) == 'gaussian'  # (a settings object from before the knob)
    xn, _, sett = _cpu_structs()
    assert _obs(xn, sett) is xn.dat


@pytest.mark.parametrize('name', ['scaling', 'unified_rigid', 'slice_gain'])
def test_fit_refuses_the_gaussian_updates_with_rician_by_name(name):
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.max_iter = 3
    sett.noise_model = 'rician'
    setattr(sett, name, True)
    with pytest.raises(NotImplementedError, match=r"sett\.%s with sett\.noise_model = 'rician'" % name):
        U.fit([[xn]], [y], sett)
    assert getattr(xn, '_rician_dat', None) is None and xn.slice_gain is None  # refused before anything was made


@pytest.mark.parametrize('bad', ['rice', 'Rician', None, 1])
def test_fit_refuses_an_unknown_noise_model(bad):
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.noise_model = bad
    with pytest.raises(ValueError, match='sett.noise_model'):
        U.fit([[xn]], [y], sett)


@pytest.mark.parametrize('value', [-1e-3, float('nan'), float('inf')])
def test_fit_refuses_negative_or_non_finite_magnitude_data_naming_channel_and_repeat(value):
    import unires_amd as U
    good, _, _ = _cpu_structs()
    xn, y, sett = _cpu_structs()
    xn.dat[1, 2, 3] = value
    sett.noise_model = 'rician'
    with pytest.raises(ValueError, match='negative or non-finite') as err:
        U.fit([[good, xn]], [y], sett)
    assert 'x[0][1].dat' in str(err.value)
    # the Gaussian term takes the same data, and a CT repeat keeps it under 'rician'
    from unires_amd.run import _init_rician
    sett.noise_model = 'gaussian'
    _init_rician([[good, xn]], sett)
    xn.ct = True
    sett.noise_model = 'rician'
    _init_rician([[good, xn]], sett)
    assert xn._rician_dat is None and torch.equal(good._rician_dat, good.dat)


def test_fit_clones_the_observations_and_forgets_them_under_gaussian():
    import unires_amd as U
    from unires_amd._update import _obs
    xn, y, sett = _cpu_structs()
    sett.noise_model = 'rician'
    U.fit([[xn]], [y], sett)
    assert torch.equal(xn._rician_dat, xn.dat) and xn._rician_dat.data_ptr() != xn.dat.data_ptr()
    assert xn._rician_dat.dtype == torch.float32
    assert _obs(xn, sett) is xn._rician_dat
    sett.noise_model = 'gaussian'
    assert _obs(xn, sett) is xn.dat  # (a stale buffer is not read under the Gaussian model)
    xn2, y2, sett2 = _cpu_structs()
    xn2._rician_dat = xn._rician_dat
    U.fit([[xn2]], [y2], sett2)
    assert xn2._rician_dat is None


# ---- (5) symbols --------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_in_the_header_and_in_the_ctypes_table():
    import re
    from unires_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    assert re.search(r'\bint\s+unires_rician_terms\s*\(', header)
    assert 'unires_rician_terms' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['unires_rician_terms'][1]) == 10
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert "'rician.hip'" in entry and "'rician.hpp'" in entry
