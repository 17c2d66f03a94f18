"""The slice gains in the rigid Gauss-Newton update, without a GPU: the derivatives tests/gne64.py
states against finite differences of the data term in float64, the switch ``sett.gain_gn`` and what fit() refuses with
and without it, the new symbol and its argument checks (they come before anything touches the device; the pointers are
never followed), and gne64's float32 restatement against its float64 one."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gain64, gne64, slice64, voxel64
from tests.test_gain import _cpu_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53


# ---- the derivatives ----------------------------------------------------------------------------------------------------
def _problem(with_g, with_u, axis=1, shape=(6, 5, 4)):
    """x with zeros, a != 0, generic gains in [0.5, 2]; a and the step are dyadic, so a +- h is exact."""
    gen = torch.Generator().manual_seed(7 + 2 * with_g + with_u)
    x = (torch.rand(shape, generator=gen) * 10).double().numpy()
    x[x < 2.0] = 0.0
    a = (torch.randint(32, 640, shape, generator=gen).double() / 64.0).numpy()  # in [0.5, 10), multiples of 2^-6
    g = voxel64.weights(shape, 'ramp').double().numpy() if with_g else None
    u = slice64.weights(shape[axis], 'ramp', seed=3).double().numpy() if with_u else None
    e = gain64.gains(shape[axis], 'generic').double().numpy()
    return x, a, g, u, e, axis


@pytest.mark.parametrize('with_u', [False, True])
@pytest.mark.parametrize('with_g', [False, True])
def test_residual_and_hessian_weight_are_the_derivatives_of_the_data_term(with_g, with_u):
    """E is a quadratic in every component of a, so the central difference IS the derivative and the second difference
    IS the curvature, whatever the step: what is left is the rounding of the three evaluations of E.  One evaluation
    adds N terms of at most 5 roundings each (e a, the difference, g u, and two products) and scales once:
    |fl(E) - E| <= gamma M, gamma = (N + 6) 2^-53 (1 + 1e-2), M = 1/2 tau sum W (|x| + |e| (|a| + h))^2 >= E - the
    difference x - e a may cancel, so the error is relative to the magnitudes, not to E.  Hence
        |FD1 - dE/da| <= 2 gamma M / (2 h) + 8 2^-53 |tau W e| (|e a| + |x|)   (the last: the derivative's own roundings)
        |FD2 - d2E/da2| <= 4 gamma M / h^2 + 8 2^-53 tau W e^2."""
    x, a, g, u, e, axis = _problem(with_g, with_u)
    tau, h = 0.04, 0.5
    N = a.size
    W = gne64.weight64(a.shape, axis, g, u)
    ev = np.broadcast_to(gne64._at(e, a.shape, axis), a.shape)
    M = 0.5 * tau * float(np.sum(np.where(x != 0, W * (np.abs(x) + ev * (np.abs(a) + h)) ** 2, 0.0)))
    gamma = (N + 6) * U53 * 1.01
    d1, d2 = gne64.resid64(a, x, axis, g, u, e, tau), gne64.hess64(x, axis, g, u, e, tau)
    E0 = gne64.energy64(a, x, axis, g, u, e, tau)
    worst1 = worst2 = 0.0
    for idx in np.ndindex(a.shape):
        ap, am = a.copy(), a.copy()
        ap[idx] += h
        am[idx] -= h
        assert ap[idx] - a[idx] == h and a[idx] - am[idx] == h  # (the steps are exact)
        Ep, Em = gne64.energy64(ap, x, axis, g, u, e, tau), gne64.energy64(am, x, axis, g, u, e, tau)
        fd1, fd2 = (Ep - Em) / (2 * h), (Ep - 2 * E0 + Em) / (h * h)
        b1 = gamma * M / h + 8 * U53 * tau * W[idx] * ev[idx] * (ev[idx] * abs(a[idx]) + abs(x[idx]))
        b2 = 4 * gamma * M / (h * h) + 8 * U53 * tau * W[idx] * ev[idx] ** 2
        assert abs(fd1 - d1[idx]) <= b1, (idx, fd1, d1[idx], b1)
        assert abs(fd2 - d2[idx]) <= b2, (idx, fd2, d2[idx], b2)
        worst1, worst2 = max(worst1, abs(fd1 - d1[idx]) / b1), max(worst2, abs(fd2 - d2[idx]) / b2)
    assert bool((d1[x == 0] == 0).all()) and bool((d2[x == 0] == 0).all()) and bool((x == 0).any())
    assert bool((d2[(x != 0) & (W > 0)] > 0).all())
    print('g %d u %d: worst |FD1 - d1| / bound %.3g, |FD2 - d2| / bound %.3g' % (with_g, with_u, worst1, worst2))


@pytest.mark.parametrize('with_u', [False, True])
@pytest.mark.parametrize('with_g', [False, True])
def test_float32_residual_follows_the_float64_one(with_g, with_u):
    """gne64.terms_e32's residual against resid64 with tau = 1, on float32 inputs: the float32 form rounds p, the
    difference and the product - 2^-24 (|p| + |p - x|) on the difference, carried through W e, and 3 2^-24 of the result
    for t and the product; its sums are slice64's / voxel64's of the gained prediction."""
    x, a, g, u, e, axis = _problem(with_g, with_u)
    f32 = lambda v: None if v is None else np.asarray(v, np.float32)
    x, a, g, u, e = f32(x), f32(a), f32(g), f32(u), f32(e)
    out, sums, bound = gne64.terms_e32(x, a, axis, g, u, e)
    ref = gne64.resid64(a, x, axis, g, u, e)
    W = gne64.weight64(a.shape, axis, g, u)
    ev = gne64._at(e.astype(np.float64), a.shape, axis)
    p = np.abs(ev * a)
    tol = 2.0 ** -24 * 1.01 * (W * ev * (2 * p + np.abs(x)) + 3 * np.abs(ref))
    assert out.dtype == np.float32 and bool((np.abs(out - ref) <= tol).all())
    S = a.shape[axis]
    assert sums.shape == (2 * S,) and bound.shape == (2 * S,)
    # sum_s SSE_s = sum g (x - e a)^2 = E at tau = 2 without u; a float32 term is within 8 2^-24 g (|x| + |p|)^2 of its own
    E = gne64.energy64(a, x, axis, g, None, e, tau=2.0)
    Wg = gne64.weight64(a.shape, axis, g, None)
    assert abs(float(sums[:S].sum()) - E) <= 8 * 2.0 ** -24 * float(np.sum(np.where(x != 0, Wg * (np.abs(x) + p) ** 2, 0.0)))


def test_tables_and_decimation():
    e = gain64.gains(16, 'generic').numpy()
    u = slice64.weights(16, 'ramp', seed=3).numpy()
    for uu in (None, u):
        w_mat, w_rhs, t = gne64.tables(uu, e)
        want_mat, want_rhs = gain64.compose32(uu, e)
        assert np.array_equal(w_mat.view(np.uint32), want_mat.view(np.uint32))
        assert np.array_equal(t.view(np.uint32), want_rhs.view(np.uint32)) and np.array_equal(w_rhs, t)
    assert np.array_equal(gne64.tables(None, e)[2].view(np.uint32), e.view(np.uint32))  # (u None: t = e)
    ones = np.ones(16, np.float32)
    assert np.array_equal(gne64.tables(u, ones)[0], u) and np.array_equal(gne64.tables(u, ones)[2], u)
    assert gne64.decimate_gain(np.arange(16), 2, 8).tolist() == list(range(0, 16, 2))
    assert gne64.decimate_gain(np.arange(16), 6, 2).tolist() == [0, 6]
    assert gne64.decimate_gain(np.arange(16), 1, 16).tolist() == list(range(16))


# ---- the switch ---------------------------------------------------------------------------------------------------------
def test_gain_gn_is_off_by_default():
    from unires_amd.struct import settings
    assert settings().gain_gn is False


@pytest.mark.parametrize('user', [False, True])
def test_init_accepts_unified_rigid_with_gain_gn(user):
    from unires_amd.run import _init_slice_gains
    xn, y, sett = _cpu_structs()
    sett.gain_gn = sett.unified_rigid = True
    if user:
        xn.slice_gain = torch.full((5,), 1.25)
    else:
        sett.slice_gain = True
    _init_slice_gains([[xn]], sett, torch.device('cpu'))
    assert xn.slice_gain.dtype == torch.float32 and xn.slice_gain.tolist() == [1.25 if user else 1.0] * 5


@pytest.mark.parametrize('user', [False, True])
def test_fit_runs_validation_with_gain_gn(user):
    """max_iter = 0: validation, no iteration, nothing on a device."""
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.gain_gn = sett.unified_rigid = True
    sett.clean_fov = False
    xn.po.rigid = torch.eye(4, dtype=torch.float64)
    if user:
        xn.slice_gain = torch.ones(5)
    else:
        sett.slice_gain = True
    info = U.fit([[xn]], [y], sett)[3]
    assert info['n_iter'] == 0 and info['slice_gain'][0][0].tolist() == [1.0] * 5


@pytest.mark.parametrize('user', [False, True])
def test_scaling_stays_refused_with_gain_gn(user):
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.gain_gn = sett.scaling = True
    if user:
        xn.slice_gain = torch.ones(5)
    else:
        sett.slice_gain = True
    with pytest.raises(ValueError, match='sett.scaling'):
        U.fit([[xn]], [y], sett)


@pytest.mark.parametrize('user', [False, True])
def test_fit_still_refuses_unified_rigid_without_gain_gn(user):
    """tests/test_gain.py's pinned refusal, restated: the same exception type, the setting still named - and the way
    out named with it."""
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    assert sett.gain_gn is False
    sett.unified_rigid = True
    if user:
        xn.slice_gain = torch.ones(5)
    else:
        sett.slice_gain = True
    with pytest.raises(NotImplementedError, match='sett.unified_rigid') as err:
        U.fit([[xn]], [y], sett)
    assert 'sett.gain_gn' in str(err.value)


def test_update_ignores_the_gains_without_gain_gn():
    from unires_amd._update import _gn_gain
    from unires_amd.struct import settings
    xn, _, sett = _cpu_structs()
    xn.slice_gain = torch.ones(5)
    assert _gn_gain(xn, sett) is None and _gn_gain(xn, settings()) is None
    sett.gain_gn = True
    with pytest.raises(ValueError, match='device tensor'):  # (on: the gains must be what fit() leaves)
        _gn_gain(xn, sett)
    xn.slice_gain = None
    assert _gn_gain(xn, sett) is None


# ---- the symbol, argument checks ------------------------------------------------------------------------------------------
def test_symbol_declared_bound_and_exported(lib):
    from unires_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    assert re.search(r'\bint\s+unires_rigid_terms_e\s*\(', hdr)
    assert 'unires_rigid_terms_e' in _lib.SIGNATURES
    assert getattr(lib, 'unires_rigid_terms_e') is not None
    assert lib.unires_abi_version() == 1
    assert re.search(r'#define\s+UNIRES_HIP_ABI_VERSION\s+1\b', hdr)


def test_argument_errors_before_device_work(lib):
    """unires_slice_sums' codes for the same mistakes; g, u and out may be NULL."""
    from unires_amd import _lib
    buf, other = np.zeros(64, dtype=np.float32), np.zeros(64, dtype=np.float32)
    out = np.zeros(8, dtype=np.float64)
    p, q, o = buf.ctypes.data, other.ctypes.data, out.ctypes.data
    ok = _lib.i3((4, 4, 4))
    f = lib.unires_rigid_terms_e
    assert f(None, p, None, None, p, ok, 2, o, None, None) == lib.unires_slice_sums(None, p, ok, 2, o, None) == 1
    assert f(p, None, None, None, p, ok, 2, o, None, None) == lib.unires_slice_sums(p, None, ok, 2, o, None) == 1
    assert f(p, p, None, None, None, ok, 2, o, None, None) == 1
    assert f(p, p, None, None, p, ok, 2, None, None, None) == lib.unires_slice_sums(p, p, ok, 2, None, None) == 1
    for bad in (-1, 3):
        assert f(p, p, None, None, p, ok, bad, o, None, None) == lib.unires_slice_sums(p, p, ok, bad, o, None) == 3
    for dims in ((0, 4, 4), (4, -1, 4)):
        d = _lib.i3(dims)
        assert f(p, p, None, None, p, d, 2, o, None, None) == lib.unires_slice_sums(p, p, d, 2, o, None) == 2
    # the inputs are only read: out may be ay, not x or g
    assert f(p, q, None, None, q, ok, 1, o, p, None) == 3
    assert b'out must not be' in lib.unires_last_error()
    assert f(q, q, p, None, q, ok, 1, o, p, None) == 3
