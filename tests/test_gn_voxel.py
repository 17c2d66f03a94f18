"""The voxel weights in the scaling and rigid Gauss-Newton updates, without a GPU: the switch
``sett.voxel_gn`` and what fit() refuses without it, the new symbols and their argument checks (they come before
anything touches the device; the pointers are never followed), and tests/gnv64.py's restatement against tests/gn64.py's
slice-weighted one and against voxel-by-voxel loops in rational arithmetic on tiny shapes."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import gn64, gnv64, slice64, voxel64
from tests.test_gn_weights import bits, data
from tests.test_voxel import _cpu_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7, 6), (4, 1, 9)]
NEW_SYMBOLS = ('unires_scaling_sums_g', 'unires_rigid_resid_g')


# ---- the switch ---------------------------------------------------------------------------------------------------------
def test_voxel_gn_is_off_by_default():
    from unires_amd.struct import settings
    assert settings().voxel_gn is False


@pytest.mark.parametrize('name', ['scaling', 'unified_rigid'])
@pytest.mark.parametrize('how', ['user', 'robust'])
def test_fit_still_refuses_without_voxel_gn(name, how):
    """tests/test_voxel.py's pinned refusal, restated: the same exception type, the setting still named - and the way
    out named with it."""
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    assert sett.voxel_gn is False
    setattr(sett, name, True)
    if how == 'user':
        xn.weight = torch.ones(4, 5, 6)
    else:
        sett.voxel_robust = True
    with pytest.raises(NotImplementedError, match='sett.' + name) as err:
        U.fit([[xn]], [y], sett)
    assert 'sett.voxel_gn' in str(err.value)


@pytest.mark.parametrize('name', ['scaling', 'unified_rigid'])
@pytest.mark.parametrize('how', ['user', 'robust'])
def test_fit_does_not_refuse_with_voxel_gn(name, how):
    """max_iter = 0: validation, no iteration, nothing on a device."""
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.voxel_gn, sett.clean_fov = True, False
    xn.po.rigid = torch.eye(4, dtype=torch.float64)  # (fit() returns the rigid matrices)
    setattr(sett, name, True)
    if how == 'user':
        xn.weight = torch.ones(4, 5, 6)
    else:
        sett.voxel_robust = True
    info = U.fit([[xn]], [y], sett)[3]
    assert info['n_iter'] == 0 and torch.equal(info['voxel_w'][0][0], torch.ones(4, 5, 6))


def test_update_functions_ignore_the_map_without_voxel_gn():
    from unires_amd._update import _gn_weight
    from unires_amd.struct import settings
    xn, _, sett = _cpu_structs()
    xn.weight = torch.ones(4, 5, 6)
    assert _gn_weight(xn, sett) is None and _gn_weight(xn, settings()) is None
    sett.voxel_gn = True
    with pytest.raises(ValueError, match='device tensor'):  # (on: the map must be what fit() leaves)
        _gn_weight(xn, sett)
    xn.weight = None
    assert _gn_weight(xn, sett) is None


# ---- symbols, argument checks ---------------------------------------------------------------------------------------------
def test_symbols_declared_and_bound(lib):
    from unires_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % sym, hdr), sym
        assert sym in _lib.SIGNATURES, sym
        assert getattr(lib, sym) is not None
    assert lib.unires_abi_version() == 1
    assert re.search(r'#define\s+UNIRES_HIP_ABI_VERSION\s+1\b', hdr)


def test_argument_errors_before_device_work(lib):
    from unires_amd import _lib
    buf, other = np.zeros(64, dtype=np.float32), np.zeros(64, dtype=np.float32)
    out = np.zeros(8, dtype=np.float64)
    p, q, o = buf.ctypes.data, other.ctypes.data, out.ctypes.data
    ok = _lib.i3((4, 4, 4))
    # unires_scaling_sums_g: u may be NULL, g and the rest may not; dim_thick; dims
    assert lib.unires_scaling_sums_g(p, p, ok, 2, None, p, o, None) == 1
    assert lib.unires_scaling_sums_g(None, p, ok, 2, p, None, o, None) == 1
    assert lib.unires_scaling_sums_g(p, None, ok, 2, p, None, o, None) == 1
    assert lib.unires_scaling_sums_g(p, p, ok, 2, p, None, None, None) == 1
    for bad in (-1, 3):
        assert lib.unires_scaling_sums_g(p, p, ok, bad, p, None, o, None) == 3
        assert b'dim_thick' in lib.unires_last_error()
    for dims in ((0, 4, 4), (4, -1, 4)):
        assert lib.unires_scaling_sums_g(p, p, _lib.i3(dims), 2, p, p, o, None) == 2
    # unires_rigid_resid_g: u may be NULL, nothing else; axis; dims; out must not be g
    assert lib.unires_rigid_resid_g(None, p, p, ok, 0, None, q, None) == 1
    assert lib.unires_rigid_resid_g(p, None, p, ok, 0, None, q, None) == 1
    assert lib.unires_rigid_resid_g(p, p, None, ok, 0, None, q, None) == 1
    assert lib.unires_rigid_resid_g(p, p, p, ok, 0, None, None, None) == 1
    for bad in (-1, 3):
        assert lib.unires_rigid_resid_g(p, p, p, ok, bad, None, q, None) == 3
        assert b'axis' in lib.unires_last_error()
    for dims in ((4, 0, 4), (4, 4, -2)):
        assert lib.unires_rigid_resid_g(p, p, p, _lib.i3(dims), 1, p, q, None) == 2
    assert lib.unires_rigid_resid_g(p, q, q, ok, 1, None, q, None) == 3
    assert b'out must not be g' in lib.unires_last_error()


# ---- gnv64 against gn64 and against loops -----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_unit_map_gives_the_slice_weighted_references_exactly(shape, axis):
    x, ay = data(shape)
    ones = np.ones(shape, np.float32)
    u = slice64.weights(shape[axis], 'ramp').numpy()
    ref, tol = gnv64.scaling_sums_g(x, ay, axis, ones, u)
    ref_w, tol_w = gn64.scaling_sums_w(x, ay, axis, u)
    assert ref == ref_w
    assert all(t >= tw for t, tw in zip(tol, tol_w))  # (one rounding per summand more, never less)
    ref1, tol1 = gnv64.scaling_sums_g(x, ay, axis, ones, None)
    ref1_w, tol1_w = gn64.scaling_sums_w(x, ay, axis, np.ones(shape[axis], np.float32))
    assert ref1 == ref1_w and tol1 == tol1_w
    for uu in (None, u):
        assert np.array_equal(bits(gnv64.rigid_resid_g32(x, ay, axis, ones, uu)), bits(gn64.rigid_resid32(x, ay, axis, uu)))


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_map_constant_on_every_slice_is_the_slice_weighted_sum(axis):
    shape = (5, 7, 6)
    x, ay = data(shape)
    u = slice64.weights(shape[axis], 'ramp').numpy()
    g = slice64.spread(torch.from_numpy(u), shape, axis).numpy().astype(np.float32)
    assert gnv64.scaling_sums_g(x, ay, axis, g, None) == gn64.scaling_sums_w(x, ay, axis, u)


@pytest.mark.parametrize('pattern', ['pow2', 'ramp'])
@pytest.mark.parametrize('with_u', [False, True])
def test_scaling_sums_g_against_a_loop_in_rational_arithmetic(pattern, with_u):
    """Voxel by voxel: the float32 terms as numpy forms them, times g u as rationals, summed as rationals; the
    restatement's exact sums are those, rounded once."""
    shape, axis = (5, 7, 6), 1
    x, ay = data(shape)
    g = voxel64.weights(shape, pattern).numpy()
    u = slice64.weights(shape[axis], 'ramp', seed=3).numpy() if with_u else None
    want = [Fraction(0)] * 5
    for idx in np.ndindex(*shape):
        xv, yv = x[idx], ay[idx]
        if xv == 0:
            continue
        r = np.float32(xv - yv)
        w = Fraction(float(g[idx])) * (Fraction(float(u[idx[axis]])) if with_u else 1)
        even = idx[axis] & 1
        want[0] += w * Fraction(float(np.float32(r * r)))
        want[1 if even else 2] += w * Fraction(float(np.float32(yv * r)))
        want[3 if even else 4] += w * Fraction(float(np.float32(yv * yv)))
    ref, tol = gnv64.scaling_sums_g(x, ay, axis, g, u)
    assert ref == [float(v) for v in want]
    assert all(t > 0 for t in tol) and any(v != 0 for v in ref)


@pytest.mark.parametrize('with_u', [False, True])
def test_rigid_resid_g32_against_a_loop(with_u):
    shape, axis = (4, 1, 9), 2
    x, ay = data(shape)
    g = voxel64.weights(shape, 'ramp').numpy()
    u = slice64.weights(shape[axis], 'ramp', seed=3).numpy() if with_u else None
    got = gnv64.rigid_resid_g32(x, ay, axis, g, u)
    for idx in np.ndindex(*shape):
        if x[idx] == 0 or ay[idx] == 0:
            assert got[idx].view(np.uint32) == 0, idx  # +0, never -0
            continue
        r = np.float32(ay[idx] - x[idx])
        if with_u:
            want = np.float32((np.float64(g[idx]) * np.float64(u[idx[axis]])) * np.float64(r))
        else:
            want = np.float32(g[idx] * r)
        assert got[idx].view(np.uint32) == want.view(np.uint32), idx
    assert ((x == 0) | (ay == 0)).any() and (got != 0).any()


def test_zero_one_map_is_the_data_without_those_voxels():
    shape, axis = (5, 7, 6), 0
    x, ay = data(shape)
    g = gnv64.box_weights(shape, ((1, 4), (2, 3), (0, 5)))
    xz = np.where(g == 0, np.float32(0.0), x)
    assert (g == 0).sum() == 15 and (x[g == 0] != 0).any()
    assert gnv64.scaling_sums_g(x, ay, axis, g, None)[0] == gnv64.scaling_sums_g(xz, ay, axis, np.ones_like(g), None)[0]


def test_decimation_rule():
    """sk = (2, 1, 3): voxels 0, 2, 4, ... / all / 0, 3, 6, ... from the first, then cut to dim_x - entry by entry."""
    w = np.arange(7 * 5 * 8, dtype=np.float32).reshape(7, 5, 8)
    sk, dim_x = (2, 1, 3), (3, 5, 3)
    got = gnv64.decimate(w, sk, dim_x)
    assert got.shape == dim_x and got.flags['C_CONTIGUOUS']
    for i in range(dim_x[0]):
        for j in range(dim_x[1]):
            for k in range(dim_x[2]):
                assert got[i, j, k] == w[2 * i, j, 3 * k]
    assert np.array_equal(gnv64.decimate(w, (1, 1, 1), w.shape), w)
    # the slicing the update applies to the device tensor is the same rule
    t = torch.from_numpy(w)
    assert np.array_equal(t[::sk[0], ::sk[1], ::sk[2]][:dim_x[0], :dim_x[1], :dim_x[2]].contiguous().numpy(), got)
