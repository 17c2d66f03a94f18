"""The slice weights in the scaling and rigid Gauss-Newton updates, without a GPU: tests/gn64.py's
restatement against tests/admm64.py's unweighted one, the new symbols, and the argument checks of the two entry points
(they come before anything touches the device; the pointers are never followed)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import admm64, gn64, slice64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7, 6), (4, 1, 9)]
NEW_SYMBOLS = ('unires_scaling_sums_w', 'unires_rigid_resid')


def data(shape, seed=3):
    """x with exact zeros and -0.0, ay with planted exact zeros."""
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = (torch.rand(shape, generator=g) * 10).float()
    x[x < 1.5] = 0.0
    x.view(-1)[5::13] = -0.0
    ay = (torch.rand(shape, generator=g) * 10 - 1).float()
    ay.view(-1)[2::7] = 0.0
    return x.numpy(), ay.numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def zeroed(x, axis, u):
    """x with the slices of weight 0 set to 0."""
    out = np.array(x, copy=True)
    sl = [slice(None)] * 3
    sl[axis] = np.flatnonzero(np.asarray(u) == 0)
    out[tuple(sl)] = 0.0
    return out


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_unit_weights_give_the_unweighted_references(shape, axis):
    x, ay = data(shape)
    ref, tol = gn64.scaling_sums_w(x, ay, axis, np.ones(shape[axis], np.float32))
    ref0, tol0 = admm64.scaling_sums(x, ay, axis)
    assert ref == ref0 and tol == tol0


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_zero_one_weights_are_the_data_without_those_slices(shape, axis):
    x, ay = data(shape)
    u = np.ones(shape[axis], np.float32)
    u[::2] = 0.0
    ref, _ = gn64.scaling_sums_w(x, ay, axis, u)
    ref0, _ = admm64.scaling_sums(zeroed(x, axis, u), ay, axis)
    assert ref == ref0
    assert any(r != 0 for r in ref) or shape[axis] == 1


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_the_sums_are_linear_in_the_weights(shape, axis):
    """sum_s u_s ref(e_s) = ref(u).  Each ref is an exact sum rounded once (2^-53 relative), each product u_s ref(e_s)
    rounds once more, math.fsum and ref(u) once each: 2^-52 (sum_s |u_s ref(e_s)| + |ref(u)|) covers them."""
    x, ay = data(shape)
    S = shape[axis]
    u = slice64.weights(S, 'ramp').numpy()
    ref, _ = gn64.scaling_sums_w(x, ay, axis, u)
    one_hot = [gn64.scaling_sums_w(x, ay, axis, np.eye(S, dtype=np.float32)[s])[0] for s in range(S)]
    for k in range(5):
        parts = [float(u[s]) * one_hot[s][k] for s in range(S)]
        tol = 2.0 ** -52 * (math.fsum(abs(p) for p in parts) + abs(ref[k]))
        assert abs(math.fsum(parts) - ref[k]) <= tol, (k, math.fsum(parts), ref[k], tol)


@pytest.mark.parametrize('shape', SHAPES)
def test_unweighted_residual_is_the_masked_difference(shape):
    """u = None: (ay - x) with 0 where x == 0 or ay == 0, as _rigid.py's tensor form masks it."""
    x, ay = data(shape)
    xt, at = torch.from_numpy(x), torch.from_numpy(ay)
    d = at - xt
    d[(xt == 0) | (at == 0)] = 0
    for axis in (0, 1, 2):
        got = gn64.rigid_resid32(x, ay, axis, None)
        assert np.array_equal(bits(got), bits(d.numpy()))
        assert np.array_equal(bits(gn64.rigid_resid32(x, ay, axis, np.ones(shape[axis], np.float32))), bits(got))
    assert (got[(x == 0) | (ay == 0)].view(np.uint32) == 0).all()  # +0, never -0


def test_weighted_sse_at_unit_weights_is_the_masked_sum():
    x, ay = data((5, 7, 6))
    for axis in (0, 1, 2):
        ref, tol = gn64.weighted_sse(x, ay, axis, np.ones(x.shape[axis], np.float32))
        ref0, _ = admm64.masked_sse(x, ay)
        assert abs(ref - ref0) <= 2.0 ** -52 * ref0 and 0 < tol < 1e-12 * ref0


def test_symbols_declared_and_bound(lib):
    from unires_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    declared = set(re.findall(r'\b(unires_[a-z0-9_]+)\s*\(', hdr))
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in _lib.SIGNATURES, sym
        assert getattr(lib, sym) is not None
    assert lib.unires_abi_version() == 1
    assert re.search(r'#define\s+UNIRES_HIP_ABI_VERSION\s+1\b', hdr)


def test_argument_errors_before_device_work(lib):
    from unires_amd import _lib
    buf = np.zeros(64, dtype=np.float32)
    out = np.zeros(8, dtype=np.float64)
    p, o = buf.ctypes.data, out.ctypes.data
    ok = _lib.i3((4, 4, 4))
    # unires_scaling_sums_w: NULL u (and every other pointer), dim_thick, dims
    assert lib.unires_scaling_sums_w(p, p, ok, 2, None, o, None) == 1
    assert lib.unires_scaling_sums_w(None, p, ok, 2, p, o, None) == 1
    assert lib.unires_scaling_sums_w(p, p, ok, 2, p, None, None) == 1
    for bad in (-1, 3):
        assert lib.unires_scaling_sums_w(p, p, ok, bad, p, o, None) == 3
        assert b'dim_thick' in lib.unires_last_error()
    for dims in ((0, 4, 4), (4, -1, 4)):
        assert lib.unires_scaling_sums_w(p, p, _lib.i3(dims), 2, p, o, None) == 2
    # unires_rigid_resid: u may be NULL, nothing else; axis; dims
    assert lib.unires_rigid_resid(None, p, ok, 0, None, p, None) == 1
    assert lib.unires_rigid_resid(p, None, ok, 0, None, p, None) == 1
    assert lib.unires_rigid_resid(p, p, ok, 0, None, None, None) == 1
    for bad in (-1, 3):
        assert lib.unires_rigid_resid(p, p, ok, bad, None, p, None) == 3
        assert b'axis' in lib.unires_last_error()
    for dims in ((4, 0, 4), (4, 4, -2)):
        assert lib.unires_rigid_resid(p, p, _lib.i3(dims), 1, p, p, None) == 2
