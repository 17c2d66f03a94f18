"""Per-voxel weights without a device: the algebra of the weighted y-update system on dense float64 matrices built from
tests/ref64.py's Operator64, the Huber rule's restatement, and the host side: the settings' defaults, fit()'s validation
of a user's weight map, the combinations fit() and init() refuse by name, and the new names in the header and the
ctypes table.

The system is  sum_n tau_n A_n^T diag(g_n) A_n + rho lam^2 D^T D  with g_n >= 0 one weight per x-space voxel.  The
reference has no counterpart.  Every test of this file fails on the commit before the feature (no ``tests.voxel64``, no
``_input.weight``, no ``sett.voxel_robust``, no ``unires_voxel_*``).
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import diff64, ref64, slice64, voxel64
from tests.helpers import make_problem, oracle_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM_Y = (5, 4, 3)


@pytest.fixture(scope='module')
def tiny():
    """One thick-slice repeat at 5 x 4 x 3 (thick 2 along z, a general rigid): the dense matrices of A and A^T."""
    prob = make_problem(seed=3, dim_y=DIM_Y, thick=2, thick_axes=[2], rot=0.1, trans=0.4, scl=0.1)
    xs, ys = oracle_structs(prob)
    po = xs[0][0].po
    op = ref64.Operator64(po, 'super-resolution')
    ny, nx = int(np.prod(DIM_Y)), int(np.prod(op.dim_x))
    eye = lambda n, i: torch.nn.functional.one_hot(torch.tensor(i), n).double()
    A = torch.stack([op.A(eye(ny, j).reshape(DIM_Y)).reshape(-1) for j in range(ny)], 1).numpy()
    At = torch.stack([op.At(eye(nx, i).reshape(op.dim_x)).reshape(-1) for i in range(nx)], 1).numpy()
    assert np.abs(At - A.T).max() <= 1e-12 * np.abs(A).max()
    return dict(op=op, A=A, At=At, axis=int(po.dim_thick), tau=float(xs[0][0].tau), lam=float(ys[0].lam))


def _weighted(t, g):
    """The dense matrix of At diag(g) A, g an x-space volume."""
    return t['At'] @ (np.asarray(g, np.float64).reshape(-1)[:, None] * t['A'])


@pytest.mark.parametrize('pattern', ['pow2', 'ramp'])
def test_weighted_normal_matrix_is_symmetric_psd(tiny, pattern):
    H = _weighted(tiny, voxel64.weights(tiny['op'].dim_x, pattern).numpy())
    scale = np.abs(tiny['At'] @ tiny['A']).max()
    assert np.abs(H - H.T).max() <= 1e-12 * scale
    assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-12 * scale


def test_unit_weights_give_ata_and_zero_weights_give_zero(tiny):
    full = tiny['At'] @ tiny['A']
    assert np.array_equal(_weighted(tiny, voxel64.weights(tiny['op'].dim_x, 'ones').numpy()), full)
    assert not _weighted(tiny, voxel64.weights(tiny['op'].dim_x, 'zeros').numpy()).any()
    # ... and one voxel's weight scales that voxel's row alone
    g = voxel64.weights(tiny['op'].dim_x, 'ones').numpy()
    g.reshape(-1)[3] = 0.25
    want = full - 0.75 * np.outer(tiny['At'][:, 3], tiny['A'][3])
    assert np.abs(_weighted(tiny, g) - want).max() <= 1e-13 * np.abs(full).max()


def test_system_is_positive_definite_whatever_the_weights(tiny):
    """g >= 0 keeps the data term PSD, and the zero-bound D^T D is positive definite: even with all weights 0."""
    reg = 0.7 * tiny['lam'] ** 2 * diff64.dense_dtd(DIM_Y, [1.0, 1.0, 1.0], 'forward')
    for pattern in ('zeros', 'pow2', 'ramp', 'ones'):
        H = tiny['tau'] * _weighted(tiny, voxel64.weights(tiny['op'].dim_x, pattern).numpy()) + reg
        assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() > 0, pattern


@pytest.mark.parametrize('pattern', ['pow2', 'ramp'])
def test_weights_constant_per_slice_reproduce_the_slice_operator(tiny, pattern):
    dim_x, a = tiny['op'].dim_x, tiny['axis']
    w = slice64.weights(dim_x[a], pattern)
    g = slice64.spread(w, dim_x, a).numpy()  # (the float32 weights, spread as float64: exact)
    u = g.reshape(-1)
    assert np.array_equal(_weighted(tiny, g), tiny['At'] @ (u[:, None] * tiny['A']))
    # ... and through slice64's operator form: A^T (W . A p) with W = g
    p = torch.rand(DIM_Y, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    via_op = tiny['op'].At(torch.from_numpy(g) * tiny['op'].A(p)).numpy().reshape(-1)
    dense = _weighted(tiny, g) @ p.numpy().reshape(-1)
    assert np.abs(via_op - dense).max() <= 1e-12 * np.abs(dense).max()


# ---- the Huber rule ----------------------------------------------------------------------------------------------------
C_TEST = np.float32(1.75)  # (no test depends on the default of sett.voxel_k)


def _huber_inputs():
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(6, 5, 7, generator=gen) * 3.0).float().numpy()
    ay = (torch.randn(6, 5, 7, generator=gen) * 3.0).float().numpy()
    x[0, 0, :3] = 0.0                      # missing voxels, whatever their residual
    ay[0, 0, 0] = 1000.0
    x[1, 1, 1], ay[1, 1, 1] = 4.0, 4.0 - float(C_TEST)   # |r| == c exactly (both representable)
    x[2, 2, 2], ay[2, 2, 2] = 5.0, 5.0 + 64.0 * float(C_TEST)  # far beyond
    return x, ay


def test_huber_weights_are_one_inside_and_c_over_r_beyond():
    x, ay = _huber_inputs()
    h = voxel64.huber64(x, ay, None, C_TEST)
    r = np.abs((x - ay).astype(np.float32))
    assert h.dtype == np.float32 and (h <= 1.0).all() and (h > 0.0).all()
    assert (h[x == 0] == 1.0).all() and h[0, 0, 0] == 1.0
    inside = (r <= C_TEST) | (x == 0)
    assert (h[inside] == 1.0).all() and h[1, 1, 1] == 1.0 and r[1, 1, 1] == C_TEST
    beyond = ~inside
    assert beyond.any() and (h[beyond] < 1.0).all()
    # h |r| = c to two float32 roundings (the quotient's and the product's)
    hr = h[beyond].astype(np.float64) * r[beyond].astype(np.float64)
    assert np.abs(hr - float(C_TEST)).max() <= 2.0 ** -23 * float(C_TEST)
    assert h[2, 2, 2] == np.float32(1.0 / 64.0)


def test_huber_prior_multiplies_and_a_zero_prior_stays_zero():
    x, ay = _huber_inputs()
    prior = voxel64.weights(x.shape, 'pow2').numpy()
    h = voxel64.huber64(x, ay, None, C_TEST)
    g = voxel64.huber64(x, ay, prior, C_TEST)
    assert np.array_equal(g, (prior * h).astype(np.float32))
    assert (g[prior == 0] == 0).all() and (prior == 0).any()
    assert np.array_equal(voxel64.huber64(x, ay, np.ones_like(x), C_TEST), h)


def test_voxel_sums64_with_unit_weights_are_the_slice_sums():
    x, ay = _huber_inputs()
    for axis in range(3):
        sse, gs, cnt, b_sse, b_g = voxel64.voxel_sums64(x, ay, np.ones_like(x), axis)
        sse_s, cnt_s, bound_s = slice64.slice_sums64(x, ay, axis)
        assert np.array_equal(sse, sse_s) and np.array_equal(gs, cnt_s) and np.array_equal(cnt, cnt_s)
        assert np.array_equal(b_sse, bound_s)


def test_apply32_is_exact_for_pow2_weights_and_composes_with_slice_weights():
    x, _ = _huber_inputs()
    g = voxel64.weights(x.shape, 'pow2').numpy()
    u = slice64.weights(x.shape[1], 'pow2').numpy()
    W = g.astype(np.float64) * u.astype(np.float64).reshape(1, -1, 1)
    assert np.array_equal(voxel64.apply32(x, g, u, 1).astype(np.float64), W * x.astype(np.float64))
    assert np.array_equal(voxel64.apply32(x, g), (g * x).astype(np.float32))
    m = (np.arange(x.size).reshape(x.shape) % 3 != 0).astype(np.uint8)
    out = voxel64.apply32(x, g, u, 1, mask=m)
    assert (out[m == 0] == 0).all() and not np.signbit(out[m == 0]).any()


# ---- the host side ----------------------------------------------------------------------------------------------------
def test_settings_and_struct_defaults():
    from unires_amd.struct import _input, settings
    s = settings()
    assert s.voxel_robust is False and s.weight is None
    assert isinstance(s.voxel_k, float) and s.voxel_k > 0
    assert _input().weight is None


def _cpu_structs():
    from unires_amd.struct import _input, _output, _proj_op, settings
    xn = _input(dat=torch.ones(4, 5, 6), mat=torch.eye(4, dtype=torch.float64))
    xn.po = _proj_op()
    xn.po.dim_thick = 1
    y = _output(dat=torch.zeros(4, 5, 6), mat=torch.eye(4, dtype=torch.float64), lam=1.0)
    sett = settings()
    sett.max_iter = 0
    return xn, y, sett


def _bad(kind):
    g = torch.ones(4, 5, 6)
    if kind == 'nan':
        g[1, 2, 3] = float('nan')
    elif kind == 'inf':
        g[1, 2, 3] = float('inf')
    elif kind == 'neg':
        g[1, 2, 3] = -0.5
    return g


@pytest.mark.parametrize('bad, word', [(torch.ones(4, 5), 'shape'), (torch.ones(6, 5, 4), 'shape'), (torch.ones(5), 'shape'),
                                       (_bad('nan'), 'finite'), (_bad('inf'), 'finite'), (_bad('neg'), '>= 0'),
                                       (torch.ones(4, 5, 6, dtype=torch.complex64), 'real'),
                                       (torch.ones(4, 5, 6, dtype=torch.bool), 'real')])
def test_fit_refuses_bad_user_weights(bad, word):
    """One real weight per voxel of the observation, finite, >= 0: checked before anything runs."""
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    xn.weight = bad
    with pytest.raises(ValueError, match=word):
        U.fit([[xn]], [y], sett)


@pytest.mark.parametrize('name', ['scaling', 'unified_rigid'])
@pytest.mark.parametrize('how', ['user', 'robust'])
def test_fit_refuses_the_gauss_newton_updates_with_voxel_weights_by_name(name, how):
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    setattr(sett, name, True)
    if how == 'user':
        xn.weight = torch.ones(4, 5, 6)
    else:
        sett.voxel_robust = True
    with pytest.raises(NotImplementedError, match='sett.' + name):
        U.fit([[xn]], [y], sett)


def test_fit_refuses_a_voxel_k_that_is_not_positive():
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.voxel_robust, sett.voxel_k = True, 0.0
    with pytest.raises(ValueError, match='voxel_k'):
        U.fit([[xn]], [y], sett)


def test_fit_validation_accepts_good_weights_and_starts_robust_fits_from_the_prior():
    from unires_amd.run import _init_voxel_weights
    cpu = torch.device('cpu')
    xn, y, sett = _cpu_structs()
    user = voxel64.weights((4, 5, 6), 'pow2').double().numpy()  # (anything torch.as_tensor takes)
    xn.weight = user
    _init_voxel_weights([[xn]], sett, cpu)
    assert xn.weight.dtype == torch.float32 and xn.weight.is_contiguous() and np.array_equal(xn.weight.numpy(), user)
    assert xn._weight_prior is None  # off: no rule, no prior kept
    xn.weight = None
    _init_voxel_weights([[xn]], sett, cpu)
    assert xn.weight is None  # off: nothing is made up
    sett.voxel_robust = True
    _init_voxel_weights([[xn]], sett, cpu)
    assert xn.weight.dtype == torch.float32 and bool((xn.weight == 1).all()) and xn._weight_prior is None
    mine = torch.from_numpy(user).float()
    xn.weight = mine
    _init_voxel_weights([[xn]], sett, cpu)
    # the prior is a private clone, the working weights another: the rule writes neither into the user's tensor
    assert torch.equal(xn._weight_prior, mine) and torch.equal(xn.weight, mine)
    assert xn._weight_prior.data_ptr() != mine.data_ptr() and xn.weight.data_ptr() != mine.data_ptr()
    assert xn.weight.data_ptr() != xn._weight_prior.data_ptr()


def _x_for_init():
    from unires_amd.struct import _input
    return [[_input(dat=torch.ones(4, 5, 6)), _input(dat=torch.ones(4, 5, 3))], [_input(dat=torch.ones(2, 5, 6))]]


def test_init_weights_are_read_from_files_and_tensors(tmp_path):
    from unires_amd import nifti
    from unires_amd._core import _read_weights
    from unires_amd.struct import settings
    sett = settings()
    g = voxel64.weights((4, 5, 3), 'ramp')
    on_disk = g.clone()
    on_disk[1, 1, 1], on_disk[2, 2, 2], on_disk[3, 3, 1] = float('nan'), float('inf'), float('-inf')
    path = str(tmp_path / 'w.nii')
    nifti.write(path, on_disk.numpy(), np.eye(4))
    sett.weight = [[None, path], voxel64.weights((2, 5, 6), 'pow2')]  # (a channel of one repeat: no inner list needed)
    x = _read_weights(_x_for_init(), sett)
    assert x[0][0].weight is None
    want = g.clone()
    want[1, 1, 1] = want[2, 2, 2] = want[3, 3, 1] = 0.0  # non-finite values of a file become 0
    assert x[0][1].weight.dtype == torch.float32 and torch.equal(x[0][1].weight, want)
    assert torch.equal(x[1][0].weight, voxel64.weights((2, 5, 6), 'pow2'))
    sett.weight = None
    assert all(xn.weight is None for xc in _read_weights(_x_for_init(), sett) for xn in xc)


@pytest.mark.parametrize('weight, word', [([[torch.ones(4, 5, 6), torch.ones(4, 5, 6)], None], 'shape'),
                                          ([[None, None]], 'per channel'), ([[None], None], 'per repeat'),
                                          (torch.ones(4, 5, 6), 'per channel')])
def test_init_refuses_weights_that_do_not_fit_the_data(weight, word):
    from unires_amd._core import _read_weights
    from unires_amd.struct import settings
    sett = settings()
    sett.weight = weight
    with pytest.raises(ValueError, match=word):
        _read_weights(_x_for_init(), sett)


def test_init_refuses_weights_with_force_inplane_res_by_name():
    from unires_amd._core import _read_weights
    from unires_amd.struct import settings
    sett = settings()
    sett.weight, sett.force_inplane_res = [[None, None], None], True
    with pytest.raises(NotImplementedError, match='force_inplane_res'):
        _read_weights(_x_for_init(), sett)


NEW_SYMBOLS = ('unires_plan_set_voxel_weights', 'unires_voxel_sums', 'unires_voxel_huber', 'unires_voxel_apply')


def test_new_entry_points_are_in_the_header_and_the_ctypes_table():
    from unires_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r'#define\s+UNIRES_HIP_ABI_VERSION\s+1\b', header)
    import unires_amd as U
    from unires_amd._plan import ChannelPlan
    assert callable(U._update_voxel_weights)
    assert callable(ChannelPlan.set_voxel_weights) and callable(ChannelPlan.sync_voxel_weights)
