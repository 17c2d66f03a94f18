"""sett.mask_zeros without a device: the algebra of the masked y-update system on dense float64 matrices built
from tests/ref64.py's Operator64, and the host side of the setting (its default, the C symbol, the regime a masked
channel's plan is built in).

With m_n(v) = [x_n(v) != 0] the system is  sum_n tau_n A_n^T diag(m_n) A_n + rho lam^2 D^T D.  The reference has no
counterpart (its AtA has no mask): what these tests pin is the project's own statement of it.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import diff64, ref64
from tests.helpers import make_problem, oracle_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM_Y = (7, 6, 9)


@pytest.fixture(scope='module')
def tiny():
    """One thick-slice repeat at 7 x 6 x 9 (thick 3 along z, a general rigid): its Operator64 and the dense matrix of
    A (rows: x space, C order; columns: y space)."""
    prob = make_problem(seed=3, dim_y=DIM_Y, thick=3, thick_axes=[2], rot=0.1, trans=0.7, scl=0.1)
    xs, ys = oracle_structs(prob)
    op = ref64.Operator64(xs[0][0].po, 'super-resolution')
    ny = int(np.prod(DIM_Y))
    cols = []
    for j in range(ny):
        e = torch.zeros(ny, dtype=torch.float64)
        e[j] = 1.0
        cols.append(op.A(e.reshape(DIM_Y)).reshape(-1))
    A = torch.stack(cols, 1).numpy()
    # the adjoint is the transpose of that matrix: At applied to the x-space basis
    nx = A.shape[0]
    rows = []
    for i in range(nx):
        e = torch.zeros(nx, dtype=torch.float64)
        e[i] = 1.0
        rows.append(op.At(e.reshape(op.dim_x)).reshape(-1))
    At = torch.stack(rows, 1).numpy()
    assert np.abs(At - A.T).max() <= 1e-12 * np.abs(A).max()
    return dict(prob=prob, op=op, A=A, At=At, vx=[1.0, 1.0, 1.0], tau=float(xs[0][0].tau), lam=float(ys[0].lam))


def _masked(t, m):
    """The dense matrix of At diag(m) A, composed from the operator's own A and At."""
    return t['At'] @ (m[:, None] * t['A'])


def _masks(nx, dim_x):
    gen = np.random.default_rng(5)
    slab = np.ones(dim_x)
    slab[:, :, : max(1, dim_x[2] // 3)] = 0.0
    box = np.ones(dim_x)
    box[: dim_x[0] // 2, : dim_x[1] // 2, : max(1, dim_x[2] // 2)] = 0.0
    rnd = (gen.random(nx) >= 0.3).astype(np.float64)
    return {'slab': slab.reshape(-1), 'box': box.reshape(-1), 'random30': rnd}


@pytest.mark.parametrize('kind', ['slab', 'box', 'random30'])
def test_masked_normal_matrix_is_symmetric_and_positive_semidefinite(tiny, kind):
    nx = tiny['A'].shape[0]
    m = _masks(nx, tiny['op'].dim_x)[kind]
    assert 0 < m.sum() < nx
    H = _masked(tiny, m)
    scale = np.abs(H).max()
    assert np.abs(H - H.T).max() <= 1e-12 * scale
    ev = np.linalg.eigvalsh(0.5 * (H + H.T))
    assert ev.min() >= -1e-10 * ev.max()
    # ... and it only removes non-negative terms: the unmasked matrix dominates it
    full = _masked(tiny, np.ones(nx))
    gap = np.linalg.eigvalsh(0.5 * ((full - H) + (full - H).T))
    assert gap.min() >= -1e-10 * ev.max()


def test_all_ones_is_the_unmasked_matrix_and_all_zeros_is_zero(tiny):
    nx = tiny['A'].shape[0]
    full = tiny['At'] @ tiny['A']
    assert np.array_equal(_masked(tiny, np.ones(nx)), full)
    assert not _masked(tiny, np.zeros(nx)).any()
    # the operator's own A^T A of a vector is that matrix's product
    p = torch.rand(DIM_Y, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    ref = tiny['op'].At(tiny['op'].A(p)).reshape(-1).numpy()
    assert np.abs(full @ p.reshape(-1).numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize('kind', ['slab', 'box', 'random30', 'zeros'])
def test_masked_system_is_positive_definite_with_the_zero_bound_regulariser(tiny, kind):
    """The zero-bound D^T D is positive definite on its own (rows [1, -1] / [-1, 2, -1] / [-1, 2]: no constant in
    its null space), so the system stays solvable whatever the mask removes - an all-zero observation included."""
    nx = tiny['A'].shape[0]
    m = np.zeros(nx) if kind == 'zeros' else _masks(nx, tiny['op'].dim_x)[kind]
    rho = float(tiny['prob']['rho'])
    c = rho * tiny['lam'] ** 2
    S = tiny['tau'] * _masked(tiny, m) + c * diff64.dense_dtd(DIM_Y, tiny['vx'], 'forward')
    ev = np.linalg.eigvalsh(0.5 * (S + S.T))
    assert ev.min() > 0
    assert ev.min() >= 0.999 * np.linalg.eigvalsh(c * diff64.dense_dtd(DIM_Y, tiny['vx'], 'forward')).min()


def test_mask_zeros_is_off_by_default():
    from unires_amd.struct import settings
    assert settings().mask_zeros is False
    from unires_amd._update import _mask_zeros

    class Bare:
        pass
    assert _mask_zeros(Bare()) is False  # a settings object from before the setting
    s = settings()
    s.mask_zeros = True
    assert _mask_zeros(s) is True


def test_set_missing_is_declared_and_bound():
    import ctypes as C
    from unires_amd import _lib
    with open(os.path.join(ROOT, 'include', 'unires_hip.h')) as f:
        hdr = f.read()
    decl = re.search(r'int\s+unires_plan_set_missing\s*\(([^)]*)\)\s*;', hdr)
    assert decl, 'unires_plan_set_missing is not declared in include/unires_hip.h'
    args = [a.strip() for a in decl.group(1).split(',')]
    assert args == ['unires_plan_t *plan', 'int32_t n', 'const float *x', 'void *stream']
    res, argtypes = _lib.SIGNATURES['unires_plan_set_missing']
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert 'UNIRES_ABI_VERSION' not in decl.group(0)
    from unires_amd._plan import ChannelPlan
    assert callable(ChannelPlan.set_missing) and callable(ChannelPlan.sync_missing)


def test_regime_of_a_channel_plan_with_and_without_the_setting():
    """A = I (do_proj false) has no x-space intermediate: under mask_zeros the channel's plan is a denoising-regime
    plan with the identity affine; every other combination is the user's regime.  Host logic only."""
    from unires_amd import _lib
    from unires_amd._plan import proj_matrix, regime_of
    from unires_amd._project import _identity_po, _plan_regime, _plan_repeats, _plan_signature
    for method in ('denoising', 'super-resolution'):
        assert _plan_regime(method, False, False) == (method, False)
        assert regime_of(*_plan_regime(method, False, False)) == _lib.REGIME_IDENTITY
        assert _plan_regime(method, False, True) == ('denoising', True)
        assert regime_of(*_plan_regime(method, False, True)) == _lib.REGIME_DENOISE
        for mz in (False, True):
            assert _plan_regime(method, True, mz) == (method, True)
    assert regime_of(*_plan_regime('super-resolution', True, True)) == _lib.REGIME_SUPERRES
    with pytest.raises(ValueError):
        _plan_regime('nope', False, True)

    class Y:
        dim = (5, 4, 3)
        mat = torch.eye(4, dtype=torch.float64)

    class X:
        tau = 0.25
        po = object()
    po = _identity_po(Y)
    mat, dim_g = proj_matrix(po, 'denoising')
    assert torch.equal(mat, torch.eye(4, dtype=torch.float64)) and tuple(dim_g) == (5, 4, 3)
    reps = _plan_repeats([X, X], Y, False, True)
    assert [tau for _, tau in reps] == [0.25, 0.25] and all(tuple(p.dim_x) == (5, 4, 3) for p, _ in reps)
    assert _plan_repeats([X], Y, False, False) == [(X.po, 0.25)]
    assert _plan_repeats([X], Y, True, True) == [(X.po, 0.25)]
    # what identifies a cached plan includes the setting
    assert _plan_signature([X], Y, 'denoising', False, False) != _plan_signature([X], Y, 'denoising', False, True)
    assert _plan_signature([X], Y, 'denoising', False) == _plan_signature([X], Y, 'denoising', False, False)
