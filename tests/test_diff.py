"""CPU checks of the float64 restatement of backward / central differences (tests/diff64.py) against dense matrices
written out from the definitions, of the identities that tie the three differences together, and of the host
surface that takes the setting (names, errors, C-ABI symbols).  The kernels themselves: tests/test_gpu_diff.py."""
import os
import re

import numpy as np
import pytest
import torch

from tests import admm64, diff64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = range(1, 8)


def table_D(n, vx, which):
    """D along one axis straight from the table: out-of-range samples are 0."""
    D = np.zeros((n, n))
    for i in range(n):
        def put(j, c):
            if 0 <= j < n:
                D[i, j] += c
        if which == 'forward':
            put(i + 1, 1 / vx), put(i, -1 / vx)
        elif which == 'backward':
            put(i, 1 / vx), put(i - 1, -1 / vx)
        else:
            put(i + 1, 0.5 / vx), put(i - 1, -0.5 / vx)
    return D


def table_Dt(n, vx, which):
    """D^T along one axis from the table's second column (NOT by transposing table_D)."""
    T = np.zeros((n, n))
    for i in range(n):
        def put(j, c):
            if 0 <= j < n:
                T[i, j] += c
        if which == 'forward':
            put(i - 1, 1 / vx), put(i, -1 / vx)
        elif which == 'backward':
            put(i, 1 / vx), put(i + 1, -1 / vx)
        else:
            put(i - 1, 0.5 / vx), put(i + 1, -0.5 / vx)
    return T


@pytest.mark.parametrize('which', diff64.WHICH)
@pytest.mark.parametrize('n', NS)
def test_transpose_rows_of_the_table_are_the_transpose(which, n):
    assert np.array_equal(table_Dt(n, 0.8, which), table_D(n, 0.8, which).T)
    assert np.array_equal(diff64.dense_1d(n, 0.8, which), table_D(n, 0.8, which))
    assert np.array_equal(diff64.dense_1d(n, 0.8, which, transpose=True), table_Dt(n, 0.8, which))


@pytest.mark.parametrize('n', NS)
def test_backward_is_the_mirrored_negated_forward_and_central_their_mean(n):
    Df, Db, Dc = (table_D(n, 1.25, w) for w in diff64.WHICH)
    P = np.eye(n)[::-1]
    assert np.array_equal(Db, -P @ Df @ P)
    assert np.array_equal(Db.T @ Db, P @ (Df.T @ Df) @ P)
    assert np.array_equal(Dc, (Df + Db) / 2)


@pytest.mark.parametrize('n', NS)
def test_dtd_rows(n):
    vx = 2.0
    B = table_D(n, vx, 'backward')
    B = B.T @ B * vx * vx
    for i in range(n):
        want = np.zeros(n)
        want[i] = 2.0 if i < n - 1 else 1.0  # [2,-1] at 0, [-1,2,-1] inside, [-1,1] at n-1
        if i > 0:
            want[i - 1] = -1.0
        if i < n - 1:
            want[i + 1] = -1.0
        if n == 1:
            want[:] = 1.0  # (y[0] - 0)^2: the single row is both ends
        assert np.array_equal(B[i], want), (n, i)
    Cm = table_D(n, vx, 'central')
    Cm = Cm.T @ Cm * 4 * vx * vx
    for i in range(n):
        want = np.zeros(n)
        want[i] = (i - 1 >= 0) + (i + 1 <= n - 1)
        if i - 2 >= 0:
            want[i - 2] = -1.0
        if i + 2 <= n - 1:
            want[i + 2] = -1.0
        assert np.array_equal(Cm[i], want), (n, i)
    if n == 1:
        assert not Cm.any()  # an axis of length 1 contributes nothing
    if n % 2 == 1:
        assert np.linalg.matrix_rank(Cm) < n  # singular for odd n


DIMS = [(nx, ny, nz) for nx in (1, 2, 5) for ny in (1, 3, 4) for nz in (1, 2, 3, 6, 7)]


def _dense3(dim, vx, which, transpose=False):
    """(3 N) x N matrix of the 3-D gradient (or N x 3 N of its transpose) from the 1-D tables."""
    blocks = []
    for d in range(3):
        f = [np.eye(dim[0]), np.eye(dim[1]), np.eye(dim[2])]
        f[d] = (table_Dt if transpose else table_D)(dim[d], vx[d], which)
        blocks.append(np.kron(np.kron(f[0], f[1]), f[2]))
    return np.hstack(blocks) if transpose else np.vstack(blocks)


@pytest.mark.parametrize('which', diff64.WHICH)
@pytest.mark.parametrize('dim', DIMS)
def test_diff64_against_dense_matrices(which, dim):
    rng = np.random.default_rng(sum(dim))
    vx = (0.8, 1.25, 2.0)
    # gradient and divergence multiply by the float32 reciprocal fl(1 / vx), the stencil divides by the float32 vx^2
    vr = tuple(1.0 / s for s in diff64.inv_vx(vx))
    v32 = tuple(float(np.float32(v)) for v in vx)
    y = rng.standard_normal(dim).astype(np.float32)
    g3 = rng.standard_normal((3,) + dim).astype(np.float32)
    n = y.size
    G = _dense3(dim, vr, which)
    ref, tol = diff64.gradient(y, vx, which)
    assert np.allclose(ref.ravel(), G @ y.ravel().astype(np.float64), rtol=0, atol=1e-13)
    assert np.allclose(tol.ravel(), diff64.UU * diff64.C_G * (np.abs(G) @ np.abs(y.ravel().astype(np.float64))), rtol=1e-12, atol=0)
    Gt = _dense3(dim, vr, which, transpose=True)
    ref, tol = diff64.divergence(g3, vx, which)
    assert np.allclose(ref.ravel(), Gt @ g3.ravel().astype(np.float64), rtol=0, atol=1e-13)
    assert np.allclose(tol.ravel(), diff64.UU * diff64.C_DIV * (np.abs(Gt) @ np.abs(g3.ravel().astype(np.float64))), rtol=1e-12, atol=0)
    G, Gt = _dense3(dim, v32, which), _dense3(dim, v32, which, transpose=True)
    A = Gt @ G
    assert np.allclose(diff64.dtd(y, vx, which).ravel(), A @ y.ravel().astype(np.float64), rtol=0, atol=1e-12)
    assert np.allclose(diff64.dense_dtd(dim, vx, which), A, rtol=0, atol=1e-13)
    assert np.allclose(diff64.dtd_abs(y, vx, which).ravel(), (np.abs(Gt) @ np.abs(G)) @ np.abs(y.ravel().astype(np.float64)),
                       rtol=1e-12, atol=0)
    assert n == G.shape[1]


def test_forward_restatement_is_the_existing_one():
    """diff64 with which='forward' restates what tests/admm64.py and tests/ref64.py already state."""
    from tests import ref64
    rng = np.random.default_rng(3)
    y = rng.standard_normal((4, 5, 6)).astype(np.float32)
    s = admm64.grad_scales(0.37, (0.8, 1.25, 2.0))
    a, b = admm64.grad64(y, s), diff64.grad64(y, s, 'forward')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    vx = torch.tensor((0.8, 1.25, 2.0), dtype=torch.float32).double()
    want = ref64.dtd_abs(torch.from_numpy(np.abs(y)).double(), vx).numpy()
    assert np.allclose(diff64.dtd_abs(y, (0.8, 1.25, 2.0), 'forward'), want, rtol=1e-14, atol=0)


def test_unknown_name_is_a_value_error_naming_the_argument(lib):
    import unires_amd as U
    from unires_amd import _lib, _plan, spatial
    with pytest.raises(ValueError, match='which'):
        diff64.coef('sideways')
    with pytest.raises(ValueError, match='which'):
        spatial.im_gradient(torch.zeros(4, 4, 4), which='sideways')
    with pytest.raises(ValueError, match='which'):
        spatial.im_divergence(torch.zeros(3, 4, 4, 4), which='upwind')
    with pytest.raises(ValueError, match='diff'):
        U._DtD(torch.zeros(4, 4, 4), (1, 1, 1), diff='upwind')
    with pytest.raises(ValueError, match='diff'):
        U._proj('AtA', torch.zeros(4, 4, 4), [], None, diff='upwind')
    with pytest.raises(ValueError, match='diff'):
        _plan.ChannelPlan((4, 4, 4), (1, 1, 1), [], 'denoising', False, diff='upwind')
    assert _lib.diff_code('forward') == 0 and _lib.diff_code('backward') == 1 and _lib.diff_code('central') == 2
    # the other two settings stay refused as they were
    with pytest.raises(NotImplementedError):
        spatial.im_gradient(torch.zeros(4, 4, 4), which='central', bound='dct2')
    with pytest.raises(NotImplementedError):
        U._DtD(torch.zeros(4, 4, 4), (1, 1, 1), bound='dct2', diff='central')
    # a known name still needs a device tensor: there is no CPU path
    with pytest.raises(RuntimeError, match='no CPU path'):
        spatial.im_gradient(torch.zeros(4, 4, 4), which='central')
    with pytest.raises(RuntimeError, match='no CPU path'):
        U._DtD(torch.zeros(4, 4, 4), (1, 1, 1), diff='backward')


NEW_SYMBOLS = ('unires_grad_which', 'unires_div_which', 'unires_dtd_which', 'unires_zw_update_which',
               'unires_nll_prior_which', 'unires_plan_set_diff')


def test_new_symbols_are_declared_bound_and_exported(lib):
    from unires_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    declared = set(re.findall(r'\b(unires_[a-z0-9_]+)\s*\(', hdr))
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in _lib.SIGNATURES, sym
        assert getattr(lib, sym) is not None
    for name, val in (('UNIRES_DIFF_FORWARD', 0), ('UNIRES_DIFF_BACKWARD', 1), ('UNIRES_DIFF_CENTRAL', 2)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, val), hdr), name
    assert lib.unires_abi_version() == 1


def test_unknown_which_is_an_argument_error_at_the_c_abi(lib):
    """An unknown `which` returns UNIRES_ERR_ARG before anything touches the device (no GPU needed: the argument
    checks come first; the pointers are never followed)."""
    from unires_amd import _lib
    buf = np.zeros(3 * 64, dtype=np.float32)
    p = buf.ctypes.data
    ok, vx = _lib.i3((4, 4, 4)), _lib.f3((1, 1, 1))
    for bad in (-1, 3, 7):
        assert lib.unires_grad_which(p, ok, vx, bad, p, None) == 3
        assert lib.unires_div_which(p, ok, vx, bad, p, None) == 3
        assert lib.unires_dtd_which(p, ok, vx, bad, 0.0, 1.0, p + 64, None) == 3
        assert b'which' in lib.unires_last_error()
