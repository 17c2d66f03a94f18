"""nitorch.spatial-shaped entry points for the functions UniRes imports from it
(unires/_project.py:2-3, unires/_update.py:5-7), backed by the HIP library.

The dense coordinate grid that the reference materialises on every operator call
(affine_grid, unires/_project.py:159) never exists here: pull/push take the 4x4
affine itself and compute coordinates in registers.  Two calling forms are accepted:

    grid_pull(input, mat, shape)        # the efficient one: the affine and the grid shape
    grid_pull(input, grid)              # nitorch's own: a dense (1, X, Y, Z, 3) grid that IS an
                                        # affine grid (what unires/_project.py:159 builds); the
                                        # affine is recovered from it and checked.  A grid that is
                                        # not affine raises NotImplementedError: the path only ever
                                        # builds affine grids.
This is a convenience layer over ``_ops``; the drop-in seam of the path is one level up
(``_proj`` / ``_proj_apply`` / ``_update_admm``).
"""
import numpy as np
import torch

from . import _ops


def voxel_size(mat):
    """Column norms of the linear part of an affine (float64 CPU tensor)."""
    m = torch.as_tensor(mat, dtype=torch.float64, device='cpu')
    return (m[:3, :3] ** 2).sum(0).sqrt()


def affine_matrix_classic(prm):
    """nitorch.spatial.affine_matrix_classic for the one form the path calls it with
    (unires/_core.py:251): three translations -> the 4x4 float64 translation matrix  [recalled].
    Rotations, zooms and shears (parameters 4 - 12 of SPM's spm_matrix) are not built."""
    t = torch.as_tensor(prm, dtype=torch.float64).detach().cpu().reshape(-1)
    if t.numel() > 3:
        raise NotImplementedError('affine_matrix_classic: only translations (3 parameters) are built')
    mat = torch.eye(4, dtype=torch.float64)
    mat[:t.numel(), 3] = t
    return mat


# SPM's visiting order of the 48 signed permutations: six permutations (the row of the one in each
# column), eight sign patterns each (bit k of the counter set: +1 on row k)  [recalled]
_SPM_PERMS = ((0, 1, 2), (1, 0, 2), (2, 0, 1), (2, 1, 0), (0, 2, 1), (1, 2, 0))


def _signed_perms():
    out = []
    for perm in _SPM_PERMS:
        R1 = np.zeros((3, 3))
        for col, row in enumerate(perm):
            R1[row, col] = 1.0
        for bits in range(8):
            F = np.diag([2.0 * ((bits >> k) & 1) - 1.0 for k in range(3)])
            out.append(F @ R1)
    return out


def _canonical(M, dim):
    """The grid (M, dim) stored near-axially: M right-multiplied by the voxel map [R2^-1 | off] of the
    signed permutation R2 that brings its unit axes closest to the identity."""
    vx = np.sqrt((M[:3, :3] ** 2).sum(0))
    R = M[:3, :3] / vx
    best, best_ss = None, np.inf
    for R2 in _signed_perms():
        ss = ((R @ R2.T - np.eye(3)) ** 2).sum()  # (R2^-1 = R2^T)
        if ss < best_ss:
            best, best_ss = R2, ss
    Q = np.eye(4)
    Q[:3, :3] = best.T
    # a flipped stored axis k (a -1 in row k of R2^-1) starts from its last voxel
    Q[:3, 3] = np.where(best.T.sum(1) < 0, np.asarray(dim, dtype=np.float64) - 1.0, 0.0)
    return M @ Q


def _logm_mean(mats):
    """Matrix-log mean: M <- M expm(mean_i logm(M^-1 M_i)) from M = I until the update vanishes."""
    from scipy.linalg import expm, logm
    M = np.eye(4)
    for _ in range(1024):
        S = np.mean([np.real(logm(np.linalg.solve(M, Mi))) for Mi in mats], axis=0)
        M = M @ expm(S)
        if (S ** 2).sum() < 1e-20:
            break
    return M


def _no_shear(A):
    """(R, z): the rotation R and zooms z > 0 with R diag(z) closest to A in Frobenius norm, by
    alternating the polar factor of A diag(z) with z = diag(R^T A)."""
    z = np.sqrt((A ** 2).sum(0))
    R = np.eye(3)
    for _ in range(10000):
        U, _, Vt = np.linalg.svd(A * z)
        U[:, -1] *= np.sign(np.linalg.det(U @ Vt))
        R = U @ Vt
        z_new = np.einsum('ij,ij->j', R, A)
        done = np.abs(z_new - z).max() <= 1e-15 * np.abs(z).max()
        z = z_new
        if done:
            break
    return R, z


_FOV_EPS = 1e-10  # voxels: rounding noise the floor / ceil of the field of view must not see


def _mean_space(Mat, Dim, vx=None):
    """Mean orientation matrix and field of view of N grids: ``Mat`` (N, 4, 4) voxel-to-world,
    ``Dim`` (N, 3), ``vx`` the voxel size wanted (a scalar, three values, or None: the mean's own).
    Returns float64 CPU tensors ``(mat (4, 4), dim (3,), vx (3,))``.

    nitorch's ``_mean_space`` (unires/_core.py:228) restated from the published algorithm it ports,
    SPM12's mean-space code (J. Ashburner)  [recalled]: every grid is re-stored near-axially; the
    matrix-log mean of the results is taken; its shears are removed; the voxel size is applied; the
    field of view is the bounding box of every grid's corner voxel centres, without padding.  All
    arithmetic is float64 on the host."""
    Mat = torch.as_tensor(Mat, dtype=torch.float64).detach().cpu().numpy().reshape(-1, 4, 4)
    Dim = torch.as_tensor(Dim, dtype=torch.float64).detach().cpu().numpy().reshape(-1, 3)
    if len(Mat) == 0 or len(Mat) != len(Dim):
        raise ValueError('_mean_space: one dimension triple per matrix, at least one')
    M = _logm_mean([_canonical(m, d) for m, d in zip(Mat, Dim)])
    R, z = _no_shear(M[:3, :3])
    if vx is not None:
        z = np.broadcast_to(torch.as_tensor(vx, dtype=torch.float64).detach().cpu().numpy().reshape(-1), (3,))
    mat = np.eye(4)
    mat[:3, :3] = R * z
    mat[:3, 3] = M[:3, 3]
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for m, d in zip(Mat, Dim):
        c = np.array([[i, j, k, 1.0] for i in (0.0, d[0] - 1) for j in (0.0, d[1] - 1) for k in (0.0, d[2] - 1)])
        p = (np.linalg.solve(mat, m) @ c.T)[:3]
        lo, hi = np.minimum(lo, p.min(1)), np.maximum(hi, p.max(1))
    mn, mx = np.floor(lo + _FOV_EPS), np.ceil(hi - _FOV_EPS)
    T = np.eye(4)
    T[:3, 3] = mn
    return (torch.from_numpy(mat @ T), torch.from_numpy(mx - mn + 1.0),
            torch.from_numpy(np.array(z, dtype=np.float64)))


def _m12(mat):
    """float32 row-major 3x4 of a (4,4)/(3,4) affine - the cast the reference does
    at grid creation (mat.type(dat.dtype), unires/_project.py:159)."""
    m = np.asarray(torch.as_tensor(mat).detach().cpu().numpy(), dtype=np.float64)
    return m[:3, :4].astype(np.float32).reshape(-1)


def affine_grid(mat, shape, jitter=False):
    """Dense voxel-coordinate grid ``(*shape, 3)`` of an affine, float32 like the reference's call
    (unires/_project.py:159).  Only for callers that insist on a grid: the kernels never read one."""
    m = torch.as_tensor(mat).detach().cpu().to(torch.float32)
    ax = [torch.arange(int(n), dtype=torch.float32) for n in shape]
    ijk = torch.stack(torch.meshgrid(*ax, indexing='ij'), -1)
    return ijk @ m[:3, :3].T + m[:3, 3]


def _affine_of_grid(grid):
    """(mat 4x4 float64, shape) of a dense grid that is an affine grid, else NotImplementedError."""
    g = torch.as_tensor(grid).detach()
    if g.dim() == 5 and g.shape[0] == 1:
        g = g[0]
    if g.dim() != 4 or g.shape[-1] != 3:
        raise ValueError('grid must be (1, X, Y, Z, 3) or (X, Y, Z, 3)')
    shape = tuple(int(n) for n in g.shape[:3])
    g = g.to('cpu', torch.float64)
    o = g[0, 0, 0]
    mat = torch.eye(4, dtype=torch.float64)
    mat[:3, 3] = o
    for d in range(3):
        if shape[d] > 1:
            idx = [0, 0, 0]
            idx[d] = shape[d] - 1
            mat[:3, d] = (g[tuple(idx)] - o) / (shape[d] - 1)
    # EVERY grid point must lie on the affine (float32 grids: a few ulps of the coordinates): a dense
    # deformation that happens to vanish at a handful of probe points must not be sampled as if it were
    # one (one vectorised pass on the host; this facade is a convenience path, not the hot one)
    tol = 1e-4 * max(1.0, float(g.abs().max()))
    ax = [torch.arange(n, dtype=torch.float64) for n in shape]
    ijk = torch.stack(torch.meshgrid(*ax, indexing='ij'), -1)
    want = ijk @ mat[:3, :3].T + mat[:3, 3]
    if float((g - want).abs().max()) > tol:
        raise NotImplementedError('unires_amd: only affine sampling grids are built (the reference '
                                  'path never makes another kind, unires/_project.py:159)')
    return mat, shape


def _mat_shape(mat_or_grid, shape):
    t = torch.as_tensor(mat_or_grid)
    if t.dim() >= 4:
        return _affine_of_grid(t)
    if shape is None:
        raise ValueError('shape is required with an affine matrix')
    return t, tuple(int(n) for n in shape)


def grid_pull(input, mat, shape=None, interpolation='linear', bound='zero', extrapolate=False):
    """nitorch grid_pull(input, affine_grid(mat, shape), ...); ``mat`` may be that grid itself.
    ``interpolation`` 0 / 'nearest' takes the nearest-neighbour pull (unires/_core.py:484)."""
    nearest = _is_nearest(interpolation)
    _only_linear_zero(1 if nearest else interpolation, bound, extrapolate)  # (bound / extrapolate as for order 1)
    m, shp = _mat_shape(mat, shape)
    return (_ops.pull_nearest if nearest else _ops.pull_affine)(input, _m12(m), shp)


def grid_grad(input, mat, shape=None, interpolation='linear', bound='zero', extrapolate=False):
    """nitorch grid_grad(input, affine_grid(mat, shape), ...) -> (..., *shape, 3)."""
    _only_linear_zero(interpolation, bound, extrapolate)
    m, shp = _mat_shape(mat, shape)
    return _ops.pull_grad_affine(input, _m12(m), shp)


def grid_push(input, mat, shape, interpolation='linear', bound='zero', extrapolate=False):
    """nitorch grid_push(input, affine_grid(mat, input.shape[-3:]), shape=shape, ...); ``mat`` may
    be that grid itself (its spatial shape must be the input's)."""
    _only_linear_zero(interpolation, bound, extrapolate)
    t = torch.as_tensor(mat)
    if t.dim() >= 4:
        m, gshape = _affine_of_grid(t)
        if tuple(input.shape[-3:]) != gshape:
            raise ValueError('grid_push: grid and input shapes differ')
        mat = m
    return _ops.push_affine(input, _m12(mat), shape)


def im_gradient(dat, vx=None, which='forward', bound='zero'):
    """nitorch im_gradient, zero bound: ``which`` = 'forward' | 'backward' | 'central'  (diff1d  [recalled])."""
    _only_zero_bound(which, bound)
    return _ops.grad(dat, vx, which)


def im_divergence(dat, vx=None, which='forward', bound='zero'):
    """nitorch im_divergence: the positive transpose of :func:`im_gradient` (div1d  [recalled])."""
    _only_zero_bound(which, bound)
    return _ops.div(dat, vx, which)


def _is_nearest(interpolation):
    return not isinstance(interpolation, bool) and interpolation in (0, 'nearest')


def _only_linear_zero(interpolation, bound, extrapolate):
    if interpolation not in ('linear', 1) or bound != 'zero' or extrapolate:
        raise NotImplementedError('unires_amd builds the reference defaults only: '
                                  "interpolation='linear', bound='zero', extrapolate=False "
                                  '(unires/struct.py:64,85; unires/_project.py:162,181)')


def _only_zero_bound(which, bound):
    from ._lib import diff_code
    diff_code(which, 'which')  # ValueError for a name that is none of the three
    if bound != 'zero':
        raise NotImplementedError("unires_amd builds the reference default only: "
                                  "bound='zero' (unires/struct.py:64)")
