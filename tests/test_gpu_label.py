"""Label warping (one-pass vote, k_warp_label) and the nearest-neighbour pull (k_pull_nearest) on the
GPU against the restated reference (tests/label_restated.py: one oracle pull per label value,
ascending, strict '>'), and the label path end to end: _read_label -> _init_y_label,
_resample_inplane, fit()."""
import math

import numpy as np
import pytest
import torch

from oracle import nitorch_restated as N
from tests import label_restated as R
from tests.helpers import gpu_structs, make_problem

pytestmark = pytest.mark.gpu
TOL_FOV = 5e-2


def _rot(a, b, c):
    K = torch.tensor([[0, -c, b], [c, 0, -a], [-b, a, 0]], dtype=torch.float64)
    return torch.linalg.matrix_exp(K)


def _affine(lin, off):
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.as_tensor(lin, dtype=torch.float64)
    M[:3, 3] = torch.as_tensor(off, dtype=torch.float64)
    return M


def _labels(shape, n, seed, device='cpu'):
    """Voronoi parcellation with n distinct values, 0 and negative values among them."""
    gen = torch.Generator().manual_seed(seed)
    vals = (torch.randperm(4 * n, generator=gen)[:n] - n).float()
    if not bool((vals == 0).any()):
        vals[0] = 0.0
    return R.voronoi_labels(shape, vals, gen, device)


# ---- 1. exact geometries: every coordinate exact in float32 on both sides --------------------------
SRC = (13, 11, 9)
EXACT = {
    'identity': (_affine(torch.eye(3), [0, 0, 0]), SRC),
    'identity_margin': (_affine(torch.eye(3), [-2, -1, -3]), (17, 14, 15)),
    'half_x': (_affine(torch.eye(3), [0.5, 0, 0]), SRC),
    'half_xy': (_affine(torch.eye(3), [-0.5, 0.5, 0]), SRC),
    'half_xyz': (_affine(torch.eye(3), [0.5, -0.5, 0.5]), (14, 12, 10)),
    'scale2': (_affine(2 * torch.eye(3), [-0.5, 0.5, -1.5]), (8, 7, 6)),
    'scale_half': (_affine(0.5 * torch.eye(3), [-0.5, 0.5, -0.25]), (28, 24, 21)),
    'scale_half_mixed': (_affine(torch.diag(torch.tensor([0.5, 2.0, 0.5])), [0.25, -0.5, 0.5]), (27, 7, 19)),
    # signed permutation: x' = -z + 8, y' = x, z' = -y + 10.5
    'signed_perm': (_affine([[0, 0, -1], [1, 0, 0], [0, -1, 0]], [8, 0, 10.5]), (10, 13, 12)),
}


@pytest.mark.parametrize('name', sorted(EXACT))
@pytest.mark.parametrize('n_labels', [2, 7, 40])
def test_warp_label_exact_geometries_bit_for_bit(dev, name, n_labels):
    from unires_amd import _core
    M, shape = EXACT[name]
    lab = _labels(SRC, n_labels, seed=n_labels)
    want, p = R.warp_label(lab, R.affine_grid(M, shape))
    got = _core._warp_label(lab.to(dev), M, shape)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    got = got.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    assert bool((p > 0).any())


def test_warp_label_single_slice_and_dense_grid(dev):
    """A one-slice label volume (pull_issue's single-slice loads) and the dense-grid calling form."""
    from unires_amd import _core, spatial
    lab = _labels((9, 8, 1), 5, seed=3)
    M = _affine(torch.eye(3), [0.5, -0.5, 0.0])
    grid = spatial.affine_grid(M, (10, 9, 3))
    want = R.warp_label(lab, R.affine_grid(M, (10, 9, 3)))[0]
    assert torch.equal(_core._warp_label(lab.to(dev), grid).cpu(), want)
    assert torch.equal(_core._warp_label(lab.to(dev), grid[None]).cpu(), want)
    # integer labels come back in their own dtype
    got = _core._warp_label(lab.to(torch.int16).to(dev), M, (10, 9, 3))
    assert got.dtype == torch.int16 and torch.equal(got.cpu(), want.to(torch.int16))


# ---- 2. general rigids at mid size: disagreements are ties within reach ------------------------------
def _allowed(got, want, p_best, p_got, grid, sdim, eps=1e-5):
    """Voxels where got != want although neither a near-tie nor a near-FOV-threshold explains it."""
    diff = got != want
    tie = (p_best - p_got) <= eps
    near = torch.zeros_like(diff)
    for d in range(3):
        g = grid[..., d].double()
        near |= ((g + TOL_FOV).abs() <= eps) | ((g - (sdim[d] - 1 + TOL_FOV)).abs() <= eps)
    return diff, diff & ~tie & ~near


def _rigid_case(seed, sdim, gdim):
    gen = torch.Generator().manual_seed(seed)
    ang = (torch.rand(3, generator=gen, dtype=torch.float64) * 2 - 1) * 0.1
    t = (torch.rand(3, generator=gen, dtype=torch.float64) * 2 - 1) * 5.0
    lin = _rot(*ang) @ torch.diag(torch.tensor([s / g for s, g in zip(sdim, gdim)], dtype=torch.float64))
    cg = torch.tensor([(g - 1) / 2 for g in gdim], dtype=torch.float64)
    cs = torch.tensor([(s - 1) / 2 for s in sdim], dtype=torch.float64)
    return _affine(lin, cs + t - lin @ cg)


@pytest.mark.slow
@pytest.mark.parametrize('n_labels,seed', [(20, 11), (120, 12)])
def test_warp_label_rigid_midsize_ties_only(dev, n_labels, seed):
    from unires_amd import _core
    sdim, gdim = (48, 45, 34), (96, 90, 102)
    lab = _labels(sdim, n_labels, seed)
    M = _rigid_case(seed, sdim, (96, 90, 68))  # output z reaches past the volume: FOV edges
    got = _core._warp_label(lab.to(dev), M, gdim).cpu()
    grid = R.affine_grid(M, gdim)
    want, p_best, p_got = R.warp_label(lab, grid, p_of=got)
    diff, unexplained = _allowed(got, want, p_best, p_got, grid, sdim)
    assert int(unexplained.sum()) == 0, unexplained.nonzero()[:5].tolist()
    assert int(diff.sum()) < 1e-4 * got.numel(), int(diff.sum())
    assert len(got.unique()) > n_labels // 2 and bool((got == 0).any())


# ---- 3. full size against the reference's form on the GPU (one pull + one select per value) ----------
def _per_label_form(lab, M12, gdim, p_of=None):
    from unires_amd import _ops
    f = torch.zeros(gdim, dtype=torch.float32, device=lab.device)
    p = torch.zeros_like(f)
    q = torch.zeros_like(f) if p_of is not None else None
    for v in lab.unique():
        t = _ops.pull_affine((lab == v).float(), M12, gdim)
        m = t > p
        p = torch.where(m, t, p)
        f = torch.where(m, v, f)
        if q is not None:
            q = torch.where(p_of == v, t, q)
    return f, p, q


@pytest.mark.slow
def test_warp_label_full_size_against_per_label_pulls(dev):
    from unires_amd import _ops
    from unires_amd.spatial import _m12
    sdim, gdim = (181, 217, 181), (256, 256, 256)
    lab = _labels(sdim, 100, seed=21, device=dev)
    M12 = _m12(_rigid_case(21, sdim, gdim))
    a = _ops.warp_label(lab, M12, gdim)
    b = _ops.warp_label(lab, M12, gdim)
    assert torch.equal(a, b)
    f, p, q = _per_label_form(lab, M12, gdim, p_of=a)
    diff = a != f
    assert int((diff & ((p - q) > 1e-5)).sum()) == 0
    assert int(diff.sum()) < 1e-4 * a.numel(), int(diff.sum())
    assert len(a.unique()) > 90


# ---- 4. nearest-neighbour pull against the oracle's order 0 -----------------------------------------
# coordinates are float32 on both sides but summed in another order (lin @ ijk + off vs the kernel's FMA
# chain): up to a few ulps apart, ~1e-5 at these magnitudes
def _half_way(grid, eps=1e-5):
    fr = grid.double() - grid.double().floor()
    return ((fr - 0.5).abs() <= eps).any(-1)


def _near_fov(grid, sdim, eps=1e-5):
    near = torch.zeros(grid.shape[:3], dtype=torch.bool)
    for d in range(3):
        g = grid[..., d].double()
        near |= ((g + TOL_FOV).abs() <= eps) | ((g - (sdim[d] - 1 + TOL_FOV)).abs() <= eps)
    return near


@pytest.mark.parametrize('seed', [0, 1])
def test_pull_nearest_matches_oracle(dev, seed):
    from unires_amd import spatial
    gen = torch.Generator().manual_seed(seed)
    sdim, gdim = (20, 18, 16), (27, 25, 23)
    src = torch.rand(sdim, generator=gen) - 0.5
    lin = _rot(0.2, -0.15, 0.1) @ torch.diag(torch.tensor([0.8, 0.75, 0.7], dtype=torch.float64))
    M = _affine(lin, [-1.3, 0.7, -0.4])
    grid = R.affine_grid(M, gdim)
    want = N.grid_pull(src[None, None], grid[None], interpolation=0, bound='zero', extrapolate=False)[0, 0]
    for form in ('affine', 'grid'):
        if form == 'affine':
            got = spatial.grid_pull(src.to(dev), M, gdim, interpolation=0).cpu()
        else:
            got = spatial.grid_pull(src.to(dev), spatial.affine_grid(M, gdim)[None], interpolation='nearest').cpu()
        keep = ~_half_way(grid) & ~_near_fov(grid, sdim)
        assert int((~keep).sum()) < 10
        assert torch.equal(got[keep], want[keep])
        assert bool((got == 0).any()) and bool((got != 0).any())


def test_pull_nearest_half_way_and_fov_edge(dev):
    from unires_amd import _ops
    from unires_amd.spatial import _m12
    sdim = (6, 5, 7)
    src = torch.arange(1, 1 + math.prod(sdim), dtype=torch.float32).reshape(sdim)
    # half-way everywhere: rint rounds to even, like torch.round
    M = _affine(torch.eye(3), [0.5, 1.5, -0.5])
    grid = R.affine_grid(M, sdim)
    want = N.grid_pull(src[None, None], grid[None], interpolation=0, bound='zero', extrapolate=False)[0, 0]
    got = _ops.pull_nearest(src.to(dev), _m12(M), sdim).cpu()
    assert torch.equal(got, want)
    assert float(got[0, 0, 1]) == float(src[0, 2, 0])  # (0.5, 1.5, 0.5) -> (0, 2, 0)
    # the FOV edge along each axis: 0.04 outside the volume is inside the tolerance, 0.06 is not
    for d in range(3):
        for shift, inside in ((-0.04, True), (-0.06, False), (0.04, True), (0.06, False)):
            off = [0.0, 0.0, 0.0]
            off[d] = shift
            M = _affine(torch.eye(3), off)
            got = _ops.pull_nearest(src.to(dev), _m12(M), sdim).cpu()
            grid = R.affine_grid(M, sdim)
            want = N.grid_pull(src[None, None], grid[None], interpolation=0, bound='zero', extrapolate=False)[0, 0]
            assert torch.equal(got, want), (d, shift)
            idx = [slice(None)] * 3
            idx[d] = 0 if shift < 0 else sdim[d] - 1
            edge = got[tuple(idx)]
            assert bool((edge != 0).all()) if inside else bool((edge == 0).all()), (d, shift)


# ---- 5. end to end ----------------------------------------------------------------------------------
def _obs(lab, mat, dev, seed):
    import unires_amd as U
    gen = torch.Generator().manual_seed(seed)
    xn = U._input(dat=torch.rand(lab.shape, generator=gen).to(dev), mat=mat)
    return xn


def test_read_label_then_init_y_label(dev, tmp_path):
    import unires_amd as U
    from unires_amd import nifti
    sett = U.settings()
    sett.device = dev
    labs = [_labels((12, 10, 8), 9, seed=31), _labels((11, 9, 8), 4, seed=32)]
    mats = [_affine(torch.diag(torch.tensor([1.0, 1.0, 2.0])), [-4, 3, 2]),
            _affine(torch.diag(torch.tensor([1.0, 2.0, 1.0])), [-5, 2, 1])]
    x = []
    for c, (lab, mat) in enumerate(zip(labs, mats)):
        pth = str(tmp_path / ('lab%d.nii.gz' % c))
        nifti.write(pth, lab.numpy(), mat.numpy())
        xc = [_obs(lab, mat, dev, c), _obs(lab, mat, dev, 10 + c)]
        U._read_label(xc[0], pth, sett)
        assert xc[0].label[0].device.type == dev.type and xc[0].label[0].dtype == torch.float32
        x.append(xc)
    x[1][1].label = None
    mat_y = _affine(torch.diag(torch.tensor([0.5, 0.5, 1.0])), [-4.25, 2.75, 1.5])
    y = [U._output(dat=torch.zeros(20, 18, 16, device=dev), mat=mat_y) for _ in x]
    U._init_y_label(x, y, sett)
    xr = [[type('X', (), dict(label=[xc[0].label[0].cpu()], mat=xc[0].mat))()] for xc in x]
    yr = [type('Y', (), dict(dim=(20, 18, 16), mat=mat_y, label=None))() for _ in x]
    R.init_y_label(xr, yr)
    for c in range(2):
        assert y[c].label.device.type == dev.type and torch.equal(y[c].label.cpu(), yr[c].label)
        assert len(y[c].label.unique()) > 2


@pytest.mark.parametrize('vx', [1.0, [1.5, 0.75, 1.0]])
def test_resample_inplane(dev, vx):
    import unires_amd as U
    sett = U.settings()
    sett.device, sett.force_inplane_res, sett.vx = dev, True, vx
    lab = _labels((16, 14, 6), 8, seed=41)
    mat = _affine(torch.diag(torch.tensor([0.5, 0.5, 2.0])), [-3, 2, 1])
    x = [[_obs(lab, mat, dev, 1), _obs(lab, _affine(torch.diag(torch.tensor([2.0, 2.0, 2.0])), [0, 0, 0]), dev, 2)]]
    x[0][0].label = [lab.to(dev), None]
    ref = [[type('X', (), dict(dat=xn.dat.cpu(), mat=xn.mat.clone(), dim=xn.dim,
                                label=None if xn.label is None else [xn.label[0].cpu()]))() for xn in x[0]]]
    R.resample_inplane(ref, True, sett.max_iter, vx)
    U._resample_inplane(x, sett)
    assert x[0][0].dim != lab.shape and x[0][1].dim == lab.shape  # the 2 mm image is skipped
    for a, b in zip(x[0], ref[0]):
        assert tuple(a.dim) == tuple(b.dim) and tuple(a.dat.shape) == tuple(b.dim)
        assert torch.equal(a.dat.cpu(), b.dat) and torch.equal(torch.as_tensor(a.mat), b.mat)
        assert (a.label is None) == (b.label is None)
        if a.label is not None:
            assert torch.equal(a.label[0].cpu(), b.label[0])
    # off unless force_inplane_res and max_iter > 0
    for force, it in ((False, 5), (True, 0)):
        sett.force_inplane_res, sett.max_iter = force, it
        x2 = [[_obs(lab, mat, dev, 1)]]
        U._resample_inplane(x2, sett)
        assert x2[0][0].dim == lab.shape


def test_fit_leaves_labels_alone(dev):
    import unires_amd as U
    prob = make_problem(dim_y=(16, 14, 12), n_channels=1, thick=3, seed=51)
    xg, yg, sett = gpu_structs(prob, dev)
    for c in range(len(yg)):
        yg[c].lam0 = float(yg[c].lam) / 4.0
        yg[c].label = _labels(prob['dim_y'], 6, seed=52).to(dev)
    keep = [y.label.clone() for y in yg]
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 3, 1e-4, 4.0, 1
    U.fit(xg, yg, sett)
    for y, k in zip(yg, keep):
        assert torch.equal(y.label, k)
