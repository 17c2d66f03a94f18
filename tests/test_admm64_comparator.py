"""The per-voxel and per-sum bounds of tests/admm64.py, checked on the CPU: they are sound (the float32 oracle's
update_zw, compute_nll, its masked likelihood sum, the slice-scaling sums of update_scaling, the rigid sums in
update_rigid_channel's order and grid_grad all pass them) and sharp (one z voxel off by 10x its tolerance, one
64 x 4 patch of the shrinkage image off by 1e-3, one slice counted on the wrong parity, one 256-term block missing
from the masked sum, one rigid voxel off by 1e-6 and one gradient voxel off by 10x its tolerance all fail them,
while the relative gates of the GPU parity tests pass the first two)."""
import math

import numpy as np
import pytest
import torch

from oracle import nitorch_restated as N
from oracle import unires_restated as O
from tests import admm64
from tests.helpers import rel_err

VX = {'iso': (1.0, 1.0, 1.0), 'aniso': (0.8, 1.25, 2.0)}


def _mat(vx):
    return torch.diag(torch.tensor(list(vx) + [1.0], dtype=torch.float64))


def _oracle_zw(ys, lam, z, w, rho, alpha, vx):
    yo = [O.make_output(ys[c].clone(), _mat(vx), torch.tensor(lam[c])) for c in range(len(ys))]
    return O.update_zw(yo, z.clone(), w.clone(), torch.tensor(rho), alpha=alpha)


def _check(out, ref, tol):
    err = np.abs(np.asarray(out, dtype=np.float64) - ref)
    bad = err > tol
    return dict(ok=not bad.any(), n_bad=int(bad.sum()), max_ratio=float((err / np.maximum(tol, 1e-300)).max()),
                first=tuple(int(i) for i in np.argwhere(bad)[0]) if bad.any() else None)


@pytest.mark.parametrize('C,alpha,vx', [(1, 1.0, 'iso'), (3, 1.0, 'aniso'), (3, 1.5, 'iso'), (2, 0.7, 'aniso'),
                                        (10, 1.0, 'aniso'), (9, 1.5, 'iso')])
def test_float32_oracle_passes_the_zw_bounds(C, alpha, vx):
    rho = 0.37
    dim = (9, 13, 70)
    ys, lam, z, w = admm64.zw_inputs(dim, C, rho, alpha, vx=VX[vx])
    zo, wo, so = _oracle_zw(ys, lam, z, w, rho, alpha, VX[vx])
    B = admm64.zw_update(ys.numpy(), lam, VX[vx], rho, alpha, z.numpy(), w.numpy())
    s = B['s'][0]
    # both sides of the kink are populated
    assert 0.3 < float((s > 0).mean()) < 0.7, float((s > 0).mean())
    r = _check(so.numpy(), *B['s'])
    assert r['ok'], ('s', r)
    assert r['max_ratio'] > 0.0
    for c in range(C):
        Bc = B['chan'](c)
        for key, out in (('z', zo[c]), ('w', wo[c])):
            r = _check(out.numpy(), *Bc[key])
            assert r['ok'], (key, c, r)
            assert r['max_ratio'] > 0.0
    # the prior term: compute_nll with no observations is sum_v sqrt(sum_c |lam_c D y_c|^2)
    yo = [O.make_output(ys[c].clone(), _mat(VX[vx]), torch.tensor(lam[c])) for c in range(C)]
    _, _, nll_y = O.compute_nll([[] for _ in range(C)], yo, 'denoising', False)
    ref, tol = admm64.nll_prior(ys.numpy(), lam, VX[vx])
    assert abs(float(nll_y) - ref) <= tol, (float(nll_y), ref, tol)


def test_zw_bounds_catch_one_voxel_and_one_patch_that_rel_gates_pass():
    rho = 0.37
    dim = (64, 128, 130)
    ys, lam, z, w = admm64.zw_inputs(dim, 2, rho, vx=VX['aniso'])
    B = admm64.zw_update(ys.numpy(), lam, VX['aniso'], rho, 1.0, z.numpy(), w.numpy())
    zr, dz = B['chan'](1)['z']
    zr0 = B['chan'](0)['z'][0]
    assert _check(zr, zr, dz)['ok']
    # one z voxel off by 10x its tolerance: the 2e-5 relative gate of the zw tests (on z of all channels) cannot
    # see it
    v = (2, 20, 64, 65)
    bad = zr.copy()
    bad[v] += 10 * dz[v]
    assert rel_err(torch.from_numpy(np.stack([zr0, bad])), torch.from_numpy(np.stack([zr0, zr]))) < 2e-5
    r = _check(bad, zr, dz)
    assert not r['ok'] and r['n_bad'] == 1 and r['first'] == v
    # one 64 x 4 (z, y) patch of the shrinkage image off by 1e-3 relative
    s, ds = B['s']
    bad = s.copy()
    bad[17, 40:44, 64:128] *= 1 + 1e-3
    assert rel_err(torch.from_numpy(bad), torch.from_numpy(s)) < 2e-5
    r = _check(bad, s, ds)
    assert not r['ok'] and r['n_bad'] > 64


def test_masked_sse_bound_is_sound_and_sees_one_block():
    g = torch.Generator().manual_seed(3)
    x = (torch.rand((256, 256, 42), generator=g) * 100).float()
    x[::7, :, 3] = 0
    x[5, 5, :] = -0.0
    ay = (torch.rand((256, 256, 42), generator=g) * 100).float()
    msk = x != 0
    oracle = torch.sum((x[msk] - ay[msk]) ** 2, dtype=torch.float64).item()
    ref, tol = admm64.masked_sse(x.numpy(), ay.numpy())
    assert abs(oracle - ref) <= tol, (oracle, ref, tol)
    # one 256-term block dropped
    r = (x.numpy() - ay.numpy()).ravel()[msk.numpy().ravel()]
    block = math.fsum((r[4096:4352] * r[4096:4352]).astype(np.float64).tolist())
    assert abs((ref - block) - ref) > tol


@pytest.mark.parametrize('dim_thick', [0, 1, 2])
def test_scaling_sums_bound_is_sound_and_sees_one_swapped_slice(dim_thick):
    g = torch.Generator().manual_seed(4 + dim_thick)
    dim = (37, 29, 31)
    x = (torch.rand(dim, generator=g) * 10).float()
    x[x < 1] = 0
    ay = (torch.rand(dim, generator=g) * 10).float()
    ref, tol = admm64.scaling_sums(x.numpy(), ay.numpy(), dim_thick)
    # the oracle's sums (update_scaling, :330-345)
    msk = x != 0
    xo = O.even_odd(x, 'odd', dim_thick)[O.even_odd(msk, 'odd', dim_thick)]
    xe = O.even_odd(x, 'even', dim_thick)[O.even_odd(msk, 'even', dim_thick)]
    yo = O.even_odd(ay, 'odd', dim_thick)[O.even_odd(msk, 'odd', dim_thick)]
    ye = O.even_odd(ay, 'even', dim_thick)[O.even_odd(msk, 'even', dim_thick)]
    oracle = [torch.sum((x[msk] - ay[msk]) ** 2, dtype=torch.float64), torch.sum(ye * (xe - ye), dtype=torch.float64),
              torch.sum(yo * (xo - yo), dtype=torch.float64), torch.sum(ye ** 2, dtype=torch.float64),
              torch.sum(yo ** 2, dtype=torch.float64)]
    r = admm64.check_sums([float(v) for v in oracle], ref, tol)
    assert r['ok'], r
    # slice 12 along dim_thick counted on the wrong parity
    s0, gg, hh, ev = admm64.scaling_terms(x.numpy(), ay.numpy(), dim_thick)
    idx = np.indices(dim)[dim_thick][msk.numpy()]
    ev = np.where(idx == 12, ~ev, ev)
    bad = admm64.scaling_sums_of((s0, gg, hh, ev))
    r = admm64.check_sums(bad, ref, tol)
    assert not r['ok'] and r['first'] == 1
    assert abs(bad[3] + bad[4] - ref[3] - ref[4]) <= tol[3] + tol[4]  # (even + odd = all still holds)


@pytest.mark.parametrize('ctc', [False, True])
def test_rigid_sums_bound_is_sound_and_sees_one_voxel(ctc):
    g = torch.Generator().manual_seed(8)
    dim = (13, 11, 7)
    gr3 = torch.randn(dim + (3,), generator=g).float()
    diff = torch.randn(dim, generator=g).float()
    c = (torch.rand(dim, generator=g) + 0.5).float() if ctc else None
    D = (torch.randn((6, 3, 4), generator=g) * 0.1).float()
    ref, tol = admm64.rigid_sums(gr3.numpy(), diff.numpy(), None if c is None else c.numpy(), D.numpy())
    # update_rigid_channel's order (:639-655): per axis d and parameter, a float64 sum of gr_m[..., d] dAff[i][d];
    # its per-voxel products kept in float64
    id_x = N.affine_grid(torch.eye(4, dtype=torch.float64), dim)
    gr = gr3.double() * diff.double()[..., None]
    lkp = [[0, 3, 4], [3, 1, 5], [4, 5, 2]]
    g64 = gr3.double()
    hes = torch.stack([g64[..., 0] ** 2, g64[..., 1] ** 2, g64[..., 2] ** 2, g64[..., 0] * g64[..., 1],
                       g64[..., 0] * g64[..., 2], g64[..., 1] * g64[..., 2]], -1)
    if c is not None:
        hes = hes * c.double()[..., None]
    Dd = D.double()
    dAff = [[Dd[i, d, 0] * id_x[..., 0] + Dd[i, d, 1] * id_x[..., 1] + Dd[i, d, 2] * id_x[..., 2] + Dd[i, d, 3]
             for d in range(3)] for i in range(6)]
    grad = [sum(torch.sum(gr[..., d] * dAff[i][d]).item() for d in range(3)) for i in range(6)]
    H = np.zeros((6, 6))
    for d1 in range(3):
        for d2 in range(3):
            for i1 in range(6):
                for i2 in range(i1, 6):
                    H[i1, i2] += torch.sum(hes[..., lkp[d1][d2]] * dAff[i1][d1] * dAff[i2][d2]).item()
    oracle = grad + [H[a, b] for a in range(6) for b in range(a, 6)]
    r = admm64.check_sums(oracle, ref, tol)
    assert r['ok'], r
    # one voxel's residual off by 1e-6 relative
    bad_diff = diff.clone()
    bad_diff[6, 5, 3] *= 1 + 1e-6
    bad, _ = admm64.rigid_sums(gr3.numpy(), bad_diff.numpy(), None if c is None else c.numpy(), D.numpy())
    assert not admm64.check_sums(bad, ref, tol)['ok']


@pytest.mark.parametrize('geom', ['int_shift', 'rotated'])
def test_clean_fov_reference_matches_the_oracle_restatement(geom):
    from tests.helpers import rigid_matrix
    dim_y, dim_x = (23, 19, 30), (20, 17, 10)
    if geom == 'int_shift':
        M = torch.tensor([[1.0, 0, 0, -2.0], [0, 1.0, 0, 1.0], [0, 0, 0.5, -3.0], [0, 0, 0, 1]], dtype=torch.float64)
    else:
        M = rigid_matrix([1.5, -0.7, -4.0], [0.1, -0.05, 0.2]) @ torch.diag(
            torch.tensor([1.0, 1.0, 1 / 3, 1.0], dtype=torch.float64))
    y = (torch.rand(dim_y, generator=torch.Generator().manual_seed(2)) + 0.5).float()
    out, tie = admm64.clean_fov(y.numpy(), M[:3].numpy(), dim_x)
    # test_gpu_path's restatement of run.py:150-164 (float32 affine_grid)
    gg = N.affine_grid(M.float(), dim_y)
    keep = torch.ones(dim_y, dtype=torch.bool)
    for d in range(3):
        keep &= (gg[..., d] >= 0) & (gg[..., d] < dim_x[d])
    ref = torch.where(keep, y, torch.zeros_like(y)).numpy()
    assert 0 < int(keep.sum()) < keep.numel()
    assert np.array_equal(out[~tie], ref[~tie])
    if geom == 'int_shift':
        assert not tie.any()
        # voxels exactly on a threshold: 0 is kept, dim_x is not
        assert out[2, 0, 6] == y[2, 0, 6] and out[22, 0, 6] == 0.0 and out[2, 0, 26] == 0.0
    else:
        assert int(tie.sum()) < 0.01 * tie.size


def _grad_affines():
    from tests.test_gpu_ops import _affines
    return _affines()


@pytest.mark.parametrize('name', ['int_shift', 'thick', 'small_rigid', 'big_rigid'])
def test_pull_grad_bound_is_sound_and_sees_one_voxel(name):
    M = _grad_affines()[name]
    sdim, gdim = (12, 10, 9), (11, 12, 10)
    src = torch.rand(sdim, generator=torch.Generator().manual_seed(1))
    ref, tol, tie = admm64.pull_grad(src.numpy(), M[:3].numpy(), gdim)
    # the oracle's grid_grad on its float32 grid
    oracle = N.grid_grad(src[None, None], N.affine_grid(M.float(), gdim)[None])[0, 0].numpy()
    keep = ~tie[..., None]
    err = np.abs(oracle.astype(np.float64) - ref)
    assert not ((err > tol) & keep).any(), (name, float((err / np.maximum(tol, 1e-300) * keep).max()))
    assert int(tie.sum()) < 0.05 * tie.size
    if name in ('int_shift', 'thick'):
        assert not tie.any()  # (rows computed exactly: every coordinate on an integer plane is tested as it is)
    # one voxel's derivative off by 10x its tolerance (or by 1e-6 where the bound is 0)
    v = tuple(int(i) for i in np.argwhere((ref != 0) & keep)[len(np.argwhere((ref != 0) & keep)) // 2])
    bad = ref.copy()
    bad[v] += max(10 * tol[v], 1e-6)
    assert ((np.abs(bad - ref) > tol) & keep).sum() == 1
