"""The ADMM and Gauss-Newton kernels of admm.hip, per voxel or per sum, against the float64 references and bounds of
tests/admm64.py, in process: k_jtv_scale / k_zw_update (the shrinkage image s, z and w), unires_nll_prior,
k_masked_sse, k_scaling_sums, k_rigid_sums, k_clean_fov and k_pull_grad (grid_grad).  Every output the kernels
write (z, w, the shrinkage image, y, the gradients, the float64 sums) lies inside a buffer padded with sentinels on
both sides; nothing outside may change, and the outputs that start as sentinels must all be written.

The shapes are those where the kernels' index arithmetic turns: partial 64 x 4 (z, y) patches; jtv_grid's x slots
fewer than d.x (50 x 200 x 130: 3 x 50 patches, 27 slots) and a single slot (2 x 1100 x 1000: 16 x 275 patches);
1 to 4 channels compiled in, 5 - 8 in the generic form, 9 and 17 as chained launches carrying the running sum of
squares; alpha != 1 reading the old z in place; k_masked_sse's lanes at 1, 255 - 257 terms and beyond one stride
(131 072); k_scaling_sums' carry arithmetic, which only walks past 1024 x 256 voxels (300 001 and 2 x 3 x 50 000
along z, 600 x 600 x 1 in planes of one row, 300 x 3 x 301), and a volume below one workgroup; k_rigid_sums'
(i, j, k) decomposition past one 512 x 256 stride (96 x 90 x 102).

Observed on an MI355X (largest err / tol over the case; no tie excluded anywhere): z / w / s and the prior term
0.107 (37 x 41 x 53), 0.100 (3 x 5 x 130, 1 x 17 x 65), 0.093 (9 x 1 x 64), 0.061 (9 x 7 x 1), 0.124 / 0.078
(50 x 200 x 130, C 3 / 9), 0.090 / 0.083 (2 x 1100 x 1000, C 3 / 9); masked_sse 0 (exact) up to 257 terms, 0.061,
0.038, 0.027 beyond; scaling_sums 0 - 0.058; rigid_sums 0.005 - 0.010; clean_fov bit-exact with 0 ties in all
three geometries (the rotated one has no float64 coordinate within its rounding band of a threshold); grid_grad
0 (exact) with the integer affines, 0.259 - 0.609 with the rotations, 0 - 5 ties per case.  No case failed: the
suite found no kernel bug.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import admm64
from tests.helpers import rigid_matrix

pytestmark = pytest.mark.gpu

SENT = -7.75e37  # sentinel of the guard pads
U64 = 2.0 ** -53
PAD = 4096
RHO = 0.37
VX = {'iso': (1.0, 1.0, 1.0), 'aniso': (0.8, 1.25, 2.0)}


def _padded(t, dev, dtype=torch.float32):
    """A device buffer [PAD sentinels | t | PAD sentinels] and the view of t in it."""
    t = t.reshape(-1).to(dtype)
    buf = torch.full((2 * PAD + t.numel(),), SENT, dtype=dtype, device=dev)
    buf[PAD:PAD + t.numel()] = t.to(dev)
    return buf, buf[PAD:PAD + t.numel()]


def _guard_ok(buf, n):
    buf = buf.cpu()
    s = torch.full((PAD,), SENT, dtype=buf.dtype)
    return torch.equal(buf[:PAD], s) and torch.equal(buf[PAD + n:], s)


def _lib():
    from unires_amd import _lib as L
    return L.load()


def _run_zw(dev, ys, lam, vx, alpha, z, w):
    from unires_amd._lib import check, f3, i3
    from unires_amd._ops import _ptr, _stream
    Cn = len(lam)
    dim = tuple(ys.shape[1:])
    yd = [ys[c].contiguous().to(dev) for c in range(Cn)]
    ptrs = (C.c_void_p * Cn)(*[t.data_ptr() for t in yd])
    lams = (C.c_float * Cn)(*lam)
    zb, zv = _padded(z, dev)
    wb, wv = _padded(w, dev)
    jb, jv = _padded(torch.full(dim, SENT), dev)  # (every voxel of s must be written)
    nb, nv = _padded(torch.zeros(1, dtype=torch.float64), dev, torch.float64)
    lib = _lib()
    with torch.cuda.device(dev):
        check(lib.unires_zw_update(ptrs, lams, Cn, i3(dim), f3(vx), float(RHO), float(alpha), _ptr(zv), _ptr(wv),
                                   _ptr(jv), _stream()))
        check(lib.unires_nll_prior(ptrs, lams, Cn, i3(dim), f3(vx), _ptr(nv), _stream()))
    torch.cuda.synchronize(dev)
    for b, n in ((zb, z.numel()), (wb, w.numel()), (jb, int(np.prod(dim))), (nb, 1)):
        assert _guard_ok(b, n)
    return (jv.cpu().numpy().reshape(dim), zv.cpu().numpy().reshape(z.shape), wv.cpu().numpy().reshape(w.shape),
            float(nv.cpu()[0]))


def _zw_case(dev, dim, Cn, alpha, vx):
    ys, lam, z, w = admm64.zw_inputs(dim, Cn, RHO, alpha, vx=VX[vx])
    s, zo, wo, nll = _run_zw(dev, ys, lam, VX[vx], alpha, z, w)
    B = admm64.zw_update(ys.numpy(), lam, VX[vx], RHO, alpha, z.numpy(), w.numpy())

    def check(key, out, ref, tol):
        err = np.abs(out.astype(np.float64) - ref)
        bad = err > tol  # (a voxel left at the sentinel is off by 7.75e37)
        assert not bad.any(), (dim, Cn, alpha, vx, key, tuple(int(i) for i in np.argwhere(bad)[0]), int(bad.sum()))
        return float((err / np.maximum(tol, 1e-300)).max())

    worst = check('s', s, *B['s'])
    for c in range(Cn):
        Bc = B['chan'](c)
        worst = max(worst, check('z%d' % c, zo[c], *Bc['z']), check('w%d' % c, wo[c], *Bc['w']))
    ref, tol = admm64.nll_prior(ys.numpy(), lam, VX[vx])
    assert abs(nll - ref) <= tol, (dim, Cn, 'nll', nll, ref, tol)
    return max(worst, abs(nll - ref) / tol)


TAIL_SHAPES = [(37, 41, 53), (3, 5, 130), (1, 17, 65), (9, 1, 64), (9, 7, 1)]


@pytest.mark.parametrize('dim', TAIL_SHAPES)
def test_zw_update_and_nll_prior_per_voxel_at_tail_shapes(dev, dim):
    """Every channel count 1, 2, 3, 4, 5, 8, 9, 17 and alpha 1, 1.5, 0.7, isotropic and (0.8, 1.25, 2.0) voxels in
    turn."""
    worst = 0.0
    for i, Cn in enumerate((1, 2, 3, 4, 5, 8, 9, 17)):
        for j, alpha in enumerate((1.0, 1.5, 0.7)):
            worst = max(worst, _zw_case(dev, dim, Cn, alpha, 'aniso' if (i + j) % 2 else 'iso'))
    print('zw %s: max err/tol %.3f' % (dim, worst), flush=True)


@pytest.mark.parametrize('dim,Cn,alpha', [((50, 200, 130), 3, 1.0), ((50, 200, 130), 9, 0.7),
                                          ((2, 1100, 1000), 3, 1.5), ((2, 1100, 1000), 9, 1.0)])
def test_zw_update_and_nll_prior_per_voxel_across_x_slots(dev, dim, Cn, alpha):
    """jtv_grid with fewer x slots than d.x (50 x 200 x 130) and with one slot (2 x 1100 x 1000).  The launch is
    host code (admm.hip ``jtv_grid``, used by launch_jtv_scale) that no entry point reports: admm64.jtv_grid restates
    it, and must follow it when it changes."""
    tz, ty, gx = admm64.jtv_grid(dim)
    assert gx < dim[0] if dim[0] == 50 else gx == 1
    print('zw %s C %d alpha %.1f: max err/tol %.3f' % (dim, Cn, alpha, _zw_case(dev, dim, Cn, alpha, 'aniso')),
          flush=True)


def _sums_out(dev, k):
    return _padded(torch.zeros(k, dtype=torch.float64), dev, torch.float64)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 131073, 512 * 256 * 3 + 17, 256 * 256 * 42])
def test_masked_sse_exact_terms(dev, n):
    from unires_amd._lib import check
    from unires_amd._ops import _ptr, _stream
    g = torch.Generator().manual_seed(n % 1000)
    x = (torch.rand(n, generator=g) * 100 - 20).float()
    ay = (torch.rand(n, generator=g) * 100 - 20).float()
    x[::7] = 0.0
    x[3::11] = -0.0
    if n == 1:
        x[0] = 3.5
    ob, ov = _sums_out(dev, 1)
    xd, ad = x.to(dev), ay.to(dev)
    with torch.cuda.device(dev):
        check(_lib().unires_masked_sse(_ptr(xd), _ptr(ad), n, _ptr(ov), _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(ob, 1)
    ref, tol = admm64.masked_sse(x.numpy(), ay.numpy())
    out = float(ov.cpu()[0])
    assert abs(out - ref) <= tol, (n, out, ref, tol)
    print('masked_sse %d: err/tol %.3f' % (n, abs(out - ref) / tol), flush=True)


SCALING_SHAPES = [(67, 45, 91), (1, 1, 300001), (600, 600, 1), (2, 3, 50000), (300, 3, 301), (5, 7, 6)]


@pytest.mark.parametrize('dim', SCALING_SHAPES)
def test_scaling_sums_exact_terms(dev, dim):
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    g = torch.Generator().manual_seed(sum(dim))
    x = (torch.rand(dim, generator=g) * 10).float()
    x[x < 1.5] = 0.0
    x.view(-1)[5::13] = -0.0
    ay = (torch.rand(dim, generator=g) * 10 - 1).float()
    xd, ad = x.to(dev), ay.to(dev)
    for dim_thick in (0, 1, 2):
        ob, ov = _sums_out(dev, 5)
        with torch.cuda.device(dev):
            check(_lib().unires_scaling_sums(_ptr(xd), _ptr(ad), i3(dim), dim_thick, _ptr(ov), _stream()))
        torch.cuda.synchronize(dev)
        assert _guard_ok(ob, 5)
        out = ov.cpu().tolist()
        ref, tol = admm64.scaling_sums(x.numpy(), ay.numpy(), dim_thick)
        r = admm64.check_sums(out, ref, tol)
        assert r['ok'], (dim, dim_thick, r)
        # even + odd = all, against totals formed without the parity split: nothing lost or counted twice
        tot, ttol = admm64.scaling_totals(x.numpy(), ay.numpy())
        for k, (e, o) in enumerate(((1, 2), (3, 4))):
            assert abs(out[e] + out[o] - tot[k]) <= ttol[k] + U64 * (abs(out[e]) + abs(out[o])), (dim, dim_thick, k)
        print('scaling_sums %s dim_thick %d: max err/tol %.3f' % (dim, dim_thick, r['max_ratio']), flush=True)


@pytest.mark.parametrize('dim', [(13, 11, 7), (70, 66, 31), (96, 90, 102)])
@pytest.mark.parametrize('ctc', [False, True])
def test_rigid_sums_float64(dev, dim, ctc):
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    g = torch.Generator().manual_seed(dim[0] + ctc)
    gr3 = torch.randn(dim + (3,), generator=g).float()
    diff = torch.randn(dim, generator=g).float()
    c = (torch.rand(dim, generator=g) + 0.5).float() if ctc else None
    D = (torch.randn((6, 3, 4), generator=g) * 0.1).float()
    d72 = (C.c_float * 72)(*D.reshape(-1).tolist())
    gd, dd = gr3.to(dev), diff.to(dev)
    cd = c.to(dev) if ctc else None
    ob, ov = _sums_out(dev, 27)
    with torch.cuda.device(dev):
        check(_lib().unires_rigid_sums(_ptr(gd), _ptr(dd), _ptr(cd) if ctc else None, i3(dim), d72, _ptr(ov),
                                       _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(ob, 27)
    ref, tol = admm64.rigid_sums(gr3.numpy(), diff.numpy(), None if c is None else c.numpy(), D.numpy())
    r = admm64.check_sums(ov.cpu().tolist(), ref, tol)
    assert r['ok'], (dim, ctc, r)
    print('rigid_sums %s ctc %d: max err/tol %.3f' % (dim, ctc, r['max_ratio']), flush=True)


def _clean_fov_geoms():
    return {
        # every coordinate an exact float32 value: voxels land exactly on 0 and on dim_x
        'int_shift': (torch.tensor([[1.0, 0, 0, -2.0], [0, 1.0, 0, 1.0], [0, 0, 0.5, -3.0]], dtype=torch.float64),
                      (23, 19, 30), (20, 17, 10)),
        'int_perm': (torch.tensor([[0, 1.0, 0, -3.0], [0, 0, -1.0, 40.0], [2.0, 0, 0, -5.0]], dtype=torch.float64),
                     (31, 70, 65), (60, 33, 50)),
        'rotated': ((rigid_matrix([1.5, -0.7, -4.0], [0.1, -0.05, 0.2]) @ torch.diag(
            torch.tensor([1.0, 1.0, 1 / 3, 1.0], dtype=torch.float64)))[:3], (45, 70, 131), (40, 66, 40)),
    }


@pytest.mark.parametrize('geom', list(_clean_fov_geoms()))
def test_clean_fov_exact_outside_ties(dev, geom):
    from unires_amd import _lib as L
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    M, dim_y, dim_x = _clean_fov_geoms()[geom]
    y = (torch.rand(dim_y, generator=torch.Generator().manual_seed(2)) + 0.5).float()
    yb, yv = _padded(y, dev)
    n = y.numel()
    with torch.cuda.device(dev):
        check(_lib().unires_clean_fov(_ptr(yv), i3(dim_y), L.c_f32x12(*M.float().reshape(-1).tolist()), i3(dim_x),
                                      _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(yb, n)
    out = yv.cpu().numpy().reshape(dim_y)
    ref, tie = admm64.clean_fov(y.numpy(), M.numpy(), dim_x)
    assert 0 < int((ref == 0).sum()) < n
    # bit for bit away from ties: 0.0 where outside, the input's bits where inside
    same = out.view(np.int32) == ref.view(np.int32)
    assert same[~tie].all(), (geom, tuple(int(i) for i in np.argwhere(~same & ~tie)[0]))
    assert np.all((out[tie] == 0) | (out[tie].view(np.int32) == y.numpy()[tie].view(np.int32)))
    if geom.startswith('int'):
        assert not tie.any()
    else:
        assert int(tie.sum()) < 0.01 * n
    print('clean_fov %s: %d ties of %d' % (geom, int(tie.sum()), n), flush=True)


def _grad_affines():
    from tests.test_gpu_ops import _affines
    return _affines()


@pytest.mark.parametrize('sdim,gdim', [((12, 10, 9), (11, 12, 10)), ((5, 70, 131), (6, 66, 140)),
                                       ((1, 1, 1), (2, 3, 4)), ((4, 3, 1), (9, 5, 65))])
def test_grid_grad_per_voxel(dev, sdim, gdim):
    """k_pull_grad (spatial.grid_grad) with the affines of test_gpu_ops: partial 64 x 4 (z, y) tiles of the grid,
    single-slice sources (no z pair to load); every coordinate on integer planes where the affine is exact."""
    from unires_amd._lib import check, f12, i3
    from unires_amd._ops import _ptr, _stream
    src = torch.rand(sdim, generator=torch.Generator().manual_seed(1))
    sd = src.to(dev)
    n = int(np.prod(gdim)) * 3
    for name, M in _grad_affines().items():
        ob, ov = _padded(torch.full((n,), SENT), dev)
        with torch.cuda.device(dev):
            check(_lib().unires_pull_grad3d_affine(_ptr(sd), i3(sdim), f12(M[:3].float().reshape(-1).tolist()),
                                                   _ptr(ov), i3(gdim), 0.05, _stream()))
        torch.cuda.synchronize(dev)
        assert _guard_ok(ob, n), name
        out = ov.cpu().numpy().reshape(tuple(gdim) + (3,)).astype(np.float64)
        ref, tol, tie = admm64.pull_grad(src.numpy(), M[:3].numpy(), gdim)
        err = np.abs(out - ref)
        bad = (err > tol) & ~tie[..., None]
        assert not bad.any(), (sdim, gdim, name, tuple(int(i) for i in np.argwhere(bad)[0]), int(bad.sum()))
        # tie voxels: still written (the sentinel is far from any gradient of values in [0, 1))
        assert np.all(np.abs(out) < 10.0), name
        print('grid_grad %s -> %s %s: max err/tol %.3f, %d ties' % (
            sdim, gdim, name, float((err / np.maximum(tol, 1e-300) * ~tie[..., None]).max()), int(tie.sum())),
            flush=True)
