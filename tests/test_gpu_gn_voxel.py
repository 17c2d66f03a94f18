"""The voxel weights in the scaling and rigid Gauss-Newton updates on the GPU, in process, with
``sett.voxel_gn`` on unless a test says otherwise:

(1) unires_scaling_sums_g against tests/gnv64.py's exact sums, at tests/test_gpu_gn_weights.py's shapes, slices along
    every axis, `pow2` and `ramp` maps, with and without slice weights; g = 1 the bits of unires_scaling_sums_w /
    unires_scaling_sums; g constant per slice the bits of unires_scaling_sums_w; g in {0, 1} the bits of the data with
    those voxels zeroed; two runs the same bits;
(2) unires_rigid_resid_g bit for bit against gnv64.rigid_resid_g32: out of place and on ay, with and without slice
    weights, each buffer in turn off its 16-byte boundary, x and g unchanged, nothing written outside the output;
    g = 1 the bits of unires_rigid_resid;
(3) a voxel of weight 0 does not reach _update_scaling, _update_rigid or a fit() that runs both: clean data and data
    with a 12 x 3 x 12 box multiplied by 0.3 give the same bits; with the switch off the map is ignored;
(4) g = 1 through both updates: the bits of the unweighted path, or of the slice-weighted one; the rigid objective is
    _compute_nll's; a repeat whose map is all zero is left alone; fit() with every switch on runs, repeats bit for bit
    and returns the Huber weights of the residuals its last iteration saw;
(5) planted motion with a corrupted box: the update with the box at weight 0 ends nearer the planted matrix.

Every output of (1) and (2) lies inside a buffer padded with sentinels on both sides.

Observed on an MI355X: (1) worst err / tol 0.082 over the 60 cases; (2) bit-exact; (3) from the identity the phantom was
made with, the rigid line search of fit() keeps the identity, so the fit() arms start the second repeat from OFFSET;
(4) ll at g = 1 without slice weights: error 0; every switch on: 0 weights differ from the rule, 0.988 / 0.986 of them
exactly 1; (5) distances 0.1321 with the map, 0.1322 without, 1.0004 at the start - the box barely moves this registration.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import admm64, gn64, gnv64, slice64, voxel64
from tests.helpers import rigid_matrix
from tests.test_gpu_admm64 import PAD, SENT, _guard_ok, _lib, _padded, _sums_out
from tests.test_gpu_gn_weights import (OFFSET, RESID_SHAPES, SCALING_SHAPES, _phantom, _resid, _resid_inputs, _rigid_state,
                                       _same_state, _scaling, _scl, same_bits)

pytestmark = pytest.mark.gpu

BOX = ((10, 22), (5, 8), (14, 26))  # of the second repeat, (48, 16, 40): 12 x 3 x 12, three of its 16 slices, none whole
BOX_SL = tuple(slice(a, b) for a, b in BOX)


# ---- (1) the five sums --------------------------------------------------------------------------------------------------
def _scaling_g(dev, xd, ad, dim, dim_thick, gd, ud):
    """unires_scaling_sums_g into a guarded buffer -> (5,) float64."""
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    ob, ov = _sums_out(dev, 5)
    ob[PAD:PAD + 5] = SENT  # (every one of the five must be written)
    with torch.cuda.device(dev):
        check(_lib().unires_scaling_sums_g(_ptr(xd), _ptr(ad), i3(dim), dim_thick, _ptr(gd),
                                           None if ud is None else _ptr(ud), _ptr(ov), _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(ob, 5)
    return ov.cpu().clone()


@pytest.mark.parametrize('dim', SCALING_SHAPES)
def test_scaling_sums_g_exact_terms(dev, dim):
    gen = torch.Generator().manual_seed(sum(dim))
    x = (torch.rand(dim, generator=gen) * 10).float()
    x[x < 1.5] = 0.0
    x.view(-1)[5::13] = -0.0
    ay = (torch.rand(dim, generator=gen) * 10 - 1).float()
    xd, ad = x.to(dev), ay.to(dev)
    ones = torch.ones(dim, device=dev)
    worst = 0.0
    for dim_thick in (0, 1, 2):
        S = dim[dim_thick]
        u = slice64.weights(S, 'ramp', seed=3)
        ud = u.to(dev)
        for pattern in ('pow2', 'ramp'):
            g = voxel64.weights(dim, pattern)
            gd = g.to(dev)
            for uu, uud in ((None, None), (u, ud)):
                out = _scaling_g(dev, xd, ad, dim, dim_thick, gd, uud)
                ref, tol = gnv64.scaling_sums_g(x.numpy(), ay.numpy(), dim_thick, g.numpy(), None if uu is None else uu.numpy())
                r = admm64.check_sums(out.tolist(), ref, tol)
                worst = max(worst, r['max_ratio'])
                print('scaling_sums_g %s dim_thick %d %s u %d: max err/tol %.3f' % (dim, dim_thick, pattern, uu is not None,
                                                                                     r['max_ratio']), flush=True)
                assert r['ok'], (dim, dim_thick, pattern, uu is not None, r)
                assert same_bits(out, _scaling_g(dev, xd, ad, dim, dim_thick, gd, uud))  # the same bits every run
        # g = 1: the slice-weighted and the unweighted kernels' bits
        assert same_bits(_scaling_g(dev, xd, ad, dim, dim_thick, ones, ud), _scaling(dev, xd, ad, dim, dim_thick, ud))
        assert same_bits(_scaling_g(dev, xd, ad, dim, dim_thick, ones, None), _scaling(dev, xd, ad, dim, dim_thick, None))
        # g constant on every slice: the slice-weighted kernel's bits with those constants
        spread = slice64.spread(u, dim, dim_thick).float().contiguous().to(dev)
        assert same_bits(_scaling_g(dev, xd, ad, dim, dim_thick, spread, None), _scaling(dev, xd, ad, dim, dim_thick, ud))
        # g in {0, 1}: the data without those voxels, through the unweighted kernel
        g01 = (voxel64.weights(dim, 'pow2') >= 0.5).float()
        xz = torch.where(g01 == 0, torch.zeros(()), x)
        assert same_bits(_scaling_g(dev, xd, ad, dim, dim_thick, g01.to(dev), None),
                         _scaling(dev, xz.to(dev), ad, dim, dim_thick, None))
    print('scaling_sums_g %s: worst err/tol %.3f' % (dim, worst), flush=True)


# ---- (2) the residual ---------------------------------------------------------------------------------------------------
def _resid_g(dev, x, ay, g, dim, axis, u, inplace, off=(0, 0, 0, 0)):
    """unires_rigid_resid_g into a guarded buffer (ay's own when ``inplace``); ``off``: floats past a 16-byte boundary
    the views of x, ay, g and out start at (in place out is ay: its offset) -> the output on the CPU."""
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    n = x.numel()
    ox, oa, og, oo = off
    if inplace:
        oo = oa

    def view(t, o):
        b, v = _padded(torch.cat([torch.zeros(o), t.reshape(-1)]), dev)
        assert v[o:].data_ptr() % 16 == 4 * o % 16
        return b, v[o:]

    xb, xv = view(x, ox)
    ab, av = view(ay, oa)
    gb, gv = view(g, og)
    ob, ov = (ab, av) if inplace else view(torch.full((n,), SENT), oo)
    x0, g0 = xv.clone(), gv.clone()
    ud = None if u is None else u.to(dev)
    with torch.cuda.device(dev):
        check(_lib().unires_rigid_resid_g(_ptr(xv), _ptr(av), _ptr(gv), i3(dim), axis, None if ud is None else _ptr(ud),
                                          _ptr(ov), _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(ob, n + oo) and bool((ob[PAD:PAD + oo] == 0).all())
    assert _guard_ok(xb, n + ox) and _guard_ok(gb, n + og) and _guard_ok(ab, n + oa)
    assert same_bits(xv, x0) and same_bits(gv, g0)  # x and g are only read
    if not inplace:
        assert same_bits(av, ay.reshape(-1).to(dev))
    return ov.cpu().reshape(dim)


@pytest.mark.parametrize('dim', RESID_SHAPES + [(1, 1, 3)])
def test_rigid_resid_g_bit_for_bit(dev, dim):
    x, ay = _resid_inputs(dim)
    g = voxel64.weights(dim, 'ramp')
    ones = torch.ones(dim)
    for axis in (0, 1, 2):
        for u in (None, slice64.weights(dim[axis], 'ramp', seed=3)):
            un = None if u is None else u.numpy()
            want = torch.from_numpy(gnv64.rigid_resid_g32(x.numpy(), ay.numpy(), axis, g.numpy(), un))
            for inplace in (False, True):
                got = _resid_g(dev, x, ay, g, dim, axis, u, inplace)
                assert same_bits(got, want), (dim, axis, u is not None, inplace)
            # g = 1: the slice-weighted kernel's bits with the same u
            assert same_bits(_resid_g(dev, x, ay, ones, dim, axis, u, False), _resid(dev, x, ay, dim, axis, u, False))
    # planted exact zeros of x and ay give +0, whatever the weight's sign bit would make of them
    masked = ((x == 0) | (ay == 0)).numpy()
    assert masked.any() or x.numel() < 30  # (_resid_inputs plants them from the third voxel on)
    assert (want.numpy()[masked].view(np.uint32) == 0).all()
    assert (got.numpy()[masked].view(np.uint32) == 0).all()


@pytest.mark.parametrize('which', ['x', 'ay', 'g', 'out'])
def test_rigid_resid_g_off_a_16_byte_boundary(dev, which):
    dim = (41, 38, 60)
    x, ay = _resid_inputs(dim)
    g = voxel64.weights(dim, 'ramp')
    off = tuple(int(which == name) for name in ('x', 'ay', 'g', 'out'))
    for axis, u in ((1, slice64.weights(dim[1], 'ramp')), (2, None)):
        want = torch.from_numpy(gnv64.rigid_resid_g32(x.numpy(), ay.numpy(), axis, g.numpy(), None if u is None else u.numpy()))
        for inplace in ((False,) if which == 'out' else (False, True)):
            assert same_bits(_resid_g(dev, x, ay, g, dim, axis, u, inplace, off), want), (which, axis, inplace)


# ---- (3) zero-weight voxels are not read -------------------------------------------------------------------------------------
def _arm(dev, corrupt, weights, start=None, gn=True):
    """Fresh structs of DESIGN.md 8.6's phantom; the box of the second repeat multiplied by 0.3 (``corrupt``: sign and
    non-zeroness stay) and given weight 0 by a map (``weights``); ``sett.voxel_gn`` = ``gn``.  ``start``: the second
    repeat's rigid_q (and po.rigid) instead of the identity the phantom was made with."""
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _expm, affine_basis
    prob, (xg, yg, sett) = _phantom(dev)
    x1 = xg[0][1]
    assert tuple(x1.dat.shape) == (48, 16, 40) and _slice_axis(x1) == 1
    if corrupt:
        x1.dat[BOX_SL] *= 0.3
    if weights:
        x1.weight = torch.from_numpy(gnv64.box_weights(x1.dat.shape, BOX)).to(dev)
    sett.voxel_gn = gn
    for xn in xg[0]:
        xn.rigid_q = torch.zeros(6, dtype=torch.float64)
    if start is not None:
        x1.rigid_q = torch.tensor(start, dtype=torch.float64)
        x1.po.rigid = _expm(x1.rigid_q, affine_basis('SE'))
    return prob, xg, yg, sett


ARMS = (('clean', False, True, True), ('corrupt', True, True, True), ('unweighted', True, False, True),
        ('off', True, True, False))


def test_update_scaling_does_not_read_zero_weight_voxels(dev):
    from unires_amd._update import _update_scaling
    res = {}
    for name, corrupt, weights, gn in ARMS:
        _, xg, yg, sett = _arm(dev, corrupt, weights, gn=gn)
        xg, sll = _update_scaling(xg, yg, sett, max_niter_gn=1, num_linesearch=6)
        res[name] = (_scl(xg), float(sll))
        print('scaling, %s: scl %s sll %r' % (name, res[name][0], res[name][1]), flush=True)
    i64 = lambda v: np.array(v, dtype=np.float64).view(np.int64)
    assert np.array_equal(i64(res['clean'][0]), i64(res['corrupt'][0])) and i64(res['clean'][1]) == i64(res['corrupt'][1])
    assert all(v != 0.0 for v in res['clean'][0])  # (a step was taken)
    assert res['unweighted'][0][1] != res['corrupt'][0][1] and res['unweighted'][1] != res['corrupt'][1]
    assert res['unweighted'][0][0] == res['corrupt'][0][0]  # (the clean repeat's step does not depend on the other)
    # the switch off: the map is ignored, bit for bit
    assert np.array_equal(i64(res['off'][0]), i64(res['unweighted'][0])) and i64(res['off'][1]) == i64(res['unweighted'][1])


@pytest.mark.parametrize('samp', [0, 1])
@pytest.mark.parametrize('mean_correct', [False, True])
@pytest.mark.parametrize('start', [None, OFFSET])
def test_update_rigid_does_not_read_zero_weight_voxels(dev, samp, mean_correct, start):
    """From the identity the phantom was made with, where the line search may keep the identity and only sll tells the
    arms apart, and from tests/test_gpu_gn_weights.py's start half a voxel and 0.02 rad off, where a step is taken."""
    from unires_amd._rigid import _update_rigid
    res = {}
    for name, corrupt, weights, gn in ARMS[:3]:
        _, xg, yg, sett = _arm(dev, corrupt, weights, start=start, gn=gn)
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=mean_correct, max_niter_gn=1, num_linesearch=4, samp=samp)
        res[name] = _rigid_state(xg, sll)
        print('rigid samp %d mean_correct %d, %s: q[1] %s sll %r' % (samp, mean_correct, name,
              ['%.3e' % v for v in res[name][0][1].tolist()], float(sll)), flush=True)
    assert _same_state(res['clean'], res['corrupt'])
    assert not same_bits(res['unweighted'][2], res['corrupt'][2])
    if start is not None:
        q0 = torch.tensor(start, dtype=torch.float64)
        if mean_correct:
            q0 = q0 / 2  # (had no step been taken: the mean of 0 and the start taken off)
        assert not same_bits(res['clean'][0][1], q0)  # (a step was taken)
        assert not same_bits(res['unweighted'][0][1], res['corrupt'][0][1])
        assert not same_bits(res['unweighted'][1][1], res['corrupt'][1][1])


def test_update_rigid_decimates_the_map_with_the_observation(dev):
    """samp = 6 decimates the second repeat by (6, 2, 6): of the box the voxels (12, 18) x (6) x (18, 24) remain - 2, 3 x
    3 x 3, 4 of the decimated observation - with the weights g[::6, ::2, ::6] cut to dim_x.  With the switch off the
    map is ignored."""
    from unires_amd._rigid import _update_rigid
    res = {}
    for name, corrupt, weights, gn in ARMS:
        _, xg, yg, sett = _arm(dev, corrupt, weights, start=OFFSET, gn=gn)
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=6)
        res[name] = _rigid_state(xg, sll)
    assert _same_state(res['clean'], res['corrupt'])
    assert not same_bits(res['unweighted'][0][1], res['corrupt'][0][1])
    assert _same_state(res['off'], res['unweighted'])


def test_update_rigid_in_the_denoising_regime_does_not_read_zero_weight_voxels(dev):
    """Pull / push only: the Hessian's weight is the map itself where the unweighted step passes none."""
    from tests.helpers import gpu_structs, make_problem
    from unires_amd._rigid import _update_rigid
    box = ((4, 10), (5, 8), (10, 20))
    res = {}
    for name, corrupt, weights, gn in ARMS[:3]:
        prob = make_problem(dim_y=(20, 18, 33), n_channels=1, regime='dn', rot=0.08, trans=1.5, seed=1)
        xg, yg, sett = gpu_structs(prob, dev)
        sett.voxel_gn = gn
        xn = xg[0][0]
        if corrupt:
            xn.dat[tuple(slice(a, b) for a, b in box)] *= 0.3
        if weights:
            xn.weight = torch.from_numpy(gnv64.box_weights(xn.dat.shape, box)).to(dev)
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
        res[name] = _rigid_state(xg, sll)
    assert _same_state(res['clean'], res['corrupt'])
    assert not same_bits(res['unweighted'][2], res['corrupt'][2])


def _fit_arm(dev, corrupt, gn):
    import unires_amd as U
    _, xg, yg, sett = _arm(dev, corrupt, True, start=OFFSET)
    yg[0].lam0 = float(yg[0].lam) / 4.0
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 4, 1e-4, 4.0, 0
    sett.cgs_max_iter, sett.cgs_tol = 5, 0.0
    sett.clean_fov = False
    sett.scaling = sett.unified_rigid = gn
    sett.rigid_mod = 1
    dat, _, R, info = U.fit(xg, yg, sett)
    torch.cuda.synchronize()
    assert info['n_iter'] == 4
    return dat.cpu(), R.clone(), torch.tensor(_scl(xg), dtype=torch.float64)


@pytest.mark.parametrize('gn', [False, True])
def test_fit_does_not_read_zero_weight_voxels(dev, gn):
    """fit(), 4 ADMM iterations of 5 CG iterations (cgs_tol = 0), a user map 0 on the box, sett.voxel_gn on; with both
    Gauss-Newton updates (scaling, and the rigid update every iteration) and, as the control, with neither.  The
    second repeat starts from tests/test_gpu_gn_weights.py's OFFSET: from the identity the phantom was made with the
    rigid line search of this fit keeps the identity (observed), and R would say nothing."""
    from unires_amd._rigid import _expm, affine_basis
    clean, corrupt = _fit_arm(dev, False, gn), _fit_arm(dev, True, gn)
    for a, b, name in zip(clean, corrupt, ('dat_y', 'R', 'scl')):
        assert same_bits(a, b), name
    R0 = _expm(torch.tensor(OFFSET, dtype=torch.float64), affine_basis('SE'))
    if gn:
        assert bool((clean[2] != 0).all()) and not torch.equal(clean[1][1], R0)  # (both updates took steps)
    else:
        assert bool((clean[2] == 0).all()) and torch.equal(clean[1][1], R0)


# ---- (4) unit maps, the objective, empty repeats, everything on ------------------------------------------------------------------
@pytest.mark.parametrize('with_u', [False, True])
def test_unit_map_gives_the_step_of_the_path_without_it(dev, with_u):
    """g = 1 beside no slice weights: the unweighted path's residual, Hessian weight, 27 sums and step, bit for bit, and ll
    inside _slice_ll's float64 bound; beside slice weights: the slice-weighted path's, ll included."""
    from unires_amd import _ops
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    from unires_amd._project import _taps
    from unires_amd._rigid import (_ctc, _expm, _grid_matrix, _rigid_terms, _spread, _update_rigid, _voxel_times,
                                   affine_basis)
    from unires_amd._update import _update_scaling
    from unires_amd.spatial import _m12
    _, xg, yg, sett = _arm(dev, True, False)
    xn, y = xg[0][1], yg[0].dat
    po, tau, a = xn.po, float(xn.tau), 1
    u = slice64.weights(16, 'ramp', seed=5).to(dev) if with_u else None
    ones = torch.ones(tuple(xn.dat.shape), device=dev)
    rigid = rigid_matrix((0.3, -0.2, 0.1), (0.01, -0.02, 0.015))
    with torch.cuda.device(dev):
        ll0, gr0, d0 = _rigid_terms(xn.dat, y, po, tau, rigid, sett, diff=True, slice_w=u, axis=a if with_u else None)
        ll1, gr1, d1 = _rigid_terms(xn.dat, y, po, tau, rigid, sett, diff=True, slice_w=u, axis=a, weight=ones)
        dim = tuple(po.dim_yx)
        c0 = _ctc(po, dim, dev, u, a) if with_u else _ctc(po, dim, dev)
        c1 = _ctc(po, dim, dev, u, a, weight=ones)
        assert same_bits(d0, d1) and same_bits(gr0, gr1) and same_bits(c0, c1)
        if with_u:  # (the denoising regime's Hessian weight: the volume g u against the spread u)
            assert same_bits(_voxel_times(torch.ones_like(ones), ones, u, a), _spread(u, ones.shape, a).contiguous())
        _, d_rigid = _expm(torch.zeros(6, dtype=torch.float64), affine_basis('SE'), grad_X=True)
        D = torch.stack([torch.linalg.solve(po.mat_y, d_rigid[i].mm(po.mat_yx)) for i in range(6)])
        d72 = (C.c_float * 72)(*D[:, :3, :].reshape(-1).float().tolist())
        sums = []
        for d, c in ((d0, c0), (d1, c1)):
            ob, ov = _sums_out(dev, 27)
            check(_lib().unires_rigid_sums(_ptr(gr0), _ptr(d), _ptr(c), i3(dim), d72, _ptr(ov), _stream()))
            torch.cuda.synchronize(dev)
            assert _guard_ok(ob, 27)
            sums.append(ov.cpu().clone())
        assert same_bits(sums[0], sums[1]) and bool((sums[0] != 0).all())
        mat, _ = _grid_matrix(po, rigid, sett.method)
        Ay = _ops.conv_down(_ops.pull_affine(y, _m12(mat), dim), _taps(po), po.ratio, float(po.scl), po.dim_thick)
        Ay = Ay.reshape(tuple(xn.dat.shape))
    if with_u:
        assert same_bits(ll0, ll1)  # (unires_voxel_sums at g = 1 has unires_slice_sums' bits: the same expression)
    else:
        xh, ah = xn.dat.cpu().numpy(), Ay.cpu().numpy()
        exact, _ = admm64.masked_sse(xh, ah)
        ref, tol = gn64.weighted_sse(xh, ah, a, np.ones(16, np.float32))
        assert abs(ref - exact) <= 2.0 ** -52 * exact
        err = abs(float(ll1) - 0.5 * tau * exact)
        bound = 0.5 * tau * tol + 2.0 ** -52 * 0.5 * tau * exact  # (the product with tau / 2 rounds once more)
        print('rigid ll at g = 1: err / bound %.3g (ll %r, unweighted %r)' % (err / bound, float(ll1), float(ll0)), flush=True)
        assert err <= bound
    # and whole updates: the same steps
    rig, scl = [], []
    for w in (False, True):
        for update in ('rigid', 'scaling'):
            _, xg, yg, sett = _arm(dev, True, False)
            x1 = xg[0][1]
            if with_u:
                x1.slice_w = u.clone()
            if w:
                x1.weight = torch.ones(tuple(x1.dat.shape), device=dev)
            if update == 'rigid':
                xg, _ = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=0, samp=0)
                rig.append(xg[0][1].rigid_q.clone())
            else:
                xg, sll = _update_scaling(xg, yg, sett, max_niter_gn=1, num_linesearch=6)
                scl.append(torch.tensor(_scl(xg) + [float(sll)], dtype=torch.float64))
    assert same_bits(rig[0], rig[1]) and bool((rig[0] != 0).any())
    assert same_bits(scl[0], scl[1]) and bool((scl[0] != 0).all())


def test_rigid_objective_is_the_objective_of_compute_nll(dev):
    """The second repeat with a map and slice weights, the first with a map alone: sum_n ll_n of the rigid step at
    po.rigid, added in _compute_nll's order, has the bits of its nll_xy - the same y, weights and rigid through the same
    expression (unires_voxel_sums, _update._slice_ll)."""
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _rigid_terms
    from unires_amd._update import _compute_nll, _gn_weight
    prob, xg, yg, sett = _arm(dev, True, True)
    xg[0][0].weight = voxel64.weights(xg[0][0].dat.shape, 'ramp').to(dev)
    xg[0][1].weight = voxel64.weights((48, 16, 40), 'ramp', seed=5).to(dev)
    xg[0][1].slice_w = slice64.weights(16, 'ramp', seed=5).to(dev)
    with torch.cuda.device(dev):
        nll_xy = _compute_nll(xg, yg, sett, prob['rho'])[1]
        ll = torch.zeros((), dtype=torch.float64, device=dev)
        for xn in xg[0]:
            ll = ll + _rigid_terms(xn.dat, yg[0].dat, xn.po, xn.tau, xn.po.rigid, sett, slice_w=getattr(xn, 'slice_w', None),
                                   axis=_slice_axis(xn), weight=_gn_weight(xn, sett))[0]
    print('rigid objective %r, nll_xy %r' % (float(ll), float(nll_xy)), flush=True)
    assert same_bits(ll, nll_xy)


def test_a_repeat_with_an_all_zero_map_is_left_alone(dev):
    from unires_amd._rigid import _update_rigid
    from unires_amd._update import _update_scaling
    for update in ('scaling', 'rigid'):
        got = {}
        for name in ('both', 'first'):
            _, xg, yg, sett = _arm(dev, False, False)
            x1 = xg[0][1]
            x1.weight = torch.zeros(tuple(x1.dat.shape), device=dev)
            scl1, q1, r1 = x1.po.scl, x1.rigid_q, x1.po.rigid
            if name == 'first':
                xg = [xg[0][:1]]
            if update == 'scaling':
                xg, sll = _update_scaling(xg, yg, sett, max_niter_gn=1, num_linesearch=6)
            else:
                xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
            assert x1.po.scl is scl1 and x1.rigid_q is q1 and x1.po.rigid is r1
            assert bool(torch.isfinite(sll))
            got[name] = (sll.cpu().clone(), float(xg[0][0].po.scl), xg[0][0].rigid_q.clone())
        assert same_bits(got['both'][0], got['first'][0])  # (the empty repeat adds 0 to sll)
        assert got['both'][1] == got['first'][1] and same_bits(got['both'][2], got['first'][2])


def _fit_everything(dev, monkeypatch):
    """fit() with voxel_robust, voxel_gn, scaling and unified_rigid on, the corrupted box and no map.  The Huber rule
    runs inside _update_admm, before the iteration's scaling and rigid updates: po.scl and po.rigid as the last
    _update_admm left them are recorded on the way."""
    import unires_amd as U
    from unires_amd import run
    _, xg, yg, sett = _arm(dev, True, False)
    yg[0].lam0 = float(yg[0].lam) / 4.0
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 4, 1e-4, 4.0, 0
    sett.cgs_max_iter, sett.cgs_tol = 5, 0.0
    sett.clean_fov = False
    sett.voxel_robust = sett.scaling = sett.unified_rigid = True
    sett.rigid_mod = 1
    seen = []
    inner = run._update_admm

    def spy(x, *args, **kwargs):
        out = inner(x, *args, **kwargs)
        seen.append([(xn.po.scl, xn.po.rigid.clone()) for xn in x[0]])
        return out

    monkeypatch.setattr(run, '_update_admm', spy)
    dat, _, R, info = U.fit(xg, yg, sett)
    torch.cuda.synchronize()
    monkeypatch.setattr(run, '_update_admm', inner)
    assert info['n_iter'] == 4 and len(seen) == 4
    return dat, R, info, (xg, yg, sett), seen[-1]


def test_fit_with_every_switch_on(dev, monkeypatch):
    """It runs; a second run gives the same bits of dat_y, R, every po.scl and every returned weight; the returned
    weights are tests/voxel64.huber64 of the residuals the last iteration's rule saw."""
    import unires_amd as U
    a = _fit_everything(dev, monkeypatch)
    b = _fit_everything(dev, monkeypatch)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert _scl(a[3][0]) == _scl(b[3][0]) and all(v != 0.0 for v in _scl(a[3][0]))
    assert not torch.equal(a[1][1], torch.eye(4, dtype=torch.float64))  # (the rigid update moved the second repeat)
    for n in range(2):
        assert same_bits(a[2]['voxel_w'][0][n], b[2]['voxel_w'][0][n])
    dat, R, info, (xg, yg, sett), last = a
    vw = info['voxel_w']
    assert len(vw) == 1 and len(vw[0]) == 2 and all(t.is_cuda and t.dtype == torch.float32 for t in vw[0])
    for n, (scl, rigid) in enumerate(last):
        xg[0][n].po.scl, xg[0][n].po.rigid = scl, rigid
    for n in range(2):
        Ay = U._proj('A', yg[0].dat, xg[0], yg[0], n=n, method=sett.method, do=sett.do_proj)
        c = np.float32(float(sett.voxel_k) / float(xg[0][n].tau) ** 0.5)
        want = voxel64.huber64(xg[0][n].dat.cpu().numpy(), Ay.cpu().numpy(), None, c)
        got = vw[0][n].cpu().numpy()
        differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print('every switch on, repeat %d: %d of %d weights differ from the rule; %.4f of them exactly 1'
              % (n, differ, got.size, float((got == 1.0).mean())), flush=True)
        assert differ == 0
    assert float(vw[0][1][BOX_SL].mean()) < float(vw[0][1].mean())  # (the corrupted box is down-weighted)


# ---- (5) planted motion ---------------------------------------------------------------------------------------------------
def test_a_map_keeps_a_corrupted_box_out_of_the_registration(dev):
    """DESIGN.md 8.7's experiment with a box for the slices: the second repeat is the truth seen through a planted rigid
    (1 voxel along x, 0.02 rad about z), its box raised by 20 noise standard deviations; y is the truth.  Three rigid
    updates from the identity, with the box at weight 0 and with no map: the one with the map ends nearer the planted
    matrix than the one without and than the start, and no more than that is asserted."""
    import unires_amd as U
    from unires_amd._rigid import _update_rigid
    planted_rigid = rigid_matrix((1.0, 0.0, 0.0), (0.0, 0.0, 0.02))
    noise_sd = 5.0  # (_phantom's)
    dist = {}
    for arm in ('map', 'no map'):
        prob, xg, yg, sett = _arm(dev, False, arm == 'map')
        truth = prob['truth'][0].float().to(dev)
        yg[0].dat = truth.clone()
        x1 = xg[0][1]
        x1.po.rigid = planted_rigid.clone()
        with torch.cuda.device(dev):
            dat = U._proj('A', truth, xg[0], yg[0], n=1, method=sett.method, do=sett.do_proj).clone()
        dat = dat.reshape(tuple(x1.dat.shape)).contiguous()
        dat[BOX_SL] += 20.0 * noise_sd
        x1.dat = dat
        x1.po.rigid = torch.eye(4, dtype=torch.float64)
        for _ in range(3):
            xg, _ = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
        dist[arm] = float((xg[0][1].po.rigid.double().cpu() - planted_rigid).norm())
    start = float((torch.eye(4, dtype=torch.float64) - planted_rigid).norm())
    print('planted motion: distance of po.rigid from the planted matrix: start %.4f, with the map %.4f, without %.4f'
          % (start, dist['map'], dist['no map']), flush=True)
    assert dist['map'] < dist['no map'] and dist['map'] < start
