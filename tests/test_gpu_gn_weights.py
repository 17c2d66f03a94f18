"""The slice weights in the scaling and rigid Gauss-Newton updates on the GPU, in process:

(1) unires_scaling_sums_w against tests/gn64.py's exact sums, at the shapes where k_scaling_sums' carry arithmetic turns
    (tests/test_gpu_admm64.py), slices along every axis, `pow2` and `ramp` weights; u = 1 the bits of
    unires_scaling_sums; u in {0, 1} the bits of the data with those slices zeroed; two runs the same bits;
(2) unires_rigid_resid bit for bit against gn64.rigid_resid32: out of place and on ay, with and without weights, one
    buffer off its 16-byte boundary, x unchanged, nothing written outside the output;
(3) a slice of weight 0 does not reach _update_scaling, _update_rigid or a fit() that runs both: clean data and data
    with those slices multiplied by 0.3 give the same bits;
(4) u = 1 through the rigid step: the bits of the unweighted residual, Hessian weight and 27 sums, ll inside its bound;
    the rigid objective is _compute_nll's; a repeat whose weights are all zero is left alone;
(5) planted motion with corrupted slices: the weighted update ends nearer the planted matrix than the unweighted one.

Every output of (1) and (2) lies inside a buffer padded with sentinels on both sides.

Observed on an MI355X: (1) worst err / tol 0.084 over the 30 cases; (2) bit-exact; (3) on the commit before the weights
reached the two updates every test of (3) but the control - fit() with both updates off - fails; from the identity the
phantom was made with the rigid line search of every arm keeps the identity, so there only sll tells the weighted step
from the unweighted one; (4) ll at u = 1: error 0; (5) distances 0.1304 weighted, 0.8263 unweighted, 1.0004 at the start.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import admm64, gn64, slice64
from tests.helpers import rigid_matrix
from tests.test_gpu_admm64 import PAD, SENT, _guard_ok, _lib, _padded, _sums_out

pytestmark = pytest.mark.gpu

PLANTED = (3, 7, 11)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- (1) the five weighted sums -----------------------------------------------------------------------------------------
SCALING_SHAPES = [(67, 45, 91), (1, 1, 300001), (600, 600, 1), (300, 3, 301), (5, 7, 6)]


def _scaling(dev, xd, ad, dim, dim_thick, ud):
    """unires_scaling_sums_w (ud a device tensor) or unires_scaling_sums (ud None) into a guarded buffer -> (5,) float64."""
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    ob, ov = _sums_out(dev, 5)
    ob[PAD:PAD + 5] = SENT  # (every one of the five must be written)
    with torch.cuda.device(dev):
        if ud is None:
            check(_lib().unires_scaling_sums(_ptr(xd), _ptr(ad), i3(dim), dim_thick, _ptr(ov), _stream()))
        else:
            check(_lib().unires_scaling_sums_w(_ptr(xd), _ptr(ad), i3(dim), dim_thick, _ptr(ud), _ptr(ov), _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(ob, 5)
    return ov.cpu().clone()


@pytest.mark.parametrize('dim', SCALING_SHAPES)
def test_scaling_sums_w_exact_terms(dev, dim):
    g = torch.Generator().manual_seed(sum(dim))
    x = (torch.rand(dim, generator=g) * 10).float()
    x[x < 1.5] = 0.0
    x.view(-1)[5::13] = -0.0
    ay = (torch.rand(dim, generator=g) * 10 - 1).float()
    xd, ad = x.to(dev), ay.to(dev)
    for dim_thick in (0, 1, 2):
        S = dim[dim_thick]
        for pattern in ('pow2', 'ramp'):
            u = slice64.weights(S, pattern)
            out = _scaling(dev, xd, ad, dim, dim_thick, u.to(dev))
            ref, tol = gn64.scaling_sums_w(x.numpy(), ay.numpy(), dim_thick, u.numpy())
            r = admm64.check_sums(out.tolist(), ref, tol)
            print('scaling_sums_w %s dim_thick %d %s: max err/tol %.3f' % (dim, dim_thick, pattern, r['max_ratio']),
                  flush=True)
            assert r['ok'], (dim, dim_thick, pattern, r)
            assert same_bits(out, _scaling(dev, xd, ad, dim, dim_thick, u.to(dev)))  # the same bits every run
        ones = torch.ones(S, device=dev)
        assert same_bits(_scaling(dev, xd, ad, dim, dim_thick, ones), _scaling(dev, xd, ad, dim, dim_thick, None))
        u01 = (slice64.weights(S, 'pow2') >= 0.5).float()
        xz = x.clone()
        xz.index_fill_(dim_thick, torch.nonzero(u01 == 0).reshape(-1), 0.0)
        assert same_bits(_scaling(dev, xd, ad, dim, dim_thick, u01.to(dev)),
                         _scaling(dev, xz.to(dev), ad, dim, dim_thick, ones))


# ---- (2) the residual ---------------------------------------------------------------------------------------------------
RESID_SHAPES = [(1, 1, 1), (5, 7, 6), (67, 1, 65), (3, 130, 9), (300, 3, 5), (5, 7, 300), (41, 38, 60)]


def _resid_inputs(dim):
    g = torch.Generator().manual_seed(7 + sum(dim))
    x = (torch.rand(dim, generator=g) * 10 - 2).float()
    x[torch.rand(dim, generator=g) < 0.2] = 0.0
    x.view(-1)[5::13] = -0.0
    ay = (torch.rand(dim, generator=g) * 10 - 2).float()
    ay.view(-1)[2::7] = 0.0  # exact zeros: the mask's second clause
    ay.view(-1)[3::29] = -0.0
    return x, ay


def _resid(dev, x, ay, dim, axis, u, inplace, offset=0):
    """unires_rigid_resid into a guarded buffer (ay's own when ``inplace``; the views start ``offset`` floats past a
    16-byte boundary) -> the output on the CPU."""
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    n = x.numel()
    pad0 = torch.zeros(offset)
    ab, av = _padded(torch.cat([pad0, ay.reshape(-1)]), dev)
    av = av[offset:]
    if inplace:
        ob, ov = ab, av
    else:
        ob, ov = _padded(torch.cat([pad0, torch.full((n,), SENT)]), dev)
        ov = ov[offset:]
    xd = x.to(dev).contiguous()
    x0 = xd.clone()
    assert av.data_ptr() % 16 == 4 * offset % 16
    ud = None if u is None else u.to(dev)
    with torch.cuda.device(dev):
        check(_lib().unires_rigid_resid(_ptr(xd), _ptr(av), i3(dim), axis, None if ud is None else _ptr(ud), _ptr(ov),
                                        _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(ob, n + offset) and bool((ob[PAD:PAD + offset] == 0).all())
    assert same_bits(xd, x0)
    if not inplace:
        assert same_bits(av, ay.reshape(-1).to(dev))
    return ov.cpu().reshape(dim)


@pytest.mark.parametrize('dim', RESID_SHAPES)
def test_rigid_resid_bit_for_bit(dev, dim):
    x, ay = _resid_inputs(dim)
    for axis in (0, 1, 2):
        for u in (None, slice64.weights(dim[axis], 'ramp')):
            want = torch.from_numpy(gn64.rigid_resid32(x.numpy(), ay.numpy(), axis, None if u is None else u.numpy()))
            for inplace in (False, True):
                got = _resid(dev, x, ay, dim, axis, u, inplace)
                assert same_bits(got, want), (dim, axis, u is not None, inplace)
    # without weights: the tensor form of _rigid_terms
    d = ay.to(dev) - x.to(dev)
    d[(x.to(dev) == 0) | (ay.to(dev) == 0)] = 0
    assert same_bits(_resid(dev, x, ay, dim, 0, None, False), d.cpu())


@pytest.mark.parametrize('inplace', [False, True])
def test_rigid_resid_off_a_16_byte_boundary(dev, inplace):
    dim = (41, 38, 60)
    x, ay = _resid_inputs(dim)
    for axis, u in ((1, slice64.weights(dim[1], 'ramp')), (2, None)):
        want = torch.from_numpy(gn64.rigid_resid32(x.numpy(), ay.numpy(), axis, None if u is None else u.numpy()))
        assert same_bits(_resid(dev, x, ay, dim, axis, u, inplace, offset=1), want)


# ---- (3) zero-weight slices are not read -------------------------------------------------------------------------------------
def _phantom(dev):
    """DESIGN.md 8.6's phantom: 48 x 48 x 40, two repeats with 3 mm slices (thick along z, then along y: the second is
    (48, 16, 40), its slices planes of constant y); y as gpu_structs leaves it."""
    from tests.helpers import gpu_structs, make_problem
    prob = make_problem(seed=5, dim_y=(48, 48, 40), thick=3, n_repeats=2, rot=0.0, trans=0.0, noise_sd=5.0,
                        thick_axes=None, shift=(0.0, 0.0, 0.0))
    return prob, gpu_structs(prob, dev)


OFFSET = (0.4, -0.3, 0.2, 0.01, -0.01, 0.02)


def _arm(dev, corrupt, weights, planted=PLANTED, start=None):
    """Fresh structs; the second repeat's planted slices multiplied by 0.3 (``corrupt``: sign and non-zeroness stay) and
    given weight 0 (``weights``).  ``start``: the second repeat's rigid_q (and po.rigid) instead of the identity the
    phantom was made with - at the identity the line search finds nothing to gain and keeps it."""
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _expm, affine_basis
    prob, (xg, yg, sett) = _phantom(dev)
    x1 = xg[0][1]
    assert _slice_axis(x1) == 1 and x1.dat.shape[1] > max(planted)
    if corrupt:
        for s in planted:
            x1.dat[:, s, :] *= 0.3
    if weights:
        w = torch.ones(x1.dat.shape[1])
        w[list(planted)] = 0.0
        x1.slice_w = w.to(dev)
    for xn in xg[0]:
        xn.rigid_q = torch.zeros(6, dtype=torch.float64)
    if start is not None:
        x1.rigid_q = torch.tensor(start, dtype=torch.float64)
        x1.po.rigid = _expm(x1.rigid_q, affine_basis('SE'))
    return prob, xg, yg, sett


def _scl(xg):
    return [float(xn.po.scl) for xc in xg for xn in xc]


def test_update_scaling_does_not_read_zero_weight_slices(dev):
    from unires_amd._update import _update_scaling
    res = {}
    for name, corrupt, weights in (('clean', False, True), ('corrupt', True, True), ('unweighted', True, False)):
        _, xg, yg, sett = _arm(dev, corrupt, weights)
        xg, sll = _update_scaling(xg, yg, sett, max_niter_gn=1, num_linesearch=6)
        res[name] = (_scl(xg), float(sll))
        print('scaling, %s: scl %s sll %r' % (name, res[name][0], res[name][1]), flush=True)
    assert np.array_equal(np.array(res['clean'][0]).view(np.int64), np.array(res['corrupt'][0]).view(np.int64))
    assert np.float64(res['clean'][1]).view(np.int64) == np.float64(res['corrupt'][1]).view(np.int64)
    assert all(v != 0.0 for v in res['clean'][0])  # (a step was taken)
    assert res['unweighted'][0][1] != res['corrupt'][0][1] and res['unweighted'][1] != res['corrupt'][1]
    assert res['unweighted'][0][0] == res['corrupt'][0][0]  # (the clean repeat's step does not depend on the other)


def _rigid_state(xg, sll):
    return ([xn.rigid_q.clone() for xc in xg for xn in xc], [xn.po.rigid.double().cpu().clone() for xc in xg for xn in xc],
            sll.detach().cpu().clone())


def _same_state(a, b):
    return all(same_bits(p, q) for p, q in zip(a[0], b[0])) and all(same_bits(p, q) for p, q in zip(a[1], b[1])) \
        and same_bits(a[2], b[2])


@pytest.mark.parametrize('samp', [0, 1])
@pytest.mark.parametrize('mean_correct', [False, True])
@pytest.mark.parametrize('start', [None, OFFSET])
def test_update_rigid_does_not_read_zero_weight_slices(dev, samp, mean_correct, start):
    """From the identity the phantom was made with, where the line search of either arm keeps the identity (observed:
    only sll tells the arms apart), and from a start half a voxel and 0.02 rad off, where a step is taken."""
    from unires_amd._rigid import _update_rigid
    res = {}
    for name, corrupt, weights in (('clean', False, True), ('corrupt', True, True), ('unweighted', True, False)):
        _, xg, yg, sett = _arm(dev, corrupt, weights, start=start)
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


def test_update_rigid_decimates_the_weights_with_the_observation(dev):
    """samp = 6 decimates the second repeat by (6, 2, 6): its slices 0, 2, 4, ... remain, with the weights
    u[::2][:8].  Slices 2, 6 and 10 - 1, 3 and 5 of the decimated observation - have weight 0."""
    from unires_amd._rigid import _update_rigid
    planted = (2, 6, 10)
    res = {}
    for name, corrupt, weights in (('clean', False, True), ('corrupt', True, True), ('unweighted', True, False)):
        _, xg, yg, sett = _arm(dev, corrupt, weights, planted)
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=6)
        res[name] = _rigid_state(xg, sll)
    assert _same_state(res['clean'], res['corrupt'])
    assert not same_bits(res['unweighted'][0][1], res['corrupt'][0][1])


def test_update_rigid_in_the_denoising_regime_does_not_read_zero_weight_slices(dev):
    """Pull / push only: the Hessian's weight is the volume u[s(v)] where the unweighted step passes none."""
    from tests.helpers import gpu_structs, make_problem
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _update_rigid
    planted = (2, 5, 6)
    res = {}
    for name, corrupt, weights in (('clean', False, True), ('corrupt', True, True), ('unweighted', True, False)):
        prob = make_problem(dim_y=(20, 18, 33), n_channels=1, regime='dn', rot=0.08, trans=1.5, seed=1)
        xg, yg, sett = gpu_structs(prob, dev)
        xn = xg[0][0]
        a = _slice_axis(xn)
        idx = torch.tensor(planted, device=dev)
        if corrupt:
            xn.dat.index_copy_(a, idx, xn.dat.index_select(a, idx) * 0.3)
        if weights:
            w = torch.ones(xn.dat.shape[a])
            w[list(planted)] = 0.0
            xn.slice_w = w.to(dev)
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
        res[name] = _rigid_state(xg, sll)
    assert _same_state(res['clean'], res['corrupt'])
    assert not same_bits(res['unweighted'][2], res['corrupt'][2])


def _fit_arm(dev, corrupt, gn):
    import unires_amd as U
    _, xg, yg, sett = _arm(dev, corrupt, True)
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
def test_fit_does_not_read_zero_weight_slices(dev, gn):
    """fit(), 4 ADMM iterations of 5 CG iterations (cgs_tol = 0), user weights 0 on the planted slices; with both
    Gauss-Newton updates (scaling, and the rigid update every iteration) and, as the control, with neither."""
    clean, corrupt = _fit_arm(dev, False, gn), _fit_arm(dev, True, gn)
    for a, b, name in zip(clean, corrupt, ('dat_y', 'R', 'scl')):
        assert same_bits(a, b), name
    if gn:
        assert bool((clean[2] != 0).all()) and not torch.equal(clean[1][1], torch.eye(4, dtype=torch.float64))


# ---- (4) unit weights, the objective, empty repeats ---------------------------------------------------------------------------
def test_unit_weights_give_the_unweighted_rigid_step(dev):
    from unires_amd import _ops
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    from unires_amd._project import _taps
    from unires_amd._rigid import _ctc, _grid_matrix, _rigid_terms, _update_rigid, affine_basis, _expm
    from unires_amd.spatial import _m12
    _, xg, yg, sett = _arm(dev, True, False)
    xn, y = xg[0][1], yg[0].dat
    po, tau, a = xn.po, float(xn.tau), 1
    ones = torch.ones(xn.dat.shape[a], device=dev)
    rigid = rigid_matrix((0.3, -0.2, 0.1), (0.01, -0.02, 0.015))
    with torch.cuda.device(dev):
        ll0, gr0, d0 = _rigid_terms(xn.dat, y, po, tau, rigid, sett, diff=True)
        ll1, gr1, d1 = _rigid_terms(xn.dat, y, po, tau, rigid, sett, diff=True, slice_w=ones, axis=a)
        dim = tuple(po.dim_yx)
        c0, c1 = _ctc(po, dim, dev), _ctc(po, dim, dev, ones, a)
        assert same_bits(d0, d1) and same_bits(gr0, gr1) and same_bits(c0, c1)
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
        # ll: the per-slice sums' float64 form against the exact sum of the same float32 terms
        mat, _ = _grid_matrix(po, rigid, sett.method)
        Ay = _ops.conv_down(_ops.pull_affine(y, _m12(mat), dim), _taps(po), po.ratio, float(po.scl), po.dim_thick)
        Ay = Ay.reshape(tuple(xn.dat.shape))
    xh, ah = xn.dat.cpu().numpy(), Ay.cpu().numpy()
    exact, _ = admm64.masked_sse(xh, ah)
    ref, tol = gn64.weighted_sse(xh, ah, a, ones.cpu().numpy())
    assert abs(ref - exact) <= 2.0 ** -52 * exact
    err = abs(float(ll1) - 0.5 * tau * exact)
    bound = 0.5 * tau * tol + 2.0 ** -52 * 0.5 * tau * exact  # (the product with tau / 2 rounds once more)
    print('rigid ll at u = 1: err / bound %.3g (ll %r, unweighted %r)' % (err / bound, float(ll1), float(ll0)), flush=True)
    assert err <= bound
    # and a whole update: the same step
    out = []
    for w in (False, True):
        _, xg, yg, sett = _arm(dev, True, False)
        if w:
            xg[0][1].slice_w = torch.ones(16, device=dev)
        xg, _ = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=0, samp=0)
        out.append(xg[0][1].rigid_q.clone())
    assert same_bits(out[0], out[1]) and bool((out[0] != 0).any())


def test_rigid_objective_is_the_objective_of_compute_nll(dev):
    """Both repeats weighted: sum_n ll_n of the rigid step at po.rigid, added in _compute_nll's order, has the bits of its
    nll_xy - the same y, weights and rigid through the same expression (_update._slice_ll)."""
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _rigid_terms
    from unires_amd._update import _compute_nll
    prob, xg, yg, sett = _arm(dev, True, True)
    xg[0][0].slice_w = slice64.weights(xg[0][0].dat.shape[2], 'ramp').to(dev)
    xg[0][1].slice_w = slice64.weights(16, 'ramp', seed=5).to(dev)
    with torch.cuda.device(dev):
        nll_xy = _compute_nll(xg, yg, sett, prob['rho'])[1]
        ll = torch.zeros((), dtype=torch.float64, device=dev)
        for xn in xg[0]:
            ll = ll + _rigid_terms(xn.dat, yg[0].dat, xn.po, xn.tau, xn.po.rigid, sett, slice_w=xn.slice_w,
                                   axis=_slice_axis(xn))[0]
    print('rigid objective %r, nll_xy %r' % (float(ll), float(nll_xy)), flush=True)
    assert same_bits(ll, nll_xy)


def test_a_repeat_with_all_zero_weights_is_left_alone(dev):
    from unires_amd._rigid import _update_rigid
    from unires_amd._update import _update_scaling
    for update in ('scaling', 'rigid'):
        got = {}
        for name in ('both', 'first'):
            _, xg, yg, sett = _arm(dev, False, False)
            x1 = xg[0][1]
            x1.slice_w = torch.zeros(16, device=dev)
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


# ---- (5) planted motion ---------------------------------------------------------------------------------------------------
def test_weights_keep_corrupted_slices_out_of_the_registration(dev):
    """The second repeat is the truth seen through a planted rigid (1 voxel along x, 0.02 rad about z), its planted slices
    multiplied by 0.3; y is the truth.  Three rigid updates from the identity, with weight 0 on those slices and without
    weights: the weighted one ends nearer the planted matrix, and no more than that is asserted.  Observed on an MI355X
    (Frobenius distance of po.rigid from the planted matrix): 1.0004 at the start, 0.1304 weighted, 0.8263 unweighted."""
    import unires_amd as U
    from unires_amd._rigid import _update_rigid
    planted_rigid = rigid_matrix((1.0, 0.0, 0.0), (0.0, 0.0, 0.02))
    dist = {}
    for arm in ('weighted', 'unweighted'):
        prob, xg, yg, sett = _arm(dev, False, arm == 'weighted')
        truth = prob['truth'][0].float().to(dev)
        yg[0].dat = truth.clone()
        x1 = xg[0][1]
        x1.po.rigid = planted_rigid.clone()
        with torch.cuda.device(dev):
            dat = U._proj('A', truth, xg[0], yg[0], n=1, method=sett.method, do=sett.do_proj).clone()
        for s in PLANTED:
            dat[:, s, :] *= 0.3
        x1.dat = dat.reshape(tuple(x1.dat.shape)).contiguous()
        x1.po.rigid = torch.eye(4, dtype=torch.float64)
        for _ in range(3):
            xg, _ = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
        dist[arm] = float((xg[0][1].po.rigid.double().cpu() - planted_rigid).norm())
    start = float((torch.eye(4, dtype=torch.float64) - planted_rigid).norm())
    print('planted motion: distance of po.rigid from the planted matrix: start %.4f, weighted %.4f, unweighted %.4f'
          % (start, dist['weighted'], dist['unweighted']), flush=True)
    assert dist['weighted'] < dist['unweighted']
