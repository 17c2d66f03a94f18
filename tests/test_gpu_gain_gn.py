"""The slice gains in the rigid Gauss-Newton update on the GPU, in process, with ``sett.gain_gn`` on
unless a test says otherwise:

(1) unires_rigid_terms_e bit for bit against the composition of entry points it replaces (unires_slice_apply, then
    unires_slice_sums / unires_voxel_sums and unires_rigid_resid / unires_rigid_resid_g on the gained prediction) and
    against tests/gne64.py (the residual bit for bit, the sums inside the float64 accumulation bound), slices along every
    axis, with and without g and u, without ``out``, with it and on ay; inputs unchanged, NaN-prefilled outputs fully
    written, nothing written outside them, two runs the same bits, e = 1 the bits of the calls without gains;
(2) each buffer in turn off its 16-byte boundary; (3) the status codes of unires_slice_sums for the same mistakes;
(4) e = 1 through _rigid_terms, _ctc and _update_rigid: the bits of the path without gains;
(5) the rigid objective is _compute_nll's; (6) the gains are decimated with the observation, and ignored with the switch
    off; (7) the denoising regime; (8) a repeat whose weights are all zero is left alone; (9) planted motion of a
    banded repeat; (10) the y-update after a rigid update has the bits of one on fresh structs; (11) fit().

Every output of (1) and (2) lies inside a buffer padded with sentinels on both sides.  Every test fails on the commit
before the feature: the library has no ``unires_rigid_terms_e`` and the update functions no ``gain=``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import admm64, gain64, gn64, gne64, slice64, voxel64
from tests.test_gpu_admm64 import PAD, SENT, _guard_ok, _lib, _padded, _sums_out
from tests.test_gpu_gn_voxel import _arm
from tests.test_gpu_gn_weights import OFFSET, _rigid_state, _same_state, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(300, 3, 5), (3, 130, 9), (5, 7, 300), (67, 1, 65), (1, 1, 1), (41, 38, 60)]
ARMS = ((False, False), (False, True), (True, False), (True, True))  # (g, u)
PATTERN = (1.0, 0.85, 1.15)  # the planted banding of (9) and (11), repeated along the stack


# ---- (1) the entry point ------------------------------------------------------------------------------------------------
def _inputs(dim, axis):
    """x with 30 % zeros, some -0.0 and - where there is more than one slice - one slice all zero; ay with exact zeros of
    both signs; generic voxel weights, slice weights and gains in [0.5, 2]."""
    gen = torch.Generator().manual_seed(11 + sum(dim) + axis)
    x = (torch.rand(dim, generator=gen) * 10 - 2).float()
    x[torch.rand(dim, generator=gen) < 0.3] = 0.0
    x.view(-1)[5::13] = -0.0
    S = dim[axis]
    if S > 1:
        x.select(axis, S // 2).zero_()
    ay = (torch.rand(dim, generator=gen) * 10 - 2).float()
    ay.view(-1)[2::7] = 0.0
    ay.view(-1)[3::29] = -0.0
    g = voxel64.weights(dim, 'ramp')
    u = slice64.weights(S, 'ramp', seed=3)
    e = gain64.gains(S, 'generic')
    return x.contiguous(), ay.contiguous(), g, u, e


def _terms_e(dev, x, ay, g, u, e, dim, axis, form, off=(0, 0, 0, 0)):
    """unires_rigid_terms_e with every volume in a guarded buffer; ``form``: 'null' (no out), 'out', 'inplace' (out is
    ay); ``off``: floats past a 16-byte boundary the views of x, ay, g and out start at (in place out is ay: its
    offset) -> (sums (2 S,) float64, out or None), on the CPU.  The outputs start as NaN."""
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    n, S = x.numel(), dim[axis]
    ox, oa, og, oo = off
    if form == 'inplace':
        oo = oa

    def view(t, o):
        b, v = _padded(torch.cat([torch.zeros(o), t.reshape(-1)]), dev)
        assert v[o:].data_ptr() % 16 == 4 * o % 16
        return b, v[o:]

    xb, xv = view(x, ox)
    ab, av = view(ay, oa)
    gb, gv = (None, None) if g is None else view(g, og)
    if form == 'null':
        ob, ov = None, None
    elif form == 'inplace':
        ob, ov = ab, av
    else:
        ob, ov = view(torch.full((n,), float('nan')), oo)
    ud, ed = None if u is None else u.to(dev), e.to(dev)
    x0, g0, u0, e0 = xv.clone(), None if g is None else gv.clone(), None if u is None else ud.clone(), ed.clone()
    sb, sv = _sums_out(dev, 2 * S)
    sv.fill_(float('nan'))
    with torch.cuda.device(dev):
        check(_lib().unires_rigid_terms_e(_ptr(xv), _ptr(av), None if g is None else _ptr(gv),
                                          None if u is None else _ptr(ud), _ptr(ed), i3(dim), axis, _ptr(sv),
                                          None if ov is None else _ptr(ov), _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(sb, 2 * S) and _guard_ok(xb, n + ox) and _guard_ok(ab, n + oa)
    assert g is None or _guard_ok(gb, n + og)
    assert same_bits(xv, x0) and same_bits(ed, e0)  # x, g, u, e are only read
    assert g is None or same_bits(gv, g0)
    assert u is None or same_bits(ud, u0)
    if form != 'inplace':
        assert same_bits(av, ay.reshape(-1).to(dev))
    sums = sv.cpu().clone()
    assert not bool(torch.isnan(sums).any())  # (every one of the 2 S entries is written)
    if ov is None:
        return sums, None
    assert _guard_ok(ob, n + oo) and bool((ob[PAD:PAD + oo] == 0).all())
    out = ov.cpu().reshape(dim).clone()
    assert not bool(torch.isnan(out).any())
    return sums, out


def _composition(dev, x, ay, g, u, e, dim, axis, gained=True):
    """What the fused call replaces, from the existing entry points: P = unires_slice_apply(ay, e) (``gained`` False:
    ay itself), unires_slice_sums(x, P) / unires_voxel_sums(x, P, g), unires_rigid_resid(x, P, t) /
    unires_rigid_resid_g(x, P, g, t), t = fl32(fl64(u e)) (``gained`` False: u, which may be None)."""
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    lib = _lib()
    S = dim[axis]
    xd, ad = x.to(dev), ay.to(dev)
    gd = None if g is None else g.to(dev)
    with torch.cuda.device(dev):
        if gained:
            P = torch.empty_like(ad)
            check(lib.unires_slice_apply(_ptr(ad), _ptr(P), _ptr(e.to(dev)), i3(dim), axis, _stream()))
            t = torch.from_numpy(gne64.tables(None if u is None else u.numpy(), e.numpy())[2]).to(dev)
        else:
            P, t = ad, None if u is None else u.to(dev)
        sums = torch.empty(2 * S, dtype=torch.float64, device=dev)
        out = torch.empty_like(ad)
        tp = None if t is None else _ptr(t)
        if g is None:
            check(lib.unires_slice_sums(_ptr(xd), _ptr(P), i3(dim), axis, _ptr(sums), _stream()))
            check(lib.unires_rigid_resid(_ptr(xd), _ptr(P), i3(dim), axis, tp, _ptr(out), _stream()))
        else:
            check(lib.unires_voxel_sums(_ptr(xd), _ptr(P), _ptr(gd), i3(dim), axis, _ptr(sums), _stream()))
            check(lib.unires_rigid_resid_g(_ptr(xd), _ptr(P), _ptr(gd), i3(dim), axis, tp, _ptr(out), _stream()))
    torch.cuda.synchronize(dev)
    return sums.cpu(), out.cpu()


@pytest.mark.parametrize('dim', SHAPES)
def test_rigid_terms_e_bit_for_bit(dev, dim):
    worst = 0.0
    for axis in (0, 1, 2):
        x, ay, g, u, e = _inputs(dim, axis)
        S = dim[axis]
        ones = torch.ones(S)
        for with_g, with_u in ARMS:
            gg, uu = g if with_g else None, u if with_u else None
            tag = (dim, axis, with_g, with_u)
            want_sums, want_out = _composition(dev, x, ay, gg, uu, e, dim, axis)
            ref_out, ref_sums, ref_bound = gne64.terms_e32(x.numpy(), ay.numpy(), axis, None if gg is None else gg.numpy(),
                                                           None if uu is None else uu.numpy(), e.numpy())
            got = {form: _terms_e(dev, x, ay, gg, uu, e, dim, axis, form) for form in ('null', 'out', 'inplace')}
            for form, (sums, out) in got.items():
                assert same_bits(sums, want_sums), tag + (form,)
                if form != 'null':
                    assert same_bits(out, want_out), tag + (form,)
                    assert same_bits(out, torch.from_numpy(ref_out)), tag + (form,)
            err = np.abs(got['null'][0].numpy() - ref_sums)
            assert (err <= ref_bound).all(), tag + (err, ref_bound)
            worst = max(worst, float((err[ref_bound > 0] / ref_bound[ref_bound > 0]).max()) if (ref_bound > 0).any() else 0.0)
            # the same bits every run
            again = _terms_e(dev, x, ay, gg, uu, e, dim, axis, 'out')
            assert same_bits(again[0], got['out'][0]) and same_bits(again[1], got['out'][1]), tag
            # e = 1: the calls without gains, on ay itself
            unit = _terms_e(dev, x, ay, gg, uu, ones, dim, axis, 'out')
            plain = _composition(dev, x, ay, gg, uu, ones, dim, axis, gained=False)
            assert same_bits(unit[0], plain[0]) and same_bits(unit[1], plain[1]), tag
        # the all-zero slice: SSE 0 and count 0; masked voxels +0
        if S > 1:
            s = got['out'][0]
            assert float(s[S // 2]) == 0.0 and float(s[S + S // 2]) == 0.0
        p = gne64.gained32(ay.numpy(), e.numpy(), axis)
        masked = (x.numpy() == 0) | (p == 0)
        assert (got['out'][1].numpy()[masked].view(np.uint32) == 0).all()
    print('rigid_terms_e %s: worst sums err / bound %.3f' % (dim, worst), flush=True)


# ---- (2) off a 16-byte boundary --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['x', 'ay', 'g', 'out'])
def test_rigid_terms_e_off_a_16_byte_boundary(dev, which):
    dim = (41, 38, 60)
    off = tuple(int(which == name) for name in ('x', 'ay', 'g', 'out'))
    for axis in (1, 2):
        x, ay, g, u, e = _inputs(dim, axis)
        want_sums, want_out = _composition(dev, x, ay, g, u, e, dim, axis)
        for form in (('out',) if which == 'out' else ('null', 'out', 'inplace')):
            sums, out = _terms_e(dev, x, ay, g, u, e, dim, axis, form, off)
            assert same_bits(sums, want_sums), (which, axis, form)
            assert out is None or same_bits(out, want_out), (which, axis, form)


# ---- (3) status codes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', ['x', 'ay', 'e', 'sums', 'axis', 'dim'])
def test_rigid_terms_e_status_codes(dev, bad):
    """A null x, ay, e or sums, a bad axis and a bad dim give unires_slice_sums' codes, and nothing is launched: the
    NaN-prefilled sums stay NaN."""
    from unires_amd._lib import i3
    lib = _lib()
    dim = (4, 5, 6)
    x, ay = torch.ones(dim, device=dev), torch.ones(dim, device=dev)
    e = torch.ones(6, device=dev)
    sums = torch.full((12,), float('nan'), dtype=torch.float64, device=dev)
    a = dict(x=x.data_ptr(), ay=ay.data_ptr(), e=e.data_ptr(), sums=sums.data_ptr(), axis=2, dim=i3(dim))
    if bad in ('x', 'ay', 'e', 'sums'):
        a[bad] = None
    elif bad == 'axis':
        a['axis'] = 3
    else:
        a['dim'] = i3((4, 0, 6))
    mine = lib.unires_rigid_terms_e(a['x'], a['ay'], None, None, a['e'], a['dim'], a['axis'], a['sums'], None, None)
    if bad == 'e':
        theirs = 1  # (unires_slice_sums has no e: UNIRES_ERR_NULL, as for its own pointers)
    else:
        theirs = lib.unires_slice_sums(a['x'], a['ay'], a['dim'], a['axis'], a['sums'], None)
    torch.cuda.synchronize(dev)
    assert mine == theirs != 0
    assert bool(torch.isnan(sums).all())


# ---- (4) unit gains ---------------------------------------------------------------------------------------------------------
def _gains(dev, S, pattern='generic'):
    return gain64.gains(S, pattern).to(dev).contiguous()


@pytest.mark.parametrize('with_u', [False, True])
def test_unit_gains_give_the_step_of_the_path_without_them(dev, with_u):
    """e = 1 beside slice weights: the slice-weighted path's residual, Hessian weight, 27 sums, step and ll, bit for bit;
    beside nothing: the unweighted path's residual, Hessian weight, sums and step bit for bit, and ll inside _slice_ll's
    float64 bound."""
    from unires_amd import _ops
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    from unires_amd._project import _taps
    from unires_amd._rigid import _ctc, _expm, _grid_matrix, _rigid_terms, _update_rigid, affine_basis
    from unires_amd.spatial import _m12
    from tests.helpers import rigid_matrix
    _, xg, yg, sett = _arm(dev, False, False)
    xn, y = xg[0][1], yg[0].dat
    po, tau, a = xn.po, float(xn.tau), 1
    u = slice64.weights(16, 'ramp', seed=5).to(dev) if with_u else None
    ones = torch.ones(16, device=dev)
    rigid = rigid_matrix((0.3, -0.2, 0.1), (0.01, -0.02, 0.015))
    with torch.cuda.device(dev):
        ll0, gr0, d0 = _rigid_terms(xn.dat, y, po, tau, rigid, sett, diff=True, slice_w=u, axis=a if with_u else None)
        ll1, gr1, d1 = _rigid_terms(xn.dat, y, po, tau, rigid, sett, diff=True, slice_w=u, axis=a, gain=ones)
        ll2 = _rigid_terms(xn.dat, y, po, tau, rigid, sett, slice_w=u, axis=a, gain=ones)[0]  # (a line-search evaluation)
        dim = tuple(po.dim_yx)
        c0 = _ctc(po, dim, dev, u, a) if with_u else _ctc(po, dim, dev)
        c1 = _ctc(po, dim, dev, u, a, gain=ones)
        assert same_bits(d0, d1) and same_bits(gr0, gr1) and same_bits(c0, c1) and same_bits(ll1, ll2)
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
        assert same_bits(ll0, ll1)
    else:
        xh, ah = xn.dat.cpu().numpy(), Ay.cpu().numpy()
        exact, _ = admm64.masked_sse(xh, ah)
        ref, tol = gn64.weighted_sse(xh, ah, a, np.ones(16, np.float32))
        assert abs(ref - exact) <= 2.0 ** -52 * exact
        err = abs(float(ll1) - 0.5 * tau * exact)
        bound = 0.5 * tau * tol + 2.0 ** -52 * 0.5 * tau * exact  # (the product with tau / 2 rounds once more)
        print('rigid ll at e = 1: err / bound %.3g (ll %r, unweighted %r)' % (err / bound, float(ll1), float(ll0)), flush=True)
        assert err <= bound
    # and whole updates: the same steps
    rig = []
    for gains in (False, True):
        _, xg, yg, sett = _arm(dev, False, False, start=OFFSET)
        sett.gain_gn = True
        x1 = xg[0][1]
        if with_u:
            x1.slice_w = u.clone()
        if gains:
            x1.slice_gain = torch.ones(16, device=dev)
        xg, _ = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=0, samp=0)
        rig.append(xg[0][1].rigid_q.clone())
    assert same_bits(rig[0], rig[1]) and not same_bits(rig[0], torch.tensor(OFFSET, dtype=torch.float64))


# ---- (5) the objective --------------------------------------------------------------------------------------------------------
def test_rigid_objective_is_the_objective_of_compute_nll(dev):
    """User gains (sett.slice_gain off: no ridge); the second repeat with a map, slice weights and gains, the first with
    gains alone: sum_n ll_n of the rigid step at po.rigid, added in _compute_nll's order, has the bits of its nll_xy."""
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _rigid_terms
    from unires_amd._update import _compute_nll, _gn_gain, _gn_weight
    prob, xg, yg, sett = _arm(dev, False, False)
    sett.gain_gn = True
    x0, x1 = xg[0]
    x0.slice_gain = _gains(dev, int(x0.dat.shape[_slice_axis(x0)]))
    x1.slice_gain = gain64.gains(16, 'generic', seed=5).to(dev)
    x1.weight = voxel64.weights((48, 16, 40), 'ramp', seed=5).to(dev)
    x1.slice_w = slice64.weights(16, 'ramp', seed=5).to(dev)
    with torch.cuda.device(dev):
        nll_xy = _compute_nll(xg, yg, sett, prob['rho'])[1]
        ll = torch.zeros((), dtype=torch.float64, device=dev)
        for xn in xg[0]:
            assert _gn_gain(xn, sett) is xn.slice_gain
            ll = ll + _rigid_terms(xn.dat, yg[0].dat, xn.po, xn.tau, xn.po.rigid, sett, slice_w=getattr(xn, 'slice_w', None),
                                   axis=_slice_axis(xn), weight=_gn_weight(xn, sett), gain=_gn_gain(xn, sett))[0]
        # and without the gains in the step it is another number
        other = sum(_rigid_terms(xn.dat, yg[0].dat, xn.po, xn.tau, xn.po.rigid, sett, slice_w=getattr(xn, 'slice_w', None),
                                 axis=_slice_axis(xn), weight=_gn_weight(xn, sett))[0] for xn in xg[0])
    print('rigid objective %r, nll_xy %r (without gains %r)' % (float(ll), float(nll_xy), float(other)), flush=True)
    assert same_bits(ll, nll_xy) and float(other) != float(ll)


# ---- (6) decimation -------------------------------------------------------------------------------------------------------------
def test_update_rigid_decimates_the_gains_with_the_observation(dev):
    """samp = 6 keeps every sk-th slice of the second repeat (48, 16, 40; slices along axis 1), cut to dim_x: changing
    the gains of dropped slices changes no bit, changing a kept one does; with the switch off the gains are ignored."""
    from unires_amd._project import _proj_info
    from unires_amd._rigid import _update_rigid
    base = gain64.gains(16, 'generic')
    res = {}
    for name in ('base', 'dropped', 'kept', 'off', 'none'):
        _, xg, yg, sett = _arm(dev, False, False, start=OFFSET)
        x1 = xg[0][1]
        po = _proj_info(x1.po.dim_y, x1.po.mat_y, x1.po.dim_x, x1.po.mat_x, rigid=x1.po.rigid, prof_ip=sett.profile_ip,
                        prof_tp=sett.profile_tp, gap=sett.gap, device=dev, scl=x1.po.scl, samp=6)
        sk, n = int(po.sk[1]), int(po.dim_x[1])
        kept = list(range(0, 16, sk))[:n]
        assert sk > 1 and 0 < len(kept) < 16
        assert gne64.decimate_gain(np.arange(16), sk, n).tolist() == kept
        e = base.clone()
        if name == 'dropped':
            for s in range(16):
                if s not in kept:
                    e[s] = 1.9 - 0.05 * s
        if name == 'kept':
            e[kept[len(kept) // 2]] *= 1.25
        sett.gain_gn = name != 'off'
        if name != 'none':
            x1.slice_gain = e.to(dev)
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=6)
        res[name] = _rigid_state(xg, sll)
    assert _same_state(res['base'], res['dropped'])
    assert not same_bits(res['base'][0][1], res['kept'][0][1]) and not same_bits(res['base'][2], res['kept'][2])
    assert _same_state(res['off'], res['none'])
    assert not same_bits(res['base'][0][1], res['none'][0][1])


# ---- (7) the denoising regime -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_g', [False, True])
def test_update_rigid_in_the_denoising_regime(dev, with_g):
    """Pull / push only: the Hessian's weight is the volume w_mat[s(v)] (g . w_mat with a map) where the unweighted step
    passes none; the step is rebuilt here from the existing entry points - the residual of u := t on the gained
    prediction, unires_rigid_sums with that volume - and has the update's bits."""
    from tests.helpers import gpu_structs, make_problem
    from unires_amd import _ops
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _expm, _logq, _spread, _update_rigid, _voxel_times, affine_basis
    from unires_amd.spatial import _m12
    prob = make_problem(dim_y=(20, 18, 33), n_channels=1, regime='dn', rot=0.08, trans=1.5, seed=1)
    xg, yg, sett = gpu_structs(prob, dev)
    sett.gain_gn = sett.voxel_gn = True
    xn = xg[0][0]
    a = _slice_axis(xn)
    dim = tuple(int(v) for v in xn.dat.shape)
    S = dim[a]
    u, e = slice64.weights(S, 'ramp', seed=5), gain64.gains(S, 'generic')
    g = voxel64.weights(dim, 'ramp') if with_g else None
    xn.slice_w, xn.slice_gain = u.to(dev), e.to(dev)
    if with_g:
        xn.weight = g.to(dev)
    basis = affine_basis('SE')
    q0 = _logq(xn.po.rigid, basis)
    po, tau, dat_x, y = xn.po, float(xn.tau), xn.dat.contiguous(), yg[0].dat
    w_mat, _, t = gne64.tables(u.numpy(), e.numpy())
    with torch.cuda.device(dev):
        rigid, d_rigid = _expm(q0, basis, grad_X=True)
        D = torch.stack([torch.linalg.solve(po.mat_y, d_rigid[i].mm(po.mat_x)) for i in range(6)])
        M = _m12(torch.linalg.solve(po.mat_y, rigid.mm(po.mat_x)))
        Ay = _ops.pull_affine(y, M, dim).reshape(dim).contiguous()
        gr3 = _ops.pull_grad_affine(y, M, dim).reshape(dim + (3,))
        _, dg = _composition(dev, dat_x.cpu(), Ay.cpu(), g, u, e, dim, a)
        wd = torch.from_numpy(w_mat).to(dev)
        CtC = _spread(wd, dim, a).contiguous() if g is None else _voxel_times(torch.ones(dim, device=dev), g.to(dev), wd, a)
        sums = torch.empty(27, dtype=torch.float64, device=dev)
        d72 = (C.c_float * 72)(*D[:, :3, :].reshape(-1).float().tolist())
        check(_lib().unires_rigid_sums(_ptr(gr3), _ptr(dg.to(dev)), _ptr(CtC), i3(dim), d72, _ptr(sums), _stream()))
        s = sums.cpu().numpy()
    Hes = np.zeros((6, 6))
    Hes[np.triu_indices(6)] = s[6:]
    Hes = Hes + np.triu(Hes, 1).T
    want = q0 - torch.from_numpy(np.linalg.solve(Hes, s[:6]))
    xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=0, samp=0)
    assert same_bits(xg[0][0].rigid_q, want) and not same_bits(want, q0)
    # without the gains in the step: another step
    xg2, yg2, sett2 = gpu_structs(prob, dev)
    sett2.voxel_gn = True
    xg2[0][0].slice_w, xg2[0][0].slice_gain = u.to(dev), e.to(dev)
    if with_g:
        xg2[0][0].weight = g.to(dev)
    xg2, _ = _update_rigid(xg2, yg2, sett2, mean_correct=False, max_niter_gn=1, num_linesearch=0, samp=0)
    assert not same_bits(xg2[0][0].rigid_q, want)


# ---- (8) empty repeats ----------------------------------------------------------------------------------------------------------
def test_a_repeat_with_all_zero_weights_beside_gains_is_left_alone(dev):
    from unires_amd._rigid import _update_rigid
    got = {}
    for name in ('both', 'first'):
        _, xg, yg, sett = _arm(dev, False, False)
        sett.gain_gn = True
        x1 = xg[0][1]
        x1.slice_w = torch.zeros(16, device=dev)
        x1.slice_gain = _gains(dev, 16)
        q1, r1 = x1.rigid_q, x1.po.rigid
        if name == 'first':
            xg = [xg[0][:1]]
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
        assert x1.rigid_q is q1 and x1.po.rigid is r1
        assert bool(torch.isfinite(sll))
        got[name] = (sll.cpu().clone(), xg[0][0].rigid_q.clone())
    assert same_bits(got['both'][0], got['first'][0])  # (the empty repeat adds 0 to sll)
    assert same_bits(got['both'][1], got['first'][1])


# ---- (9) planted motion -------------------------------------------------------------------------------------------------------------
def _star(S):
    return torch.tensor([PATTERN[s % 3] for s in range(S)])


def test_registration_of_a_banded_repeat(dev):
    """The second repeat is the truth seen through OFFSET's rigid, then multiplied slice-wise by (1, 0.85, 1.15)
    repeated; y is the truth and the user's gains are the planted ones.  Three rigid updates from the identity end
    nearer the planted matrix than the start, and sll does not increase; no more is asserted.  The arm that ignores the
    gains (the switch off) is printed for DESIGN.md 8.13."""
    import unires_amd as U
    from unires_amd._rigid import _expm, _update_rigid, affine_basis
    planted = _expm(torch.tensor(OFFSET, dtype=torch.float64), affine_basis('SE'))
    dist, slls = {}, {}
    for arm in ('gains', 'ignored'):
        prob, xg, yg, sett = _arm(dev, False, False)
        sett.gain_gn = arm == 'gains'
        truth = prob['truth'][0].float().to(dev)
        yg[0].dat = truth.clone()
        x1 = xg[0][1]
        x1.po.rigid = planted.clone()
        with torch.cuda.device(dev):
            dat = U._proj('A', truth, xg[0], yg[0], n=1, method=sett.method, do=sett.do_proj).clone()
        star = _star(16)
        x1.dat = (dat.reshape(tuple(x1.dat.shape)) * star.to(dev).reshape(1, 16, 1)).contiguous()
        x1.slice_gain = star.to(dev)
        x1.po.rigid = torch.eye(4, dtype=torch.float64)
        slls[arm] = []
        for _ in range(3):
            xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
            slls[arm].append(float(sll))
        dist[arm] = float((xg[0][1].po.rigid.double().cpu() - planted).norm())
    start = float((torch.eye(4, dtype=torch.float64) - planted).norm())
    print('banded repeat: distance of po.rigid from the planted matrix: start %.4f, with the gains %.4f, ignoring them '
          '%.4f; sll with the gains %s' % (start, dist['gains'], dist['ignored'], ['%.6g' % v for v in slls['gains']]),
          flush=True)
    assert dist['gains'] < start
    assert slls['gains'][1] <= slls['gains'][0] and slls['gains'][2] <= slls['gains'][1]


# ---- (10) plans after a rigid update ---------------------------------------------------------------------------------------------------
def plans_after_rigid(dev):
    """_update_y, _update_rigid on the gained second repeat, _update_y again from the first y on the same structs,
    against _update_y on fresh structs built at the new po.rigid with the same gains and y, and against the same without
    the gains -> what the test below asserts, as a dict of numbers."""
    import unires_amd as U
    from unires_amd._rigid import _update_rigid

    def y_update(prob, xg, yg, sett):
        z, w = prob['z'].to(dev), prob['w'].to(dev)
        tmp = torch.zeros_like(yg[0].dat)
        U._update_y(xg, yg, z, w, prob['rho'], tmp, sett)
        torch.cuda.synchronize(dev)
        return yg[0].dat.clone()

    def structs(rigids=None, gains=True):
        prob, xg, yg, sett = _arm(dev, False, False, start=OFFSET)
        sett.gain_gn = True
        sett.cgs_max_iter, sett.cgs_tol = 5, 0.0
        xg[0][1].dat *= _star(16).to(dev).reshape(1, 16, 1)
        xg[0][1].slice_gain = _star(16).to(dev) if gains else None
        xg[0][1].slice_w = slice64.weights(16, 'ramp', seed=5).to(dev)
        for xn, r in zip(xg[0], rigids or ()):
            xn.po.rigid = r.clone()
        return prob, xg, yg, sett

    prob, xg, yg, sett = structs()
    y0 = yg[0].dat.clone()
    first = y_update(prob, xg, yg, sett)
    yg[0].dat.copy_(y0)
    old = [xn.po.rigid.clone() for xn in xg[0]]
    xg, _ = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
    new = [xn.po.rigid.clone() for xn in xg[0]]
    second = y_update(prob, xg, yg, sett)
    prob2, xg2, yg2, sett2 = structs(new)
    same_start = same_bits(yg2[0].dat, y0)
    fresh = y_update(prob2, xg2, yg2, sett2)
    prob3, xg3, yg3, sett3 = structs(new, gains=False)
    bare = y_update(prob3, xg3, yg3, sett3)
    return dict(moved=int(not torch.equal(old[1], new[1])), same_start=int(same_start),
                fresh_bits=int(same_bits(second, fresh)), differs_from_first=int(not same_bits(second, first)),
                gains_reach=int(not same_bits(bare, fresh)), max_diff=float((second - fresh).abs().max()),
                max_diff_bare=float((bare - fresh).abs().max()), scale=float(fresh.abs().max()))


_PLANS_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_gain_gn import plans_after_rigid
np.savez(sys.argv[1], **plans_after_rigid(torch.device('cuda:0')))
'''


def test_y_update_after_a_rigid_update_sees_the_gains_on_the_new_geometry(dev, tmp_path):
    """After _update_rigid on a gained repeat the plan is rebuilt in place (unires_plan_set_repeat) and keeps the gains:
    _update_y on the same structs has the bits of _update_y on fresh structs built at the new po.rigid with the same
    gains and y - matvec tables, the cached tau At (w e x), the Jacobi diagonal - and not those of the first y-update
    or of the structs without the gains.

    A rebuilt plan packs its splat schedules by the quick rule and a created one by the thorough rule unless
    UNIRES_S2_EXACT=0 and UNIRES_F1_EXACT=0 make creation pack quickly too (tests/test_gpu_set_repeat.py (2): only then
    is a rebuilt plan a fresh plan bit for bit, whatever it carries), and the library reads both once per process: the
    bit identity is taken in one child under that environment.  In this process, under the default rules, the two
    differ by the order of the splat's additions alone; the difference is printed beside the one the gains make, and
    what does not depend on the packing is asserted here too."""
    from tests.test_gpu_mask import _run
    from tests.test_gpu_set_repeat import QUICK_ENV, ROOT
    here = plans_after_rigid(dev)
    print('plans after a rigid update, default packing: max |rebuilt - fresh| %.3g (max |y| %.3g); without the gains '
          'max |bare - fresh| %.3g' % (here['max_diff'], here['scale'], here['max_diff_bare']), flush=True)
    assert here['moved'] and here['same_start'] and here['differs_from_first'] and here['gains_reach']
    res = _run(tmp_path, 'plans_after_rigid', _PLANS_CHILD % dict(root=ROOT), env=QUICK_ENV, timeout=120)
    assert int(res['moved']) and int(res['same_start'])
    assert int(res['fresh_bits']), float(res['max_diff'])
    assert int(res['differs_from_first']) and int(res['gains_reach'])


# ---- (11) fit() ----------------------------------------------------------------------------------------------------------------------
def _fit(dev, gain_gn=True, everything=False):
    import unires_amd as U
    _, xg, yg, sett = _arm(dev, False, False, start=OFFSET)
    xg[0][1].dat *= _star(16).to(dev).reshape(1, 16, 1)
    yg[0].lam0 = float(yg[0].lam) / 4.0
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 4, 1e-4, 4.0, 0
    sett.cgs_max_iter, sett.cgs_tol = 5, 0.0
    sett.clean_fov = False
    sett.slice_gain, sett.gain_gn, sett.unified_rigid, sett.rigid_mod = True, gain_gn, True, 1
    sett.voxel_gn = everything
    sett.slice_robust = sett.voxel_robust = everything
    dat, _, R, info = U.fit(xg, yg, sett)
    torch.cuda.synchronize()
    assert info['n_iter'] == 4
    return dat.cpu(), R.clone(), info['slice_gain']


def test_fit_with_gains_and_unified_rigid(dev):
    """slice_gain, gain_gn, unified_rigid every iteration, 4 ADMM x 5 CG iterations, the banded second repeat started at
    OFFSET: it runs, repeats bit for bit, and the second repeat's R ends nearer the matrix the phantom was made with
    (the identity) than the start; with slice_robust, voxel_robust and voxel_gn on as well it runs and repeats; with
    gain_gn off the same call raises tests/test_gain.py's pinned NotImplementedError."""
    from unires_amd._rigid import _expm, affine_basis
    a, b = _fit(dev), _fit(dev)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    for ea, eb in zip(a[2][0], b[2][0]):
        assert ea.dtype == torch.float32 and ea.device.type == 'cpu' and same_bits(ea, eb)
    eye = torch.eye(4, dtype=torch.float64)
    R0 = _expm(torch.tensor(OFFSET, dtype=torch.float64), affine_basis('SE'))
    d0, d1 = float((R0 - eye).norm()), float((a[1][1] - eye).norm())
    print('fit with gains and unified_rigid: distance of R[1] from the identity: start %.4f, end %.4f; gains of the '
          'second repeat %s' % (d0, d1, [float('%.3f' % v) for v in a[2][0][1].tolist()]), flush=True)
    assert d1 < d0
    c, d = _fit(dev, everything=True), _fit(dev, everything=True)
    assert same_bits(c[0], d[0]) and same_bits(c[1], d[1])
    for ec, ed in zip(c[2][0], d[2][0]):
        assert same_bits(ec, ed)
    with pytest.raises(NotImplementedError, match='sett.unified_rigid'):
        _fit(dev, gain_gn=False)
