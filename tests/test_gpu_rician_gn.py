"""The Rician noise model in the rigid Gauss-Newton update and the gain estimate on the GPU (sett.rician_gn; DESIGN.md
8.15), in process:

(1) unires_rigid_terms_r bit for bit against the composition of entry points it replaces - unires_slice_apply,
    unires_rigid_terms_e (without gains: unires_slice_sums / unires_voxel_sums), unires_rician_terms, and
    unires_rigid_resid / unires_rigid_resid_g on the effective observation - and against tests/rgn64.py's float64
    statement inside its stated bound; slices along every axis, the arms {none, g, u, e, all}, without ``out``, with it
    and on ay; inputs unchanged, NaN-prefilled outputs fully written, nothing written outside them, two runs the same
    bits; (2) a planted underflow of x R(z): the mask reads the true x; (3) each buffer in turn off its 16-byte
    boundary; (4) the status codes of unires_slice_sums for the same mistakes;
(5) CT repeats and the Gaussian model with the switch on: the bits of the existing path; (6) the rigid objective is
    _compute_nll's; (7) planted motion on Rician data at 1 - 3 sigma; (8) the gain estimate reads the effective
    observation; (9) fit().

Every output of (1) - (3) lies inside a buffer padded with sentinels on both sides.  (1) - (4) and (6) - (9) fail on the
commit before the feature: the library has no ``unires_rigid_terms_r``, the update functions no ``rician=``, and fit()
raises NotImplementedError.
"""
import numpy as np
import pytest
import torch

from tests import admm64, gain64, gn64, rgn64, rician64, slice64, voxel64
from tests.test_gpu_admm64 import PAD, _guard_ok, _lib, _padded, _sums_out
from tests.test_gpu_gn_voxel import _arm
from tests.test_gpu_gn_weights import OFFSET, _rigid_state, _same_state, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(300, 3, 5), (3, 130, 9), (5, 7, 300), (67, 1, 65), (1, 1, 1), (41, 38, 60)]
ARMS = ('none', 'g', 'u', 'e', 'all')
TAU = 0.1  # x in [0, 10), ay in [-2, 8): z = tau x e ay lies on both sides of 0 and of the branch point 3.75
# planted (x, ay) at the first flat offsets of a volume that has them: z = tau x ay at 1e-30, just below and just above
# 3.75, at 2e6, and a negative prediction beyond the branch
PLANTED = ((1, 1.0, 1e-29), (7, 5.0, 7.4999), (11, 5.0, 7.5001), (17, 2000.0, 1e4), (23, 6.0, -9.0))


# ---- (1) the entry point ------------------------------------------------------------------------------------------------
def _inputs(dim, axis):
    """x >= 0 with 30 % zeros and - where there is more than one slice - one slice all zero; ay with exact zeros of both
    signs and negatives; the planted voxels; generic voxel weights, slice weights and gains in [0.5, 2]."""
    gen = torch.Generator().manual_seed(13 + sum(dim) + axis)
    x = (torch.rand(dim, generator=gen) * 10).float()
    x[torch.rand(dim, generator=gen) < 0.3] = 0.0
    ay = (torch.rand(dim, generator=gen) * 10 - 2).float()
    ay.view(-1)[2::7] = 0.0
    ay.view(-1)[3::29] = -0.0
    S = dim[axis]
    if S > 1:
        x.select(axis, S // 2).zero_()
    if x.numel() > 32:  # (the planted voxels: at the k-th flat offsets outside the all-zero slice)
        s_of = torch.arange(S).reshape([S if a == axis else 1 for a in range(3)]).expand(dim).reshape(-1)
        free = torch.nonzero(s_of != S // 2 if S > 1 else torch.ones_like(s_of, dtype=torch.bool)).view(-1)
        for k, xv, av in PLANTED:
            x.view(-1)[free[k]], ay.view(-1)[free[k]] = xv, av
    if S > 1:
        assert not bool(x.select(axis, S // 2).any())
    g = voxel64.weights(dim, 'ramp')
    u = slice64.weights(S, 'ramp', seed=3)
    e = gain64.gains(S, 'generic')
    return x.contiguous(), ay.contiguous(), g, u, e


def _pick(arm, g, u, e):
    return (g if arm in ('g', 'all') else None, u if arm in ('u', 'all') else None, e if arm in ('e', 'all') else None)


def _terms_r(dev, x, ay, g, u, e, dim, axis, form, off=(0, 0, 0, 0), tau=TAU):
    """unires_rigid_terms_r with every volume in a guarded buffer; ``form``: 'null' (no out), 'out', 'inplace' (out is
    ay); ``off``: floats past a 16-byte boundary the views of x, ay, g and out start at (in place out is ay: its
    offset) -> (sums (3 S,) float64, out or None), on the CPU.  The outputs start as NaN."""
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
    ud, ed = None if u is None else u.to(dev), None if e is None else e.to(dev)
    keep = [None if t is None else t.clone() for t in (xv, gv, ud, ed)]
    sb, sv = _sums_out(dev, 3 * S)
    sv.fill_(float('nan'))
    with torch.cuda.device(dev):
        check(_lib().unires_rigid_terms_r(_ptr(xv), _ptr(av), None if g is None else _ptr(gv),
                                          None if u is None else _ptr(ud), None if e is None else _ptr(ed), i3(dim), axis,
                                          tau, _ptr(sv), None if ov is None else _ptr(ov), _stream()))
    torch.cuda.synchronize(dev)
    assert _guard_ok(sb, 3 * S) and _guard_ok(xb, n + ox) and _guard_ok(ab, n + oa)
    assert g is None or _guard_ok(gb, n + og)
    for now, was in zip((xv, gv, ud, ed), keep):  # x, g, u, e are only read
        assert was is None or same_bits(now, was)
    if form != 'inplace':
        assert same_bits(av, ay.reshape(-1).to(dev))
    sums = sv.cpu().clone()
    assert not bool(torch.isnan(sums).any())  # (every one of the 3 S entries is written)
    if ov is None:
        return sums, None
    assert _guard_ok(ob, n + oo) and bool((ob[PAD:PAD + oo] == 0).all())
    out = ov.cpu().reshape(dim).clone()
    assert not bool(torch.isnan(out).any())
    return sums, out


def _composition(dev, x, ay, g, u, e, dim, axis, tau=TAU):
    """What the fused call replaces, from the existing entry points: P = unires_slice_apply(ay, e) (no e: ay itself);
    (X~, L) = unires_rician_terms(x, ay, g, e); SSE and count from unires_rigid_terms_e(x, ay, g, u, e) (no e:
    unires_slice_sums(x, ay) / unires_voxel_sums(x, ay, g)); out = unires_rigid_resid(X~, P, t) /
    unires_rigid_resid_g(X~, P, g, t), t = rgn64.factor32(u, e) -> (sums (3 S,), out, X~, P) on the CPU."""
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    lib = _lib()
    S = dim[axis]
    xd, ad = x.to(dev), ay.to(dev)
    gd = None if g is None else g.to(dev)
    ud, ed = None if u is None else u.to(dev), None if e is None else e.to(dev)
    t = rgn64.factor32(None if u is None else u.numpy(), None if e is None else e.numpy())
    td = None if t is None else torch.from_numpy(t).to(dev)
    Q = lambda v: None if v is None else _ptr(v)
    with torch.cuda.device(dev):
        P = ad
        if e is not None:
            P = torch.empty_like(ad)
            check(lib.unires_slice_apply(_ptr(ad), _ptr(P), _ptr(ed), i3(dim), axis, _stream()))
        xt = torch.empty_like(ad)
        L = torch.empty(S, dtype=torch.float64, device=dev)
        check(lib.unires_rician_terms(_ptr(xd), _ptr(ad), Q(gd), Q(ed), i3(dim), axis, tau, _ptr(xt), _ptr(L), _stream()))
        sums = torch.empty(2 * S, dtype=torch.float64, device=dev)
        if e is not None:
            check(lib.unires_rigid_terms_e(_ptr(xd), _ptr(ad), Q(gd), Q(ud), _ptr(ed), i3(dim), axis, _ptr(sums), None,
                                           _stream()))
        elif g is None:
            check(lib.unires_slice_sums(_ptr(xd), _ptr(ad), i3(dim), axis, _ptr(sums), _stream()))
        else:
            check(lib.unires_voxel_sums(_ptr(xd), _ptr(ad), _ptr(gd), i3(dim), axis, _ptr(sums), _stream()))
        out = torch.empty_like(ad)
        if g is None:
            check(lib.unires_rigid_resid(_ptr(xt), _ptr(P), i3(dim), axis, Q(td), _ptr(out), _stream()))
        else:
            check(lib.unires_rigid_resid_g(_ptr(xt), _ptr(P), _ptr(gd), i3(dim), axis, Q(td), _ptr(out), _stream()))
    torch.cuda.synchronize(dev)
    return torch.cat([sums, L]).cpu(), out.cpu(), xt.cpu(), P.cpu()


def _np(t):
    return None if t is None else t.numpy()


@pytest.mark.parametrize('dim', SHAPES)
def test_rigid_terms_r_bit_for_bit(dev, dim):
    """The bit contract, and against float64: ``out`` within rgn64.terms_r64's bound
        1.01 { |t g| [2^-24 |p| + (2e-6 + 4 2^-24) |x R(z)|] + 3 2^-24 |out| } + (1 + |t g|) 2^-149
    (R's cap of 2e-6 relative, three roundings of z where R's elasticity is at most 1, and the residual's own
    roundings), the SSE and count within their float64 accumulation bounds, L within its own plus rician64's cap on c,
    sum g 1e-6 (1 + |c|)."""
    worst_out = worst_sum = 0.0
    for axis in (0, 1, 2):
        x, ay, g, u, e = _inputs(dim, axis)
        S = dim[axis]
        for arm in ARMS:
            gg, uu, ee = _pick(arm, g, u, e)
            tag = (dim, axis, arm)
            want_sums, want_out, xt, P = _composition(dev, x, ay, gg, uu, ee, dim, axis)
            # the two masks coincide on these inputs: x~ != 0 wherever x != 0 and p != 0
            live = (x != 0) & (P != 0)
            assert bool((xt[live] != 0).all()), tag
            got = {form: _terms_r(dev, x, ay, gg, uu, ee, dim, axis, form) for form in ('null', 'out', 'inplace')}
            for form, (sums, out) in got.items():
                assert same_bits(sums, want_sums), tag + (form,)
                if form != 'null':
                    assert same_bits(out, want_out), tag + (form,)
            again = _terms_r(dev, x, ay, gg, uu, ee, dim, axis, 'out')  # the same bits every run
            assert same_bits(again[0], got['out'][0]) and same_bits(again[1], got['out'][1]), tag
            # float64
            ref, bound, ref_sums, sums_bound = rgn64.terms_r64(x.numpy(), ay.numpy(), axis, _np(gg), _np(uu), _np(ee), TAU)
            err = np.abs(got['out'][1].numpy().astype(np.float64) - ref)
            assert (err <= bound).all(), tag + (float((err / np.where(bound > 0, bound, 1.0)).max()),)
            if (bound > 0).any():
                worst_out = max(worst_out, float((err[bound > 0] / bound[bound > 0]).max()))
            _, z32 = rician64.z32(x.numpy(), ay.numpy(), _np(ee), TAU, axis)
            c64 = rician64.c64(z32.astype(np.float64))  # (at the kernel's own float32 z: the cap is stated there)
            cap = rician64.sums64(1e-6 * (1.0 + np.abs(c64)), _np(gg), axis)[0]
            l64 = rician64.sums64(c64, _np(gg), axis)[0]
            serr = np.abs(got['null'][0].numpy() - np.concatenate([ref_sums[:2 * S], l64]))
            sbound = sums_bound + np.concatenate([np.zeros(2 * S), cap])
            assert (serr <= sbound).all(), tag + (serr, sbound)
            if (sbound > 0).any():
                worst_sum = max(worst_sum, float((serr[sbound > 0] / sbound[sbound > 0]).max()))
        # the all-zero slice: SSE 0, count 0 and L 0; masked voxels +0
        s, out = got['out']
        if S > 1:
            assert float(s[S // 2]) == 0.0 and float(s[S + S // 2]) == 0.0 and float(s[2 * S + S // 2]) == 0.0
        masked = (x.numpy() == 0) | (P.numpy() == 0)
        assert (out.numpy()[masked].view(np.uint32) == 0).all()
    print('rigid_terms_r %s: worst |out - out64| / bound %.3f, worst sums err / bound %.3f' % (dim, worst_out, worst_sum),
          flush=True)


# ---- (2) a planted underflow -----------------------------------------------------------------------------------------------
def test_the_mask_reads_the_true_observation(dev):
    """x = 1e-20, ay = 1e-10 at tau = 0.1: z = 1e-31, R(z) = 5e-32 and x R(z) = 5e-52 underflows to +0 in float32 while
    x != 0 and p != 0.  The composition masks such a voxel (it reads the mask on x~); the fused call does not: its
    residual there is t g (p - 0), the bits of rgn64.resid32, and everywhere else the composition's."""
    dim, axis = (5, 7, 6), 1
    x, ay, g, u, e = _inputs(dim, axis)
    spots = (3, 40, 100)
    for o in spots:
        x.view(-1)[o], ay.view(-1)[o] = 1e-20, 1e-10
    for arm in ARMS:
        gg, uu, ee = _pick(arm, g, u, e)
        want_sums, comp_out, xt, P = _composition(dev, x, ay, gg, uu, ee, dim, axis)
        under = (x != 0) & (P != 0) & (xt == 0)
        assert sorted(torch.nonzero(under.view(-1)).view(-1).tolist()) == list(spots), arm
        sums, out = _terms_r(dev, x, ay, gg, uu, ee, dim, axis, 'out')
        ref = torch.from_numpy(rgn64.resid32(x.numpy(), ay.numpy(), axis, _np(gg), _np(uu), _np(ee), TAU))
        assert same_bits(sums, want_sums), arm
        assert same_bits(out[~under], comp_out[~under]), arm
        # (a slice weight of 0 among the planted voxels' slices gives 0 times p there: not every one is non-zero)
        assert same_bits(out[under], ref[under]) and bool((out[under] != 0).any()) and bool((comp_out[under] == 0).all()), arm


# ---- (3) off a 16-byte boundary --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['x', 'ay', 'g', 'out'])
def test_rigid_terms_r_off_a_16_byte_boundary(dev, which):
    dim = (41, 38, 60)
    off = tuple(int(which == name) for name in ('x', 'ay', 'g', 'out'))
    for axis in (1, 2):
        x, ay, g, u, e = _inputs(dim, axis)
        want_sums, want_out, _, _ = _composition(dev, x, ay, g, u, e, dim, axis)
        for form in (('out',) if which == 'out' else ('null', 'out', 'inplace')):
            sums, out = _terms_r(dev, x, ay, g, u, e, dim, axis, form, off)
            assert same_bits(sums, want_sums), (which, axis, form)
            assert out is None or same_bits(out, want_out), (which, axis, form)


# ---- (4) status codes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', ['x', 'ay', 'sums', 'axis', 'dim', 'out_is_x', 'out_is_g'])
def test_rigid_terms_r_status_codes(dev, bad):
    """A null x, ay or sums, a bad axis and a bad dim give unires_slice_sums' codes; out == x or out == g the
    invalid-argument code; nothing is launched: the NaN-prefilled sums stay NaN."""
    from unires_amd._lib import i3
    lib = _lib()
    dim = (4, 5, 6)
    x, ay, g = (torch.ones(dim, device=dev) for _ in range(3))
    sums = torch.full((18,), float('nan'), dtype=torch.float64, device=dev)
    a = dict(x=x.data_ptr(), ay=ay.data_ptr(), sums=sums.data_ptr(), axis=2, dim=i3(dim), out=None)
    if bad in ('x', 'ay', 'sums'):
        a[bad] = None
    elif bad == 'axis':
        a['axis'] = 3
    elif bad == 'dim':
        a['dim'] = i3((4, 0, 6))
    else:
        a['out'] = x.data_ptr() if bad == 'out_is_x' else g.data_ptr()
    mine = lib.unires_rigid_terms_r(a['x'], a['ay'], g.data_ptr(), None, None, a['dim'], a['axis'], 1.0, a['sums'],
                                    a['out'], None)
    if bad.startswith('out'):
        theirs = 3  # (UNIRES_ERR_ARG)
        assert b'out must not be' in lib.unires_last_error()
    else:
        theirs = lib.unires_slice_sums(a['x'], a['ay'], a['dim'], a['axis'], a['sums'], None)
    torch.cuda.synchronize(dev)
    assert mine == theirs != 0
    assert bool(torch.isnan(sums).all()) and bool((x == 1).all()) and bool((g == 1).all())


# ---- (5) what the switch leaves alone -------------------------------------------------------------------------------------------
def _magnitude(xg):
    for xc in xg:
        for xn in xc:
            xn.dat = xn.dat.abs().contiguous()
    return xg


@pytest.mark.parametrize('case', ['gaussian', 'ct'])
def test_the_switch_leaves_gaussian_and_ct_repeats_alone(dev, case):
    """'gaussian' with sett.rician_gn on, and 'rician' with it on where every repeat is CT: rigid_q, po.rigid and sll
    have the bits of the update without the switch under 'gaussian'; slice weights on the second repeat, so that the
    weighted path is among what is compared.  And the Rician arm differs."""
    from unires_amd._rigid import _update_rigid
    res = {}
    for name in ('base', 'on', 'rician'):
        _, xg, yg, sett = _arm(dev, False, False, start=OFFSET)
        _magnitude(xg)
        xg[0][1].slice_w = slice64.weights(16, 'ramp', seed=5).to(dev)
        if case == 'ct' and name != 'rician':
            for xn in xg[0]:
                xn.ct = True
        if name == 'on':
            sett.rician_gn = True
            sett.noise_model = 'gaussian' if case == 'gaussian' else 'rician'
        if name == 'rician':
            sett.rician_gn, sett.noise_model = True, 'rician'
        xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
        res[name] = _rigid_state(xg, sll)
    assert _same_state(res['base'], res['on'])
    assert not same_bits(res['base'][2], res['rician'][2]) and not same_bits(res['base'][0][1], res['rician'][0][1])


# ---- (6) the objective ------------------------------------------------------------------------------------------------------------
def _rician_structs(dev, sigma_of_median=0.5, seed=3, planted=None):
    """DESIGN.md 8.6's phantom with y the truth and the second repeat Rician: the truth seen through ``planted`` (None:
    the identity), with Rice noise of sigma = ``sigma_of_median`` x the median of the clean prediction - half of the
    volume below 2 sigma at the default - and tau = 1 / sigma^2.  The first repeat keeps its magnitude data.  po.rigid
    of the second repeat is left at the identity."""
    import unires_amd as U
    prob, xg, yg, sett = _arm(dev, False, False)
    _magnitude(xg)
    truth = prob['truth'][0].float().to(dev)
    yg[0].dat = truth.clone()
    x1 = xg[0][1]
    if planted is not None:
        x1.po.rigid = planted.clone()
    with torch.cuda.device(dev):
        clean = U._proj('A', truth, xg[0], yg[0], n=1, method=sett.method, do=sett.do_proj).clone()
    x1.po.rigid = torch.eye(4, dtype=torch.float64)
    clean = clean.reshape(tuple(x1.dat.shape)).double().cpu()
    sigma = sigma_of_median * float(clean.median())
    gen = torch.Generator().manual_seed(seed)
    x1.dat = rician64.rice(clean, sigma, tuple(clean.shape), gen).float().to(dev).contiguous()
    x1.tau = 1.0 / sigma ** 2
    return prob, xg, yg, sett, sigma


@pytest.mark.parametrize('weighted', [True, False])
def test_rigid_objective_is_the_objective_of_compute_nll(dev, weighted):
    """One Rician repeat.  With a map, slice weights and (user) gains the rigid step's ll at po.rigid has the bits of
    _compute_nll's nll_xy: the same sums, the same two dot products, one addition.  Without any, _compute_nll takes the
    Gaussian part from unires_masked_sse and the step from the slice sums: L_s has the same bits, and the Gaussian part
    lies within _slice_ll's float64 bound of the exact sum."""
    from unires_amd import _ops
    from unires_amd._project import _slice_axis, _taps
    from unires_amd._rigid import _grid_matrix, _rigid_terms
    from unires_amd._update import _compute_nll, _gn_gain, _gn_weight, _is_rician, _rician_ll, _rician_terms
    from unires_amd.spatial import _m12
    prob, xg, yg, sett, _ = _rician_structs(dev)
    sett.noise_model, sett.rician_gn, sett.gain_gn, sett.voxel_gn = 'rician', True, True, True
    x1 = xg[0][1]
    xg = [[x1]]
    if weighted:
        x1.slice_gain = gain64.gains(16, 'generic', seed=5).to(dev)
        x1.weight = voxel64.weights((48, 16, 40), 'ramp', seed=5).to(dev)
        x1.slice_w = slice64.weights(16, 'ramp', seed=5).to(dev)
    a = _slice_axis(x1)
    with torch.cuda.device(dev):
        assert _is_rician(x1, sett)
        nll_xy = _compute_nll(xg, yg, sett, prob['rho'])[1]
        kw = dict(slice_w=getattr(x1, 'slice_w', None), axis=a, weight=_gn_weight(x1, sett), gain=_gn_gain(x1, sett))
        ll = _rigid_terms(x1.dat, yg[0].dat, x1.po, x1.tau, x1.po.rigid, sett, rician=True, **kw)[0]
        ll_diff = _rigid_terms(x1.dat, yg[0].dat, x1.po, x1.tau, x1.po.rigid, sett, diff=True, rician=True, **kw)[0]
        gauss = _rigid_terms(x1.dat, yg[0].dat, x1.po, x1.tau, x1.po.rigid, sett, **kw)[0]
        L = _rician_ll(getattr(x1, 'slice_w', None), _rician_terms(xg, yg, sett, write=False)[(0, 0)])
        # (A y as the rigid step forms it: the float64 bound below is about its sums, not about the operator)
        po, dim = x1.po, tuple(x1.po.dim_yx)
        mat, _ = _grid_matrix(po, po.rigid, sett.method)
        Ay = _ops.conv_down(_ops.pull_affine(yg[0].dat, _m12(mat), dim), _taps(po), po.ratio, float(po.scl), po.dim_thick)
    print('rician rigid objective %r, nll_xy %r (gaussian part %r)' % (float(ll), float(nll_xy), float(gauss)), flush=True)
    assert same_bits(ll, ll_diff) and float(gauss) != float(ll)
    if weighted:
        assert same_bits(ll, nll_xy)
        return
    tau = float(x1.tau)
    xh, ah = x1.dat.cpu().numpy(), Ay.reshape(tuple(x1.dat.shape)).cpu().numpy()
    exact, _ = admm64.masked_sse(xh, ah)
    _, tol = gn64.weighted_sse(xh, ah, a, np.ones(16, np.float32))
    # (the product with tau / 2 rounds once, the addition of L once, the subtraction below once)
    bound = 0.5 * tau * tol + 2.0 ** -52 * 0.5 * tau * exact + 2.0 ** -52 * abs(float(ll))
    err = abs((float(ll) - float(L)) - 0.5 * tau * exact)
    print('unweighted: |ll - L - tau/2 SSE| / bound %.3g; ll - nll_xy %.3g' % (err / bound, float(ll) - float(nll_xy)), flush=True)
    assert err <= bound


# ---- (7) planted motion ---------------------------------------------------------------------------------------------------------------
def test_registration_on_rician_data_descends(dev):
    """The second repeat is the truth seen through OFFSET's rigid with Rice noise, half the volume below 2 sigma; y is
    the truth.  Three rigid updates from the identity: sll does not increase, and a step is taken.  The distance
    of po.rigid from the planted matrix is printed for the Rician arm and for the Gaussian one (the switch off: the step
    aligns to the Rician mean) and not asserted: nobody has measured it."""
    from unires_amd._rigid import _expm, _update_rigid, affine_basis
    planted = _expm(torch.tensor(OFFSET, dtype=torch.float64), affine_basis('SE'))
    dist, slls = {}, {}
    for arm in ('rician', 'gaussian'):
        _, xg, yg, sett, sigma = _rician_structs(dev, planted=planted)
        if arm == 'rician':
            sett.noise_model, sett.rician_gn = 'rician', True
        slls[arm] = []
        for _ in range(3):
            xg, sll = _update_rigid(xg, yg, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
            slls[arm].append(float(sll))
        dist[arm] = float((xg[0][1].po.rigid.double().cpu() - planted).norm())
    start = float((torch.eye(4, dtype=torch.float64) - planted).norm())
    print('rician repeat (sigma %.1f): distance of po.rigid from the planted matrix: start %.4f, rician %.4f, gaussian '
          '%.4f; sll rician %s' % (sigma, start, dist['rician'], dist['gaussian'], ['%.6f' % v for v in slls['rician']]),
          flush=True)
    s = slls['rician']
    assert s[1] <= s[0] and s[2] <= s[1]
    assert dist['rician'] != start  # (a step was taken; which arm ends nearer is printed, not asserted)


# ---- (8) the gain estimate ------------------------------------------------------------------------------------------------------------
def test_update_slice_gains_reads_the_effective_observation(dev):
    """After _rician_terms has written x~ at the current (y, e) - what _update_admm does before it - _update_slice_gains
    leaves the bits of gain_rule(unires_gain_sums(x~, A y, g, u)), kappa from the true observation; with the switch off
    (a direct call) it reads the true observation, and the two differ."""
    import unires_amd as U
    from unires_amd._lib import check, i3
    from unires_amd._ops import _ptr, _stream
    from unires_amd._update import _rician_terms, _update_slice_gains, gain_kappa, gain_rule
    got = {}
    for on in (True, False):
        _, xg, yg, sett, _ = _rician_structs(dev)
        sett.noise_model, sett.rician_gn, sett.slice_gain = 'rician', on, True
        x1 = xg[0][1]
        xg = [[x1]]
        x1.slice_gain = gain64.gains(16, 'generic', seed=5).to(dev)
        x1.weight = voxel64.weights((48, 16, 40), 'ramp', seed=5).to(dev)
        x1.slice_w = slice64.weights(16, 'ramp', seed=5).to(dev)
        with torch.cuda.device(dev):
            _rician_terms(xg, yg, sett, sums=False)
            xt = x1._rician_dat.clone()
            assert not torch.equal(xt, x1.dat) and bool(((xt != 0) == (x1.dat != 0)).all())
            Ay = U._proj('A', yg[0].dat, xg[0], yg[0], n=0, method=sett.method, do=sett.do_proj).contiguous()
            sums = torch.empty(48, dtype=torch.float64, device=dev)
            obs = xt if on else x1.dat
            check(_lib().unires_gain_sums(_ptr(obs), _ptr(Ay), _ptr(x1.weight), _ptr(x1.slice_w), i3(x1.dat.shape), 1,
                                          _ptr(sums), _stream()))
            want = gain_rule(sums, x1.tau, gain_kappa(x1, 0.1), 2.0).float()
            _update_slice_gains(xg, yg, sett)
        torch.cuda.synchronize(dev)
        assert same_bits(x1.slice_gain.cpu(), want.cpu()) and same_bits(x1._gain_sums.cpu(), sums.cpu()), on
        assert same_bits(x1._rician_dat, xt)  # (the gain step does not touch the effective observation)
        got[on] = x1.slice_gain.cpu().clone()
    assert not same_bits(got[True], got[False])


# ---- (9) fit() ----------------------------------------------------------------------------------------------------------------------------
def _fit(dev, rician_gn=True):
    import unires_amd as U
    _, xg, yg, sett = _arm(dev, False, False, start=OFFSET)
    _magnitude(xg)
    yg[0].lam0 = float(yg[0].lam) / 4.0
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 4, 1e-4, 4.0, 0
    sett.cgs_max_iter, sett.cgs_tol = 5, 0.0
    sett.clean_fov = False
    sett.noise_model, sett.rician_gn = 'rician', rician_gn
    sett.slice_gain, sett.gain_gn, sett.unified_rigid, sett.rigid_mod = True, True, True, 1
    dat, _, R, info = U.fit(xg, yg, sett)
    torch.cuda.synchronize()
    assert info['n_iter'] == 4
    return dat.cpu(), R.clone(), info['slice_gain'], info['obj']


def test_fit_with_rician_unified_rigid_and_gains(dev):
    """'rician' with rician_gn, unified_rigid every iteration, slice_gain and gain_gn, 4 ADMM x 5 CG iterations, the
    second repeat started at OFFSET: it runs, repeats bit for bit, the objective trace is finite and the rigid update
    moved the second repeat; with rician_gn off the same call raises tests/test_rician.py's pinned NotImplementedError."""
    a, b = _fit(dev), _fit(dev)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[3], b[3])
    for ea, eb in zip(a[2][0], b[2][0]):
        assert ea.dtype == torch.float32 and ea.device.type == 'cpu' and same_bits(ea, eb)
    assert a[3].shape == (4, 3) and bool(torch.isfinite(a[3]).all()) and bool(torch.isfinite(a[0]).all())
    from unires_amd._rigid import _expm, affine_basis
    R0 = _expm(torch.tensor(OFFSET, dtype=torch.float64), affine_basis('SE'))
    assert not torch.equal(a[1][1], R0)
    print('fit with rician_gn: obj %s; gains of the second repeat %s' % (['%.6g' % v for v in a[3][:, 0].tolist()],
          [float('%.3f' % v) for v in a[2][0][1].tolist()]), flush=True)
    with pytest.raises(NotImplementedError, match=r"sett\.unified_rigid with sett\.noise_model = 'rician'"):
        _fit(dev, rician_gn=False)
