"""The per-voxel comparator of tests/ref64.py, checked on the CPU: it is sound (the float32 oracle, a correct
float32 implementation of the same operator, passes it for A, At, AtA and the matvec) and sharp (one voxel off by
10x its tolerance, one 8x4x30 tile off by 1e-3 and one non-zero value outside the operator's support all fail it,
while the relative-L2 gates of the GPU parity tests pass the first two; one x-space row at a block seam of the
stride-2 conv kernels off by 1e-3 fails it too).  The cases of tests/test_gpu_voxelwise.py are held to their
conditions here, on the reference alone: the tie cap, and a comb spacing wider than the footprint of their taps; and
where a one-kernel case is there for the right apron of its z lines, the last x-space slice's share of A^T A p, taken
out of the float32 oracle's result, fails the bound."""
import pytest
import torch

from oracle import nitorch_restated as N
from oracle import unires_restated as O
from tests import ref64
from tests.helpers import make_problem, oracle_structs, rel_err
from tests.test_gpu_voxelwise import (DIFF_CASES, ONE_KERNEL_CASES, SEAM_CASES, diff_reference, inputs, spacings,
                                      tie_cap_ok)

PROBLEMS = {
    'small_thick3': dict(dim_y=(16, 14, 12), thick=3, rot=0.1, trans=0.7),
    'mid_thick6z_scl': dict(dim_y=(41, 38, 61), thick=6, thick_axes=[2], rot=0.12, trans=2.0, scl=0.1),
    'mid_iso2_gauss': dict(dim_y=(34, 30, 36), thick=2, iso=(2, 2, 2), prof_ip=2, rot=0.1, trans=1.0),
    'mid_denoise': dict(dim_y=(33, 29, 40), regime='dn', rot=0.1, trans=2.0),
    # (the sep2_gauss geometry of tests/test_gpu_voxelwise.py, with its seed: no voxel excluded)
    'seam_sep2_gauss': dict(SEAM_CASES['sep2_gauss']['kw'], seed=SEAM_CASES['sep2_gauss']['seed']),
}


def _setup(kw, seed=3):
    kw = dict(kw)
    seed = kw.pop('seed', seed)
    prob = make_problem(seed=seed, **kw)
    xs, ys = oracle_structs(prob)
    xc, yc = xs[0], ys[0]
    po = xc[0].po
    op = ref64.Operator64(po, prob['method'])
    gen = torch.Generator().manual_seed(seed + 1)
    p = (torch.rand(prob['dim_y'], generator=gen) * 10 - 2).float()
    v = (torch.rand(tuple(po.dim_x), generator=gen) * 10 - 2).float()
    return prob, xc, yc, po, op, p, v


def _oracle32(op_name, dat, po, method):
    return O.proj_apply(op_name, dat[None, None], po, method=method)[0, 0]


@pytest.mark.parametrize('name', list(PROBLEMS))
def test_float32_oracle_passes_the_per_voxel_bound(name):
    prob, xc, yc, po, op, p, v = _setup(PROBLEMS[name])
    m = prob['method']
    mx, my, myy, _ = op.tie_masks(po)
    ref, tol = op.bound_A(p)
    r = ref64.compare(_oracle32('A', p, po, m), ref, tol, mx)
    assert r['ok'], ('A', r)
    ref, tol = op.bound_At(v)
    r = ref64.compare(_oracle32('At', v, po, m), ref, tol, my)
    assert r['ok'], ('At', r)
    ref, tol = op.bound_AtA(p)
    r = ref64.compare(_oracle32('AtA', p, po, m), ref, tol, myy)
    assert r['ok'], ('AtA', r)
    rho = torch.tensor(prob['rho'], dtype=torch.float32)
    vx = N.voxel_size(prob['mat_y']).float()
    q32 = O.proj('AtA', p, xc, yc, method=m, do=True, rho=rho, vx_y=vx)
    ref, tol = op.bound_matvec(p, xc[0].tau, rho, yc.lam, vx)
    r = ref64.compare(q32, ref, tol, myy)
    assert r['ok'], ('matvec', r)
    assert r['max_ratio'] > 0.0  # (the oracle's float32 result really differs from the float64 one)


def test_comparator_catches_one_voxel_and_one_tile_that_l2_gates_pass():
    # mid-size, a partial tile on every axis: 97 = 12 * 8 + 1, 90 = 22 * 4 + 2, 121 = 4 * 30 + 1
    prob, xc, yc, po, op, p, v = _setup(dict(dim_y=(97, 90, 121), thick=6, thick_axes=[2], rot=0.12, trans=2.0,
                                             scl=0.1))
    ref, tol = op.bound_AtA(p)
    out = ref.clone()
    assert ref64.compare(out, ref, tol)['ok']
    # (b) one voxel 10x its tolerance off: the relative-L2 gate of the mid-size tests (2e-5) cannot see it
    c = tuple(s // 2 for s in prob['dim_y'])
    bad = out.clone()
    bad[c] += 10 * tol[c]
    assert rel_err(bad, ref) < 2e-5
    r = ref64.compare(bad, ref, tol)
    assert not r['ok'] and r['n_bad'] == 1 and r['first'] == c
    # (c) one 8 x 4 x 30 tile (k_splat2 / k_ata1) scaled by 1 + 1e-3: the 256^3 gate (1e-4) passes it
    bad = out.clone()
    bad[40:48, 44:48, 60:90] *= 1 + 1e-3
    assert rel_err(bad, ref) < 1e-4
    r = ref64.compare(bad, ref, tol)
    assert not r['ok'] and r['n_bad'] > 100


def test_comparator_catches_one_row_at_a_block_seam_that_the_l2_gate_passes():
    """sep2_gauss of tests/test_gpu_voxelwise.py (x space 13 x 35 x 36): k_conv_ydown_xdownup2 owns x-space rows in
    blocks of 32, so row 32 of the x-space intermediate is the first of its second y block.  That row's contribution
    to A^T A p, scaled by 1 + 1e-3 before the conv_up half, fails the per-voxel bound - as the whole row and as the share
    of it that one workgroup forms (x run 1: x-space planes 6 .. 11; z block 0: x-space z 0 .. 31).  The relative-L2
    gate of the path tests (1e-4) passes the workgroup's share (8.6e-5); the whole row comes to 1.29e-4, which that
    gate sees at this size: 35 rows are few.  At benchmark size (192 rows, 4 runs and 6 z blocks a row) a row is
    1 / sqrt(192) of the norm, 7e-5."""
    case = SEAM_CASES['sep2_gauss']
    prob = make_problem(seed=case['seed'], **case['kw'])
    xs, _ = oracle_structs(prob)
    po = xs[0][0].po
    assert tuple(po.dim_x) == (13, 35, 36)
    op = ref64.Operator64(po, prob['method'])
    _, _, myy, _ = op.tie_masks(po)
    p = inputs(prob['dim_y'], po.dim_x)[0]
    ref, tol = op.bound_AtA(p)
    mid = op.A(p.double())
    assert ref64.compare(op.At(mid).float(), ref, tol, myy)['ok']  # (the unplanted product, cast, passes)
    own = 32  # kYXRows of conv.hip with gy = 0
    row = mid.clone()
    row[:, own, :] *= 1 + 1e-3
    share = mid.clone()
    share[6:12, own, 0:32] *= 1 + 1e-3
    for label, x, l2_passes in (('row', row, None), ('one workgroup\'s share', share, True)):
        bad = op.At(x).float()
        r = ref64.compare(bad, ref, tol, myy)
        l2 = rel_err(bad, ref)
        print('seam plant %-22s n_bad %5d max err/tol %.3f rel_err %.3g' % (label, r['n_bad'], r['max_ratio'], l2))
        assert not r['ok'] and r['n_bad'] > 100, (label, r)
        if l2_passes:
            assert l2 < 1e-4, (label, l2)


def test_comparator_demands_exact_zero_outside_the_support():
    # one impulse: A^T A e_j is confined to the voxels within reach of the grid points e_j's x voxels read
    prob, xc, yc, po, op, p, v = _setup(PROBLEMS['mid_thick6z_scl'])
    e = torch.zeros(prob['dim_y'])
    e[20, 19, 30] = 1.0
    ref, tol = op.bound_AtA(e)
    assert (tol == 0).any() and (tol > 0).any()
    r = ref64.compare(_oracle32('AtA', e, po, prob['method']), ref, tol)
    assert r['ok'], r
    far = tuple(int(i) for i in torch.nonzero(tol == 0)[0])
    bad = ref.clone()
    bad[far] = 1e-30  # (d) a single non-zero value outside the support
    r = ref64.compare(bad, ref, tol)
    assert not r['ok'] and r['first'] == far


# ---- sett.diff = 'backward' / 'central': the matvec and right-hand side bounds with a `which` ------------------------
NONFWD = ('backward', 'central')
ANISO = (0.8, 1.25, 2.0)
NF_PROBLEMS = {
    'mid_thick6z_scl': PROBLEMS['mid_thick6z_scl'],
    'mid_denoise': PROBLEMS['mid_denoise'],
    'sr_2rep': dict(dim_y=(41, 38, 61), thick=4, n_repeats=2, rot=0.1, trans=2.0, scl=0.1),
    'dn_aniso': dict(PROBLEMS['mid_denoise'], aniso=ANISO),
}
_NF_CACHE = {}


def _nf_setup(name, seed=3):
    """The problem, one Operator64 per repeat with the unions of their tie masks, the input p, and what does not
    depend on the difference (the repeats' A^T A parts of p, the A^T bounds of their observations): built once."""
    if name not in _NF_CACHE:
        prob = make_problem(seed=seed, **NF_PROBLEMS[name])
        xs, ys = oracle_structs(prob)
        xc, yc = xs[0], ys[0]
        ops = [ref64.Operator64(xn.po, prob['method']) for xn in xc]
        my = torch.zeros(prob['dim_y'], dtype=torch.bool)
        myy = my.clone()
        for op, xn in zip(ops, xc):
            _, a, b, _ = op.tie_masks(xn.po)
            my |= a
            myy |= b
        gen = torch.Generator().manual_seed(seed + 1)
        p = (torch.rand(prob['dim_y'], generator=gen) * 10 - 2).float()
        _NF_CACHE[name] = dict(
            prob=prob, xc=xc, yc=yc, ops=ops, my=my, myy=myy, p=p, taus=[xn.tau for xn in xc],
            rho=torch.tensor(prob['rho'], dtype=torch.float32), vx=N.voxel_size(prob['mat_y']).float(),
            parts=[op.parts_AtA(p) for op in ops], at=[op.bound_At(xn.dat) for op, xn in zip(ops, xc)])
    return _NF_CACHE[name]


def _nf_bounds(S, which):
    q = ref64.bound_matvec_reps(S['ops'], S['taus'], S['p'], S['rho'], S['yc'].lam, S['vx'], which, parts=S['parts'])
    b = ref64.bound_rhs(S['ops'], S['taus'], [xn.dat for xn in S['xc']], S['prob']['w'][0], S['prob']['z'][0],
                        S['rho'], S['yc'].lam, S['vx'], which, at=S['at'])
    return q, b


@pytest.mark.parametrize('which', NONFWD)
@pytest.mark.parametrize('name', list(NF_PROBLEMS))
def test_float32_composition_passes_the_backward_and_central_bounds(monkeypatch, name, which):
    """Sound: the float32 oracle with its gradient / divergence replaced by `which`'s (tests/test_gpu_diff.py
    ``_patch_oracle``) - a correct float32 implementation of the matvec and of the right-hand side - passes
    ``bound_matvec(which)`` / ``bound_matvec_reps`` and ``bound_rhs`` outside ties, and really differs from float64."""
    from tests.test_gpu_diff import _patch_oracle
    S = _nf_setup(name)
    prob, xc, yc = S['prob'], S['xc'], S['yc']
    assert int(S['myy'].sum()) < 0.01 * S['p'].numel()
    (refq, tolq), (refb, tolb) = _nf_bounds(S, which)
    if len(xc) == 1:  # the method of one repeat is the same bound
        r1, t1 = S['ops'][0].bound_matvec(S['p'], xc[0].tau, S['rho'], yc.lam, S['vx'], which)
        assert torch.equal(r1, refq) and torch.equal(t1, tolq)
    _patch_oracle(monkeypatch, which)
    q32 = O.proj('AtA', S['p'], xc, yc, method=prob['method'], do=True, rho=S['rho'], vx_y=S['vx'], diff=which)
    r = ref64.compare(q32, refq, tolq, S['myy'])
    assert r['ok'] and r['max_ratio'] > 0.0, ('matvec', r)
    b32 = O.y_rhs(xc, yc, prob['z'][0], prob['w'][0], S['rho'], S['vx'], prob['method'], True)
    rb = ref64.compare(b32, refb, tolb, S['my'])
    assert rb['ok'] and rb['max_ratio'] > 0.0, ('rhs', rb)
    print('sound %s %s: matvec %.3f, rhs %.3f of the bound' % (name, which, r['max_ratio'], rb['max_ratio']))


def test_forward_matvec_bound_is_the_parent_formula_bit_for_bit():
    """``bound_matvec`` without a `which` (and with 'forward') returns what it returned before it had one: compared
    with a copy of that formula."""
    prob, xc, yc, po, op, p, v = _setup(PROBLEMS['small_thick3'])
    rho = torch.tensor(prob['rho'], dtype=torch.float32)
    vx = N.voxel_size(prob['mat_y']).float()

    def parent(self, p, tau, rho, lam, vx):
        tau, rho, lam = (float(torch.tensor(float(v), dtype=torch.float32)) for v in (tau, rho, lam))
        vx = torch.as_tensor(vx, dtype=torch.float32).double()
        ref, M, G, D = self.parts_AtA(p)
        c = rho * lam * lam
        p64 = p.double()
        ref = tau * ref + c * O.DtD(p64, vx)
        Md = c * ref64.dtd_abs(p64.abs(), vx)
        tol = (ref64.U + ref64.U64) * (self.c_AtA + ref64.C_DTD) * (tau * M + Md) + tau * G + tau * D
        return ref, tol

    want = parent(op, p, xc[0].tau, rho, yc.lam, vx)
    args = (p, xc[0].tau, rho, yc.lam, vx)
    for got in (op.bound_matvec(*args), op.bound_matvec(*args, 'forward')):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # ... and the `which`-general form states the same operator for 'forward' (its own rounding apart)
    ref2, tol2 = ref64.bound_matvec_reps([op], [xc[0].tau], p, rho, yc.lam, vx, 'forward')
    assert torch.allclose(ref2, want[0], rtol=1e-12, atol=0) and torch.allclose(tol2, want[1], rtol=1e-12, atol=0)


def _stencil(S, which, vx=None, axis_scale=(1.0, 1.0, 1.0)):
    """c DtD_which p in float64 with per-axis factors on the weights (a plant's handle)."""
    from tests import diff64
    c = ref64._f32(S['rho']) * ref64._f32(S['yc'].lam) ** 2
    vx = [float(v) for v in (S['vx'] if vx is None else vx)]
    p = S['p'].double().numpy()
    out = 0.0
    for d in range(3):
        dtd_d = diff64._apply(diff64._apply(p, d, which, False, False), d, which, True, False)
        out = out + axis_scale[d] * dtd_d / vx[d] ** 2
    return c * torch.from_numpy(out)


def _plants(name, which):
    """(label, planted float64 matvec) pairs for the case: each a wrong closing pass a kernel could plausibly run."""
    S = _nf_setup(name)
    (refq, _), _ = _nf_bounds(S, which)
    data = refq - _stencil(S, which)  # sum tau AtA p
    nz = S['p'].shape[2]
    out = [('other stencil', data + _stencil(S, 'forward' if which == 'backward' else 'backward'))]
    if which == 'central':
        out.append(('no 1/4 on y', data + _stencil(S, which, axis_scale=(1.0, 4.0, 1.0))))
        # k = nz - 2 treated as a face: the (p[k + 2] (= 0) - p[k]) / 4 term is dropped there
        vz = float(S['vx'][2])
        c = ref64._f32(S['rho']) * ref64._f32(S['yc'].lam) ** 2
        off = refq.clone()
        off[:, :, nz - 2] -= c * 0.25 / vz ** 2 * S['p'].double()[:, :, nz - 2]
        out.append(('plane nz - 2 a face', off))
    if name == 'dn_aniso':
        out.append(('cx, cz swapped', data + _stencil(S, which, vx=[S['vx'][2], S['vx'][1], S['vx'][0]])))
    if name == 'sr_2rep':
        out.append(('stencil twice', data + 2 * _stencil(S, which)))
        out.append(('no stencil', data))
    ends = refq.clone()  # head and tail of an unaligned q: the first / last 3 voxels of the flat array not closed
    ends.view(-1)[:3] = data.reshape(-1)[:3]
    ends.view(-1)[-3:] = data.reshape(-1)[-3:]
    out.append(('3 + 3 end voxels left at the data term', ends))
    return S, out


@pytest.mark.parametrize('which', NONFWD)
@pytest.mark.parametrize('name', ['mid_denoise', 'dn_aniso', 'sr_2rep'])
def test_comparator_catches_wrong_closing_passes(name, which):
    """Sharp: each planted error, cast to float32, fails ``bound_matvec(which)`` outside ties, in at least as many
    voxels as it touches.  Whether the relative-L2 gate of tests/test_gpu_diff.py (1e-4) would have passed it is
    printed.  Observed: none passes it at these sizes against this reference - the smallest are the six end voxels
    (rel_err 3.4e-3 - 7.2e-3, six voxels at 1.6e5 - 2.4e5 times their tolerance) and central's plane nz - 2 (4.9e-3 -
    2.4e-2); what let such errors through in that test was not the gate's width but its cases (isotropic voxels:
    cx = cy = cz, so swapped weights are the same weights) and its reference (the GPU's own op-level kernels)."""
    S, plants = _plants(name, which)
    (refq, tolq), _ = _nf_bounds(S, which)
    assert ref64.compare(refq.float(), refq, tolq, S['myy'])['ok']  # (the unplanted reference, cast, passes)
    for label, bad in plants:
        bad32 = bad.float()
        r = ref64.compare(bad32, refq, tolq, S['myy'])
        l2 = rel_err(bad32, refq)
        print('plant %s %s %-40s n_bad %6d max err/tol %9.3g rel_err %.3g (%s the 1e-4 gate)'
              % (name, which, label, r['n_bad'], r['max_ratio'], l2, 'passes' if l2 < 1e-4 else 'fails'))
        assert not r['ok'] and r['n_bad'] >= 3, (label, r)


@pytest.mark.parametrize('name', list(DIFF_CASES))
def test_tie_cap_of_the_nonforward_table(name):
    """A condition on the cases of tests/test_gpu_voxelwise.py's DIFF_CASES, met by the reference alone: fewer than
    1 % of the voxels are excluded as FOV ties (none in a volume below 100 voxels), for the matvec and the
    right-hand side."""
    R = diff_reference(DIFF_CASES[name])
    n = R['p'].numel()
    print('ties %s: %d (matvec) %d (rhs) of %d' % (name, int(R['myy'].sum()), int(R['my'].sum()), n))
    assert tie_cap_ok(R), (name, int(R['myy'].sum()), int(R['my'].sum()), n)
    if n < 100:
        assert int(R['myy'].sum()) == 0


@pytest.mark.parametrize('name', list(SEAM_CASES))
def test_tie_cap_and_comb_spacing_of_the_seam_cases(name):
    """Conditions on the seam cases of tests/test_gpu_voxelwise.py, met by the reference alone.  Their seeds are part of
    the cases: with them fewer than 1 % of the voxels are excluded as FOV ties, in x space (A) and in y space (A^T,
    A^T A) - other seeds of the same geometries exclude up to half the volume.  And the impulse combs see every column
    on its own: the y-space spacing is at least the footprint of A^T A along each axis, 2 (taps - 1 + 2) + 1 for the
    taps the plan keeps."""
    case = SEAM_CASES[name]
    prob = make_problem(seed=case['seed'], **case['kw'])
    xs, _ = oracle_structs(prob)
    po = xs[0][0].po
    op = ref64.Operator64(po, prob['method'])
    mx, my, myy, _ = op.tie_masks(po)
    print('ties %s: %d (A) %d (At) %d (AtA)' % (name, int(mx.sum()), int(my.sum()), int(myy.sum())))
    assert int(mx.sum()) < 0.01 * mx.numel() and int(my.sum()) < 0.01 * my.numel() and int(myy.sum()) < 0.01 * myy.numel()
    kept = [int(k.sum()) for k in ref64.trimmed_taps(po.smo_ker_1d)]
    sy, _ = spacings(case['kw'], case['spacing'])
    assert all(s >= 2 * (n - 1 + 2) + 1 for s, n in zip(sy, kept)), (name, sy, kept)


_OK_PROJ = [n for n, c in ONE_KERNEL_CASES.items() if c['kw'].get('regime', 'sr') != 'id']


def _one_kernel_setup(name):
    case = ONE_KERNEL_CASES[name]
    prob = make_problem(seed=case['seed'], **case['kw'])
    xs, _ = oracle_structs(prob)
    po = xs[0][0].po
    return case, prob, po, ref64.Operator64(po, prob['method'])


@pytest.mark.parametrize('name', _OK_PROJ)
def test_tie_cap_and_comb_spacing_of_the_one_kernel_cases(name):
    """Conditions on ONE_KERNEL_CASES of tests/test_gpu_voxelwise.py (A != I), met by the reference alone, as for the
    seam cases: fewer than 1 % of the voxels excluded as FOV ties in x space (A) and in y space (A^T, A^T A), and a
    y-space comb spacing of at least the footprint of A^T A, 2 (taps - 1 + 2) + 1 for the taps the plan keeps."""
    case, prob, po, op = _one_kernel_setup(name)
    mx, my, myy, _ = op.tie_masks(po)
    print('ties %s: %d (A) %d (At) %d (AtA)' % (name, int(mx.sum()), int(my.sum()), int(myy.sum())))
    assert int(mx.sum()) < 0.01 * mx.numel() and int(my.sum()) < 0.01 * my.numel() and int(myy.sum()) < 0.01 * myy.numel()
    kept = [int(k.sum()) for k in ref64.trimmed_taps(po.smo_ker_1d)]
    sy, _ = spacings(case['kw'], case['spacing'])
    assert all(s >= 2 * (n - 1 + 2) + 1 for s, n in zip(sy, kept)), (name, sy, kept)


@pytest.mark.parametrize('name, last', [('tr_zpos', 8), ('int_zpos', 9)])
def test_comparator_catches_a_lost_last_slice_at_the_right_apron(name, last):
    """tr_zpos / int_zpos translate the observation up along z, so that the taps of its last x-space slices reach past
    the end of the z line: what the one-kernel forms read from their right apron (padr > 0).  The float32 oracle's
    A^T A p passes the per-voxel bound; the same product without the last live x-space slice - what a kernel forms
    whose apron is a slice short - fails it, in most of the z lines.  ``last``: that slice.  int_zpos: slice 9 of 10,
    whose grid points lie at z 59 .. 65 of 61, two of them inside.  tr_zpos: slice 9 (z 59.6 .. 65.6 of 60) lies wholly
    outside the FOV and the oracle returns exact zeros for it, so taking it out changes nothing; the last live slice is
    8 (z 53.6 .. 59.6), whose window of the blended line ends at z = 60, one past the line."""
    case, prob, po, op = _one_kernel_setup(name)
    _, _, myy, _ = op.tie_masks(po)
    p = inputs(prob['dim_y'], po.dim_x)[0]
    ref, tol = op.bound_AtA(p)
    m = prob['method']
    assert ref64.compare(_oracle32('AtA', p, po, m), ref, tol, myy)['ok']
    mid = _oracle32('A', p, po, m)
    live = [k for k in range(mid.shape[2]) if float(mid[:, :, k].abs().max()) > 0.0]
    assert live[-1] == last, (name, live)
    mid[:, :, last] = 0.0
    r = ref64.compare(_oracle32('At', mid, po, m), ref, tol, myy)
    print('apron plant %s: slice %d, n_bad %d max err/tol %.3g' % (name, last, r['n_bad'], r['max_ratio']))
    assert not r['ok'] and r['n_bad'] >= prob['dim_y'][0] * prob['dim_y'][1] // 2, (name, r)
