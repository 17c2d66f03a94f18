"""sett.mask_zeros on the GPU: the y-update's system with the zero voxels of an observation treated as missing,

    ( sum_n tau_n A_n^T diag(m_n) A_n + rho lam^2 D^T D ) y = b,        m_n(v) = [x_n(v) != 0]

(a) the matvec q and the Jacobi diagonal per voxel against float64, for every form an unmasked plan would have taken
    in one kernel (k_ata1, k_ata_shift*, k_ata_aligned*, the hybrid) and for the forms that stay; (b) bit identities in
    fresh processes; (c) CG against the dense float64 solution; (d) the captured solve after set_missing; (e) fit().

The reference has no counterpart (its AtA has no mask), so nothing here is pinned against it: the float64 side is
tests/ref64.py's Operator64 with the mask put between its A and its At.

The tolerance of (a) is ``ref64.bound_matvec_reps`` of the UNMASKED operator.  It stays a bound: a masked repeat
runs the same forward and the same push around a pass that multiplies by 1 (exact) or stores 0 (exact), and every
magnitude sum of the bound (M = |A|^T |A| |p|, G, D) only loses non-negative terms when entries of the intermediate
are zeroed.  Ties (voxels a grid point within reach of an in-FOV threshold can change) are excluded under
tests/test_gpu_voxelwise.py's cap, fewer than 1 % of the volume.

The Jacobi diagonal M = tau A^T (m . A 1) + 2 rho lam^2 sum_d 1 / vx_d^2 is held to
(u + 2^-53) (c_AtA + C_DTD) (tau |A|^T |A| 1 + const) + tau (G + D): the A^T A chain of ones, the product with tau and
the add of the constant (2 of C_DTD's 20), and the constant's own float32 chain - 1 / (vx vx) per axis (2 each), their
sum (2), rho lam^2 (2), the factor 2 (exact), the product (1): 11 roundings, inside the rest of C_DTD.

Children are started the way tests/test_gpu_voxelwise.py starts them: one at a time, each under a time limit, and
after a child that exited non-zero or timed out nothing more is started on the GPU.

Observed on an MI355X (largest err / tol over the masks of a case; no voxel excluded as a tie in any case): the matvec
z_rigid 0.047 (all-zero observation 0.037), dn_rigid 0.165, translate 0.039, int_shift 0.025, iso 0.039, orient_9
0.046, sr_2rep 0.099, identity 0.016, z_central 0.091; the Jacobi diagonal 0.002 - 0.053, dn_rigid 0.223; the objectives
below 0.001 of their bound.  CG: 31 iterations, 1.8e-7 from the dense solution (the unmasked system's solution is 0.18
away).  fit(): RMSE inside the slab's footprint 77.2 with the setting off, 21.6 with it on; outside 1.4e-6 relative.
Three masked channels on streams of their own against one after the other: inside 1e-5 in three attempts.

Every test of this file fails on the commit before the setting existed: ``_channel_plan`` has no ``mask_zeros``,
``ChannelPlan`` no ``set_missing``, the library no ``unires_plan_set_missing``.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_voxelwise import _DN, _ISO, _Z, inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-4  # tests/test_gpu_diff.py's, for the dense solve
KINDS = ('slab', 'box', 'random30')
SEED = 11  # tests/test_gpu_voxelwise.py's


def zeroed(dat, kind):
    """A copy of the observation with the voxels of mask ``kind`` set to 0 (the caller's layout): 'slab': the first
    third of its slices (whole slices along the last axis); 'box': the corner box of half the extent along every
    axis; 'random30': 30 % of the voxels; 'zeros': all of them; 'none': none."""
    out = dat.clone()
    nx, ny, nz = out.shape
    if kind == 'slab':
        out[:, :, :max(1, nz // 3)] = 0
    elif kind == 'box':
        out[:max(1, nx // 2), :max(1, ny // 2), :max(1, nz // 2)] = 0
    elif kind == 'random30':
        gen = torch.Generator().manual_seed(29)
        out[(torch.rand(tuple(out.shape), generator=gen) < 0.3).to(out.device)] = 0
    elif kind == 'zeros':
        out.zero_()
    else:
        assert kind == 'none', kind
    return out


def _case(kw, expect, masked=(0,), diff='forward', kinds=KINDS, obj=False):
    return dict(kw=kw, expect=expect, masked=list(masked), diff=diff, kinds=list(kinds), obj=obj)


_two_kernel = lambda i: i['masked'] and not i['shift'] and not i['fused']
CASES = {
    # the z-profile pair under a general rigid; the last mask also through the objective epilogue ('max_gain_fresh');
    # first an all-zero observation: q is the stencil term alone
    'z_rigid': _case(_Z, lambda i: _two_kernel(i) and i['pull2'] and i['splat2_axis'] == 2, kinds=('zeros',) + KINDS,
                     obj=True),
    # the denoising regime under a general rigid: would be k_ata1
    'dn_rigid': _case(_DN, lambda i: _two_kernel(i) and i['pull2'] and i['splat2_axis'] == -1, obj=True),
    # a pure translation: would be k_ata_shift*
    'translate': _case(dict(_Z, dim_y=(41, 38, 60), rot=0.0), _two_kernel),
    # identity + integer shift with a z profile: would be k_ata_aligned*
    'int_shift': _case(dict(_Z, shift=(2.0, -1.0, 3.0)), _two_kernel),
    # an x / y / z profile: would be the hybrid (pull2 + AXIS 2 splat with 1-D passes either side)
    'iso': _case(_ISO, lambda i: _two_kernel(i) and i['splat2_axis'] != 2),
    # an observation stored in a permuted, flipped orientation: the mask is kept in the canonical layout
    'orient_9': _case(dict(_Z, thick=4, scl=0.0, orient=9),
                      lambda i: _two_kernel(i) and (i['perm'] != (0, 1, 2) or any(i['flip']))),
    # two repeats, only the second masked (tests/test_gpu_voxelwise.py's sr_2rep)
    'sr_2rep': _case(dict(dim_y=(41, 38, 61), thick=4, n_repeats=2, rot=0.1, trans=2.0, scl=0.1), None, masked=(1,)),
    # A = I: the channel's plan is a denoising-regime plan with the identity affine (tests/test_gpu_voxelwise.py's identity)
    'identity': _case(dict(dim_y=(37, 41, 53), regime='id'), _two_kernel),
    'z_central': _case(_Z, _two_kernel, diff='central'),
}

_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import SIGNED_PERMS, make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED, zeroed
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan
cases, out = json.loads(%(cases)r), sys.argv[1]
res = {}
d = lambda t: t.to('cuda:0')
for name, case in cases.items():
    kw = case['kw']
    if 'orient' in kw:
        kw = dict(kw, orient=[SIGNED_PERMS[kw['orient']]])
    prob = make_problem(seed=SEED, **kw)
    xg, yg, sett = gpu_structs(prob, 'cuda:0')
    vx = N.voxel_size(prob['mat_y']).float()
    ident = not prob['do_proj']
    get = lambda: _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, diff=case['diff'],
                                mask_zeros=True if ident else None)
    orig = [xn.dat.clone() for xn in xg[0]]
    assert all(bool((o != 0).all()) for o in orig)
    p = d(inputs(prob['dim_y'], prob['dim_y'])[0])
    rho, lam = prob['rho'], yg[0].lam
    plan = None if ident else get()
    for kind in case['kinds']:
        for n in case['masked']:
            xg[0][n].dat = zeroed(orig[n], kind)
            if not ident:
                plan.set_missing(n, xg[0][n].dat)
        if ident:  # the setting's own path: regime choice and masks from the observation tensors (all repeats)
            plan = get()
        key = name + '/' + kind
        res[key + '/info'] = json.dumps([plan.repeat_info(n) for n in range(len(xg[0]))])
        dot = torch.zeros((), dtype=torch.float64, device='cuda:0')
        res[key + '/q'] = plan.matvec(p, rho, lam, dot=dot).cpu().numpy()
        torch.cuda.synchronize()
        res[key + '/dot'] = np.array(dot.item())
        if len(xg[0]) == 1:
            M = torch.empty(prob['dim_y'], dtype=torch.float32, device='cuda:0')
            plan.precond_build(rho, lam, mode='jacobi', out=M)
            res[key + '/M'] = M.cpu().numpy()
    if case['obj']:
        # a 'max_gain_fresh' solve of one iteration from x0 = p: trace[1] comes from the objective epilogue of the push
        b = plan.rhs([xn.dat for xn in xg[0]], d(prob['w'][0]), d(prob['z'][0]), rho, lam)
        x = p.clone()
        it, trace = plan.cg(b, x, rho, lam, max_iter=1, tolerance=1e-3, stop='max_gain_fresh')
        torch.cuda.synchronize()
        assert it >= 1, it
        res[name + '/b'] = b.cpu().numpy()
        res[name + '/obj1'] = np.array(trace[1])
        res[name + '/x1'] = x.cpu().numpy()
        res[name + '/q1'] = plan.matvec(x, rho, lam).cpu().numpy()
np.savez(out, **res)
'''

_DEAD = []  # set by the first child that exits non-zero or times out: nothing more runs on the GPU after it


def _run(tmp_path, tag, script, env=None, timeout=120):
    assert not _DEAD, ('an earlier child died: not started', _DEAD)
    path = str(tmp_path / ('%s.npz' % tag))
    e = dict(os.environ)
    e.update(env or {})
    try:
        r = subprocess.run([sys.executable, '-c', script, path], env=e, capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, (tag, r.returncode, r.stderr[-3000:])
    except (AssertionError, subprocess.TimeoutExpired) as err:
        _DEAD.append((tag, repr(err)[:300]))
        raise
    return dict(np.load(path))


def reference(case):
    """The float64 side of a case, everything that does not depend on the mask: the problem, one Operator64 per
    repeat with its parts of A^T A p and of A^T A 1, A p per repeat, the union of the tie masks."""
    from oracle import nitorch_restated as N
    from tests import ref64
    from tests.helpers import SIGNED_PERMS, make_problem, oracle_structs
    kw = case['kw']
    if 'orient' in kw:
        kw = dict(kw, orient=[SIGNED_PERMS[kw['orient']]])
    prob = make_problem(seed=SEED, **kw)
    xs, ys = oracle_structs(prob)
    xc, yc = xs[0], ys[0]
    R = dict(prob=prob, xc=xc, lam=yc.lam, vx=N.voxel_size(prob['mat_y']).float(), taus=[xn.tau for xn in xc],
             rho=torch.tensor(prob['rho'], dtype=torch.float32), p=inputs(prob['dim_y'], prob['dim_y'])[0])
    method = prob['method']
    R['ops'] = [ref64.Operator64(xn.po, method) for xn in xc]
    R['myy'] = torch.zeros(prob['dim_y'], dtype=torch.bool)
    for op, xn in zip(R['ops'], xc):
        R['myy'] |= op.tie_masks(xn.po)[2]
    R['parts'] = [op.parts_AtA(R['p']) for op in R['ops']]
    R['Ap'] = [op.A(R['p'].double()) for op in R['ops']]
    return R


def masks_of(case, R, kind):
    """m_n over x space (the caller's layout), float64 0 / 1, per repeat: ones for a repeat without a mask."""
    out = []
    for n, xn in enumerate(R['xc']):
        masked = n in case['masked'] or not R['prob']['do_proj']  # (A = I: the setting masks every repeat)
        z = zeroed(xn.dat, kind if n in case['masked'] else 'none')
        out.append((z != 0).double() if masked else torch.ones(tuple(xn.dat.shape), dtype=torch.float64))
    return out


def masked_matvec64(case, R, kind, p=None):
    """(ref, tol): sum_n tau_n At_n(m_n . A_n p) + rho lam^2 D^T D p in float64, and ref64.bound_matvec_reps's
    tolerance of the unmasked operator."""
    from tests import ref64
    p = R['p'] if p is None else p
    parts = R['parts'] if p is R['p'] else [op.parts_AtA(p) for op in R['ops']]
    ref, tol = ref64.bound_matvec_reps(R['ops'], R['taus'], p, R['rho'], R['lam'], R['vx'], case['diff'], parts=parts)
    ms = masks_of(case, R, kind)
    for n, (op, tau, m) in enumerate(zip(R['ops'], R['taus'], ms)):
        Ap = R['Ap'][n] if p is R['p'] else op.A(p.double())
        ref = ref + ref64._f32(tau) * (op.At(m * Ap) - parts[n][0])  # (the unmasked term out, the masked one in)
    return ref, tol


def check_case(name, case, res, R=None):
    from tests import ref64
    R = reference(case) if R is None else R
    p, myy = R['p'], R['myy']
    n_vox = p.numel()
    assert int(myy.sum()) < 0.01 * n_vox, (name, 'tie cap', int(myy.sum()))
    p64 = p.double()
    rep = {}
    for kind in case['kinds']:
        key = name + '/' + kind
        infos = json.loads(str(res[key + '/info']))
        for n, info in enumerate(infos):
            info['perm'], info['flip'] = tuple(info['perm']), tuple(info['flip'])
            masked = n in case['masked'] or not R['prob']['do_proj']
            assert info['masked'] == masked, (key, n, info)
            if masked:  # the one-kernel matvecs and the single-pass kernel were not taken
                assert not info['shift'] and not info['fused'], (key, n, info)
        assert case['expect'] is None or case['expect'](infos[0]), (key, infos)
        q = torch.from_numpy(res[key + '/q'])
        refq, tolq = masked_matvec64(case, R, kind)
        r = ref64.compare(q, refq, tolq, myy)
        print('mask %-22s matvec err/tol %.3f (excluded %d)' % (key, r['max_ratio'], r['excluded']), flush=True)
        assert r['ok'], (key, 'matvec', r)
        rep[kind] = r['max_ratio']
        # the mask did something: the unmasked reference is further away than the bound somewhere
        if kind != 'none' and case['diff'] == 'forward':
            ref_u, _ = ref64.bound_matvec_reps(R['ops'], R['taus'], p, R['rho'], R['lam'], R['vx'], case['diff'],
                                              parts=R['parts'])
            assert not ref64.compare(q, ref_u, tolq, myy)['ok'], (key, 'the matvec is the unmasked one')
        # the dot: a float64 sum of products p q formed in float32 (forward's epilogue; exact for the closing pass)
        pq = p64 * q.double()
        slack = float(pq.abs().sum()) * (ref64.U + (n_vox + 32) * 2.0 ** -53)
        assert abs(float(res[key + '/dot']) - float(pq.sum())) <= slack, (key, 'dot')
        if key + '/M' in res:
            op, tau = R['ops'][0], ref64._f32(R['taus'][0])
            if 'ones' not in R:
                one = torch.ones(R['prob']['dim_y'])
                R['ones'] = (op.parts_AtA(one), op.A(one.double()))
            (_, M1, G1, D1), A1 = R['ones']
            m = masks_of(case, R, kind)[0]
            vx = [float(v) for v in R['vx'].double()]
            c = ref64._f32(R['rho']) * ref64._f32(R['lam']) ** 2
            const = 2.0 * c * sum(1.0 / (v * v) for v in vx)
            refM = tau * op.At(m * A1) + const
            tolM = (ref64.U + ref64.U64) * (op.c_AtA + ref64.C_DTD) * (tau * M1 + const) + tau * (G1 + D1)
            r = ref64.compare(torch.from_numpy(res[key + '/M']), refM, tolM, myy)
            print('mask %-22s Jacobi err/tol %.3f' % (key, r['max_ratio']), flush=True)
            assert r['ok'], (key, 'Jacobi diagonal', r)
    if case['obj']:
        # tests/test_gpu_voxelwise.py's obj_check: |obj - 0.5 sum (refq - 2 b) x| <= 0.5 sum |x| (tolq + 3 u (|refq|
        # + 2 |b|)) + 0.5 sum_ties |x| |q - refq|, on the iterate the solve left and the stored right-hand side
        kind = case['kinds'][-1]
        x1, b64 = torch.from_numpy(res[name + '/x1']), torch.from_numpy(res[name + '/b']).double()
        ref1, tol1 = masked_matvec64(case, R, kind, p=x1)
        x64 = x1.double()
        tie = float((x64.abs() * (torch.from_numpy(res[name + '/q1']).double() - ref1).abs())[myy].sum())
        want = 0.5 * float(((ref1 - 2 * b64) * x64).sum())
        tol = 0.5 * float((x64.abs() * (tol1 + 3 * ref64.U * (ref1.abs() + 2 * b64.abs()))).sum()) + 0.5 * tie
        got = float(res[name + '/obj1'])
        print('mask %-22s objective |got - want| / tol %.3f' % (name, abs(got - want) / tol), flush=True)
        assert abs(got - want) <= tol, (name, 'objective', got, want, tol)
    return rep


@pytest.mark.parametrize('name', list(CASES))
def test_masked_matvec_and_jacobi_per_voxel_against_float64(tmp_path, name):
    case = CASES[name]
    jcase = dict(case, expect=None)
    res = _run(tmp_path, name, _CHILD % dict(root=ROOT, cases=json.dumps({name: jcase})))
    check_case(name, case, res)


# ---- (b) bit identities ----------------------------------------------------------------------------------------------
BIT_CASES = {'z_rigid': _Z, 'dn_rigid': _DN, 'translate': dict(_Z, dim_y=(41, 38, 60), rot=0.0),
             'int_shift': dict(_Z, shift=(2.0, -1.0, 3.0)), 'iso': _ISO}
TWO_KERNEL_ENV = {'UNIRES_NO_ATA1': '1', 'UNIRES_NO_ALIGNED': '1', 'UNIRES_NO_HYBRID': '1'}

_BIT_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan
cases, masked, out = json.loads(%(cases)r), %(masked)r, sys.argv[1]
res = {}
for name, kw in cases.items():
    prob = make_problem(seed=SEED, **kw)
    xg, yg, sett = gpu_structs(prob, 'cuda:0')
    assert all(bool((xn.dat != 0).all()) for xn in xg[0])  # not a single zero: m = 1 everywhere
    vx = N.voxel_size(prob['mat_y']).float()
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, mask_zeros=masked)
    info = plan.repeat_info(0)
    assert info['masked'] == masked and not (masked and (info['shift'] or info['fused'])), info
    p = inputs(prob['dim_y'], prob['dim_y'])[0].to('cuda:0')
    dot = torch.zeros((), dtype=torch.float64, device='cuda:0')
    res[name + '/q'] = plan.matvec(p, prob['rho'], yg[0].lam, dot=dot).cpu().numpy()
    torch.cuda.synchronize()
    res[name + '/dot'] = np.array(dot.item())
    M = torch.empty(prob['dim_y'], dtype=torch.float32, device='cuda:0')
    plan.precond_build(prob['rho'], yg[0].lam, mode='jacobi', out=M)
    res[name + '/M'] = M.cpu().numpy()
np.savez(out, **res)
'''


def test_an_observation_without_zeros_gives_the_bits_of_the_two_kernel_forms(tmp_path):
    """mask_zeros on an observation without a single zero against the unmasked plan forced onto the same two-kernel
    forms by the existing switches, in fresh processes: q, its dot and the Jacobi diagonal, bit for bit."""
    args = dict(root=ROOT, cases=json.dumps(BIT_CASES))
    on = _run(tmp_path, 'bits_masked', _BIT_CHILD % dict(args, masked=True))
    off = _run(tmp_path, 'bits_forced', _BIT_CHILD % dict(args, masked=False), env=TWO_KERNEL_ENV)
    for name in BIT_CASES:
        for what in ('q', 'dot', 'M'):
            assert np.array_equal(on['%s/%s' % (name, what)], off['%s/%s' % (name, what)]), (name, what)


_ZERO_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan
out = sys.argv[1]
prob = make_problem(seed=SEED, **%(kw)r)
xg, yg, sett = gpu_structs(prob, 'cuda:0')
vx = N.voxel_size(prob['mat_y']).float()
p = inputs(prob['dim_y'], prob['dim_y'])[0].to('cuda:0')
res = {}
# both repeats, the second all zero and masked
xg[0][1].dat = torch.zeros_like(xg[0][1].dat)
plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
plan.set_missing(1, xg[0][1].dat)
assert plan.repeat_info(1)['masked'] and not plan.repeat_info(0)['masked']
res['both'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
plan.close()
# the plan without that repeat
yg[0]._plan = None
plan = _channel_plan(xg[0][:1], yg[0], prob['method'], prob['do_proj'], vx)
res['alone'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
np.savez(out, **res)
'''


def test_an_all_zero_observation_adds_nothing(tmp_path):
    """Two repeats under a general rigid, the second all zero and masked: q has the bits of the plan without that
    repeat (the remaining repeat takes the same two kernels in both plans: a general rigid has no one-kernel form;
    the second repeat's push accumulates exact zeros).  One repeat, all zero: the stencil term alone, within (a)'s
    bound - CASES['z_rigid'] with the mask 'zeros'."""
    kw = CASES['sr_2rep']['kw']
    res = _run(tmp_path, 'all_zero', _ZERO_CHILD % dict(root=ROOT, kw=kw))
    assert np.array_equal(res['both'], res['alone'])
    assert np.abs(res['both']).max() > 0


# ---- (c) CG, (d) the captured solve ---------------------------------------------------------------------------------
def _dense(op):
    ny = int(np.prod(op.dim_y))
    cols = []
    for j in range(ny):
        e = torch.zeros(ny, dtype=torch.float64)
        e[j] = 1.0
        cols.append(op.A(e.reshape(op.dim_y)).reshape(-1))
    return torch.stack(cols, 1).numpy()


def _small(dev):
    from oracle import nitorch_restated as N
    from tests.helpers import gpu_structs, make_problem
    prob = make_problem(seed=41, dim_y=(10, 9, 8), thick=2, n_repeats=2, rot=0.08, trans=0.7, scl=0.05)
    xg, yg, sett = gpu_structs(prob, dev)
    xg[0][1].dat = zeroed(xg[0][1].dat, 'slab')
    return prob, xg, yg, N.voxel_size(prob['mat_y']).float()


def test_cg_converges_to_the_dense_solution_of_the_masked_normal_equations(dev):
    from tests import diff64, ref64
    from tests.helpers import oracle_structs, rel_err
    from unires_amd._project import _channel_plan
    prob, xg, yg, vx = _small(dev)
    xs, ys = oracle_structs(prob)
    dim = prob['dim_y']
    rho, lam = ref64._f32(prob['rho']), ref64._f32(ys[0].lam)
    S = rho * lam * lam * diff64.dense_dtd(dim, [float(v) for v in vx], 'forward')
    for n, xn in enumerate(xs[0]):
        A = _dense(ref64.Operator64(xn.po, prob['method']))
        m = (xg[0][n].dat != 0).double().cpu().numpy().reshape(-1) if n == 1 else np.ones(A.shape[0])
        S = S + ref64._f32(xn.tau) * (A.T @ (m[:, None] * A))
    assert 0 < m.sum() < m.size
    g = torch.Generator().manual_seed(9)
    b = (torch.rand(dim, generator=g) * 0.1).float()
    want = np.linalg.solve(S, b.double().numpy().ravel()).reshape(dim)
    # enough iterations to converge, and no more (tests/test_gpu_diff.py: 2 r^n <= 1e-6 in the A-norm)
    sk = float(np.sqrt(np.linalg.cond(S)))
    n_it = int(np.ceil(np.log(0.5e-6) / np.log((sk - 1.0) / (sk + 1.0))))
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
    plan.set_missing(1, xg[0][1].dat)
    assert plan.repeat_info(1)['masked'] and not plan.repeat_info(0)['masked']
    x = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), x, rho, lam, max_iter=n_it, tolerance=0.0)
    err = rel_err(x.cpu(), torch.from_numpy(want))
    # ... and it is not the solution of the unmasked system
    plan.set_missing(1, None)
    xu = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), xu, rho, lam, max_iter=n_it, tolerance=0.0)
    print('masked CG: %d iterations, rel_err %.3g; unmasked solution %.3g away' % (n_it, err, rel_err(xu.cpu(), torch.from_numpy(want))),
          flush=True)
    assert err < GATE
    assert rel_err(xu.cpu(), torch.from_numpy(want)) > 10 * GATE
    plan.close()


def test_set_missing_drops_the_captured_solve(dev):
    """Two tol = 0 solves on one plan (the second replays the captured graph), set_missing, a third solve: the bits
    of a fresh plan with that mask, not the captured result; a change of the observation's values and clearing the
    mask follow the same way."""
    from unires_amd._plan import ChannelPlan
    prob, xg, yg, vx = _small(dev)
    reps = [(xn.po, xn.tau) for xn in xg[0]]
    vxl = [float(v) for v in vx]
    rho, lam = float(prob['rho']), float(yg[0].lam)
    g = torch.Generator().manual_seed(2)
    b = (torch.rand(prob['dim_y'], generator=g) * 0.1).to(dev)
    x0 = prob['y0'][0].to(dev)

    def solve(plan):
        x = x0.clone()
        plan.cg(b, x, rho, lam, max_iter=6, tolerance=0.0)
        torch.cuda.synchronize()
        return x

    def fresh(dat):
        pl = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
        if dat is not None:
            pl.set_missing(1, dat)
        x = solve(pl)
        pl.close()
        return x

    plan = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
    first = solve(plan)
    assert torch.equal(solve(plan), first)
    slab, box = xg[0][1].dat, zeroed(xg[0][1].dat, 'box')
    plan.set_missing(1, slab)
    got = solve(plan)
    assert torch.equal(solve(plan), got)
    assert not torch.equal(got, first)
    assert torch.equal(got, fresh(slab))
    plan.set_missing(1, box)  # the observation's values changed
    got2 = solve(plan)
    assert not torch.equal(got2, got) and torch.equal(got2, fresh(box))
    plan.set_missing(1, None)
    assert torch.equal(solve(plan), first)
    plan.close()


# ---- (e) end to end ---------------------------------------------------------------------------------------------------
def test_fit_recovers_a_zero_filled_slab(dev):
    """A 48 x 48 x 40 phantom, one channel, two repeats with 3 mm slices (thick along z and along y), the second
    zero-filled over a quarter of its slices; fit() for 3 iterations with mask_zeros off and on.  Inside the slab's
    footprint the reconstruction with the setting is closer to the phantom; outside it, away from its border by the
    reach of the operators and the stencil, the two agree to 1e-4 relative.

    The solves run 20 CG iterations with cgs_tol = 0.  The two settings solve different systems, and a solve stopped by
    the default rule (gain below 1e-3) leaves an error of that order spread over the WHOLE volume, different for each
    system: the far field would then compare two stopping errors, not the two solutions (measured so: 1.2e-3).  Twenty
    iterations from the previous ADMM iterate at this system's condition number (below 20: the A-norm error falls by
    0.62 per iteration at least, 1e-4 in all) leave the solutions themselves, whose difference decays with the
    distance from the slab by the screened-Poisson length sqrt(rho lam^2 / tau), a fraction of a voxel here.

    Observed on an MI355X: RMSE inside 77.167 (off), 21.641 (on); outside 1.39e-6 (the test prints them)."""
    import unires_amd as U
    from tests.helpers import gpu_structs, make_problem
    dim = (48, 48, 40)
    N_ADMM = 3
    prob = make_problem(seed=5, dim_y=dim, thick=3, n_repeats=2, rot=0.0, trans=0.0, noise_sd=5.0,
                        thick_axes=None, shift=(0.0, 0.0, 0.0))
    truth = prob['truth'][0]
    out = {}
    for on in (False, True):
        xg, yg, sett = gpu_structs(prob, dev)
        x1 = xg[0][1].dat  # thick along y: (48, 16, 40); its slices are planes of constant y
        nsl = x1.shape[1] // 4
        x1[:, :nsl, :] = 0
        yg[0].lam0 = float(yg[0].lam) / 4.0
        sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = N_ADMM, 1e-4, 4.0, 0
        sett.cgs_max_iter, sett.cgs_tol = 20, 0.0
        sett.clean_fov = False
        sett.mask_zeros = on
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == N_ADMM
        out[on] = dat[..., 0].cpu()
    # the slab's footprint in y space: y < 3 nsl.  The rows of the two systems differ within the reach of A^T A across
    # its border: a 3 mm slice's profile (4 taps) and a trilinear corner, 3 voxels, once for A and once for A^T: 6.
    # From there the difference travels through the z / w update: every ADMM iteration applies D to y and D^T to
    # w - rho z in the next right-hand side, one voxel each, so after N_ADMM iterations it has reached 6 + 2 N_ADMM
    # voxels past the border; beyond that only the tail of the solves' Green's function is left (it falls by e per
    # sqrt(rho lam^2 / tau), a third of a voxel here).  Measured with 12 iterations: 1.6e-4 from 6 voxels on, 6.6e-6
    # from 12 on - the front, not a solve's error.  Inside leaves out the last thick slice before the border, whose
    # voxels the first valid slice's profile still reaches
    edge = 3 * nsl
    inside = (slice(None), slice(0, edge - 3), slice(None))
    outside = (slice(None), slice(edge + 6 + 2 * N_ADMM, None), slice(None))
    rmse = lambda a, s: float(((a[s].double() - truth[s].double()) ** 2).mean().sqrt())
    r_off, r_on = rmse(out[False], inside), rmse(out[True], inside)
    far = float((out[True][outside].double() - out[False][outside].double()).norm() / out[False][outside].double().norm())
    print('fit with a zero-filled slab: RMSE inside the footprint off %.3f on %.3f; outside rel. difference %.3g'
          % (r_off, r_on, far), flush=True)
    assert r_on < r_off
    assert far <= 1e-4


# ---- the channels of a y-update on streams of their own ----------------------------------------------------------------
def test_masked_y_update_on_channel_streams(dev):
    """Three channels with mask_zeros, every observation zero-filled over a slab: _update_y with the channels on
    streams of their own against one channel after the other, on fresh structs each time (the masks are built in the
    first y-update, on the main stream, and read by the solves on the channels' streams: the update fetches its plans
    before it records the event those streams wait for).  The two runs differ by the order of the float64 sums alone
    (a plan told about its neighbours sizes its grids for them): the alpha and beta of an iteration agree to 1e-12,
    the float32 iterates to a few ulps per iteration - 1e-5 after 8 iterations, where a solve that read an unwritten
    mask would be off by the unmasked system's distance, which the last assertion shows to be beyond 1e-3."""
    import unires_amd as U
    from tests.helpers import gpu_structs, make_problem, rel_err
    from unires_amd._project import _channel_plan
    prob = make_problem(seed=7, dim_y=(40, 36, 33), n_channels=3, thick=3, rot=0.08, trans=1.0, scl=0.05)

    def run(streams, mask):
        xg, yg, sett = gpu_structs(prob, dev)
        for xc in xg:
            xc[0].dat = zeroed(xc[0].dat, 'slab')
        sett.channel_streams, sett.mask_zeros = streams, mask
        sett.cgs_max_iter, sett.cgs_tol = 8, 0.0
        z, w = prob['z'].to(dev), prob['w'].to(dev)
        tmp = torch.zeros_like(yg[0].dat)
        U._update_y(xg, yg, z, w, prob['rho'], tmp, sett)
        torch.cuda.synchronize()
        for c in range(len(xg)):
            info = _channel_plan(xg[c], yg[c], sett.method, sett.do_proj).repeat_info(0)
            assert info['masked'] == mask, (c, info)
        return [yc.dat.cpu() for yc in yg]

    serial = run(False, True)
    for attempt in range(3):
        side = run(True, True)
        for c in range(3):
            assert rel_err(side[c], serial[c]) < 1e-5, (attempt, c, rel_err(side[c], serial[c]))
    plain = run(True, False)
    assert min(rel_err(plain[c], serial[c]) for c in range(3)) > 1e-3
