"""Per-slice weights on the GPU (sett.slice_robust, _input.slice_w): the y-update's system

    ( sum_n tau_n A_n^T diag(u_n . m_n) A_n + rho lam^2 D^T D ) y = sum_n tau_n A_n^T (u_n . x_n) - lam D^T (w - rho z)

with u_n one weight per slice along po.dim_thick and m_n the validity mask of sett.mask_zeros (or 1).

(1) unires_slice_sums against float64; (2) the weighted matvec, Jacobi diagonal and objective epilogue per voxel against
float64 for tests/test_gpu_mask.py's cases; (3) bit identities in fresh processes; (4) the right-hand side; (5) CG
against the dense solution; (6) the captured solve across a change of weight values; (7) the rule on the device;
(8) fit(); (9) the channels of a y-update on streams of their own.

The reference has no counterpart: the float64 side is tests/slice64.py (ref64.Operator64 with the weights between its A
and its At, the rule restated in numpy).  Tolerances: slice64.weighted_matvec64 - ref64.bound_matvec_reps of the
UNWEIGHTED operator, which stays a bound for weights in [0, 1], plus for weights whose products round ('ramp') one
float32 rounding of the intermediate carried through tau |A|^T.  Ties are excluded under tests/test_gpu_voxelwise.py's
rule and cap (fewer than 1 % of the volume); every check prints how many.

Children are started the way tests/test_gpu_voxelwise.py starts them (tests/test_gpu_mask.py's ``_run``: one at a time,
each under a time limit, nothing more on the GPU after one that exited non-zero or timed out).

Observed on an MI355X (worst err / tol, 'pow2' / 'ramp'; no voxel excluded as a tie in any case): the matvec z_rigid 0.047 /
0.038, dn_rigid 0.165 / 0.146, translate 0.035 / 0.034, int_shift 0.025, iso 0.026 / 0.039, orient_9 0.046 / 0.044, sr_2rep 0.095 /
0.099, identity 0.017 / 0.013, z_central 0.091, z_rigid_slab 0.037 / 0.038; the Jacobi diagonal 0.004 - 0.053, dn_rigid 0.163 / 0.146;
the objectives below 0.001 of their bound; the slice sums at most 0.002 of theirs; the right-hand sides 0.40 and 0.26.  CG: 30
iterations, 2.4e-7 from the dense solution (the unweighted system's solution is 0.19 away).  The rule on the device: planted
weights 0.0167.  fit(): RMSE inside the corrupted slices' footprint 47.581 off, 16.501 with slice_robust, 13.784 with user
weights 0; final weights 0.0069 on the planted slices, 1 on every other.

Every test of this file fails on the commit before the feature: the library has no ``unires_slice_sums`` and no
``unires_plan_set_slice_weights``, ``ChannelPlan`` no ``set_slice_weights``, ``_channel_plan`` no ``weights``.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_mask import (BIT_CASES, CASES, GATE, SEED, TWO_KERNEL_ENV, _dense, _run, _small, masks_of, reference,
                                 zeroed)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ('pow2', 'ramp')
# tests/test_gpu_mask.py's cases, the repeats it masks weighted instead; and one that is masked AND weighted
WCASES = {name: dict(case, slab=False) for name, case in CASES.items()}
WCASES['z_rigid_slab'] = dict(CASES['z_rigid'], slab=True, obj=False)

# ---- (1) unires_slice_sums ---------------------------------------------------------------------------------------------
SUM_SHAPES = [((300, 3, 5), 0), ((3, 130, 9), 1), ((5, 7, 300), 2), ((67, 1, 65), 0), ((67, 1, 65), 1), ((67, 1, 65), 2),
              ((1, 1, 1), 0), ((1, 1, 1), 1), ((1, 1, 1), 2), ((41, 38, 60), 0), ((41, 38, 60), 1), ((41, 38, 60), 2)]


def sums_inputs(shape, axis, seed=23):
    """(x, ay) float32 CPU: x with 30 % zeros and one all-zero slice along ``axis`` (the middle one)."""
    gen = torch.Generator().manual_seed(seed + 7 * axis + sum(shape))
    x = torch.randn(shape, generator=gen) * 50.0 + 100.0
    x[torch.rand(shape, generator=gen) < 0.3] = 0.0
    sl = [slice(None)] * 3
    sl[axis] = shape[axis] // 2
    x[tuple(sl)] = 0.0
    ay = torch.randn(shape, generator=gen) * 50.0 + 100.0
    return x.float(), ay.float()


_SUMS_CHILD = r'''
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_slice import SUM_SHAPES, sums_inputs
from unires_amd import _lib
from unires_amd._lib import check, i3
lib, out, res = _lib.load(), sys.argv[1], {}
for shape, axis in SUM_SHAPES:
    x, ay = (t.to('cuda:0') for t in sums_inputs(shape, axis))
    S = shape[axis]
    key = 'x'.join(map(str, shape)) + '/%%d' %% axis
    for run in (0, 1):
        sums = torch.full((2 * S,), float('nan'), dtype=torch.float64, device='cuda:0')
        check(lib.unires_slice_sums(x.data_ptr(), ay.data_ptr(), i3(shape), axis, sums.data_ptr(), None))
        torch.cuda.synchronize()
        res[key + '/run%%d' %% run] = sums.cpu().numpy()
    tot = torch.zeros((), dtype=torch.float64, device='cuda:0')
    check(lib.unires_masked_sse(x.data_ptr(), ay.data_ptr(), x.numel(), tot.data_ptr(), None))
    torch.cuda.synchronize()
    res[key + '/sse'] = np.array(tot.item())
np.savez(out, **res)
'''


def test_slice_sums_against_float64(tmp_path):
    """Counts exact; every sum within N_s 2^-53 SSE_s of the exact sum of the float32 terms numpy reproduces
    (slice64.slice_sums64); their total against unires_masked_sse within both accumulations' bounds; two runs the same
    bits; every entry written (the output starts as NaN)."""
    from tests import slice64
    res = _run(tmp_path, 'slice_sums', _SUMS_CHILD % dict(root=ROOT))
    for shape, axis in SUM_SHAPES:
        key = 'x'.join(map(str, shape)) + '/%d' % axis
        x, ay = sums_inputs(shape, axis)
        sse, cnt, bound = slice64.slice_sums64(x.numpy(), ay.numpy(), axis)
        got = res[key + '/run0']
        S = shape[axis]
        assert got.shape == (2 * S,) and np.isfinite(got).all(), key
        assert np.array_equal(got, res[key + '/run1']), (key, 'two runs differ')
        assert np.array_equal(got[S:], cnt), (key, 'counts')
        assert cnt[S // 2] == 0 and got[S // 2] == 0.0, (key, 'the all-zero slice')
        err = np.abs(got[:S] - sse)
        worst = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
        print('slice sums %-14s worst err / bound %.3f' % (key, worst), flush=True)
        assert (err <= bound).all(), (key, 'sums', int(np.argmax(err - bound)))
        total, n = math.fsum(sse.tolist()), float(cnt.sum())
        slack = math.fsum(bound.tolist()) + 2.0 * (n + S) * 2.0 ** -53 * total
        assert abs(math.fsum(got[:S].tolist()) - float(res[key + '/sse'])) <= slack, (key, 'total against masked_sse')


# ---- (2) the weighted matvec, Jacobi diagonal and objective ------------------------------------------------------------
_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import SIGNED_PERMS, make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED, zeroed
from tests.test_gpu_slice import PATTERNS
from tests import slice64
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan, _slice_axis
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
    assert all(bool((xn.dat != 0).all()) for xn in xg[0])
    if case['slab']:
        for n in case['masked']:
            xg[0][n].dat = zeroed(xg[0][n].dat, 'slab')
    p = d(inputs(prob['dim_y'], prob['dim_y'])[0])
    rho, lam = prob['rho'], yg[0].lam
    for pattern in PATTERNS:
        for n in case['masked']:
            a = _slice_axis(xg[0][n])
            xg[0][n].slice_w = d(slice64.weights(int(xg[0][n].dat.shape[a]), pattern))
        # the settings' own path: regime choice, masks and weights from the observation structs
        plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, diff=case['diff'],
                             mask_zeros=bool(case['slab']), weights=True)
        key = name + '/' + pattern
        res[key + '/axes'] = np.array([_slice_axis(xn) for xn in xg[0]])
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


def _Ws(case, R, axes, pattern):
    """W_n = u_n[s(v)] m_n(v) per repeat as float64 x-space volumes (None: a repeat without weights or mask)."""
    from tests import slice64
    ms = masks_of(dict(case, masked=case['masked'] if case['slab'] else []), R, 'slab')
    out = []
    for n, xn in enumerate(R['xc']):
        if n not in case['masked']:
            out.append(None)
            continue
        shape = tuple(xn.dat.shape)
        out.append(slice64.spread(slice64.weights(shape[axes[n]], pattern), shape, axes[n]) * ms[n])
    return out


def check_weighted(name, case, res):
    from tests import ref64, slice64
    R = reference(case)
    p, myy = R['p'], R['myy']
    n_vox = p.numel()
    assert int(myy.sum()) < 0.01 * n_vox, (name, 'tie cap', int(myy.sum()))
    p64 = p.double()
    mv = lambda pattern, pp=None: slice64.weighted_matvec64(
        R['ops'], R['taus'], _Ws(case, R, axes, pattern), R['p'] if pp is None else pp, R['rho'], R['lam'], R['vx'],
        case['diff'], parts=R['parts'] if pp is None else None, Ap=R['Ap'] if pp is None else None,
        exact=pattern == 'pow2')
    for pattern in PATTERNS:
        key = name + '/' + pattern
        axes = [int(a) for a in res[key + '/axes']]
        for n, xn in enumerate(R['xc']):  # the slice axis is the descriptor's, in the caller's layout
            if n in case['masked'] and getattr(xn.po, 'dim_thick', None) is not None:
                assert axes[n] == int(xn.po.dim_thick), (key, n, axes)
        infos = json.loads(str(res[key + '/info']))
        for n, info in enumerate(infos):
            info['perm'], info['flip'] = tuple(info['perm']), tuple(info['flip'])
            assert info['weighted'] == (n in case['masked']), (key, n, info)
            assert info['masked'] == bool(case['slab']), (key, n, info)
            if info['weighted']:  # bit 3 set, bits 0 and 1 clear: the two-kernel form
                assert not info['shift'] and not info['fused'], (key, n, info)
        # (test_gpu_mask's expectations name the form through 'masked': here a weighted repeat stands in its place)
        assert case['expect'] is None or case['expect'](dict(infos[0], masked=True)), (key, infos)
        q = torch.from_numpy(res[key + '/q'])
        refq, tolq = mv(pattern)
        r = ref64.compare(q, refq, tolq, myy)
        print('slice %-22s matvec err/tol %.3f (excluded %d of %d)' % (key, r['max_ratio'], r['excluded'], n_vox), flush=True)
        assert r['ok'], (key, 'matvec', r)
        if case['diff'] == 'forward':  # the weights did something: the unweighted reference is beyond the bound
            ref_u, _ = ref64.bound_matvec_reps(R['ops'], R['taus'], p, R['rho'], R['lam'], R['vx'], case['diff'], parts=R['parts'])
            assert not ref64.compare(q, ref_u, tolq, myy)['ok'], (key, 'the matvec is the unweighted one')
        pq = p64 * q.double()
        slack = float(pq.abs().sum()) * (ref64.U + (n_vox + 32) * 2.0 ** -53)
        assert abs(float(res[key + '/dot']) - float(pq.sum())) <= slack, (key, 'dot')
        if key + '/M' in res:
            op, tau = R['ops'][0], ref64._f32(R['taus'][0])
            if 'ones' not in R:
                one = torch.ones(R['prob']['dim_y'])
                R['ones'] = (op.parts_AtA(one), op.A(one.double()))
            (_, M1, G1, D1), A1 = R['ones']
            W = _Ws(case, R, axes, pattern)[0]
            vx = [float(v) for v in R['vx'].double()]
            c = ref64._f32(R['rho']) * ref64._f32(R['lam']) ** 2
            const = 2.0 * c * sum(1.0 / (v * v) for v in vx)
            refM = tau * op.At(W * A1) + const
            # tests/test_gpu_mask.py's bound of the diagonal, and the intermediate's extra rounding for 'ramp'
            tolM = (ref64.U + ref64.U64) * (op.c_AtA + ref64.C_DTD) * (tau * M1 + const) + tau * (G1 + D1)
            if pattern != 'pow2':
                tolM = tolM + (ref64.U + ref64.U64) * (1.0 + op.c_A * ref64.U) * tau * op.At(W * op.A(torch.ones(R['prob']['dim_y'], dtype=torch.float64), op.Ka), op.Ka)
            r = ref64.compare(torch.from_numpy(res[key + '/M']), refM, tolM, myy)
            print('slice %-22s Jacobi err/tol %.3f' % (key, r['max_ratio']), flush=True)
            assert r['ok'], (key, 'Jacobi diagonal', r)
    if case['obj']:
        pattern = PATTERNS[-1]
        x1, b64 = torch.from_numpy(res[name + '/x1']), torch.from_numpy(res[name + '/b']).double()
        ref1, tol1 = mv(pattern, x1)
        x64 = x1.double()
        tie = float((x64.abs() * (torch.from_numpy(res[name + '/q1']).double() - ref1).abs())[myy].sum())
        want = 0.5 * float(((ref1 - 2 * b64) * x64).sum())
        tol = 0.5 * float((x64.abs() * (tol1 + 3 * ref64.U * (ref1.abs() + 2 * b64.abs()))).sum()) + 0.5 * tie
        got = float(res[name + '/obj1'])
        print('slice %-22s objective |got - want| / tol %.3f' % (name, abs(got - want) / tol), flush=True)
        assert abs(got - want) <= tol, (name, 'objective', got, want, tol)


@pytest.mark.parametrize('name', list(WCASES))
def test_weighted_matvec_and_jacobi_per_voxel_against_float64(tmp_path, name):
    case = WCASES[name]
    res = _run(tmp_path, name, _CHILD % dict(root=ROOT, cases=json.dumps({name: dict(case, expect=None)})))
    check_weighted(name, case, res)


# ---- (3) bit identities ------------------------------------------------------------------------------------------------
_BIT_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan, _slice_axis
cases, weighted, out = json.loads(%(cases)r), %(weighted)r, sys.argv[1]
res = {}
for name, kw in cases.items():
    prob = make_problem(seed=SEED, **kw)
    xg, yg, sett = gpu_structs(prob, 'cuda:0')
    vx = N.voxel_size(prob['mat_y']).float()
    if weighted:
        xn = xg[0][0]
        xn.slice_w = torch.ones(int(xn.dat.shape[_slice_axis(xn)]), device='cuda:0')
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
    info = plan.repeat_info(0)
    assert info['weighted'] == weighted and not info['masked'] and not (weighted and (info['shift'] or info['fused'])), info
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


def test_unit_weights_give_the_bits_of_the_two_kernel_forms(tmp_path):
    """u = 1 against the unweighted plan forced onto the same two-kernel forms by the existing switches, in fresh
    processes: q, its dot and the Jacobi diagonal, bit for bit."""
    args = dict(root=ROOT, cases=json.dumps(BIT_CASES))
    on = _run(tmp_path, 'bits_weighted', _BIT_CHILD % dict(args, weighted=True))
    off = _run(tmp_path, 'bits_forced', _BIT_CHILD % dict(args, weighted=False), env=TWO_KERNEL_ENV)
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
from unires_amd._project import _channel_plan, _slice_axis
out = sys.argv[1]
prob = make_problem(seed=SEED, **%(kw)r)
xg, yg, sett = gpu_structs(prob, 'cuda:0')
vx = N.voxel_size(prob['mat_y']).float()
p = inputs(prob['dim_y'], prob['dim_y'])[0].to('cuda:0')
res = {}
# both repeats, the second with weight 0 on every slice
plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
a = _slice_axis(xg[0][1])
plan.set_slice_weights(1, a, torch.zeros(int(xg[0][1].dat.shape[a]), device='cuda:0'))
assert plan.repeat_info(1)['weighted'] and not plan.repeat_info(0)['weighted']
res['both'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
plan.close()
yg[0]._plan = None
plan = _channel_plan(xg[0][:1], yg[0], prob['method'], prob['do_proj'], vx)
res['alone'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
np.savez(out, **res)
'''


def test_zero_weights_on_the_second_repeat_add_nothing(tmp_path):
    """Two repeats under a general rigid, the second with u = 0: q has the bits of the plan without that repeat (its
    push accumulates exact zeros)."""
    res = _run(tmp_path, 'zero_w', _ZERO_CHILD % dict(root=ROOT, kw=CASES['sr_2rep']['kw']))
    assert np.array_equal(res['both'], res['alone'])
    assert np.abs(res['both']).max() > 0


# ---- (4) the right-hand side -------------------------------------------------------------------------------------------
RHS_CASES = ('sr_2rep', 'orient_9')  # out of place from the caller's volume; in place on the plan's canonical copy

_RHS_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import SIGNED_PERMS, make_problem, gpu_structs
from tests.test_gpu_mask import SEED
from tests import slice64
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan, _slice_axis
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
    for n in case['masked']:
        a = _slice_axis(xg[0][n])
        xg[0][n].slice_w = d(slice64.weights(int(xg[0][n].dat.shape[a]), 'pow2'))
    before = [xn.dat.clone() for xn in xg[0]]
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
    res[name + '/axes'] = np.array([_slice_axis(xn) for xn in xg[0]])
    dats = [xn.dat for xn in xg[0]]
    w, z = d(prob['w'][0]), d(prob['z'][0])
    res[name + '/b'] = plan.rhs(dats, w, z, prob['rho'], yg[0].lam).cpu().numpy()
    b2 = torch.empty(prob['dim_y'], device='cuda:0')
    plan.rhs_cached(dats, w, z, prob['rho'], yg[0].lam, out=b2)
    res[name + '/b_cached'] = b2.cpu().numpy()
    res[name + '/atx'] = plan._atx[1].cpu().numpy()
    # new weight values: the cached sum follows them
    for n in case['masked']:
        xg[0][n].slice_w.fill_(1.0)
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
    plan.rhs_cached(dats, w, z, prob['rho'], yg[0].lam, out=b2)
    res[name + '/atx_ones'] = plan._atx[1].cpu().numpy()
    torch.cuda.synchronize()
    assert all(torch.equal(a_, b_.dat) for a_, b_ in zip(before, xg[0]))  # the observations are bit-unchanged
np.savez(out, **res)
'''


def test_weighted_right_hand_side_per_voxel_against_float64(tmp_path):
    """b and sum tau At (u . x) with 'pow2' weights (u . x is exact in float32) under ref64.bound_rhs evaluated at
    u . x; the cached form gives the same bits and follows a change of the weights' values; the observation tensors
    are bit-unchanged (asserted in the child)."""
    from tests import ref64, slice64
    cases = {name: dict(WCASES[name], expect=None) for name in RHS_CASES}
    res = _run(tmp_path, 'rhs', _RHS_CHILD % dict(root=ROOT, cases=json.dumps(cases)))
    for name in RHS_CASES:
        case = WCASES[name]
        R = reference(case)
        axes = [int(a) for a in res[name + '/axes']]
        my = torch.zeros(R['prob']['dim_y'], dtype=torch.bool)
        for op, xn in zip(R['ops'], R['xc']):
            my |= op.tie_masks(xn.po)[1]
        assert int(my.sum()) < 0.01 * my.numel(), (name, 'tie cap')
        ux, plain = [], []
        for n, xn in enumerate(R['xc']):
            plain.append(xn.dat)
            if n in case['masked']:
                shape = tuple(xn.dat.shape)
                ux.append((slice64.spread(slice64.weights(shape[axes[n]], 'pow2'), shape, axes[n]) * xn.dat.double()).float())
                assert torch.equal(ux[-1].double(), slice64.spread(slice64.weights(shape[axes[n]], 'pow2'), shape, axes[n]) * xn.dat.double())
            else:
                ux.append(xn.dat)
        w, z = R['prob']['w'][0], R['prob']['z'][0]
        ref, tol = ref64.bound_rhs(R['ops'], R['taus'], ux, w, z, R['rho'], R['lam'], R['vx'], case['diff'])
        r = ref64.compare(torch.from_numpy(res[name + '/b']), ref, tol, my)
        print('slice %-10s rhs err/tol %.3f (excluded %d)' % (name, r['max_ratio'], r['excluded']), flush=True)
        assert r['ok'], (name, 'b', r)
        assert np.array_equal(res[name + '/b'], res[name + '/b_cached']) or \
            ref64.compare(torch.from_numpy(res[name + '/b_cached']), ref, tol, my)['ok'], (name, 'cached b')
        zero = torch.zeros_like(w)
        ref_a, tol_a = ref64.bound_rhs(R['ops'], R['taus'], ux, zero, zero, R['rho'], R['lam'], R['vx'], case['diff'])
        ra = ref64.compare(torch.from_numpy(res[name + '/atx']), ref_a, tol_a, my)
        assert ra['ok'], (name, 'atx', ra)
        # ... it is not the unweighted sum, and with all weights 1 it is
        ref_p, tol_p = ref64.bound_rhs(R['ops'], R['taus'], plain, zero, zero, R['rho'], R['lam'], R['vx'], case['diff'])
        assert not ref64.compare(torch.from_numpy(res[name + '/atx']), ref_p, tol_a, my)['ok'], (name, 'atx is unweighted')
        assert ref64.compare(torch.from_numpy(res[name + '/atx_ones']), ref_p, tol_p, my)['ok'], (name, 'atx after new weights')


# ---- (5) CG, (6) the captured solve -------------------------------------------------------------------------------------
def _small_clean(dev):
    """tests/test_gpu_mask.py's 10 x 9 x 8 two-repeat problem, and the slice axis / count of its second repeat."""
    from unires_amd._project import _slice_axis
    prob, xg, yg, vx = _small(dev)
    a = _slice_axis(xg[0][1])
    return prob, xg, yg, vx, a, int(xg[0][1].dat.shape[a])


def test_cg_converges_to_the_dense_solution_of_the_weighted_normal_equations(dev):
    from tests import diff64, ref64, slice64
    from tests.helpers import oracle_structs, rel_err
    from unires_amd._project import _channel_plan
    prob, xg, yg, vx, a, S = _small_clean(dev)
    xs, ys = oracle_structs(prob)
    dim = prob['dim_y']
    rho, lam = ref64._f32(prob['rho']), ref64._f32(ys[0].lam)
    w = slice64.weights(S, 'ramp')
    Sys = rho * lam * lam * diff64.dense_dtd(dim, [float(v) for v in vx], 'forward')
    for n, xn in enumerate(xs[0]):
        A = _dense(ref64.Operator64(xn.po, prob['method']))
        u = slice64.spread(w, tuple(xn.dat.shape), a).numpy().reshape(-1) if n == 1 else np.ones(A.shape[0])
        Sys = Sys + ref64._f32(xn.tau) * (A.T @ (u[:, None] * A))
    g = torch.Generator().manual_seed(9)
    b = (torch.rand(dim, generator=g) * 0.1).float()
    want = np.linalg.solve(Sys, b.double().numpy().ravel()).reshape(dim)
    sk = float(np.sqrt(np.linalg.cond(Sys)))
    n_it = int(np.ceil(np.log(0.5e-6) / np.log((sk - 1.0) / (sk + 1.0))))
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
    plan.set_slice_weights(1, a, w.to(dev))
    assert plan.repeat_info(1)['weighted'] and not plan.repeat_info(0)['weighted']
    x = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), x, rho, lam, max_iter=n_it, tolerance=0.0)
    err = rel_err(x.cpu(), torch.from_numpy(want))
    plan.set_slice_weights(1, a, None)
    xu = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), xu, rho, lam, max_iter=n_it, tolerance=0.0)
    far = rel_err(xu.cpu(), torch.from_numpy(want))
    print('weighted CG: %d iterations, rel_err %.3g; unweighted solution %.3g away' % (n_it, err, far), flush=True)
    assert err < GATE
    assert far > 10 * GATE
    plan.close()


def test_a_captured_solve_reads_new_weight_values(dev):
    """Two tol = 0 solves on one plan with different weight VALUES in between (the second replays the captured graph,
    which reads the plan's own weight buffer): the bits of a fresh plan's solve with those weights.  Setting and
    clearing weights flips info[6] as documented; the Jacobi-preconditioned solve follows the new values too."""
    from tests import slice64
    from unires_amd._plan import ChannelPlan
    prob, xg, yg, vx, a, S = _small_clean(dev)
    xg[0][1].dat = torch.where(xg[0][1].dat == 0, torch.ones_like(xg[0][1].dat), xg[0][1].dat)
    reps = [(xn.po, xn.tau) for xn in xg[0]]
    vxl = [float(v) for v in vx]
    rho, lam = float(prob['rho']), float(yg[0].lam)
    g = torch.Generator().manual_seed(2)
    b = (torch.rand(prob['dim_y'], generator=g) * 0.1).to(dev)
    x0 = prob['y0'][0].to(dev)
    w1, w2 = slice64.weights(S, 'ramp').to(dev), slice64.weights(S, 'pow2').to(dev)

    def solve(plan):
        x = x0.clone()
        plan.cg(b, x, rho, lam, max_iter=6, tolerance=0.0)
        torch.cuda.synchronize()
        return x

    def fresh(w):
        pl = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
        if w is not None:
            pl.set_slice_weights(1, a, w)
        x = solve(pl)
        pl.close()
        return x

    plan = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
    first = solve(plan)
    info0 = plan.repeat_info(1)
    assert not info0['weighted']
    plan.set_slice_weights(1, a, w1)
    info1 = plan.repeat_info(1)
    assert info1['weighted'] and not info1['masked'] and not info1['shift'] and not info1['fused'], info1
    got1 = solve(plan)
    assert torch.equal(solve(plan), got1)  # (the replay)
    assert not torch.equal(got1, first) and torch.equal(got1, fresh(w1))
    plan.set_slice_weights(1, a, w2)  # values only
    got2 = solve(plan)
    assert not torch.equal(got2, got1)
    assert torch.equal(got2, fresh(w2))
    plan.set_slice_weights(1, a, None)
    assert plan.repeat_info(1) == info0
    assert torch.equal(solve(plan), first)
    # a wrong axis or repeat is refused
    with pytest.raises(ValueError):
        plan.set_slice_weights(1, 3, w1)
    with pytest.raises(Exception):
        plan.set_slice_weights(2, a, w1)
    plan.close()


# ---- (7) the rule on the device ----------------------------------------------------------------------------------------
PLANTED = (3, 7, 11)


def _phantom(dev, noise_sd=5.0):
    from tests.helpers import gpu_structs, make_problem
    prob = make_problem(seed=5, dim_y=(48, 48, 40), thick=3, n_repeats=2, rot=0.0, trans=0.0, noise_sd=noise_sd,
                        thick_axes=None, shift=(0.0, 0.0, 0.0))
    return prob, gpu_structs(prob, dev)


def test_update_slice_weights_against_the_float64_rule(dev):
    """x = A y + noise with the same noise in every slice (48 x 48 voxels each: the slice RMS varies by about 1.5 %),
    three slices multiplied by 0.3: every clean slice gets exactly 1, the planted ones the restatement's value from the
    exact float64 sums of the same float32 terms."""
    import unires_amd as U
    from tests import slice64
    from unires_amd._project import _slice_axis
    from unires_amd._update import _update_slice_weights
    prob, (xg, yg, sett) = _phantom(dev)
    xg, yg = [xg[0][:1]], yg[:1]  # one repeat: thick along z, (48, 48, 13)
    xn = xg[0][0]
    a = _slice_axis(xn)
    assert a == 2 and xn.dat.shape[a] > max(PLANTED)
    Ay = U._proj('A', yg[0].dat, xg[0], yg[0], n=0, method=sett.method, do=sett.do_proj)
    gen = torch.Generator().manual_seed(31)
    dat = Ay.cpu() + 5.0 * torch.randn(tuple(Ay.shape), generator=gen)
    for s in PLANTED:
        dat[:, :, s] *= 0.3
    xn.dat = dat.to(dev)
    xn.slice_w = torch.ones(xn.dat.shape[a], device=dev)
    _update_slice_weights(xg, yg, sett)
    torch.cuda.synchronize()
    got = xn.slice_w.cpu().double().numpy()
    sse, cnt, _ = slice64.slice_sums64(dat.numpy(), Ay.cpu().numpy(), a)
    want = slice64.rule64(sse, cnt, sett.slice_k)
    clean = [s for s in range(len(got)) if s not in PLANTED]
    assert all(got[s] == 1.0 for s in clean), got
    assert all(want[s] < 1.0 for s in PLANTED), want
    # float64 rounding of the sums (N_s 2^-53 relative, twice: the slice's and the median's) and one float32 rounding of
    # the stored weight
    for s in PLANTED:
        assert abs(got[s] - want[s]) <= want[s] * (2.0 ** -24 + 4 * cnt[s] * 2.0 ** -53), (s, got[s], want[s])
    print('rule on the device: planted weights %s' % [float('%.4g' % got[s]) for s in PLANTED], flush=True)


# ---- (8) end to end ----------------------------------------------------------------------------------------------------
def test_fit_rejects_corrupted_slices(dev):
    """tests/test_gpu_mask.py's 48 x 48 x 40 phantom, two repeats with 3 mm slices (thick along z and along y), three
    slices of the second multiplied by 0.3; fit() for 12 ADMM iterations of 20 CG iterations (cgs_tol = 0) with the
    weights off, with sett.slice_robust, and with user weights (0 on those three slices, slice_robust off).
    (a) inside the footprint of the corrupted slices the RMSE against the phantom is lower with either than off; (b) in
    the corrupted repeat the largest final weight among the planted slices is below the smallest among the others;
    (c) info['slice_w'] is a list per channel of one CPU float32 tensor per repeat, one weight per slice.

    Observed on an MI355X: RMSE 47.581 (off), 16.501 (slice_robust), 13.784 (user weights 0); final weights of the
    corrupted repeat 0.0069 on each planted slice and exactly 1 on every other, the clean repeat's all exactly 1 (the test
    prints them)."""
    import unires_amd as U
    prob, _ = _phantom(dev)
    truth = prob['truth'][0]
    out, infos = {}, {}
    for arm in ('off', 'robust', 'user'):
        _, (xg, yg, sett) = _phantom(dev)
        x1 = xg[0][1].dat  # thick along y: (48, 16, 40); its slices are planes of constant y
        assert x1.shape[1] > max(PLANTED)
        for s in PLANTED:
            x1[:, s, :] *= 0.3
        yg[0].lam0 = float(yg[0].lam) / 4.0
        sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 12, 1e-4, 4.0, 0
        sett.cgs_max_iter, sett.cgs_tol = 20, 0.0
        sett.clean_fov = False
        sett.slice_robust = arm == 'robust'
        if arm == 'user':
            w = torch.ones(x1.shape[1])
            w[list(PLANTED)] = 0.0
            xg[0][1].slice_w = w
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 12
        out[arm], infos[arm] = dat[..., 0].cpu(), info
    foot = torch.zeros(48, dtype=torch.bool)
    for s in PLANTED:
        foot[3 * s:3 * s + 3] = True
    rmse = lambda a: float(((a[:, foot, :].double() - truth[:, foot, :].double()) ** 2).mean().sqrt())
    r = {arm: rmse(out[arm]) for arm in out}
    sw = infos['robust']['slice_w']
    print('fit with corrupted slices: RMSE inside their footprint off %.3f robust %.3f user %.3f' % (r['off'], r['robust'], r['user']),
          flush=True)
    # (c)
    assert infos['off']['slice_w'] == [[None, None]]
    assert len(sw) == 1 and len(sw[0]) == 2
    assert all(t.device.type == 'cpu' and t.dtype == torch.float32 for t in sw[0])
    assert tuple(sw[0][0].shape) == (13,) and tuple(sw[0][1].shape) == (16,)
    assert infos['user']['slice_w'][0][0] is None and infos['user']['slice_w'][0][1].tolist() == [0.0 if s in PLANTED else 1.0 for s in range(16)]
    w1 = sw[0][1]
    others = [float(w1[s]) for s in range(16) if s not in PLANTED]
    planted = [float(w1[s]) for s in PLANTED]
    print('  final weights of the corrupted repeat: planted %s, the others min %.4f; the clean repeat min %.4f'
          % (['%.4f' % v for v in planted], min(others), float(sw[0][0].min())), flush=True)
    assert r['robust'] < r['off']  # (a)
    assert r['user'] < r['off']
    assert max(planted) < min(others)  # (b)


# ---- (9) the channels of a y-update on streams of their own -------------------------------------------------------------
def test_weighted_y_update_on_channel_streams(dev):
    """Three channels with user weights: _update_y with the channels on streams of their own against one channel after
    the other, on fresh structs each time (the weights are copied into the plans at the first y-update's plan fetch,
    on the main stream, before the event the channels' streams wait for).  tests/test_gpu_mask.py's tolerance for the
    same comparison: 1e-5 after 8 iterations; a solve that read unwritten weights would be off by the unweighted
    system's distance, which the last assertion shows to be beyond 1e-3."""
    import unires_amd as U
    from tests import slice64
    from tests.helpers import gpu_structs, make_problem, rel_err
    from unires_amd._project import _channel_plan, _slice_axis
    prob = make_problem(seed=7, dim_y=(40, 36, 33), n_channels=3, thick=3, rot=0.08, trans=1.0, scl=0.05)

    def run(streams, weighted):
        xg, yg, sett = gpu_structs(prob, dev)
        if weighted:
            for xc in xg:
                xc[0].slice_w = slice64.weights(int(xc[0].dat.shape[_slice_axis(xc[0])]), 'ramp').to(dev)
        sett.channel_streams = streams
        sett.cgs_max_iter, sett.cgs_tol = 8, 0.0
        z, w = prob['z'].to(dev), prob['w'].to(dev)
        tmp = torch.zeros_like(yg[0].dat)
        U._update_y(xg, yg, z, w, prob['rho'], tmp, sett)
        torch.cuda.synchronize()
        for c in range(len(xg)):
            info = _channel_plan(xg[c], yg[c], sett.method, sett.do_proj).repeat_info(0)
            assert info['weighted'] == weighted, (c, info)
        return [yc.dat.cpu() for yc in yg]

    serial = run(False, True)
    for attempt in range(3):
        side = run(True, True)
        for c in range(3):
            assert rel_err(side[c], serial[c]) < 1e-5, (attempt, c, rel_err(side[c], serial[c]))
    plain = run(True, False)
    assert min(rel_err(plain[c], serial[c]) for c in range(3)) > 1e-3
