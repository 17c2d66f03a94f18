"""Per-slice intensity gains on the GPU (sett.slice_gain, _input.slice_gain): repeat n is modelled as
e_n[s(v)] (A_n y)(v), and the y-update's system becomes

    ( sum_n tau_n A_n^T diag(W_n e_n^2) A_n + rho lam^2 D^T D ) y = sum_n tau_n A_n^T (W_n e_n x_n) - lam D^T (w - rho z)

with W_n = g_n . u_n . m_n the repeat's voxel weights, slice weights and mask (each 1 where it has none).

(1) unires_gain_sums against float64; (2) the tables as bit identities: a gained plan against the plan whose slice
weights are the composed table; (3) the gained matvec and right-hand side per voxel against float64; (4) CG against the
dense solution; (5) the captured solve across a change of gain values; (6) the rule on the device; (7) fit(); (8) gains
with both robust rules on channel streams.

The reference has no counterpart: the float64 side is tests/gain64.py on tests/slice64.py and tests/ref64.py.  (2) has
no tolerance: the passes of a gained repeat are the passes of a weighted one, handed another table.  (3) takes
slice64.weighted_matvec64 with W = w_mat, which bounds weights in [0, 1] only: its gains are drawn from {1/4, 1/2, 1};
gains above 1 are covered by (2).  No voxel may be excluded as a tie in (3).

Children are started the way tests/test_gpu_slice.py starts them (tests/test_gpu_mask.py's ``_run``: one at a time, each
under a time limit, nothing more on the GPU after one that exited non-zero or timed out).

Observed on an MI355X: the sums at most 0.25 of their bound (300 x 3 x 5; below 0.002 at 41 x 38 x 60); the matvec at most
0.095 of its tolerance (sr_2rep), the right-hand side 0.40, the cached sum 0.41, no voxel excluded in any case.  CG: 27
iterations, 2.75e-7 from the dense solution (the solution without gains is 0.193 away).  The rule on the device: 0.9991 -
1.0006, 0.8628 - 0.8634, 1.1364 - 1.1381 for planted 1, 0.85, 1.15.  fit(): RMSE over the banded repeat's footprint 12.687 off,
8.708 with slice_gain, 8.500 with user gains; mean estimated gains 0.8741 / 1.0071 / 1.1367.

Tests (1), (2), (3) and (5) fail on the commit before the feature: the library has no ``unires_gain_sums`` and no
``unires_plan_set_slice_gains``.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_mask import GATE, _dense, _run, masks_of, reference
from tests.test_gpu_slice import SUM_SHAPES, WCASES, _phantom, _small_clean, sums_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ('none', 'u', 'g', 'gu', '01')
PATTERN = (1.0, 0.85, 1.15)  # the planted banding of (6) and (7), repeated along the stack


def sums_weights(shape, axis, arm):
    """(g, u) float32 CPU or None each for an arm of (1): generic values in [0, 1]; '01': draws from {0, 1}."""
    gen = torch.Generator().manual_seed(61 + axis + sum(shape))
    g = torch.rand(shape, generator=gen).float()
    u = torch.rand(shape[axis], generator=gen).float()
    if arm == '01':
        return (g < 0.7).float(), (u < 0.8).float()
    return (g if 'g' in arm else None), (u if 'u' in arm else None)


# ---- (1) unires_gain_sums ----------------------------------------------------------------------------------------------
_SUMS_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_slice import SUM_SHAPES, sums_inputs
from tests.test_gpu_gain import ARMS, sums_weights
from unires_amd import _lib
from unires_amd._lib import i3
lib, out, res = _lib.load(), sys.argv[1], {}
P = lambda t: None if t is None else t.data_ptr()
for shape, axis in SUM_SHAPES:
    x, ay = (t.to('cuda:0') for t in sums_inputs(shape, axis))
    S = shape[axis]
    for arm in ARMS:
        g, u = (None if t is None else t.to('cuda:0') for t in sums_weights(shape, axis, arm))
        key = 'x'.join(map(str, shape)) + '/%%d/%%s' %% (axis, arm)
        for run in (0, 1):
            sums = torch.full((3 * S,), float('nan'), dtype=torch.float64, device='cuda:0')
            rc = lib.unires_gain_sums(x.data_ptr(), ay.data_ptr(), P(g), P(u), i3(shape), axis, sums.data_ptr(), None)
            assert rc == 0, (key, rc)
            torch.cuda.synchronize()
            res[key + '/run%%d' %% run] = sums.cpu().numpy()
# status codes: unires_slice_sums' for the same mistakes
x, ay = (t.to('cuda:0') for t in sums_inputs((5, 7, 6), 1))
o3, o2 = torch.zeros(21, dtype=torch.float64, device='cuda:0'), torch.zeros(14, dtype=torch.float64, device='cuda:0')
codes = []
for bad in ('x', 'ay', 'out', 'axis-', 'axis+', 'dim0'):
    a = dict(x=x.data_ptr(), ay=ay.data_ptr(), dim=i3((5, 7, 6)), axis=1)
    if bad in ('x', 'ay'):
        a[bad] = None
    if bad.startswith('axis'):
        a['axis'] = -1 if bad == 'axis-' else 3
    if bad == 'dim0':
        a['dim'] = i3((5, 0, 6))
    mine = lib.unires_gain_sums(a['x'], a['ay'], None, None, a['dim'], a['axis'], None if bad == 'out' else o3.data_ptr(), None)
    theirs = lib.unires_slice_sums(a['x'], a['ay'], a['dim'], a['axis'], None if bad == 'out' else o2.data_ptr(), None)
    codes.append((mine, theirs))
res['codes'] = np.array(codes)
np.savez(out, **res)
'''


def test_gain_sums_against_float64(tmp_path):
    """Every one of the 3 S entries within gain64.gain_sums64's bound of the exact sum of the summands numpy reproduces;
    the effective count exact for 0 / 1 weights and without weights; two runs the same bits; every entry written (the
    output starts as NaN); a null argument, a bad axis or a bad dim give unires_slice_sums' status codes."""
    from tests import gain64
    res = _run(tmp_path, 'gain_sums', _SUMS_CHILD % dict(root=ROOT), timeout=300)
    for shape, axis in SUM_SHAPES:
        x, ay = sums_inputs(shape, axis)
        S = shape[axis]
        for arm in ARMS:
            key = 'x'.join(map(str, shape)) + '/%d/%s' % (axis, arm)
            g, u = sums_weights(shape, axis, arm)
            want, bound = gain64.gain_sums64(x.numpy(), ay.numpy(), None if g is None else g.numpy(),
                                             None if u is None else u.numpy(), axis)
            got = res[key + '/run0']
            assert got.shape == (3 * S,) and np.isfinite(got).all(), key
            assert np.array_equal(got, res[key + '/run1']), (key, 'two runs differ')
            err = np.abs(got - want)
            worst = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
            print('gain sums %-18s worst err / bound %.3f' % (key, worst), flush=True)
            assert (err <= bound).all(), (key, int(np.argmax(err - bound)), float(err.max()))
            assert all(got[k * S + S // 2] == 0.0 for k in range(3)), (key, 'the all-zero slice')
            if arm in ('none', '01'):
                assert np.array_equal(got[2 * S:], want[2 * S:]), (key, 'effective count')
            if arm == 'none':
                other = tuple(a for a in range(3) if a != axis)
                assert np.array_equal(got[2 * S:], (x.numpy() != 0).sum(axis=other).astype(np.float64)), (key, 'count')
    codes = res['codes']
    assert (codes[:, 0] == codes[:, 1]).all() and (codes[:, 0] != 0).all(), codes


# ---- (2) the tables as bit identities, (3) per voxel against float64 -----------------------------------------------------
_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import SIGNED_PERMS, make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED, zeroed
from tests import gain64, slice64, voxel64
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan, _slice_axis
case, out = json.loads(%(case)r), sys.argv[1]
res = {}
d = lambda t: t.to('cuda:0')
kw = case['kw']
if 'orient' in kw:
    kw = dict(kw, orient=[SIGNED_PERMS[kw['orient']]])
prob = make_problem(seed=SEED, **kw)
xg, yg, sett = gpu_structs(prob, 'cuda:0')
vx = N.voxel_size(prob['mat_y']).float()
if case['slab']:
    for n in case['masked']:
        xg[0][n].dat = zeroed(xg[0][n].dat, 'slab')
p = d(inputs(prob['dim_y'], prob['dim_y'])[0])
rho, lam = prob['rho'], yg[0].lam
w, z = d(prob['w'][0]), d(prob['z'][0])
dats = [xn.dat for xn in xg[0]]
axes = [_slice_axis(xn) for xn in xg[0]]
res['axes'] = np.array(axes)


def state(tag, u=None, e=None, g=None):
    # the settings' own path: regime choice, masks, weights and gains from the observation structs
    for n in case['masked']:
        xn = xg[0][n]
        S = int(xn.dat.shape[axes[n]])
        xn.slice_w = None if u is None else d(torch.as_tensor(u(S)))
        xn.slice_gain = None if e is None else d(torch.as_tensor(e(S)))
        xn.weight = None if g is None else d(voxel64.weights(tuple(xn.dat.shape), g))
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, diff=case['diff'],
                         mask_zeros=bool(case['slab']), weights=True)
    res[tag + '/info'] = json.dumps([plan.repeat_info(n) for n in range(len(xg[0]))])
    dot = torch.zeros((), dtype=torch.float64, device='cuda:0')
    res[tag + '/q'] = plan.matvec(p, rho, lam, dot=dot).cpu().numpy()
    torch.cuda.synchronize()
    res[tag + '/dot'] = np.array(dot.item())
    if len(xg[0]) == 1:
        M = torch.empty(prob['dim_y'], dtype=torch.float32, device='cuda:0')
        plan.precond_build(rho, lam, mode='jacobi', out=M)
        res[tag + '/M'] = M.cpu().numpy()
    b = torch.empty(prob['dim_y'], device='cuda:0')
    plan.rhs_cached(dats, w, z, rho, lam, out=b)
    res[tag + '/atx'] = plan._atx[1].cpu().numpy()
    res[tag + '/b'] = plan.rhs(dats, w, z, rho, lam).cpu().numpy()


ramp = lambda S: slice64.weights(S, 'ramp')
generic = lambda S: gain64.gains(S, 'generic')
table = lambda u, e, k: (lambda S: torch.from_numpy(gain64.compose32(None if u is None else u(S).numpy(), e(S).numpy())[k]))
before = [t.clone() for t in dats]
state('A', u=ramp, e=generic)
state('B', u=table(ramp, generic, 0))
state('C', u=table(ramp, generic, 1))
state('D', u=ramp, e=lambda S: gain64.gains(S, 'ones'))
state('E', u=ramp)
state('F', g='ramp', e=generic)
state('G', g='ramp', u=table(None, generic, 0))
state('G2', g='ramp', u=generic)
state('H', u=lambda S: slice64.weights(S, 'pow2'), e=lambda S: gain64.gains(S, 'pow2'))
assert all(torch.equal(a_, b_) for a_, b_ in zip(before, dats))  # the observations are bit-unchanged
np.savez(out, **res)
'''

_RES = {}


def _case_res(tmp_path, name):
    """One child per case for (2) and (3): nine plan states on one problem."""
    if name not in _RES:
        case = dict(WCASES[name], expect=None)
        _RES[name] = _run(tmp_path, 'gain_' + name, _CHILD % dict(root=ROOT, case=json.dumps(case)), timeout=300)
    return _RES[name]


@pytest.mark.parametrize('name', list(WCASES))
def test_a_gained_plan_has_the_bits_of_the_plan_weighted_by_its_tables(tmp_path, name):
    """(a) weights u and generic gains e in [0.5, 2]: q, its dot and the Jacobi diagonal of the plan whose slice weights
    are compose32(u, e).w_mat, the cached sum tau At (.) of the plan whose slice weights are w_rhs; (b) e = 1: the plan
    without gains; (c) gains beside a voxel map, no slice weights: the voxel plan with slice weights fl32(e e), and e for
    the right-hand side; (d) info[6] bit 5 follows set and clear, and a gained repeat declines the one-kernel forms."""
    case, res = WCASES[name], _case_res(tmp_path, name)
    same = lambda a, b, what: np.array_equal(res['%s/%s' % (a, what)], res['%s/%s' % (b, what)])
    mats = ('q', 'dot') + (('M',) if 'A/M' in res else ())
    for what in mats:
        assert same('A', 'B', what), (name, 'a', what)
        assert same('D', 'E', what), (name, 'b', what)
        assert same('F', 'G', what), (name, 'c', what)
    assert same('A', 'C', 'atx') and same('A', 'C', 'b'), (name, 'a', 'right-hand side')
    assert same('D', 'E', 'atx') and same('D', 'E', 'b'), (name, 'b', 'right-hand side')
    assert same('F', 'G2', 'atx') and same('F', 'G2', 'b'), (name, 'c', 'right-hand side')
    # ... and the gains did something
    assert not same('A', 'E', 'q') and not same('A', 'E', 'atx'), (name, 'the gained plan is the weighted one')
    assert not same('B', 'C', 'q'), (name, 'w_mat is w_rhs')
    for tag, gained in (('A', True), ('B', False), ('C', False), ('D', True), ('E', False), ('F', True), ('G', False),
                        ('G2', False), ('H', True)):
        for n, info in enumerate(json.loads(str(res[tag + '/info']))):
            assert info['gained'] == (gained and n in case['masked']), (name, tag, n, info)
            if info['gained']:
                assert not info['shift'] and not info['fused'], (name, tag, n, info)
            assert info['masked'] == bool(case['slab']), (name, tag, n, info)


@pytest.mark.parametrize('name', list(WCASES))
def test_gained_matvec_and_right_hand_side_per_voxel_against_float64(tmp_path, name):
    """u from 'pow2' and e from {1/4, 1/2, 1}: w_mat = u e^2 <= 1 and w_rhs = u e are exact, and so are their float32
    products.  The matvec under slice64.weighted_matvec64(exact=True) with W = w_mat (times the mask); the right-hand
    side and the cached sum under ref64.bound_rhs evaluated at w_rhs . x.  No voxel is excluded as a tie."""
    from tests import gain64, ref64, slice64
    case, res = WCASES[name], _case_res(tmp_path, name)
    R = reference(case)
    axes = [int(a) for a in res['axes']]
    ms = masks_of(dict(case, masked=case['masked'] if case['slab'] else []), R, 'slab')
    Ws, ux = [], []
    for n, xn in enumerate(R['xc']):
        if n not in case['masked']:
            Ws.append(None)
            ux.append(xn.dat)
            continue
        shape = tuple(xn.dat.shape)
        S = shape[axes[n]]
        w_mat, w_rhs = gain64.compose32(slice64.weights(S, 'pow2').numpy(), gain64.gains(S, 'pow2').numpy())
        assert w_mat.max() <= 1.0 and np.array_equal(w_mat.astype(np.float64), (w_rhs.astype(np.float64) * gain64.gains(S, 'pow2').numpy()))
        Ws.append(slice64.spread(torch.from_numpy(w_mat), shape, axes[n]) * ms[n])
        xd = xn.dat.double() * (ms[n] if case['slab'] else 1.0)  # (the child zeroes the slab of a masked-and-weighted case)
        prod = slice64.spread(torch.from_numpy(w_rhs), shape, axes[n]) * xd
        ux.append(prod.float())
        assert torch.equal(ux[-1].double(), prod)
    assert int(R['myy'].sum()) == 0, (name, 'ties', int(R['myy'].sum()))
    ref, tol = slice64.weighted_matvec64(R['ops'], R['taus'], Ws, R['p'], R['rho'], R['lam'], R['vx'], case['diff'],
                                         parts=R['parts'], Ap=R['Ap'], exact=True)
    r = ref64.compare(torch.from_numpy(res['H/q']), ref, tol, R['myy'])
    print('gain %-14s matvec err/tol %.3f (excluded %d)' % (name, r['max_ratio'], r['excluded']), flush=True)
    assert r['ok'] and r['excluded'] == 0, (name, 'matvec', r)
    if case['diff'] == 'forward':  # the gains did something: the weighted operator without them is beyond the bound
        Wu = [None if W is None else slice64.spread(slice64.weights(W.shape[axes[n]], 'pow2'), tuple(W.shape), axes[n]) * ms[n]
              for n, W in enumerate(Ws)]
        ref_u, _ = slice64.weighted_matvec64(R['ops'], R['taus'], Wu, R['p'], R['rho'], R['lam'], R['vx'], case['diff'],
                                             parts=R['parts'], Ap=R['Ap'], exact=True)
        assert not ref64.compare(torch.from_numpy(res['H/q']), ref_u, tol, R['myy'])['ok'], (name, 'the matvec has no gains')
    my = torch.zeros(R['prob']['dim_y'], dtype=torch.bool)
    for op, xn in zip(R['ops'], R['xc']):
        my |= op.tie_masks(xn.po)[1]
    assert int(my.sum()) == 0, (name, 'ties of the push', int(my.sum()))
    w, z = R['prob']['w'][0], R['prob']['z'][0]
    refb, tolb = ref64.bound_rhs(R['ops'], R['taus'], ux, w, z, R['rho'], R['lam'], R['vx'], case['diff'])
    rb = ref64.compare(torch.from_numpy(res['H/b']), refb, tolb, my)
    zero = torch.zeros_like(w)
    refa, tola = ref64.bound_rhs(R['ops'], R['taus'], ux, zero, zero, R['rho'], R['lam'], R['vx'], case['diff'])
    ra = ref64.compare(torch.from_numpy(res['H/atx']), refa, tola, my)
    print('gain %-14s rhs err/tol %.3f, cached sum %.3f' % (name, rb['max_ratio'], ra['max_ratio']), flush=True)
    assert rb['ok'] and rb['excluded'] == 0, (name, 'b', rb)
    assert ra['ok'], (name, 'atx', ra)


# ---- (4) CG, (5) the captured solve --------------------------------------------------------------------------------------
def test_cg_converges_to_the_dense_solution_of_the_gained_normal_equations(dev):
    """10 x 9 x 8, two repeats, the second with generic gains in [0.5, 2]: tests/test_gpu_slice.py's tolerance for the
    weighted system; the solution without gains is farther away by a wide margin."""
    from tests import diff64, gain64, ref64, slice64
    from tests.helpers import oracle_structs, rel_err
    from unires_amd._project import _channel_plan
    prob, xg, yg, vx, a, S = _small_clean(dev)
    xs, ys = oracle_structs(prob)
    dim = prob['dim_y']
    rho, lam = ref64._f32(prob['rho']), ref64._f32(ys[0].lam)
    e = gain64.gains(S, 'generic')
    Sys = rho * lam * lam * diff64.dense_dtd(dim, [float(v) for v in vx], 'forward')
    for n, xn in enumerate(xs[0]):
        A = _dense(ref64.Operator64(xn.po, prob['method']))
        ev = slice64.spread(e, tuple(xn.dat.shape), a).numpy().reshape(-1) if n == 1 else np.ones(A.shape[0])
        Sys = Sys + ref64._f32(xn.tau) * (A.T @ ((ev * ev)[:, None] * A))
    g = torch.Generator().manual_seed(9)
    b = (torch.rand(dim, generator=g) * 0.1).float()
    want = np.linalg.solve(Sys, b.double().numpy().ravel()).reshape(dim)
    sk = float(np.sqrt(np.linalg.cond(Sys)))
    n_it = int(np.ceil(np.log(0.5e-6) / np.log((sk - 1.0) / (sk + 1.0))))
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
    plan.set_slice_gains(1, a, e.to(dev))
    assert plan.repeat_info(1)['gained'] and not plan.repeat_info(0)['gained']
    x = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), x, rho, lam, max_iter=n_it, tolerance=0.0)
    err = rel_err(x.cpu(), torch.from_numpy(want))
    plan.set_slice_gains(1, a, None)
    xu = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), xu, rho, lam, max_iter=n_it, tolerance=0.0)
    far = rel_err(xu.cpu(), torch.from_numpy(want))
    print('gained CG: %d iterations, rel_err %.3g; the solution without gains %.3g away' % (n_it, err, far), flush=True)
    assert err < GATE
    assert far > 10 * GATE
    plan.close()


def test_a_captured_solve_reads_new_gain_values(dev):
    """Two tol = 0 solves on one plan with different gain VALUES in between (the second replays the captured graph,
    which reads the plan's own tables): the bits of a fresh plan's solve with those gains.  Setting and clearing gains
    flips info[6] bit 5; new slice weights on a gained repeat recompose the tables; an axis other than the slice
    weights' is refused."""
    from tests import gain64, slice64
    from unires_amd._plan import ChannelPlan
    prob, xg, yg, vx, a, S = _small_clean(dev)
    xg[0][1].dat = torch.where(xg[0][1].dat == 0, torch.ones_like(xg[0][1].dat), xg[0][1].dat)
    reps = [(xn.po, xn.tau) for xn in xg[0]]
    vxl = [float(v) for v in vx]
    rho, lam = float(prob['rho']), float(yg[0].lam)
    g = torch.Generator().manual_seed(2)
    b = (torch.rand(prob['dim_y'], generator=g) * 0.1).to(dev)
    x0 = prob['y0'][0].to(dev)
    e1, e2 = gain64.gains(S, 'generic').to(dev), gain64.gains(S, 'generic', seed=44).to(dev)
    u = slice64.weights(S, 'ramp').to(dev)

    def solve(plan):
        x = x0.clone()
        plan.cg(b, x, rho, lam, max_iter=6, tolerance=0.0)
        torch.cuda.synchronize()
        return x

    def fresh(e, w=None):
        pl = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
        if w is not None:
            pl.set_slice_weights(1, a, w)
        if e is not None:
            pl.set_slice_gains(1, a, e)
        x = solve(pl)
        pl.close()
        return x

    plan = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
    first = solve(plan)
    info0 = plan.repeat_info(1)
    assert not info0['gained']
    plan.set_slice_gains(1, a, e1)
    info1 = plan.repeat_info(1)
    assert info1['gained'] and not info1['weighted'] and not info1['shift'] and not info1['fused'], info1
    got1 = solve(plan)
    assert torch.equal(solve(plan), got1)  # (the replay)
    assert not torch.equal(got1, first) and torch.equal(got1, fresh(e1))
    plan.set_slice_gains(1, a, e2)  # values only
    got2 = solve(plan)
    assert not torch.equal(got2, got1)
    assert torch.equal(got2, fresh(e2))
    plan.set_slice_weights(1, a, u)  # weights on a gained repeat: the tables are composed again
    assert plan.repeat_info(1)['gained'] and plan.repeat_info(1)['weighted']
    got3 = solve(plan)
    assert not torch.equal(got3, got2) and torch.equal(got3, fresh(e2, u))
    with pytest.raises(ValueError):  # another axis than the slice weights'
        plan.set_slice_gains(1, (a + 1) % 3, torch.ones(int(xg[0][1].dat.shape[(a + 1) % 3]), device=dev))
    plan.set_slice_weights(1, a, None)
    assert torch.equal(solve(plan), got2)
    plan.set_slice_gains(1, a, None)
    assert plan.repeat_info(1) == info0
    assert torch.equal(solve(plan), first)
    with pytest.raises(ValueError):
        plan.set_slice_gains(1, 3, e1)
    with pytest.raises(Exception):
        plan.set_slice_gains(2, a, e1)
    plan.close()


# ---- (6) the rule on the device ------------------------------------------------------------------------------------------
def _planted(S):
    return torch.tensor([PATTERN[s % 3] for s in range(S)])


def test_update_slice_gains_against_the_float64_rule(dev):
    """x = e* . (A y) + noise, e* = (1, 0.85, 1.15) repeated along the stack: the estimate is gain64.rule64 of the
    device's own sums (themselves covered by (1)) to 1e-12 relative plus one float32 rounding of the stored gain, and
    among the slices with at least half the largest count every planted-low gain lies below every planted-unity gain,
    which lies below every planted-high gain."""
    import unires_amd as U
    from tests import gain64
    from unires_amd._project import _slice_axis
    from unires_amd._update import _update_slice_gains
    prob, (xg, yg, sett) = _phantom(dev)
    xg, yg = [xg[0][:1]], yg[:1]  # one repeat: thick along z, (48, 48, 13)
    xn = xg[0][0]
    a = _slice_axis(xn)
    S = int(xn.dat.shape[a])
    assert a == 2
    Ay = U._proj('A', yg[0].dat, xg[0], yg[0], n=0, method=sett.method, do=sett.do_proj)
    gen = torch.Generator().manual_seed(31)
    star = _planted(S)
    xn.dat = (Ay.cpu() * star.reshape(1, 1, S) + 5.0 * torch.randn(tuple(Ay.shape), generator=gen)).to(dev)
    xn.slice_gain = torch.ones(S, device=dev)
    sett.slice_gain = True
    _update_slice_gains(xg, yg, sett)
    torch.cuda.synchronize()
    got = xn.slice_gain.cpu().double().numpy()
    sums, kappa = xn._gain_sums.cpu().numpy(), float(xn._gain_kappa)
    assert kappa > 0
    want = gain64.rule64(sums, xn.tau, kappa, sett.gain_max)
    assert (np.abs(got - want) <= want * (2.0 ** -24 + 1e-12)).all(), (got, want)
    cnt = sums[2 * S:]
    big = [s for s in range(S) if cnt[s] >= 0.5 * cnt.max()]
    lo, mid, hi = ([got[s] for s in big if PATTERN[s % 3] == v] for v in (0.85, 1.0, 1.15))
    print('rule on the device: gains %s' % [float('%.4f' % v) for v in got], flush=True)
    assert lo and mid and hi
    assert max(lo) < min(mid) and max(mid) < min(hi), (lo, mid, hi)
    assert 1.0 / sett.gain_max < got.min() and got.max() < sett.gain_max  # (far from the clamp)


# ---- (7) end to end ----------------------------------------------------------------------------------------------------
def test_fit_corrects_banding(dev):
    """tests/test_gpu_slice.py's 48 x 48 x 40 phantom, two repeats with 3 mm slices (thick along z and along y), the
    second multiplied slice-wise by (1, 0.85, 1.15) repeated; fit() for 12 ADMM iterations of 20 CG iterations
    (cgs_tol = 0) with the gains off, with sett.slice_gain, and with user gains equal to the planted ones.
    (a) over the second repeat's footprint the RMSE against the phantom is lower with either than off; (b) under
    sett.slice_gain the mean estimated gain of the planted-low slices lies below that of the unity slices, which lies
    below that of the high slices; (c) obj is (12, 3) with obj[:, 0] = obj[:, 1] + obj[:, 2] as before; (d)
    info['slice_gain'] is a list per channel of one CPU float32 tensor or None per repeat.

    Observed values: DESIGN.md 8.12 (the test prints them)."""
    import unires_amd as U
    prob, _ = _phantom(dev)
    truth = prob['truth'][0]
    out, infos = {}, {}
    foot = None
    for arm in ('off', 'gain', 'user'):
        _, (xg, yg, sett) = _phantom(dev)
        x1 = xg[0][1].dat  # thick along y: (48, 16, 40); its slices are planes of constant y
        S = int(x1.shape[1])
        star = _planted(S)
        x1 *= star.to(dev).reshape(1, S, 1)
        if foot is None:
            foot = (U._proj('At', torch.ones_like(x1), xg[0], yg[0], n=1, method=sett.method, do=sett.do_proj) > 0).cpu()
        yg[0].lam0 = float(yg[0].lam) / 4.0
        sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 12, 1e-4, 4.0, 0
        sett.cgs_max_iter, sett.cgs_tol = 20, 0.0
        sett.clean_fov = False
        sett.slice_gain = arm == 'gain'
        if arm == 'user':
            xg[0][1].slice_gain = star.clone()
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 12
        out[arm], infos[arm] = dat[..., 0].cpu(), info
    assert int(foot.sum()) > 0.5 * foot.numel()
    rmse = lambda v: float(((v[foot].double() - truth[foot].double()) ** 2).mean().sqrt())
    r = {arm: rmse(out[arm]) for arm in out}
    print('fit with banding: RMSE over the second repeat\'s footprint off %.3f slice_gain %.3f user %.3f'
          % (r['off'], r['gain'], r['user']), flush=True)
    # (d)
    assert infos['off']['slice_gain'] == [[None, None]]
    sg = infos['gain']['slice_gain']
    assert len(sg) == 1 and len(sg[0]) == 2
    assert all(t.device.type == 'cpu' and t.dtype == torch.float32 for t in sg[0])
    assert tuple(sg[0][0].shape) == (13,) and tuple(sg[0][1].shape) == (16,)
    us = infos['user']['slice_gain']
    assert us[0][0] is None and torch.equal(us[0][1], _planted(16))
    # (c)
    for arm in infos:
        obj = infos[arm]['obj']
        assert tuple(obj.shape) == (12, 3) and obj.dtype == torch.float64 and bool(torch.isfinite(obj).all())
        assert torch.allclose(obj[:, 0], obj[:, 1] + obj[:, 2], rtol=1e-12, atol=0.0)
    e1 = sg[0][1]
    means = [float(e1[[s for s in range(16) if PATTERN[s % 3] == v]].mean()) for v in (0.85, 1.0, 1.15)]
    print('  estimated gains of the banded repeat %s; means low %.4f unity %.4f high %.4f; the clean repeat %.4f .. %.4f'
          % ([float('%.4f' % v) for v in e1.tolist()], means[0], means[1], means[2], float(sg[0][0].min()),
             float(sg[0][0].max())), flush=True)
    assert r['gain'] < r['off']  # (a)
    assert r['user'] < r['off']
    assert means[0] < means[1] < means[2]  # (b)


# ---- (8) gains with both robust rules, the channels on streams of their own ------------------------------------------------
def test_gains_with_both_robust_rules_on_channel_streams(dev):
    """Three channels, sett.slice_gain with sett.slice_robust and sett.voxel_robust, three ADMM iterations through
    fit(): the channels on streams of their own against one channel after the other, on fresh structs each time - the
    same bits in y, in the gains and in the slice weights (the tables are composed at the y-update's plan fetch, on the
    main stream, before the event the channels' streams wait for).  The gains move: the run with the feature off
    differs."""
    import unires_amd as U
    from tests.helpers import gpu_structs, make_problem, rel_err
    from unires_amd._project import _slice_axis
    prob = make_problem(seed=7, dim_y=(40, 36, 33), n_channels=3, thick=3, rot=0.08, trans=1.0)

    def run(streams, gain=True):
        xg, yg, sett = gpu_structs(prob, dev)
        for xc in xg:
            a = _slice_axis(xc[0])
            view = [1, 1, 1]
            view[a] = int(xc[0].dat.shape[a])
            xc[0].dat *= _planted(view[a]).to(dev).reshape(view)
        for yc in yg:
            yc.lam0 = float(yc.lam)
        sett.channel_streams = streams
        sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 3, 1e-4, 1.0, 0
        sett.cgs_max_iter, sett.cgs_tol = 8, 0.0
        sett.clean_fov = False
        sett.slice_gain, sett.slice_robust, sett.voxel_robust = gain, True, True
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 3
        return dat.cpu(), info

    serial, si = run(False)
    for attempt in range(2):
        side, pi = run(True)
        print('channel streams: attempt %d rel. difference %.3g' % (attempt, rel_err(side, serial)), flush=True)
        assert torch.equal(side, serial), (attempt, rel_err(side, serial))
        for c in range(3):
            assert torch.equal(pi['slice_gain'][c][0], si['slice_gain'][c][0]), (attempt, c)
            assert torch.equal(pi['slice_w'][c][0], si['slice_w'][c][0]), (attempt, c)
    assert all(float((si['slice_gain'][c][0] - 1.0).abs().max()) > 0.01 for c in range(3))
    plain, _ = run(True, gain=False)
    assert rel_err(plain, serial) > 1e-4
