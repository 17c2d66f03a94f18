"""Per-voxel weights on the GPU (_input.weight, sett.voxel_robust): the y-update's system

    ( sum_n tau_n A_n^T diag(g_n . u_n . m_n) A_n + rho lam^2 D^T D ) y = sum_n tau_n A_n^T (g_n . u_n . x_n) - lam D^T (w - rho z)

with g_n one weight per x-space voxel, u_n the slice weights of sett.slice_robust (or 1) and m_n the validity mask of
sett.mask_zeros (or 1).

(1) the apply pass, the weighted slice sums and the Huber rule on their own, bit for bit / within a derived bound against
numpy; (2) the weighted matvec and Jacobi diagonal per voxel against float64 for tests/test_gpu_slice.py's cases;
(3) bit identities in fresh processes; (4) the right-hand side; (5) CG against the dense solution; (6) the captured
solve across a change of weight values; (7) fit(); (8) the channels of a y-update on streams of their own; (9) init()
from weight files.

The reference has no counterpart: the float64 side is tests/slice64.weighted_matvec64 with W = g . u . m, the float32
side tests/voxel64.py.  Tolerances of (2): the bound of the UNWEIGHTED operator for 'pow2' weights (every product
exact), plus one rounding of the intermediate for 'ramp' - the pass rounds g u a once: g u is exact in float64, its
product with a is rounded to float64 and then to float32, (u + 2^-53) relative, the factor slice64's extra term has.  No
voxel may be excluded as a tie in (2): asserted.

Children are started the way tests/test_gpu_slice.py starts them (tests/test_gpu_mask.py's ``_run``: one at a time, each
under a time limit, nothing more on the GPU after one that exited non-zero or timed out).

Observed on an MI355X (worst err / tol, 'pow2' / 'ramp'; no voxel excluded as a tie in any case): the matvec z_rigid 0.043 /
0.041, dn_rigid 0.088 / 0.158, translate 0.038 / 0.040, int_shift 0.025 / 0.025, iso 0.034 / 0.027, orient_9 0.044 / 0.039,
sr_2rep 0.095 / 0.095, identity 0.016 / 0.012, z_central 0.085 / 0.060, z_rigid_slab 0.037 / 0.037; the Jacobi diagonal 0.006 -
0.051, dn_rigid 0.130 / 0.156; the weighted slice sums at most 0.002 of their bound; the right-hand sides 0.40 and 0.26.  CG:
30 iterations, 1.64e-7 from the dense solution (the unweighted system's solution is 0.143 away).  fit(): RMSE inside the
planted box's footprint 36.788 off, 11.136 with the box as a 0-weight map, 16.932 with voxel_robust; largest final weight on
a planted voxel 0.3445.  Three channels on streams of their own against one after the other: the same bits, three attempts.

Every test of this file fails on the commit before the feature: the library has no ``unires_voxel_*`` and no
``unires_plan_set_voxel_weights``, ``ChannelPlan`` no ``set_voxel_weights``, ``_input`` no ``weight``.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_mask import BIT_CASES, CASES, GATE, SEED, TWO_KERNEL_ENV, _dense, _run, _small, masks_of, reference
from tests.test_gpu_slice import SUM_SHAPES, WCASES, _phantom, sums_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ('pow2', 'ramp')
bits = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)

# ---- (1) the kernels on their own ---------------------------------------------------------------------------------------
# dz = 1, dz no multiple of 4, a total under 4, groups crossing rows, more than one block, an odd total (a tail)
APPLY_SHAPES = [(1, 1, 1), (1, 1, 3), (5, 7, 1), (67, 1, 65), (5, 7, 6), (41, 38, 60)]
SLICE_VARIANTS = [(None, 0), (0, 0), (1, 1), (2, 0), (2, 1)]  # (axis of the slice weights or None, counted from the far end)
HUBER_SHAPES = [(5, 7, 1), (41, 38, 60)]
HUBER_C = 1.75


def apply_inputs(shape, seed=3):
    """(src, g 'ramp', mask bytes with 30 % zeros, [u per axis] 'ramp') on the CPU."""
    from tests import slice64, voxel64
    gen = torch.Generator().manual_seed(seed + sum(shape))
    src = (torch.randn(shape, generator=gen) * 50.0).float()
    mask = (torch.rand(shape, generator=gen) >= 0.3).to(torch.uint8)
    us = [slice64.weights(shape[a], 'ramp', seed=30 + a) for a in range(3)]
    return src, voxel64.weights(shape, 'ramp'), mask, us


def huber_inputs(shape, seed=13):
    """(x, ay, prior 'ramp'): 30 % zeros in x, one residual exactly HUBER_C, one far beyond it."""
    from tests import voxel64
    gen = torch.Generator().manual_seed(seed + sum(shape))
    x = (torch.randn(shape, generator=gen) * 3.0 + 20.0).float()
    x[torch.rand(shape, generator=gen) < 0.3] = 0.0
    ay = (x + torch.randn(shape, generator=gen) * 2.0).float()
    xf, af = x.view(-1), ay.view(-1)
    xf[-1], af[-1] = 4.0, 4.0 - HUBER_C
    xf[-2], af[-2] = 5.0, 5.0 + 64.0 * HUBER_C
    xf[0], af[0] = 0.0, 1000.0
    return x, ay, voxel64.weights(shape, 'ramp')


_KERNEL_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_voxel import APPLY_SHAPES, SLICE_VARIANTS, HUBER_SHAPES, HUBER_C, apply_inputs, huber_inputs
from tests.test_gpu_slice import SUM_SHAPES, sums_inputs
from tests import voxel64
from unires_amd import _lib
from unires_amd._lib import check, i3
lib, out, res = _lib.load(), sys.argv[1], {}
d = lambda t: t.to('cuda:0')
P = lambda t: None if t is None else t.data_ptr()
sync = torch.cuda.synchronize
for shape in APPLY_SHAPES:
    src, g, mask, us = (apply_inputs(shape))
    src, g, mask, us = d(src), d(g), d(mask), [d(u) for u in us]
    for mi, m in enumerate((None, mask)):
        for si, (axis, flip) in enumerate(SLICE_VARIANTS):
            u = None if axis is None else us[axis]
            key = 'apply/%%s/%%d/%%d' %% ('x'.join(map(str, shape)), mi, si)
            dst = torch.full(shape, float('nan'), device='cuda:0')
            before = src.clone()
            check(lib.unires_voxel_apply(P(src), P(dst), P(g), P(m), P(u), i3(shape), axis or 0, flip, None, None))
            sync()
            assert torch.equal(src.view(torch.int32), before.view(torch.int32))  # out of place: src is only read
            res[key + '/oop'] = dst.cpu().numpy()
            buf = src.clone()
            check(lib.unires_voxel_apply(P(buf), P(buf), P(g), P(m), P(u), i3(shape), axis or 0, flip, None, None))
            sync()
            res[key + '/inp'] = buf.cpu().numpy()
    # all factors 1 in place: nothing changes; a set done word: nothing is written at all
    buf, ones = src.clone(), torch.ones(shape, device='cuda:0')
    check(lib.unires_voxel_apply(P(buf), P(buf), P(ones), None, None, i3(shape), 0, 0, None, None))
    done = torch.ones(1, dtype=torch.int32, device='cuda:0')
    check(lib.unires_voxel_apply(P(buf), P(buf), P(g), P(mask), P(us[2]), i3(shape), 2, 0, P(done), None))
    dst = torch.full(shape, float('nan'), device='cuda:0')
    check(lib.unires_voxel_apply(P(src), P(dst), P(g), P(mask), P(us[2]), i3(shape), 2, 0, P(done), None))
    sync()
    assert torch.equal(buf.view(torch.int32), src.view(torch.int32)), shape
    assert bool(torch.isnan(dst).all()), shape
    done.zero_()  # ... and a clear one lets it run
    check(lib.unires_voxel_apply(P(src), P(dst), P(g), P(mask), P(us[2]), i3(shape), 2, 0, P(done), None))
    sync()
    res['apply/%%s/done0' %% 'x'.join(map(str, shape))] = dst.cpu().numpy()
    # buffers off the 16-byte boundary: the tail loop takes the whole volume
    n = src.numel()
    big = [torch.zeros(n + 4, device='cuda:0') for _ in range(3)]
    s1, d1, g1 = (b[1:1 + n].view(shape) for b in big)
    s1.copy_(src), g1.copy_(g), d1.fill_(float('nan'))
    mb = torch.zeros(n + 4, dtype=torch.uint8, device='cuda:0')
    m1 = mb[1:1 + n].view(shape)
    m1.copy_(mask)
    check(lib.unires_voxel_apply(P(s1), P(d1), P(g1), P(m1), P(us[1]), i3(shape), 1, 0, None, None))
    sync()
    res['apply/%%s/off' %% 'x'.join(map(str, shape))] = d1.cpu().numpy()
    assert float(big[1][0]) == 0.0 and float(big[1][1 + n:].abs().sum()) == 0.0  # nothing written outside
for shape, axis in SUM_SHAPES:
    x, ay = (d(t) for t in sums_inputs(shape, axis))
    g = d(voxel64.weights(shape, 'ramp'))
    S = shape[axis]
    key = 'sums/' + 'x'.join(map(str, shape)) + '/%%d' %% axis
    for name, gg in (('run0', g), ('run1', g), ('ones', torch.ones_like(g))):
        sums = torch.full((2 * S,), float('nan'), dtype=torch.float64, device='cuda:0')
        check(lib.unires_voxel_sums(P(x), P(ay), P(gg), i3(shape), axis, P(sums), None))
        sync()
        res[key + '/' + name] = sums.cpu().numpy()
    sums = torch.full((2 * S,), float('nan'), dtype=torch.float64, device='cuda:0')
    check(lib.unires_slice_sums(P(x), P(ay), i3(shape), axis, P(sums), None))
    sync()
    res[key + '/slice'] = sums.cpu().numpy()
for shape in HUBER_SHAPES:
    x, ay, prior = (d(t) for t in huber_inputs(shape))
    key = 'huber/' + 'x'.join(map(str, shape))
    for name, pr in (('plain', None), ('prior', prior)):
        g = torch.full(shape, float('nan'), device='cuda:0')
        check(lib.unires_voxel_huber(P(x), P(ay), P(pr), HUBER_C, x.numel(), P(g), None))
        sync()
        res[key + '/' + name] = g.cpu().numpy()
    g = prior.clone()  # in place on the prior
    check(lib.unires_voxel_huber(P(x), P(ay), P(g), HUBER_C, x.numel(), P(g), None))
    sync()
    res[key + '/inplace'] = g.cpu().numpy()
np.savez(out, **res)
'''


@pytest.fixture(scope='module')
def kernels(dev, tmp_path_factory):
    return _run(tmp_path_factory.mktemp('voxel_kernels'), 'kernels', _KERNEL_CHILD % dict(root=ROOT))


@pytest.mark.parametrize('shape', APPLY_SHAPES)
def test_apply_pass_bit_for_bit_against_numpy(kernels, shape):
    """Out of place and in place, every MASK x SLICE combination (slices along every axis, in either direction):
    the bits of tests/voxel64.apply32; a set done word leaves every bit (asserted in the child), a clear one does not;
    buffers off their boundary give the same bits through the scalar loop."""
    from tests import voxel64
    src, g, mask, us = (t.numpy() if torch.is_tensor(t) else [u.numpy() for u in t] for t in apply_inputs(shape))
    tag = 'x'.join(map(str, shape))
    for mi, m in enumerate((None, mask)):
        for si, (axis, flip) in enumerate(SLICE_VARIANTS):
            u = None if axis is None else (us[axis][::-1] if flip else us[axis])
            want = voxel64.apply32(src, g, u, axis or 0, m)
            for how in ('oop', 'inp'):
                got = kernels['apply/%s/%d/%d/%s' % (tag, mi, si, how)]
                assert np.array_equal(bits(got), bits(want)), (shape, mi, si, how, int((bits(got) != bits(want)).sum()))
    want = voxel64.apply32(src, g, us[2], 2, mask)
    assert np.array_equal(bits(kernels['apply/%s/done0' % tag]), bits(want)), (shape, 'done word clear')
    want = voxel64.apply32(src, g, us[1], 1, mask)
    assert np.array_equal(bits(kernels['apply/%s/off' % tag]), bits(want)), (shape, 'off the boundary')


@pytest.mark.parametrize('shape, axis', SUM_SHAPES)
def test_voxel_sums_against_float64(kernels, shape, axis):
    """Every weighted sum and every effective count within N_s 2^-53 (its exact value) of the exact sum of the float32
    terms numpy reproduces (voxel64.voxel_sums64); two runs the same bits; every entry written (the output starts as
    NaN); with g = 1 the bits of unires_slice_sums' SSE and its counts as exact integers."""
    from tests import voxel64
    key = 'sums/' + 'x'.join(map(str, shape)) + '/%d' % axis
    x, ay = sums_inputs(shape, axis)
    g = voxel64.weights(shape, 'ramp')
    sse, gs, cnt, b_sse, b_g = voxel64.voxel_sums64(x.numpy(), ay.numpy(), g.numpy(), axis)
    got, S = kernels[key + '/run0'], shape[axis]
    assert got.shape == (2 * S,) and np.isfinite(got).all(), key
    assert np.array_equal(got, kernels[key + '/run1']), (key, 'two runs differ')
    assert cnt[S // 2] == 0 and got[S // 2] == 0.0 and got[S + S // 2] == 0.0, (key, 'the all-zero slice')
    e1, e2 = np.abs(got[:S] - sse), np.abs(got[S:] - gs)
    worst = max(float((e / np.maximum(b, 1e-300))[b > 0].max()) if (b > 0).any() else 0.0 for e, b in ((e1, b_sse), (e2, b_g)))
    print('voxel sums %-14s worst err / bound %.3f' % (key, worst), flush=True)
    assert (e1 <= b_sse).all(), (key, 'sums', int(np.argmax(e1 - b_sse)))
    assert (e2 <= b_g).all(), (key, 'effective counts', int(np.argmax(e2 - b_g)))
    ones, sl = kernels[key + '/ones'], kernels[key + '/slice']
    assert np.array_equal(ones.view(np.int64), sl.view(np.int64)), (key, 'g = 1 against unires_slice_sums')
    assert np.array_equal(ones[S:], cnt), (key, 'counts')


@pytest.mark.parametrize('shape', HUBER_SHAPES)
def test_huber_rule_bit_for_bit_against_numpy(kernels, shape):
    from tests import voxel64
    x, ay, prior = (t.numpy() for t in huber_inputs(shape))
    key = 'huber/' + 'x'.join(map(str, shape))
    h = voxel64.huber64(x, ay, None, HUBER_C)
    assert h.reshape(-1)[-1] == 1.0 and h.reshape(-1)[-2] == np.float32(1.0 / 64.0) and h.reshape(-1)[0] == 1.0
    assert (h[x == 0] == 1.0).all() and (h < 1.0).any()
    assert np.array_equal(bits(kernels[key + '/plain']), bits(h)), key
    want = voxel64.huber64(x, ay, prior, HUBER_C)
    assert np.array_equal(bits(kernels[key + '/prior']), bits(want)), key
    assert np.array_equal(bits(kernels[key + '/inplace']), bits(want)), key


# ---- (2) the weighted matvec and Jacobi diagonal ------------------------------------------------------------------------
_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import SIGNED_PERMS, make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED, zeroed
from tests.test_gpu_voxel import PATTERNS
from tests import slice64, voxel64
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
            xg[0][n].weight = d(voxel64.weights(tuple(xg[0][n].dat.shape), pattern))
            if case['slab']:  # masked, slice-weighted and voxel-weighted: one pass
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
np.savez(out, **res)
'''


def _Ws(case, R, axes, pattern):
    """W_n = g_n(v) u_n[s(v)] m_n(v) per repeat as float64 x-space volumes in the caller's layout (None: a repeat
    without weights); u and m only in the case that has them."""
    from tests import slice64, voxel64
    ms = masks_of(dict(case, masked=case['masked'] if case['slab'] else []), R, 'slab')
    out = []
    for n, xn in enumerate(R['xc']):
        if n not in case['masked']:
            out.append(None)
            continue
        shape = tuple(xn.dat.shape)
        W = voxel64.weights(shape, pattern).double()
        if case['slab']:
            W = W * slice64.spread(slice64.weights(shape[axes[n]], pattern), shape, axes[n]) * ms[n]
        out.append(W)
    return out


def check_voxel(name, case, res):
    from tests import ref64, slice64
    R = reference(case)
    p, myy = R['p'], R['myy']
    n_vox = p.numel()
    p64 = p.double()
    for pattern in PATTERNS:
        key = name + '/' + pattern
        axes = [int(a) for a in res[key + '/axes']]
        infos = json.loads(str(res[key + '/info']))
        for n, info in enumerate(infos):
            info['perm'], info['flip'] = tuple(info['perm']), tuple(info['flip'])
            assert info['voxel_weighted'] == (n in case['masked']), (key, n, info)
            assert info['weighted'] == (bool(case['slab']) and n in case['masked']), (key, n, info)
            assert info['masked'] == bool(case['slab']), (key, n, info)
            if info['voxel_weighted']:  # bit 4 set, bits 0 and 1 clear: the two-kernel form
                assert not info['shift'] and not info['fused'], (key, n, info)
        assert case['expect'] is None or case['expect'](dict(infos[0], masked=True)), (key, infos)
        Ws = _Ws(case, R, axes, pattern)
        q = torch.from_numpy(res[key + '/q'])
        refq, tolq = slice64.weighted_matvec64(R['ops'], R['taus'], Ws, R['p'], R['rho'], R['lam'], R['vx'], case['diff'],
                                               parts=R['parts'], Ap=R['Ap'], exact=pattern == 'pow2')
        r = ref64.compare(q, refq, tolq, myy)
        print('voxel %-22s matvec err/tol %.3f (excluded %d of %d)' % (key, r['max_ratio'], r['excluded'], n_vox), flush=True)
        assert r['ok'], (key, 'matvec', r)
        assert r['excluded'] == 0, (key, 'a voxel was excluded as a tie', r['excluded'])
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
            W = Ws[0]
            vx = [float(v) for v in R['vx'].double()]
            c = ref64._f32(R['rho']) * ref64._f32(R['lam']) ** 2
            const = 2.0 * c * sum(1.0 / (v * v) for v in vx)
            refM = tau * op.At(W * A1) + const
            # tests/test_gpu_mask.py's bound of the diagonal, and the intermediate's extra rounding for 'ramp'
            tolM = (ref64.U + ref64.U64) * (op.c_AtA + ref64.C_DTD) * (tau * M1 + const) + tau * (G1 + D1)
            if pattern != 'pow2':
                tolM = tolM + (ref64.U + ref64.U64) * (1.0 + op.c_A * ref64.U) * tau * op.At(W * op.A(torch.ones(R['prob']['dim_y'], dtype=torch.float64), op.Ka), op.Ka)
            r = ref64.compare(torch.from_numpy(res[key + '/M']), refM, tolM, myy)
            print('voxel %-22s Jacobi err/tol %.3f (excluded %d)' % (key, r['max_ratio'], r['excluded']), flush=True)
            assert r['ok'], (key, 'Jacobi diagonal', r)
            assert r['excluded'] == 0, (key, 'a voxel was excluded as a tie', r['excluded'])


@pytest.mark.parametrize('name', list(WCASES))
def test_weighted_matvec_and_jacobi_per_voxel_against_float64(tmp_path, name):
    case = WCASES[name]
    res = _run(tmp_path, name, _CHILD % dict(root=ROOT, cases=json.dumps({name: dict(case, expect=None)})))
    check_voxel(name, case, res)


# ---- (3) bit identities ------------------------------------------------------------------------------------------------
_BIT_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import make_problem, gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_mask import SEED
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan
cases, weighted, out = json.loads(%(cases)r), %(weighted)r, sys.argv[1]
res = {}
for name, kw in cases.items():
    prob = make_problem(seed=SEED, **kw)
    xg, yg, sett = gpu_structs(prob, 'cuda:0')
    vx = N.voxel_size(prob['mat_y']).float()
    if weighted:
        xg[0][0].weight = torch.ones(tuple(xg[0][0].dat.shape), device='cuda:0')
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
    info = plan.repeat_info(0)
    assert info['voxel_weighted'] == weighted and not info['masked'] and not info['weighted'], info
    assert not (weighted and (info['shift'] or info['fused'])), info
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
    """g = 1 against the unweighted plan forced onto the same two-kernel forms by the existing switches, in fresh
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
from tests import slice64
from oracle import nitorch_restated as N
from unires_amd._project import _channel_plan, _slice_axis
out = sys.argv[1]
prob = make_problem(seed=SEED, **%(kw)r)
xg, yg, sett = gpu_structs(prob, 'cuda:0')
vx = N.voxel_size(prob['mat_y']).float()
p = inputs(prob['dim_y'], prob['dim_y'])[0].to('cuda:0')
res = {}
# both repeats, the second with weight 0 on every voxel
plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
plan.set_voxel_weights(1, torch.zeros(tuple(xg[0][1].dat.shape), device='cuda:0'))
assert plan.repeat_info(1)['voxel_weighted'] and not plan.repeat_info(0)['voxel_weighted']
res['both'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
# g constant per slice ('pow2') against the slice-weighted plan with the same values
xn = xg[0][1]
a = _slice_axis(xn)
w = slice64.weights(int(xn.dat.shape[a]), 'pow2')
plan.set_voxel_weights(1, slice64.spread(w, tuple(xn.dat.shape), a).float().to('cuda:0'))
res['per_slice_voxel'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
plan.set_voxel_weights(1, None)
assert not plan.repeat_info(1)['voxel_weighted']
plan.set_slice_weights(1, a, w.to('cuda:0'))
res['per_slice_slice'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
plan.set_slice_weights(1, a, None)
res['unweighted'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
plan.close()
yg[0]._plan = None
plan = _channel_plan(xg[0][:1], yg[0], prob['method'], prob['do_proj'], vx)
res['alone'] = plan.matvec(p, prob['rho'], yg[0].lam).cpu().numpy()
np.savez(out, **res)
'''


def test_zero_weights_add_nothing_and_weights_constant_per_slice_are_slice_weights(tmp_path):
    """Two repeats under a general rigid.  The second with g = 0: q has the bits of the plan without that repeat (its
    push accumulates exact zeros).  The second with g constant over each slice, 'pow2' values: the bits of the plan
    with those values as slice weights."""
    res = _run(tmp_path, 'zero_g', _ZERO_CHILD % dict(root=ROOT, kw=CASES['sr_2rep']['kw']))
    assert np.array_equal(res['both'], res['alone'])
    assert np.abs(res['both']).max() > 0
    assert np.array_equal(res['per_slice_voxel'], res['per_slice_slice'])
    assert not np.array_equal(res['per_slice_voxel'], res['unweighted'])


# ---- (4) the right-hand side -------------------------------------------------------------------------------------------
RHS_CASES = ('sr_2rep', 'orient_9')  # out of place from the caller's volume; in place on the plan's canonical copy

_RHS_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import SIGNED_PERMS, make_problem, gpu_structs
from tests.test_gpu_mask import SEED
from tests import voxel64
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
    for n in case['masked']:
        xg[0][n].weight = d(voxel64.weights(tuple(xg[0][n].dat.shape), 'pow2'))
    before = [xn.dat.clone() for xn in xg[0]]
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
    res[name + '/info'] = json.dumps([plan.repeat_info(n) for n in range(len(xg[0]))])
    dats = [xn.dat for xn in xg[0]]
    w, z = d(prob['w'][0]), d(prob['z'][0])
    res[name + '/b'] = plan.rhs(dats, w, z, prob['rho'], yg[0].lam).cpu().numpy()
    b2 = torch.empty(prob['dim_y'], device='cuda:0')
    plan.rhs_cached(dats, w, z, prob['rho'], yg[0].lam, out=b2)
    res[name + '/b_cached'] = b2.cpu().numpy()
    res[name + '/atx'] = plan._atx[1].cpu().numpy()
    # new weight values: the cached sum follows them
    for n in case['masked']:
        xg[0][n].weight.fill_(1.0)
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
    plan.rhs_cached(dats, w, z, prob['rho'], yg[0].lam, out=b2)
    res[name + '/atx_ones'] = plan._atx[1].cpu().numpy()
    torch.cuda.synchronize()
    assert all(torch.equal(a_.view(torch.int32), b_.dat.view(torch.int32)) for a_, b_ in zip(before, xg[0]))  # bit-unchanged
np.savez(out, **res)
'''


def test_weighted_right_hand_side_per_voxel_against_float64(tmp_path):
    """b and sum tau At (g . x) with 'pow2' weights (g . x is exact in float32) under ref64.bound_rhs evaluated at
    g . x; out of place from the caller's volume (sr_2rep) and in place on the plan's canonical copy (orient_9: a
    permuted, flipped observation - a wrong permutation of g fails here); the cached form follows a change of the
    weights' values; the observation tensors are bit-unchanged (asserted in the child)."""
    from tests import ref64, voxel64
    cases = {name: dict(WCASES[name], expect=None) for name in RHS_CASES}
    res = _run(tmp_path, 'rhs', _RHS_CHILD % dict(root=ROOT, cases=json.dumps(cases)))
    for name in RHS_CASES:
        case = WCASES[name]
        R = reference(case)
        infos = json.loads(str(res[name + '/info']))
        if name == 'orient_9':
            assert tuple(infos[0]['perm']) != (0, 1, 2) or any(infos[0]['flip']), infos
        my = torch.zeros(R['prob']['dim_y'], dtype=torch.bool)
        for op, xn in zip(R['ops'], R['xc']):
            my |= op.tie_masks(xn.po)[1]
        assert int(my.sum()) < 0.01 * my.numel(), (name, 'tie cap')
        gx, plain = [], []
        for n, xn in enumerate(R['xc']):
            plain.append(xn.dat)
            if n in case['masked']:
                g = voxel64.weights(tuple(xn.dat.shape), 'pow2').double()
                gx.append((g * xn.dat.double()).float())
                assert torch.equal(gx[-1].double(), g * xn.dat.double())
            else:
                gx.append(xn.dat)
        w, z = R['prob']['w'][0], R['prob']['z'][0]
        ref, tol = ref64.bound_rhs(R['ops'], R['taus'], gx, w, z, R['rho'], R['lam'], R['vx'], case['diff'])
        r = ref64.compare(torch.from_numpy(res[name + '/b']), ref, tol, my)
        print('voxel %-10s rhs err/tol %.3f (excluded %d)' % (name, r['max_ratio'], r['excluded']), flush=True)
        assert r['ok'], (name, 'b', r)
        assert np.array_equal(res[name + '/b'], res[name + '/b_cached']) or \
            ref64.compare(torch.from_numpy(res[name + '/b_cached']), ref, tol, my)['ok'], (name, 'cached b')
        zero = torch.zeros_like(w)
        ref_a, tol_a = ref64.bound_rhs(R['ops'], R['taus'], gx, zero, zero, R['rho'], R['lam'], R['vx'], case['diff'])
        ra = ref64.compare(torch.from_numpy(res[name + '/atx']), ref_a, tol_a, my)
        assert ra['ok'], (name, 'atx', ra)
        # ... it is not the unweighted sum, and with all weights 1 it is
        ref_p, tol_p = ref64.bound_rhs(R['ops'], R['taus'], plain, zero, zero, R['rho'], R['lam'], R['vx'], case['diff'])
        assert not ref64.compare(torch.from_numpy(res[name + '/atx']), ref_p, tol_a, my)['ok'], (name, 'atx is unweighted')
        assert ref64.compare(torch.from_numpy(res[name + '/atx_ones']), ref_p, tol_p, my)['ok'], (name, 'atx after new weights')


# ---- (5) CG, (6) the captured solve -------------------------------------------------------------------------------------
def test_cg_converges_to_the_dense_solution_of_the_weighted_normal_equations(dev):
    """10 x 9 x 8, two repeats, the second voxel-weighted ('ramp'); tests/test_gpu_slice.py's tolerance for the slice
    weights (GATE, with the iteration count the system's condition number asks for)."""
    from tests import diff64, ref64, voxel64
    from tests.helpers import oracle_structs, rel_err
    from unires_amd._project import _channel_plan
    prob, xg, yg, vx = _small(dev)
    xs, ys = oracle_structs(prob)
    dim = prob['dim_y']
    rho, lam = ref64._f32(prob['rho']), ref64._f32(ys[0].lam)
    g = voxel64.weights(tuple(xg[0][1].dat.shape), 'ramp')
    Sys = rho * lam * lam * diff64.dense_dtd(dim, [float(v) for v in vx], 'forward')
    for n, xn in enumerate(xs[0]):
        A = _dense(ref64.Operator64(xn.po, prob['method']))
        u = g.double().numpy().reshape(-1) if n == 1 else np.ones(A.shape[0])
        Sys = Sys + ref64._f32(xn.tau) * (A.T @ (u[:, None] * A))
    gen = torch.Generator().manual_seed(9)
    b = (torch.rand(dim, generator=gen) * 0.1).float()
    want = np.linalg.solve(Sys, b.double().numpy().ravel()).reshape(dim)
    sk = float(np.sqrt(np.linalg.cond(Sys)))
    n_it = int(np.ceil(np.log(0.5e-6) / np.log((sk - 1.0) / (sk + 1.0))))
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx)
    plan.set_voxel_weights(1, g.to(dev))
    assert plan.repeat_info(1)['voxel_weighted'] and not plan.repeat_info(0)['voxel_weighted']
    x = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), x, rho, lam, max_iter=n_it, tolerance=0.0)
    err = rel_err(x.cpu(), torch.from_numpy(want))
    plan.set_voxel_weights(1, None)
    xu = torch.zeros(dim, device=dev)
    plan.cg(b.to(dev), xu, rho, lam, max_iter=n_it, tolerance=0.0)
    far = rel_err(xu.cpu(), torch.from_numpy(want))
    print('voxel-weighted CG: %d iterations, rel_err %.3g; unweighted solution %.3g away' % (n_it, err, far), flush=True)
    assert err < GATE
    assert far > 10 * GATE
    plan.close()


def test_a_captured_solve_reads_new_weight_values(dev):
    """Two tol = 0 solves on one plan with different weight VALUES in between (the second replays the captured graph,
    which reads the plan's own weight buffer): the bits of a fresh plan's solve with those weights.  Setting and
    clearing weights flips info[6] as documented; a bad repeat index is refused, and so is regime A = I."""
    from tests import voxel64
    from unires_amd._plan import ChannelPlan
    prob, xg, yg, vx = _small(dev)
    reps = [(xn.po, xn.tau) for xn in xg[0]]
    vxl = [float(v) for v in vx]
    rho, lam = float(prob['rho']), float(yg[0].lam)
    gen = torch.Generator().manual_seed(2)
    b = (torch.rand(prob['dim_y'], generator=gen) * 0.1).to(dev)
    x0 = prob['y0'][0].to(dev)
    shape = tuple(xg[0][1].dat.shape)
    g1, g2 = voxel64.weights(shape, 'ramp').to(dev), voxel64.weights(shape, 'pow2').to(dev)

    def solve(plan):
        x = x0.clone()
        plan.cg(b, x, rho, lam, max_iter=6, tolerance=0.0)
        torch.cuda.synchronize()
        return x

    def fresh(g):
        pl = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
        if g is not None:
            pl.set_voxel_weights(1, g)
        x = solve(pl)
        pl.close()
        return x

    plan = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
    first = solve(plan)
    info0 = plan.repeat_info(1)
    assert not info0['voxel_weighted']
    plan.set_voxel_weights(1, g1)
    info1 = plan.repeat_info(1)
    assert info1['voxel_weighted'] and not info1['masked'] and not info1['weighted'], info1
    assert not info1['shift'] and not info1['fused'], info1
    got1 = solve(plan)
    assert torch.equal(solve(plan), got1)  # (the replay)
    assert not torch.equal(got1, first) and torch.equal(got1, fresh(g1))
    plan.set_voxel_weights(1, g2)  # values only
    got2 = solve(plan)
    assert not torch.equal(got2, got1)
    assert torch.equal(got2, fresh(g2))
    plan.set_voxel_weights(1, None)
    assert plan.repeat_info(1) == info0
    assert torch.equal(solve(plan), first)
    with pytest.raises(Exception):
        plan.set_voxel_weights(2, g1)
    with pytest.raises(ValueError):
        plan.set_voxel_weights(1, g1[:-1])
    plan.close()
    ident = ChannelPlan(prob['dim_y'], vxl, reps[:1], 'denoising', False, device=dev)
    with pytest.raises(Exception, match='(?i)unsupported|A = I'):
        ident.set_voxel_weights(0, torch.ones(prob['dim_y'], device=dev))
    ident.close()


# ---- (7) end to end ----------------------------------------------------------------------------------------------------
BOX = (slice(10, 22), slice(4, 7), slice(8, 20))  # of the second repeat, (48, 16, 40): slices 4..6 of 16, none of them whole
NOISE_SD = 5.0


def test_fit_rejects_a_box_of_corrupted_voxels(dev):
    """tests/test_gpu_mask.py's 48 x 48 x 40 phantom, two repeats with 3 mm slices (thick along z and along y); a box of
    the second repeat's voxels spanning three of its slices (and no whole slice) raised by 20 noise standard
    deviations.  fit() for 12 ADMM iterations of 20 CG iterations (cgs_tol = 0) with the weights off, with the box as
    a 0-weight map, and with sett.voxel_robust and no map.
    (a) inside the box's footprint the RMSE against the phantom is lower with either than off; (b) the weights
    voxel_robust returns are exactly 1 on at least the share of clean voxels tests/voxel64.huber64 gives for the final
    residuals, and below 1/2 on every planted voxel; (c) info['voxel_w'] is a list per channel of one device float32
    tensor per repeat, or None."""
    import unires_amd as U
    from tests import voxel64
    prob, _ = _phantom(dev, NOISE_SD)
    truth = prob['truth'][0]
    out, infos, structs = {}, {}, {}
    for arm in ('off', 'user', 'robust'):
        _, (xg, yg, sett) = _phantom(dev, NOISE_SD)
        x1 = xg[0][1].dat
        assert tuple(x1.shape) == (48, 16, 40)
        x1[BOX] += 20.0 * NOISE_SD
        yg[0].lam0 = float(yg[0].lam) / 4.0
        sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 12, 1e-4, 4.0, 0
        sett.cgs_max_iter, sett.cgs_tol = 20, 0.0
        sett.clean_fov = False
        sett.voxel_robust = arm == 'robust'
        if arm == 'user':
            g = torch.ones(tuple(x1.shape))
            g[BOX] = 0.0
            xg[0][1].weight = g
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 12
        out[arm], infos[arm], structs[arm] = dat[..., 0].cpu(), info, (xg, yg, sett)
    foot = (BOX[0], slice(3 * BOX[1].start, 3 * BOX[1].stop), BOX[2])  # the box in y space: 3 mm slices along y
    rmse = lambda a: float(((a[foot].double() - truth[foot].double()) ** 2).mean().sqrt())
    r = {arm: rmse(out[arm]) for arm in out}
    print('fit with a corrupted box: RMSE inside its footprint off %.3f user %.3f robust %.3f' % (r['off'], r['user'], r['robust']),
          flush=True)
    # (c)
    assert infos['off']['voxel_w'] == [[None, None]]
    vw = infos['user']['voxel_w']
    assert vw[0][0] is None and vw[0][1].is_cuda and vw[0][1].dtype == torch.float32
    assert float(vw[0][1][BOX].abs().max()) == 0.0 and float(vw[0][1].sum()) == vw[0][1].numel() - vw[0][1][BOX].numel()
    vw = infos['robust']['voxel_w']
    assert len(vw) == 1 and len(vw[0]) == 2 and all(t.is_cuda and t.dtype == torch.float32 for t in vw[0])
    assert tuple(vw[0][0].shape) == (48, 48, 13) and tuple(vw[0][1].shape) == (48, 16, 40)
    # (b) the returned weights are the rule's on the residuals of the last iterate: restated from the same A y
    xg, yg, sett = structs['robust']
    planted = torch.zeros(48, 16, 40, dtype=torch.bool)
    planted[BOX] = True
    for n in range(2):
        Ay = U._proj('A', yg[0].dat, xg[0], yg[0], n=n, method=sett.method, do=sett.do_proj)
        c = np.float32(float(sett.voxel_k) / float(xg[0][n].tau) ** 0.5)
        want = voxel64.huber64(xg[0][n].dat.cpu().numpy(), Ay.cpu().numpy(), None, c)
        got = vw[0][n].cpu().numpy()
        clean = ~planted.numpy() if n == 1 else np.ones(got.shape, bool)
        share_got, share_want = float((got[clean] == 1.0).mean()), float((want[clean] == 1.0).mean())
        print('  repeat %d: weights exactly 1 on %.4f of the clean voxels (the restatement: %.4f)' % (n, share_got, share_want),
              flush=True)
        assert np.array_equal(bits(got), bits(want)), (n, 'the weights are not the rule on the final residuals')
        assert share_got >= share_want
    w1 = vw[0][1].cpu()
    print('  planted voxels: largest weight %.4f' % float(w1[planted].max()), flush=True)
    assert float(w1[planted].max()) < 0.5
    assert r['user'] < r['off']  # (a)
    assert r['robust'] < r['off']


# ---- (8) the channels of a y-update on streams of their own -------------------------------------------------------------
def test_weighted_y_update_on_channel_streams(dev):
    """Three channels with user weights: _update_y with the channels on streams of their own against one channel after
    the other, on fresh structs each time (the weights are copied and permuted into the plans at the first y-update's
    plan fetch, on the main stream, before the event the channels' streams wait for): the same bits.  A solve that
    read unwritten weights would be off by the unweighted system's distance, which the last assertion shows to be
    beyond 1e-3."""
    import unires_amd as U
    from tests import voxel64
    from tests.helpers import gpu_structs, make_problem, rel_err
    from unires_amd._project import _channel_plan
    prob = make_problem(seed=7, dim_y=(40, 36, 33), n_channels=3, thick=3, rot=0.08, trans=1.0, scl=0.05)

    def run(streams, weighted):
        xg, yg, sett = gpu_structs(prob, dev)
        if weighted:
            for xc in xg:
                xc[0].weight = voxel64.weights(tuple(xc[0].dat.shape), 'ramp').to(dev)
        sett.channel_streams = streams
        sett.cgs_max_iter, sett.cgs_tol = 8, 0.0
        z, w = prob['z'].to(dev), prob['w'].to(dev)
        tmp = torch.zeros_like(yg[0].dat)
        U._update_y(xg, yg, z, w, prob['rho'], tmp, sett)
        torch.cuda.synchronize()
        for c in range(len(xg)):
            info = _channel_plan(xg[c], yg[c], sett.method, sett.do_proj).repeat_info(0)
            assert info['voxel_weighted'] == weighted, (c, info)
        return [yc.dat.cpu() for yc in yg]

    serial = run(False, True)
    for attempt in range(3):
        side = run(True, True)
        for c in range(3):
            print('channel streams: attempt %d channel %d rel. difference %.3g' % (attempt, c, rel_err(side[c], serial[c])), flush=True)
        for c in range(3):
            assert torch.equal(side[c], serial[c]), (attempt, c, rel_err(side[c], serial[c]))
    plain = run(True, False)
    assert min(rel_err(plain[c], serial[c]) for c in range(3)) > 1e-3


# ---- (9) init() from weight files ---------------------------------------------------------------------------------------
def test_init_from_weight_files_equals_the_tensors_in_memory(dev, tmp_path):
    """Two channels at 32^3: sett.weight as NIfTI paths against the same maps as tensors - the structs' weights, and the
    reconstruction preproc() makes with them, bit for bit; and it is not the unweighted reconstruction."""
    import unires_amd as U
    from tests import coreg_phantom as P
    from tests import voxel64
    from unires_amd import nifti
    from unires_amd.run import preproc
    dim = (32, 32, 32)
    mat = P.true_mat(dim, (2.0, 2.0, 2.0))
    dats = [P.observation(dim, (2.0, 2.0, 2.0), c, 60 + c, dev, scale=0.45)[0] for c in range(2)]
    maps = [voxel64.weights(dim, 'ramp'), voxel64.weights(dim, 'pow2')]
    paths = []
    for c, g in enumerate(maps):
        paths.append(str(tmp_path / ('w%d.nii.gz' % c)))
        nifti.write(paths[-1], g.numpy(), mat)

    def sett_with(weight):
        s = U.settings()
        s.device, s.max_iter, s.vx, s.write_out, s.weight = dev, 3, 0, False, weight
        return s

    data = lambda: [[d.clone(), torch.from_numpy(mat)] for d in dats]
    xf, _, _ = U.init(data(), sett_with([[paths[0]], paths[1]]))
    xm, _, _ = U.init(data(), sett_with([[maps[0]], maps[1].to(dev)]))
    for c in range(2):
        assert xf[c][0].weight.is_cuda == xf[c][0].dat.is_cuda
        assert torch.equal(xf[c][0].weight.cpu().float(), maps[c]) and torch.equal(xm[c][0].weight.cpu().float(), maps[c])
    from_files = preproc(data(), sett_with([[paths[0]], paths[1]]))[0]
    in_memory = preproc(data(), sett_with([maps[0], maps[1]]))[0]
    plain = preproc(data(), sett_with(None))[0]
    assert torch.equal(from_files, in_memory)
    assert not torch.equal(from_files, plain)
    with pytest.raises(ValueError, match='shape'):
        U.init(data(), sett_with([torch.ones(32, 32, 31), None]))
