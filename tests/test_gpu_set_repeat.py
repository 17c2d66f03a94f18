"""Plans with a history: ``ChannelPlan.set_repeat`` after a rigid change, per voxel against the float64 reference.

After every rigid Gauss-Newton step ``_project._channel_plan_any`` keeps the cached plan and calls
``unires_plan_set_repeat`` for the repeats whose operator moved.  Its full-rebuild branch differs from creation: the
quick schedule packers (the wholesale collision rule), tables rebuilt into kept allocations, the kernel family changing
under a workspace the first operator sized, and state that must follow (mask, weights, ``diff``, concurrency) or go (the
captured solve, the preconditioner, the cached sum tau At x).  Every other per-voxel check of the suite runs on a plan
``unires_plan_create`` has just built.

A chain (``CHAINS``) is one plan taken through a sequence of operators by ``plan.set_repeat(n, po_k, tau)`` - called
directly, so a refusal raises instead of being swallowed by ``_channel_plan_any``.  The observation, tau, rho, lam, taps
and dims are stage 0's throughout; stage k replaces the rigid of repeat ``moved`` by the one
``make_problem(seed=s_k, **dict(base, **rigid_kw_k))`` generates for that repeat (``stage_problems``).  Shapes are those
at which tests/test_gpu_voxelwise.py observes each form.

(1) ``test_every_stage_per_voxel``: one child per chain without a schedule switch (creation thorough, rebuilds quick).
    Every stage against its own float64 reference: A p, At v, AtA p of the moved repeat, the matvec q (run twice: the
    same bits) with its dot, AtA of the impulse combs against the trimmed-tap operator, b, the Jacobi diagonal of
    one-repeat chains, the adjoint identity; one ``[set_repeat] full rebuild`` line per call; workspace_bytes unchanged;
    and the reference of stage k - 1 fails the bound against stage k's q.
(2) ``test_a_rebuilt_plan_is_a_fresh_plan_bit_for_bit``: UNIRES_S2_EXACT=0, UNIRES_F1_EXACT=0 (creation packs under the
    wholesale rule too); at every stage a fresh ChannelPlan of the stage's operators gives the same repeat_info, A p,
    At v, q, dot, b, Jacobi diagonal (one-repeat chains: the preconditioners are built for one repeat per channel) and
    6-iteration iterate, bit for bit.
(3) what must go and what must stay: the captured solve, CG against the dense solution, the preconditioner, set_diff,
    set_concurrency.
(4) ``test_mask_and_weights_follow_a_rebuild``: a zeroed slab and 'ramp' slice weights across chains z, dn and orient.
(5) the facade: ``xn.po = _proj_info(..., rigid=new)`` and ``_channel_plan`` again.

No tolerance of its own: every per-voxel bound is ref64 / slice64 / tests/test_gpu_mask.py's for the same operator, the
tie cap is the suite's (fewer than 1 % of the volume), the dense-solve gate tests/test_gpu_mask.py's GATE.
tests/test_set_repeat.py holds every stage to the tie cap on the CPU and shows that consecutive stage references differ
beyond the bound.

Children are started the way tests/test_gpu_mask.py's ``_run`` starts them: one at a time, each under a time limit, and
after a child that exited non-zero or timed out nothing more is started on the GPU.

Observed on an MI355X.  The form of the moved repeat (``repeat_info``: pull2 / splat2 axis / shift / fused / separable), the
schedule build its last [splat2] line names (stage 0: ``unires_plan_create``'s, thorough; later stages: the rebuild's, quick;
none: no schedule), and the worst err / tol of every check of (1); no voxel is excluded as a FOV tie at any stage.  Stages
whose operator has an entry in tests/test_gpu_voxelwise.py's table ran on that entry's form (``FORMS``); no stage was
declined k_ata1 or splat2 after a quick build (the allowance ``_declined`` stays: UNIRES_F1_MIN_FILL is a threshold on a
fill the quick packing lowers by a few points, and such a stage would be reported, not failed).

| chain, stage | pull2 axis shift fused sep.  build    | A     At    AtA   q     b     combs Jacobi |
|--------------|---------------------------------------|--------------------------------------------|
| z        0   | yes   2    no    no    no    one-pass | 0.124 0.328 0.196 0.057 0.286 0.209 0.052  |
| z        1   | yes   2    yes   no    no    one-pass | 0.010 0.016 0.007 0.038 0.286 0.005 0.020  |
| z        2   | yes   2    yes   no    no    one-pass | 0.007 0.005 0.003 0.030 0.207 0.004 0.011  |
| z        3   | yes   2    no    no    no    two-pass | 0.100 0.161 0.096 0.047 0.280 0.101 0.040  |
| z        4   | yes   none no    no    no    none     | 0.106 0.168 0.123 0.043 0.280 0.114 0.044  |
| z        5   | yes   2    no    no    no    one-pass | 0.118 0.244 0.194 0.059 0.243 0.212 0.053  |
| z        6   | no    none no    no    no    none     | 0.093 0.179 0.160 0.060 0.286 0.052 0.045  |
| z        7   | yes   2    yes   no    no    one-pass | 0.009 0.014 0.010 0.035 0.286 0.004 0.017  |
| dn       0   | yes   -1   no    yes   no    one-pass | 0.278 0.400 0.390 0.165 0.399 0.290 0.223  |
| dn       1   | yes   -1   no    yes   no    two-pass | 0.158 0.133 0.122 0.069 0.244 0.097 0.042  |
| dn       2   | yes   none no    no    no    none     | 0.188 0.188 0.104 0.083 0.244 0.123 0.071  |
| dn       3   | yes   -1   no    yes   no    one-pass | 0.186 0.234 0.214 0.108 0.244 0.128 0.130  |
| dn       4   | yes   -1   no    yes   no    one-pass | 0.000 0.000 0.000 0.030 0.188 0.000 0.008  |
| dn       5   | yes   -1   no    yes   no    one-pass | 0.020 0.022 0.040 0.033 0.023 0.022 0.010  |
| iso      0   | yes   2    no    no    no    one-pass | 0.173 0.365 0.305 0.039 0.352 0.315 0.043  |
| iso      1   | yes   none no    no    no    none     | 0.089 0.183 0.144 0.027 0.256 0.125 0.039  |
| iso      2   | yes   2    no    no    no    one-pass | 0.092 0.288 0.206 0.032 0.256 0.249 0.038  |
| iso      3   | yes   2    no    no    no    two-pass | 0.053 0.142 0.059 0.034 0.232 0.162 0.035  |
| isog     0   | yes   -1   no    no    yes   one-pass | 1.000 0.853 0.370 0.013 0.523 0.284 0.011  |
| isog     1   | yes   none no    no    yes   none     | 1.000 1.000 0.985 0.012 0.834 0.121 0.010  |
| isog     2   | yes   -1   no    no    yes   one-pass | 1.000 0.863 0.326 0.015 0.481 0.211 0.013  |
| sr_2rep  0   | yes   1    no    no    no    one-pass | 0.188 0.211 0.199 0.102 0.320 0.207 -      |
| sr_2rep  1   | yes   1    no    no    no    two-pass | 0.096 0.130 0.050 0.102 0.320 0.089 -      |
| sr_2rep  2   | yes   1    no    no    no    one-pass | 0.014 0.018 0.008 0.102 0.320 0.014 -      |
| sr_2rep  3   | yes   1    no    no    no    one-pass | 0.127 0.243 0.180 0.102 0.320 0.132 -      |
| dn_2rep  0   | yes   -1   no    yes   no    one-pass | 0.156 0.181 0.132 0.069 0.174 0.107 -      |
| dn_2rep  1   | yes   -1   no    no    no    two-pass | 0.118 0.119 0.054 0.043 0.201 0.002 -      |
| dn_2rep  2   | yes   -1   no    yes   no    one-pass | 0.159 0.160 0.123 0.054 0.201 0.099 -      |
| orient   0   | yes   2    no    no    no    one-pass | 0.063 0.141 0.117 0.046 0.263 0.149 0.052  |
| orient   1   | yes   2    no    no    no    one-pass | 0.052 0.112 0.058 0.040 0.243 0.145 0.031  |
| orient   2   | yes   2    no    no    no    one-pass | 0.044 0.134 0.109 0.056 0.243 0.010 0.042  |
| orient   3   | yes   2    no    no    no    one-pass | 0.063 0.141 0.117 0.046 0.263 0.149 0.052  |

(isog's 1.000: voxels only the dropped taps reach - the kernel returns 0, err = D - as in tests/test_gpu_voxelwise.py's
iso2_gauss.  sr_2rep's q and b: the worst voxel is the untouched repeat's.  At 21 x 19 x 33 the schedule of dn_2rep survives
0.7 rad in two passes; k_ata1 does not.)

(2): every stage of every chain equal bit for bit in every output compared - no table, flag or layout of a rebuilt plan
depends on its history.  (3): every bit identity holds, with and without the captured graph; CG 29 iterations, 2.0e-7 from the
dense solution of the second operator (the first operator's solution is 0.126 away); central q 0.033 / 0.029 of its bound.
(4), worst err / tol of q / the Jacobi diagonal over the stages: z 0.050 / 0.042, dn 0.114 / 0.138, orient 0.044 / 0.050.
(5): rhs_cached 0.280 of bound_rhs for the new operator; the new plan's masked, weighted q 0.050.
No check failed: the suite found no bug in the rebuild.
"""
import functools
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_mask import GATE, zeroed
from tests.test_gpu_voxelwise import TILE, comb, inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11  # tests/test_gpu_voxelwise.py's
QUICK_ENV = {'UNIRES_S2_EXACT': '0', 'UNIRES_F1_EXACT': '0'}  # read once per process: creation packs wholesale too


def _about(angle, c=(20.0, 18.5, 30.0)):
    """T(c) Rz(angle) T(-c): a rotation about z through the centre of a 41 x 38 x 61 volume of 1 mm voxels."""
    from tests.helpers import rigid_matrix
    T = lambda t: rigid_matrix(list(t), (0.0, 0.0, 0.0))
    return T(c) @ rigid_matrix((0.0, 0.0, 0.0), (0.0, 0.0, angle)) @ T([-v for v in c])


_R = lambda rot, seed=SEED: dict(rot=rot, seed=seed)
_A = lambda *angles: dict(angles=tuple(float(a) for a in angles))
# base: make_problem kwargs; moved: the repeat whose rigid changes; stages: rigid kwargs (seed 11 unless given), 'base'
# (stage 0's rigid again) or ('about', angle) - the 4 x 4 of ``_about``
CHAINS = {
    # pull2 + splat2 AXIS 2 -> shift kernel -> aligned -> two-pass schedule build (entries grow) -> no splat2 (atomics)
    # -> back to a small schedule in the grown buffers -> no pull2 -> shift tables again
    'z': dict(base=dict(dim_y=(41, 38, 60), thick=6, thick_axes=[2], scl=0.1, trans=2.0), moved=0,
              stages=[_R(0.1), _R(0.0), dict(shift=(2.0, -1.0, 3.0)), _A(0.5, 0, 0), _A(0.7, 0, 0), _R(0.1, 12),
                      _A(0.78, 0, 0), _R(0.0, 12)]),
    # k_ata1 under the wholesale rule, its two-pass build, leaving its domain and coming back, an integer and a
    # fractional translation
    'dn': dict(base=dict(dim_y=(41, 38, 61), regime='dn', trans=2.0), moved=0,
               stages=[_R(0.1), _A(0, 0.5, 0), _A(0, 0.7, 0), _R(0.1, 12), dict(shift=(1.0, -2.0, 1.0)), _R(0.0)]),
    # the hybrid form, its fall-back inside build_repeat_kernels when the axis-2 schedule goes, hybrid again, with the
    # gbuf2 the first operator sized
    'iso': dict(base=dict(dim_y=(42, 38, 61), thick=2, iso=(2, 2, 2), scl=0.1, trans=1.0), moved=0,
                stages=[_R(0.1), _A(0.7, 0, 0), _R(0.1, 12), _A(0, 0.5, 0)]),
    # the separable passes with the window pull present, absent, present
    'isog': dict(base=dict(dim_y=(34, 30, 36), thick=2, iso=(2, 2, 2), prof_ip=2, trans=1.0), moved=0,
                 stages=[_R(0.1), _A(0.7, 0, 0), _R(0.1, 12)]),
    # one repeat rebuilt beside an untouched one; accumulating stores; the stencil added once
    'sr_2rep': dict(base=dict(dim_y=(41, 38, 61), thick=4, n_repeats=2, scl=0.1, trans=1.0), moved=1,
                    stages=[_R(0.1), _A(0, 0.5, 0), _R(0.0), _R(0.1, 12)]),
    # the same on k_ata1
    'dn_2rep': dict(base=dict(dim_y=(21, 19, 33), regime='dn', n_repeats=2, trans=1.0), moved=0,
                    stages=[_R(0.1), _A(0.7, 0, 0), _R(0.1, 12)]),
    # the relabelling changing under the plan: perm (0, 2, 1) flip (0, 1, 0) -> the same perm, flip (1, 0, 0) -> perm
    # (2, 0, 1), no flip -> back (tests/test_set_repeat.py holds the chain to these)
    'orient': dict(base=dict(dim_y=(41, 38, 61), thick=4, thick_axes=[2], scl=0.0, orient=9, rot=0.1, trans=2.0), moved=0,
                   stages=['base', ('about', math.pi - 0.04), ('about', math.pi / 2 + 0.03), 'base']),
}
ORIENT_STAGES = [((0, 2, 1), (0, 1, 0)), ((0, 2, 1), (1, 0, 0)), ((2, 0, 1), (0, 0, 0)), ((0, 2, 1), (0, 1, 0))]
MW_CHAINS = {'z': 4, 'dn': 4, 'orient': 4}  # (4): the chain's first stages with a mask and slice weights


@functools.lru_cache(maxsize=None)
def stage_problems(name):
    """One make_problem dict per stage: stage 0's, with the rigid of repeat ``moved`` replaced."""
    from tests.helpers import SIGNED_PERMS, make_problem
    ch = CHAINS[name]
    base, n = dict(ch['base']), ch['moved']
    if 'orient' in base:
        base['orient'] = [SIGNED_PERMS[base['orient']]]
    probs = []
    for k, st in enumerate(ch['stages']):
        if isinstance(st, dict):
            kw = dict(st)
            seed = kw.pop('seed', SEED)
            gen = make_problem(seed=seed, **dict(base, **kw))
            rigid = gen['chans'][0]['reps'][n]['rigid']
        elif st == 'base':
            gen = make_problem(seed=SEED, **base) if k == 0 else None
            rigid = (gen or probs[0])['chans'][0]['reps'][n]['rigid']
        else:
            gen, rigid = None, _about(st[1])
        if k == 0:
            probs.append(gen)
            continue
        c0 = probs[0]['chans'][0]
        reps = [dict(r, rigid=rigid) if i == n else r for i, r in enumerate(c0['reps'])]
        probs.append(dict(probs[0], chans=[dict(c0, reps=reps)]))
    return probs


@functools.lru_cache(maxsize=None)
def _repeat_ref(name, k, i):
    """Repeat i's float64 operator at stage k with its orientation, tie masks and A^T A parts of p."""
    from oracle import unires_restated as O
    from tests import ref64
    from tests.helpers import oracle_structs
    prob = stage_problems(name)[k]
    xn = oracle_structs(prob)[0][0][i]
    mat, _ = O.proj_matrix(xn.po, prob['method'])
    perm, flip, oriented = ref64.orientation_of(mat.float().double())
    op = ref64.Operator64(xn.po, prob['method'], oriented=oriented)
    mx, my, myy, _ = op.tie_masks(xn.po)
    p = inputs(prob['dim_y'], xn.po.dim_x)[0]
    return dict(op=op, po=xn.po, orient=(perm, flip), oriented=oriented, mx=mx, my=my, myy=myy, parts=op.parts_AtA(p),
                tau=xn.tau, dat=xn.dat)


@functools.lru_cache(maxsize=None)
def stage_reference(name, k):
    """The float64 side of stage k of a chain: one operator per repeat (an untouched repeat's is stage 0's), the unions
    of their tie masks, the inputs.  Built once and shared by every test that needs the stage."""
    from oracle import nitorch_restated as N
    from tests.helpers import oracle_structs
    ch = CHAINS[name]
    prob = stage_problems(name)[k]
    ys = oracle_structs(prob)[1]
    reps = [_repeat_ref(name, k if i == ch['moved'] else 0, i) for i in range(len(prob['chans'][0]['reps']))]
    R = dict(prob=prob, reps=reps, ops=[r['op'] for r in reps], taus=[r['tau'] for r in reps], lam=ys[0].lam,
             vx=N.voxel_size(prob['mat_y']).float(), rho=torch.tensor(prob['rho'], dtype=torch.float32),
             parts=[r['parts'] for r in reps], moved=ch['moved'])
    R['p'], R['v'] = inputs(prob['dim_y'], reps[ch['moved']]['po'].dim_x)
    R['my'] = torch.zeros(prob['dim_y'], dtype=torch.bool)
    R['myy'] = R['my'].clone()
    for r in reps:
        R['my'] |= r['my']
        R['myy'] |= r['myy']
    return R


def comb_spacing(ratio):
    """tests/test_gpu_voxelwise.py's ``spacings`` for the y-space combs, from the moved repeat's ratio: 2 (3 r + 4) + 1."""
    return tuple(2 * (3 * int(r) + 4) + 1 for r in ratio)


def tie_counts(R):
    """Voxels excluded as FOV ties: (x space, A of the moved repeat; y space, the right-hand side; y space, A^T A)."""
    return int(R['reps'][R['moved']]['mx'].sum()), int(R['my'].sum()), int(R['myy'].sum())


def tie_cap_ok(R):
    """The suite's cap: fewer than 1 % of the volume excluded, in x space and in y space."""
    nx, ny = R['v'].numel(), R['p'].numel()
    mx, my, myy = tie_counts(R)
    return mx < 0.01 * nx and my < 0.01 * ny and myy < 0.01 * ny


def matvec64(R, which='forward'):
    from tests import ref64
    return ref64.bound_matvec_reps(R['ops'], R['taus'], R['p'], R['rho'], R['lam'], R['vx'], which, parts=R['parts'])


def mw_weights(R):
    """(4)'s W = u[s(v)] m(v) of repeat 0 in the caller's layout: the 'slab' mask of tests/test_gpu_mask.py and
    slice64's 'ramp' weights along the descriptor's thick axis."""
    from tests import slice64
    r = R['reps'][0]
    shape, axis = tuple(r['dat'].shape), int(r['po'].dim_thick)
    m = (zeroed(r['dat'], 'slab') != 0).double()
    return slice64.spread(slice64.weights(shape[axis], 'ramp'), shape, axis) * m


def mw_matvec64(R):
    """(ref, tol) of the masked, weighted matvec of a one-repeat stage (slice64.weighted_matvec64; 'ramp' rounds)."""
    from tests import slice64
    return slice64.weighted_matvec64(R['ops'], R['taus'], [mw_weights(R)], R['p'], R['rho'], R['lam'], R['vx'], 'forward',
                                     parts=R['parts'], exact=False)


def jacobi64(R, W=None):
    """(ref, tol) of the Jacobi diagonal of a one-repeat stage, tests/test_gpu_mask.py's ``check_case`` bound; with
    ``W`` (mask times weights) the weighted diagonal and tests/test_gpu_slice.py's extra rounding of the intermediate."""
    from tests import ref64
    op, tau = R['ops'][0], ref64._f32(R['taus'][0])
    if 'ones' not in R:
        one = torch.ones(R['prob']['dim_y'])
        R['ones'] = (op.parts_AtA(one), op.A(one.double()))
    (AtA1, M1, G1, D1), A1 = R['ones']
    vx = [float(v) for v in R['vx'].double()]
    c = ref64._f32(R['rho']) * ref64._f32(R['lam']) ** 2
    const = 2.0 * c * sum(1.0 / (v * v) for v in vx)
    refM = tau * (AtA1 if W is None else op.At(W * A1)) + const
    tolM = (ref64.U + ref64.U64) * (op.c_AtA + ref64.C_DTD) * (tau * M1 + const) + tau * (G1 + D1)
    if W is not None:
        ones = torch.ones(R['prob']['dim_y'], dtype=torch.float64)
        tolM = tolM + (ref64.U + ref64.U64) * (1.0 + op.c_A * ref64.U) * tau * op.At(W * op.A(ones, op.Ka), op.Ka)
    return refM, tolM


# ---- the children ----------------------------------------------------------------------------------------------------
_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import gpu_structs
from tests.test_gpu_mask import zeroed
from tests.test_gpu_voxelwise import TILE, comb, inputs
from tests.test_gpu_set_repeat import CHAINS, comb_spacing, stage_problems
from tests import slice64
from oracle import nitorch_restated as N
from unires_amd._plan import ChannelPlan
from unires_amd._project import _channel_plan, _slice_axis
name, mode, n_stages, out = %(name)r, %(mode)r, %(n_stages)r, sys.argv[1]
dev = 'cuda:0'
ch = CHAINS[name]
n = ch['moved']
probs = stage_problems(name)[:n_stages]
prob = probs[0]
xg, yg, sett = gpu_structs(prob, dev)
x, y = xg[0], yg[0]
vx = N.voxel_size(prob['mat_y']).float()
vxl = [float(v) for v in vx]
method, do, dim_y = prob['method'], prob['do_proj'], prob['dim_y']
rho, lam = float(prob['rho']), float(y.lam)
d = lambda t: t.to(dev)
nrep = len(x)
sys.stderr.write('[stage] 0\n')
sys.stderr.flush()
if mode == 'mw':
    x[0].dat = zeroed(x[0].dat, 'slab')
    a = _slice_axis(x[0])
    x[0].slice_w = d(slice64.weights(int(x[0].dat.shape[a]), 'ramp'))
    plan = _channel_plan(x, y, method, do, vx, mask_zeros=True, weights=True)
else:
    plan = _channel_plan(x, y, method, do, vx)
reps = [(xn.po, xn.tau) for xn in x]
p, v = (d(t) for t in inputs(dim_y, plan.dims_x[n]))
sy = comb_spacing(x[n].po.ratio if method == 'super-resolution' else (1, 1, 1))
combs = [d(comb(dim_y, TILE, sy, ph)) for ph in (0, 1)]
w_c, z_c, y0 = d(prob['w'][0]), d(prob['z'][0]), d(prob['y0'][0])
res = {}
ws0 = plan.workspace_bytes


def matvec(pl):
    dot = torch.zeros((), dtype=torch.float64, device=dev)
    q = pl.matvec(p, rho, lam, dot=dot)
    torch.cuda.synchronize()
    return q, np.array(dot.item())


def jacobi(pl):
    M = torch.empty(dim_y, dtype=torch.float32, device=dev)
    pl.precond_build(rho, lam, mode='jacobi', out=M)
    return M


def solve(pl, b):
    xx = y0.clone()
    pl.cg(b, xx, rho, lam, max_iter=6, tolerance=0.0)
    torch.cuda.synchronize()
    return xx


for k in range(len(probs)):
    if k > 0:
        sys.stderr.write('[stage] %%d\n' %% k)
        sys.stderr.flush()
        xk = gpu_structs(probs[k], dev)[0][0][n]
        plan.set_repeat(n, xk.po, xk.tau)
        reps[n] = (xk.po, xk.tau)
    key = 's%%d/' %% k
    infos = [plan.repeat_info(i) for i in range(nrep)]
    res[key + 'info'] = json.dumps(infos)
    res[key + 'ws'] = np.array(plan.workspace_bytes == ws0)
    q, dot = matvec(plan)
    res[key + 'q'], res[key + 'dot'] = q.cpu().numpy(), dot
    if mode == 'prod':
        q2, dot2 = matvec(plan)
        res[key + 'q2'], res[key + 'dot2'] = q2.cpu().numpy(), dot2
        for op, dat in (('A', p), ('At', v), ('AtA', p)):
            res[key + op] = plan.proj_apply(n, op, dat).cpu().numpy()
        for ph in (0, 1):
            res[key + 'AtA_comb%%d' %% ph] = plan.proj_apply(n, 'AtA', combs[ph]).cpu().numpy()
        res[key + 'b'] = plan.rhs([xn.dat for xn in x], w_c, z_c, rho, lam).cpu().numpy()
    if mode == 'mw' or (mode == 'prod' and nrep == 1):
        res[key + 'M'] = jacobi(plan).cpu().numpy()
    if mode == 'fresh':
        fresh = ChannelPlan(dim_y, vxl, reps, method, do, device=dev)
        b = plan.rhs([xn.dat for xn in x], w_c, z_c, rho, lam)
        qf, dotf = matvec(fresh)
        same = dict(info=infos == [fresh.repeat_info(i) for i in range(nrep)],
                    q=torch.equal(q, qf), dot=bool(dot == dotf),
                    A=torch.equal(plan.proj_apply(n, 'A', p), fresh.proj_apply(n, 'A', p)),
                    At=torch.equal(plan.proj_apply(n, 'At', v), fresh.proj_apply(n, 'At', v)),
                    b=torch.equal(b, fresh.rhs([xn.dat for xn in x], w_c, z_c, rho, lam)),
                    M=nrep > 1 or torch.equal(jacobi(plan), jacobi(fresh)),
                    solve=torch.equal(solve(plan, b), solve(fresh, b)))
        res[key + 'same'] = json.dumps(same)
        res[key + 'q_diff'] = np.array(int((q != qf).sum()))
        res[key + 'fresh_info'] = json.dumps([fresh.repeat_info(i) for i in range(nrep)])
        fresh.close()
if mode == 'mw':
    # another dim_x under a mask: refused, and the plan is left as it was
    import unires_amd as U
    r = prob['chans'][0]['reps'][0]
    dx = list(r['dim_x'])
    dx[_slice_axis(x[0])] -= 1
    po = U._proj_info(dim_y, prob['mat_y'], tuple(dx), r['mat_x'], rigid=r['rigid'], prof_ip=r['prof_ip'],
                      prof_tp=r['prof_tp'], scl=r['scl'], device=dev)
    try:
        plan.set_repeat(0, po, x[0].tau)
        res['refusal'] = np.array('none')
    except ValueError as e:
        res['refusal'] = np.array(str(e))
    res['q_after_refusal'] = matvec(plan)[0].cpu().numpy()
np.savez(out, **res)
'''

_DEAD = []  # set by the first child that exits non-zero or times out: nothing more runs on the GPU after it


def _run(tmp_path, tag, script, env=None, timeout=120):
    """tests/test_gpu_mask.py's ``_run``, returning the child's stderr as well."""
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
    return dict(np.load(path)), r.stderr


def _chain_child(tmp_path, name, mode, n_stages=None, env=None):
    n_stages = len(CHAINS[name]['stages']) if n_stages is None else n_stages
    e = dict(env or {}, UNIRES_SET_REPEAT_VERBOSE='1', UNIRES_SPLAT2_VERBOSE='1')
    res, err = _run(tmp_path, '%s_%s' % (name, mode), _CHILD % dict(root=ROOT, name=name, mode=mode, n_stages=n_stages), e)
    return res, re.split(r'^\[stage\] \d+\n', err, flags=re.M)[1:], n_stages


def _infos(res, k):
    infos = json.loads(str(res['s%d/info' % k]))
    for info in infos:
        info['perm'], info['flip'] = tuple(info['perm']), tuple(info['flip'])
    return infos


def _form(info, log):
    """(pull2, splat2 axis, shift, fused, separable, the schedule build that ran last) of a repeat at a stage."""
    builds = re.findall(r'\[splat2\].*build (\S+), max instructions per tile (\d+)', log)
    return (info['pull2'], info['splat2_axis'], info['shift'], info['fused'], info['separable'],
            builds[-1][0] if builds else None)


# ---- (1) every stage per voxel, on the production rule ----------------------------------------------------------------
# The form of the moved repeat at every stage, as observed on an MI355X: (pull2, splat2 axis, shift, fused, separable,
# schedule build).  Stages whose operator has an entry in tests/test_gpu_voxelwise.py's table run on that entry's form.
_T, _F = True, False
_FORMS = {
    # rot 0.1; rot 0.0 (the table's translate: shift tables, the schedule built too); shift (2, -1, 3) (int_shift_z60);
    # 0.5 / 0.7 / 0.78 rad about x (sweep_z_x0.50 / 0.70 / 0.78); seed 12's rot 0.1 and rot 0.0
    'z': [(_T, 2, _F, _F, _F, 'one-pass'), (_T, 2, _T, _F, _F, 'one-pass'), (_T, 2, _T, _F, _F, 'one-pass'),
          (_T, 2, _F, _F, _F, 'two-pass'), (_T, None, _F, _F, _F, None), (_T, 2, _F, _F, _F, 'one-pass'),
          (_F, None, _F, _F, _F, None), (_T, 2, _T, _F, _F, 'one-pass')],
    # denoise; 0.5 / 0.7 rad about y (sweep_dn_y0.50 / 0.70); seed 12; the two translations stay on k_ata1
    'dn': [(_T, -1, _F, _T, _F, 'one-pass'), (_T, -1, _F, _T, _F, 'two-pass'), (_T, None, _F, _F, _F, None),
           (_T, -1, _F, _T, _F, 'one-pass'), (_T, -1, _F, _T, _F, 'one-pass'), (_T, -1, _F, _T, _F, 'one-pass')],
    # iso2_rect (the hybrid: pull2 + AXIS 2, not separable); no schedule at 0.7: the fall-back; hybrid again, twice
    'iso': [(_T, 2, _F, _F, _F, 'one-pass'), (_T, None, _F, _F, _F, None), (_T, 2, _F, _F, _F, 'one-pass'),
            (_T, 2, _F, _F, _F, 'two-pass')],
    # iso2_gauss: the separable passes
    'isog': [(_T, -1, _F, _F, _T, 'one-pass'), (_T, None, _F, _F, _T, None), (_T, -1, _F, _F, _T, 'one-pass')],
    # repeat 1 (thick along y)
    'sr_2rep': [(_T, 1, _F, _F, _F, 'one-pass'), (_T, 1, _F, _F, _F, 'two-pass'), (_T, 1, _F, _F, _F, 'one-pass'),
                (_T, 1, _F, _F, _F, 'one-pass')],
    # at 21 x 19 x 33 the schedule survives 0.7 rad (two passes); k_ata1 does not
    'dn_2rep': [(_T, -1, _F, _T, _F, 'one-pass'), (_T, -1, _F, _F, _F, 'two-pass'), (_T, -1, _F, _T, _F, 'one-pass')],
    'orient': [(_T, 2, _F, _F, _F, 'one-pass')] * 4,
}
FORMS = {(name, k): form for name, forms in _FORMS.items() for k, form in enumerate(forms)}


def _declined(want, got):
    """k_ata1 and splat2 may be declined after a quick build (the wholesale rule fills lanes a few points lower, and
    UNIRES_F1_MIN_FILL is a threshold on that): the same form but for ``fused`` off, or the schedule off."""
    return got in ((want[0], want[1], want[2], False, want[4], want[5]), (want[0], None, want[2], False, want[4], None))


def check_stage(name, k, res, R, prev):
    """Every output of stage k per voxel against the stage's float64 reference; returns {check: worst err / tol}."""
    from tests import ref64
    key = 's%d/' % k
    n, r = R['moved'], R['reps'][R['moved']]
    op, p, v = r['op'], R['p'], R['v']
    p64, v64 = p.double(), v.double()
    infos = _infos(res, k)
    for info, rr in zip(infos, R['reps']):  # the bound's orientation is restated, and must be the plan's
        assert (info['perm'], info['flip']) == rr['orient'], (name, k, info, rr['orient'])
    assert tie_cap_ok(R), (name, k, 'tie cap', tie_counts(R))
    assert bool(res[key + 'ws']), (name, k, 'workspace_bytes changed')
    rep = {}

    def per_voxel(what, got, ref, tol, ex):
        c = ref64.compare(torch.from_numpy(got), ref, tol, ex)
        assert c['ok'], (name, k, what, c)
        rep[what] = c['max_ratio']

    refA, tolA = op.bound_A(p)
    per_voxel('A', res[key + 'A'], refA, tolA, r['mx'])
    refAt, tolAt = op.bound_At(v)
    per_voxel('At', res[key + 'At'], refAt, tolAt, r['my'])
    ref, M, G, D = r['parts']
    per_voxel('AtA', res[key + 'AtA'], ref, (ref64.U + ref64.U64) * op.c_AtA * M + G + D, r['myy'])
    refq, tolq = matvec64(R)
    per_voxel('q', res[key + 'q'], refq, tolq, R['myy'])
    # a race in a packed instruction is not deterministic: the second run has the same bits
    assert np.array_equal(res[key + 'q'], res[key + 'q2']) and res[key + 'dot'] == res[key + 'dot2'], (name, k, 'two runs')
    # the float64 dot epilogue: <p, q> within sum |p| tol_q (+ the actual error in tied voxels)
    q = torch.from_numpy(res[key + 'q'])
    slack = float((p64.abs() * (q.double() - refq).abs())[R['myy']].sum())
    assert abs(float(res[key + 'dot']) - float((p64 * refq).sum())) <= float((p64.abs() * tolq).sum()) + slack, (name, k, 'dot')
    # the operator moved: the reference of the stage before is beyond this stage's bound somewhere
    if prev is not None:
        assert not ref64.compare(q, matvec64(prev)[0], tolq, R['myy'] | prev['myy'])['ok'], (name, k, 'q is the old operator\'s')
    # the float64 adjoint identity on the kernels' A and At
    Ap, Atv = torch.from_numpy(res[key + 'A']).double(), torch.from_numpy(res[key + 'At']).double()
    lhs = abs(float((Ap * v64).sum()) - float((p64 * Atv).sum()))
    slack = float(((Ap - refA).abs() * v64.abs())[r['mx']].sum() + ((Atv - refAt).abs() * p64.abs())[r['my']].sum())
    assert lhs <= float((tolA * v64.abs()).sum() + (tolAt * p64.abs()).sum()) + slack, (name, k, 'adjoint')
    refb, tolb = ref64.bound_rhs(R['ops'], R['taus'], [rr['dat'] for rr in R['reps']], R['prob']['w'][0], R['prob']['z'][0],
                                 R['rho'], R['lam'], R['vx'])
    per_voxel('b', res[key + 'b'], refb, tolb, R['my'])
    # impulse combs against the plan's own taps (D = 0): columns of A^T A
    opt = ref64.Operator64(r['po'], R['prob']['method'], trimmed=True, oriented=r['oriented'])
    sy = comb_spacing(op.ratio)
    for ph in (0, 1):
        refc, tolc = opt.bound_AtA(comb(R['prob']['dim_y'], TILE, sy, ph))
        per_voxel('AtA_comb%d' % ph, res[key + 'AtA_comb%d' % ph], refc, tolc, r['myy'])
    if key + 'M' in res:
        refM, tolM = jacobi64(R)
        per_voxel('Jacobi', res[key + 'M'], refM, tolM, R['myy'])
    return rep


@pytest.mark.parametrize('name', list(CHAINS))
def test_every_stage_per_voxel(tmp_path, name):
    res, logs, n_stages = _chain_child(tmp_path, name, 'prod')
    drift, prev = [], None
    for k in range(n_stages):
        R = stage_reference(name, k)
        rep = check_stage(name, k, res, R, prev)
        # one full rebuild per set_repeat call, and never the scaling-only branch
        assert len(re.findall(r'^\[set_repeat\] full rebuild', logs[k], re.M)) == (1 if k else 0), (name, k, logs[k][-2000:])
        assert 'scaling only' not in logs[k], (name, k)
        form = _form(_infos(res, k)[R['moved']], logs[k])
        want = FORMS[(name, k)]
        note = ''
        if form != want:
            if k > 0 and _declined(want, form):
                note = ' (declined after the quick build)'
            else:
                drift.append((name, k, form, want))
        print('set_repeat %-8s stage %d %s%s ties %s worst %s' % (name, k, form, note, tie_counts(R),
              ', '.join('%s %.3f' % kv for kv in rep.items())), flush=True)
        prev = R
    assert not drift, drift


# ---- (2) a rebuilt plan has no memory ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CHAINS))
def test_a_rebuilt_plan_is_a_fresh_plan_bit_for_bit(tmp_path, name):
    """With the wholesale rule on both sides (UNIRES_S2_EXACT=0, UNIRES_F1_EXACT=0: creation packs as the rebuild does)
    nothing the kernels read depends on what the buffers held before: at every stage the chained plan and a fresh
    ChannelPlan of the stage's operators agree bit for bit."""
    res, logs, n_stages = _chain_child(tmp_path, name, 'fresh', env=QUICK_ENV)
    bad = []
    for k in range(n_stages):
        same = json.loads(str(res['s%d/same' % k]))
        print('set_repeat %-8s stage %d against a fresh plan: %s' % (name, k, same), flush=True)
        if not all(same.values()):
            bad.append((k, [w for w, ok in same.items() if not ok], int(res['s%d/q_diff' % k]),
                        str(res['s%d/info' % k]), str(res['s%d/fresh_info' % k])))
    assert not bad, (name, bad)


# ---- (4) mask and slice weights across a rebuild ------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(MW_CHAINS))
def test_mask_and_weights_follow_a_rebuild(tmp_path, name):
    """Repeat 0's observation zeroed over a slab, 'ramp' weights along its slice axis, the plan fetched through
    ``_channel_plan(mask_zeros=True, weights=True)`` and then moved with set_repeat: the mask and the weights are in the
    caller's layout, which does not change; the canonical mask must follow a flip and a permutation, the weights'
    direction reverse with the flip (the orient chain).  Then a set_repeat with another dim_x: refused, plan untouched."""
    from tests import ref64
    res, logs, n_stages = _chain_child(tmp_path, name, 'mw', n_stages=MW_CHAINS[name], env=QUICK_ENV)
    for k in range(n_stages):
        R = stage_reference(name, k)
        assert tie_cap_ok(R), (name, k, tie_counts(R))
        info = _infos(res, k)[0]
        assert (info['perm'], info['flip']) == R['reps'][0]['orient'], (name, k, info)
        assert info['masked'] and info['weighted'] and not info['shift'] and not info['fused'], (name, k, info)
        q = torch.from_numpy(res['s%d/q' % k])
        refq, tolq = mw_matvec64(R)
        c = ref64.compare(q, refq, tolq, R['myy'])
        assert c['ok'], (name, k, 'matvec', c)
        assert not ref64.compare(q, matvec64(R)[0], tolq, R['myy'])['ok'], (name, k, 'the matvec is the plain one')
        refM, tolM = jacobi64(R, mw_weights(R))
        cm = ref64.compare(torch.from_numpy(res['s%d/M' % k]), refM, tolM, R['myy'])
        assert cm['ok'], (name, k, 'Jacobi diagonal', cm)
        print('set_repeat %-8s stage %d masked + weighted %s: q %.3f Jacobi %.3f' % (name, k, info, c['max_ratio'],
              cm['max_ratio']), flush=True)
    assert 'clear the mask first' in str(res['refusal']), res['refusal']
    assert np.array_equal(res['q_after_refusal'], res['s%d/q' % (n_stages - 1)])


# ---- (3) what must go and what must stay --------------------------------------------------------------------------------
_SMALL_KW = dict(dim_y=(10, 9, 8), thick=2, n_repeats=2, rot=0.08, trans=0.7, scl=0.05)  # tests/test_gpu_mask.py's _small


@functools.lru_cache(maxsize=None)
def small_problems(n_repeats=2):
    """tests/test_gpu_mask.py's 10 x 9 x 8 problem (no mask) and the same with repeat 0 at seed 42's rigid;
    ``n_repeats=1``: its first repeat alone (the preconditioners are built for one repeat per channel)."""
    from tests.helpers import make_problem
    kw = dict(_SMALL_KW, n_repeats=n_repeats)
    p0 = make_problem(seed=41, **kw)
    rigid = make_problem(seed=42, **kw)['chans'][0]['reps'][0]['rigid']
    c0 = p0['chans'][0]
    p1 = dict(p0, chans=[dict(c0, reps=[dict(c0['reps'][0], rigid=rigid)] + c0['reps'][1:])])
    return p0, p1


def small_rhs(dim):
    g = torch.Generator().manual_seed(9)
    return (torch.rand(dim, generator=g) * 0.1).float()


_STATE_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import gpu_structs
from tests.test_gpu_set_repeat import small_problems, small_rhs
from oracle import nitorch_restated as N
from unires_amd._plan import ChannelPlan
n_it, out = %(n_it)r, sys.argv[1]
dev = 'cuda:0'
p0, p1 = small_problems()
x0, y = gpu_structs(p0, dev)[0][0], gpu_structs(p0, dev)[1][0]
x1 = gpu_structs(p1, dev)[0][0]
dim = p0['dim_y']
vxl = [float(v) for v in N.voxel_size(p0['mat_y']).float()]
rho, lam = float(p0['rho']), float(y.lam)
b, start = small_rhs(dim).to(dev), p0['y0'][0].to(dev)
reps0, reps1 = [(xn.po, xn.tau) for xn in x0], [(xn.po, xn.tau) for xn in x1]
new = lambda reps: ChannelPlan(dim, vxl, reps, p0['method'], p0['do_proj'], device=dev)
ok, res = {}, {}


def solve(pl, tol=0.0, iters=6, precond='none'):
    x = start.clone()
    pl.cg(b, x, rho, lam, max_iter=iters, tolerance=tol, precond=precond)
    torch.cuda.synchronize()
    return x


for tol in (0.0, 1e-3):
    tag = 'tol%%g/' %% tol
    plan, fresh = new(reps0), new(reps1)
    first = solve(plan, tol)
    ok[tag + 'replay'] = torch.equal(solve(plan, tol), first)
    plan.set_repeat(0, *reps1[0])
    third = solve(plan, tol)
    ok[tag + 'fresh bits'] = torch.equal(third, solve(fresh, tol))
    ok[tag + 'not the first'] = not torch.equal(third, first)
    ok[tag + 'replays again'] = torch.equal(solve(plan, tol), third)
    plan.close(), fresh.close()
# CG converges to the new system
plan = new(reps0)
x = torch.zeros(dim, device=dev)
plan.cg(b, x, rho, lam, max_iter=n_it, tolerance=0.0)
res['x_old'] = x.cpu().numpy()
plan.set_repeat(0, *reps1[0])
x = torch.zeros(dim, device=dev)
plan.cg(b, x, rho, lam, max_iter=n_it, tolerance=0.0)
torch.cuda.synchronize()
res['x_new'] = x.cpu().numpy()
plan.close()
# the preconditioner goes with the operator (one repeat: the preconditioners are built for one repeat per channel)
q0, q1 = small_problems(1)
reps0 = [(xn.po, xn.tau) for xn in gpu_structs(q0, dev)[0][0]]
reps1 = [(xn.po, xn.tau) for xn in gpu_structs(q1, dev)[0][0]]
rho, lam = float(q0['rho']), float(gpu_structs(q0, dev)[1][0].lam)
fresh = new(reps1)
for mode in ('jacobi', 'fft'):
    plan = new(reps0)
    plan.precond_build(rho, lam, mode=mode)
    solve(plan, 1e-3, precond=mode)
    plan.set_repeat(0, *reps1[0])
    try:
        solve(plan, 1e-3, precond=mode)
        res[mode + '/error'] = np.array('none')
    except ValueError as e:
        res[mode + '/error'] = np.array(str(e))
    plan.precond_build(rho, lam, mode=mode)
    fresh.precond_build(rho, lam, mode=mode)
    ok[mode + '/apply bits'] = torch.equal(plan.precond_apply(b), fresh.precond_apply(b))
    ok[mode + '/solve bits'] = torch.equal(solve(plan, 1e-3, precond=mode), solve(fresh, 1e-3, precond=mode))
    plan.close()
fresh.close()
res['ok'] = np.array(json.dumps(ok))
np.savez(out, **res)
'''


@pytest.mark.parametrize('graph', ['1', '0'])
def test_set_repeat_drops_the_captured_solve_and_the_preconditioner(tmp_path, graph):
    """tests/test_gpu_mask.py's 10 x 9 x 8 problem, repeat 0 moved to a second rigid.  Two solves (the second replays the
    captured graph), set_repeat, a third: the bits of a fresh plan of the second operator, not the first solve's, and
    replayed to the same bits - with tolerance 0 and 1e-3 (the chunked enqueue), with and without UNIRES_CG_GRAPH=0.  CG
    reaches the dense float64 solution of the second operator's normal equations within GATE while the first operator's
    is more than 10 GATE away.  cg(precond=) raises until the preconditioner is rebuilt, then has a fresh plan's bits."""
    from oracle import nitorch_restated as N
    from tests import diff64, ref64
    from tests.helpers import oracle_structs, rel_err
    from tests.test_gpu_mask import _dense
    p0, p1 = small_problems()
    dim = p0['dim_y']
    xs, ys = oracle_structs(p1)
    vx = [float(v) for v in N.voxel_size(p1['mat_y']).float()]
    rho, lam = ref64._f32(p1['rho']), ref64._f32(ys[0].lam)
    S = rho * lam * lam * diff64.dense_dtd(dim, vx, 'forward')
    for xn in xs[0]:
        A = _dense(ref64.Operator64(xn.po, p1['method']))
        S = S + ref64._f32(xn.tau) * (A.T @ A)
    want = torch.from_numpy(np.linalg.solve(S, small_rhs(dim).double().numpy().ravel()).reshape(dim))
    # enough iterations to converge, and no more (tests/test_gpu_mask.py: 2 r^n <= 1e-6 in the A-norm)
    sk = float(np.sqrt(np.linalg.cond(S)))
    n_it = int(np.ceil(np.log(0.5e-6) / np.log((sk - 1.0) / (sk + 1.0))))
    res, _ = _run(tmp_path, 'state_graph' + graph, _STATE_CHILD % dict(root=ROOT, n_it=n_it),
                  dict(QUICK_ENV, UNIRES_CG_GRAPH=graph))
    ok = json.loads(str(res['ok']))
    err, old = rel_err(torch.from_numpy(res['x_new']), want), rel_err(torch.from_numpy(res['x_old']), want)
    print('set_repeat state (graphs %s): %s; CG %d iterations, rel_err %.3g, the old operator\'s solution %.3g away'
          % (graph, ok, n_it, err, old), flush=True)
    assert all(ok.values()), ok
    assert err < GATE and old > 10 * GATE, (err, old)
    for mode in ('jacobi', 'fft'):
        assert 'unires_precond_build' in str(res[mode + '/error']), (mode, res[mode + '/error'])


_KEEP_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import gpu_structs
from tests.test_gpu_voxelwise import inputs
from tests.test_gpu_set_repeat import stage_problems
from oracle import nitorch_restated as N
from unires_amd._plan import ChannelPlan
out, dev = sys.argv[1], 'cuda:0'
probs = stage_problems('z')[:3]
prob = probs[0]
x, y = gpu_structs(prob, dev)[0][0], gpu_structs(prob, dev)[1][0]
vxl = [float(v) for v in N.voxel_size(prob['mat_y']).float()]
new = lambda: ChannelPlan(prob['dim_y'], vxl, [(xn.po, xn.tau) for xn in x], prob['method'], prob['do_proj'], device=dev)
plain, conc, central = new(), new(), new()
conc.set_concurrency(3)      # before the transitions, and not again
central.set_diff('central')
p = inputs(prob['dim_y'], prob['dim_y'])[0].to(dev)
res = {}
for k in (1, 2):
    xk = gpu_structs(probs[k], dev)[0][0][0]
    for pl in (plain, conc, central):
        pl.set_repeat(0, xk.po, xk.tau)
    res['s%%d/plain' %% k] = plain.matvec(p, prob['rho'], y.lam).cpu().numpy()
    res['s%%d/conc3' %% k] = conc.matvec(p, prob['rho'], y.lam).cpu().numpy()
    res['s%%d/central' %% k] = central.matvec(p, prob['rho'], y.lam).cpu().numpy()
np.savez(out, **res)
'''


def test_set_repeat_keeps_diff_and_concurrency(tmp_path):
    """set_diff('central') and set_concurrency(3) before the z chain's first two transitions, not repeated after them: q
    passes ref64.bound_matvec_reps(which='central') per voxel (and is not the forward one), and with concurrency 3 has
    the bits of concurrency 1 (what tests/test_gpu_sizes.py asserts of fresh plans)."""
    from tests import ref64
    res, _ = _run(tmp_path, 'keep', _KEEP_CHILD % dict(root=ROOT))
    for k in (1, 2):
        R = stage_reference('z', k)
        refq, tolq = matvec64(R, 'central')
        q = torch.from_numpy(res['s%d/central' % k])
        c = ref64.compare(q, refq, tolq, R['myy'])
        print('set_repeat z stage %d central q err/tol %.3f' % (k, c['max_ratio']), flush=True)
        assert c['ok'], (k, c)
        assert not ref64.compare(q, matvec64(R)[0], tolq, R['myy'])['ok'], (k, 'the difference went back to forward')
        assert np.array_equal(res['s%d/conc3' % k], res['s%d/plain' % k]), (k, 'concurrency 3')


# ---- (5) the facade -----------------------------------------------------------------------------------------------------
def _gpu_po(prob, n, dev, dim_x=None):
    import unires_amd as U
    r = prob['chans'][0]['reps'][n]
    return U._proj_info(prob['dim_y'], prob['mat_y'], r['dim_x'] if dim_x is None else dim_x, r['mat_x'], rigid=r['rigid'],
                        prof_ip=r['prof_ip'], prof_tp=r['prof_tp'], scl=r['scl'], device=dev)


def test_the_facade_moves_the_cached_plan_and_drops_its_cached_atx(dev):
    """The way production goes: ``xn.po = _proj_info(..., rigid=new)`` and ``_channel_plan`` again (the z chain's stage
    0 -> 3).  The same ChannelPlan comes back, and ``rhs_cached`` after the change passes ref64.bound_rhs per voxel for
    the new operator and fails it for the old one: the cached sum tau At x was dropped."""
    from tests import ref64
    from tests.helpers import gpu_structs
    from unires_amd._project import _channel_plan
    assert not _DEAD, ('an earlier child died: nothing more runs on the GPU', _DEAD)
    probs = stage_problems('z')
    prob = probs[0]
    xg, yg, _ = gpu_structs(prob, dev)
    x, y = xg[0], yg[0]
    d = lambda t: t.to(dev)
    w_c, z_c = d(prob['w'][0]), d(prob['z'][0])
    rhs = lambda pl: pl.rhs_cached([xn.dat for xn in x], w_c, z_c, prob['rho'], y.lam, torch.empty(prob['dim_y'], device=dev)).cpu()
    bounds = []
    for k in (0, 3):
        R = stage_reference('z', k)
        bounds.append(ref64.bound_rhs(R['ops'], R['taus'], [r['dat'] for r in R['reps']], prob['w'][0], prob['z'][0], R['rho'],
                                      R['lam'], R['vx']) + (R['my'],))
    plan = _channel_plan(x, y, prob['method'], prob['do_proj'])
    b0 = rhs(plan)
    assert ref64.compare(b0, *bounds[0])['ok']
    assert torch.equal(rhs(plan), b0)  # (from the cache)
    x[0].po = _gpu_po(probs[3], 0, dev)
    again = _channel_plan(x, y, prob['method'], prob['do_proj'])
    assert again is plan
    b3 = rhs(plan)
    c = ref64.compare(b3, *bounds[1])
    print('facade: rhs_cached after the rigid changed err/tol %.3f' % c['max_ratio'], flush=True)
    assert c['ok'], c
    assert not ref64.compare(b3, bounds[0][0], bounds[1][1], bounds[0][2] | bounds[1][2])['ok']
    plan.close()


def test_the_facade_builds_a_new_plan_when_the_repeat_does_not_fit(dev):
    """A cached plan of the z chain's observation cropped by one slice, masked and weighted; then the whole observation
    (a larger dim_x: set_repeat refuses it) through ``_channel_plan``: a new plan object, masks and weights
    re-synchronised - q passes (4)'s reference of stage 0 per voxel."""
    import unires_amd as U
    from tests import ref64, slice64
    from tests.helpers import gpu_structs
    from unires_amd._project import _channel_plan, _slice_axis
    assert not _DEAD, ('an earlier child died: nothing more runs on the GPU', _DEAD)
    prob = stage_problems('z')[0]
    xg, yg, _ = gpu_structs(prob, dev)
    full, y = xg[0][0], yg[0]
    r = prob['chans'][0]['reps'][0]
    a = _slice_axis(full)
    assert a == 2
    S = int(full.dat.shape[a])
    full.dat = zeroed(full.dat, 'slab')
    full.slice_w = slice64.weights(S, 'ramp').to(dev)
    small = U._input(full.dat[:, :, :S - 1].contiguous(), r['mat_x'], r['tau'],
                     _gpu_po(prob, 0, dev, dim_x=tuple(full.dat.shape[:2]) + (S - 1,)))
    small.slice_w = slice64.weights(S - 1, 'ramp').to(dev)
    get = lambda x: _channel_plan([x], y, prob['method'], prob['do_proj'], mask_zeros=True, weights=True)
    first = get(small)
    assert first.repeat_info(0)['masked'] and first.repeat_info(0)['weighted']
    plan = get(full)
    assert plan is not first
    info = plan.repeat_info(0)
    assert info['masked'] and info['weighted'] and not info['shift'] and not info['fused'], info
    R = stage_reference('z', 0)
    q = plan.matvec(R['p'].to(dev), prob['rho'], y.lam).cpu()
    refq, tolq = mw_matvec64(R)
    c = ref64.compare(q, refq, tolq, R['myy'])
    print('facade: a new plan for a larger dim_x, masked + weighted q err/tol %.3f' % c['max_ratio'], flush=True)
    assert c['ok'], c
    assert not ref64.compare(q, matvec64(R)[0], tolq, R['myy'])['ok']
    plan.close()
