"""The bias field on the GPU (sett.bias, _input.bias_coef): repeat n is modelled as b_n . e_n . (A_n y),
b = exp(beta) a separable cosine series on the observation's grid, and the y-update's system becomes

    ( sum_n tau_n A_n^T diag(W_n b_n^2) A_n + rho lam^2 D^T D ) y = sum_n tau_n A_n^T (W_n b_n x_n) - lam D^T (w - rho z)

which the plan solves unchanged, handed g b^2 for its voxel map and x / b for its observation.

(1) unires_bias_field against tests/bias64.py; (2) unires_bias_terms against it; (3) one _update_bias step against the
restated rule; (4) a plan fetched with a field has the bits of the plan handed the two volumes by hand, and a captured
solve reads a recomposed map; (5) fit() on planted shading; (6) fixed coefficients come back unchanged; (7) the field
with both robust rules, mask_zeros and channel streams, twice.

Shapes of (1) and (2), chosen where the walks can break: a single voxel; z across a wave seam (66); two seams and a
ragged tail (130); the complete basis on 8 x 8 x 8 (projection orders up to 15); order 1 along an axis with few z.
k_bias_proj has no LDS fallback - a workgroup's table is 4 x 24 x 65 doubles whatever the shape, and z is ALWAYS walked
in groups of 64, so the smallest n_z with a second group is 65 (covered by 66 and 130); what k_bias_field chunks is the
rows of a plane, by 256: the smallest n_y with a second chunk is 257, the last case.

The raw launcher calls run in a child process (tests/test_gpu_mask.py's ``_run``: under a time limit, nothing more on
the GPU after one that exited non-zero or timed out).  Every test fails on the commit before the feature: the library
has neither symbol and the package neither ``_update_bias`` nor ``_init_bias``.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bias64
from tests.test_gpu_mask import _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (shape, orders)
CASES = [((1, 1, 1), (1, 1, 1)), ((3, 7, 66), (2, 3, 4)), ((17, 5, 130), (3, 2, 8)), ((8, 8, 8), (8, 8, 8)),
         ((6, 70, 3), (1, 3, 2)), ((2, 257, 3), (2, 4, 2))]
ARMS = (('none', 2), ('gu', 0), ('gu', 1), ('gu', 2), ('g', 1), ('u', 2))
BIAS_MAX = 4.0


def case_inputs(shape, orders):
    """float32 CPU volumes x (a tenth of it zeros), mu, b in [0.8, 1.25], g in [0, 1]; u per axis; float64 coefficients
    inside the clamp (``coef``) and far beyond it (``wild``)."""
    rng = np.random.default_rng(100 + sum(shape) + sum(orders))
    mu = (50.0 + 30.0 * rng.random(shape)).astype(np.float32)
    x = (mu * (1.0 + 0.2 * rng.standard_normal(shape))).astype(np.float32)
    if x.size > 1:
        x[rng.random(shape) < 0.1] = 0
    b = np.exp(rng.uniform(-0.22, 0.22, shape)).astype(np.float32)
    g = rng.random(shape).astype(np.float32)
    u = [rng.random(n).astype(np.float32) for n in shape]
    coef = 0.3 * rng.standard_normal(orders) / np.sqrt(np.prod(orders))
    wild = np.zeros(orders)  # (the highest term alone, times 40: it changes sign over the grid wherever an order is > 1)
    wild[tuple(k - 1 for k in orders)] = 40.0
    return dict(x=x, mu=mu, b=b, g=g, u=u, coef=coef, wild=wild)


_KERNEL_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_bias import ARMS, BIAS_MAX, CASES, case_inputs
from unires_amd import _lib
from unires_amd._lib import i3
from unires_amd._update import bias_tables
lib, out, res = _lib.load(), sys.argv[1], {}
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
P = lambda t: None if t is None else t.data_ptr()
for shape, orders in CASES:
    key = 'x'.join(map(str, shape))
    inp = case_inputs(shape, orders)
    x, mu, b, g = d(inp['x']), d(inp['mu']), d(inp['b']), d(inp['g'])
    tabs = [d(t) for t in bias_tables(shape, orders)]
    # (1) the field: with g and x, without g, and beyond the clamp
    for tag, coef, gg in (('f', inp['coef'], g), ('f1', inp['coef'], None), ('fw', inp['wild'], g)):
        c = d(coef)
        bo, gb2, xb = (torch.full(shape, float('nan'), device='cuda:0') for _ in range(3))
        rc = lib.unires_bias_field(P(c), P(tabs[0]), P(tabs[1]), P(tabs[2]), i3(orders), i3(shape), float(np.log(BIAS_MAX)),
                                   P(gg), P(x), P(bo), P(gb2), P(xb), None)
        assert rc == 0, (key, tag, rc, lib.unires_last_error())
        torch.cuda.synchronize()
        res['%%s/%%s/b' %% (key, tag)], res['%%s/%%s/gb2' %% (key, tag)], res['%%s/%%s/xb' %% (key, tag)] = \
            bo.cpu().numpy(), gb2.cpu().numpy(), xb.cpu().numpy()
    # (2) the terms
    K, Q = int(np.prod(orders)), int(np.prod([2 * k - 1 for k in orders]))
    for arm, axis in ARMS:
        gg = g if 'g' in arm else None
        uu = d(inp['u'][axis]) if 'u' in arm else None
        for run in (0, 1):
            o = torch.full((1 + K + Q,), float('nan'), dtype=torch.float64, device='cuda:0')
            rc = lib.unires_bias_terms(P(x), P(mu), P(b), P(gg), P(uu), axis, P(tabs[0]), P(tabs[1]), P(tabs[2]),
                                       i3(orders), i3(shape), P(o), None)
            assert rc == 0, (key, arm, rc, lib.unires_last_error())
            torch.cuda.synchronize()
            res['%%s/%%s%%d/run%%d' %% (key, arm, axis, run)] = o.cpu().numpy()
        o1 = torch.full((1,), float('nan'), dtype=torch.float64, device='cuda:0')
        rc = lib.unires_bias_terms(P(x), P(mu), P(b), P(gg), P(uu), axis, None, None, None, i3((0, 0, 0)), i3(shape),
                                   P(o1), None)
        assert rc == 0, (key, arm, 'objective alone', rc)
        torch.cuda.synchronize()
        res['%%s/%%s%%d/obj' %% (key, arm, axis)] = o1.cpu().numpy()
# status codes: nothing is launched on a bad argument
shape, orders = CASES[1]
inp = case_inputs(shape, orders)
x, mu, b = d(inp['x']), d(inp['mu']), d(inp['b'])
tabs = [d(t) for t in bias_tables(shape, orders)]
c, o = d(inp['coef']), torch.zeros(4096, dtype=torch.float64, device='cuda:0')
bo = torch.zeros(shape, device='cuda:0')
T = [P(t) for t in tabs]
codes = [
    lib.unires_bias_field(None, T[0], T[1], T[2], i3(orders), i3(shape), 1.0, None, None, P(bo), None, None, None),
    lib.unires_bias_field(P(c), T[0], T[1], T[2], i3((9, 1, 1)), i3(shape), 1.0, None, None, P(bo), None, None, None),
    lib.unires_bias_field(P(c), T[0], T[1], T[2], i3((0, 1, 1)), i3(shape), 1.0, None, None, P(bo), None, None, None),
    lib.unires_bias_field(P(c), T[0], T[1], T[2], i3(orders), i3((3, 0, 66)), 1.0, None, None, P(bo), None, None, None),
    lib.unires_bias_field(P(c), T[0], T[1], T[2], i3(orders), i3(shape), 0.0, None, None, P(bo), None, None, None),
    lib.unires_bias_field(P(c), T[0], T[1], T[2], i3(orders), i3(shape), 1.0, None, None, P(bo), None, P(bo), None),
    lib.unires_bias_field(P(c), T[0], T[1], T[2], i3(orders), i3(shape), 1.0, None, P(x), P(x), None, None, None),
    lib.unires_bias_terms(None, P(mu), P(b), None, None, 2, T[0], T[1], T[2], i3(orders), i3(shape), P(o), None),
    lib.unires_bias_terms(P(x), P(mu), P(b), None, None, 3, T[0], T[1], T[2], i3(orders), i3(shape), P(o), None),
    lib.unires_bias_terms(P(x), P(mu), P(b), None, None, 2, T[0], T[1], T[2], i3((2, 0, 1)), i3(shape), P(o), None),
    lib.unires_bias_terms(P(x), P(mu), P(b), None, None, 2, T[0], T[1], T[2], i3((2, 9, 1)), i3(shape), P(o), None),
    lib.unires_bias_terms(P(x), P(mu), P(b), None, None, 2, None, T[1], T[2], i3(orders), i3(shape), P(o), None),
    lib.unires_bias_terms(P(x), P(mu), P(b), None, None, 2, T[0], T[1], T[2], i3(orders), i3(shape), None, None)]
torch.cuda.synchronize()
res['codes'] = np.array(codes)
np.savez(out, **res)
'''

_RES = {}


def _kernels(tmp_path):
    if 'k' not in _RES:
        _RES['k'] = _run(tmp_path, 'bias_kernels', _KERNEL_CHILD % dict(root=ROOT), timeout=300)
    return _RES['k']


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- (1) unires_bias_field ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,orders', CASES)
def test_bias_field_against_float64(tmp_path, shape, orders):
    """b within 1 float32 ulp of bias64.field64's (the device's exp may differ in the last bit of a double, and so may
    the order of the folds); GIVEN that b, g b^2 and x / b bit for bit bias64.compose32's, with g and without; zeros of
    x stay zeros; every voxel written (the outputs start as NaN); with coefficients far beyond the clamp b stays in
    [1 / 4, 4] and reaches both ends."""
    res = _kernels(tmp_path)
    key = 'x'.join(map(str, shape))
    inp = case_inputs(shape, orders)
    want = bias64.field64(inp['coef'], shape, BIAS_MAX)
    for tag, g in (('f', inp['g']), ('f1', None)):
        b, gb2, xb = (res['%s/%s/%s' % (key, tag, n)] for n in ('b', 'gb2', 'xb'))
        assert b.dtype == np.float32 and np.isfinite(b).all() and np.isfinite(gb2).all() and np.isfinite(xb).all(), key
        worst = int(_ulps(b, want).max())
        print('bias field %-10s %s: b at most %d ulp from float64' % (key, tag, worst), flush=True)
        assert worst <= 1, (key, tag, worst)
        wg, wx = bias64.compose32(g, b, inp['x'])
        assert np.array_equal(gb2.view(np.int32), wg.view(np.int32)), (key, tag, 'g b^2')
        assert np.array_equal(xb.view(np.int32), wx.view(np.int32)), (key, tag, 'x / b')
        assert (xb[inp['x'] == 0] == 0).all() and (xb[inp['x'] != 0] != 0).all(), (key, tag, 'zeros')
    assert np.array_equal(res[key + '/f/b'], res[key + '/f1/b'])
    bw = res[key + '/fw/b']
    wantw = bias64.field64(inp['wild'], shape, BIAS_MAX)
    assert bw.min() >= np.float32(0.25) and bw.max() <= np.float32(4.0), (key, 'clamp', bw.min(), bw.max())
    assert int(_ulps(bw, wantw).max()) <= 1
    assert (bw == np.float32(4.0)).any(), (key, 'the upper clamp is reached')
    if max(orders) > 1:
        assert (bw == np.float32(0.25)).any(), (key, 'the lower clamp is reached')


def test_status_codes(tmp_path):
    """A null argument, orders outside 1 .. 8, a bad dim, a bound <= 0, aliased outputs, a bad axis: non-zero status."""
    codes = _kernels(tmp_path)['codes']
    assert (codes != 0).all(), codes


# ---- (2) unires_bias_terms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,orders', CASES)
def test_bias_terms_against_float64(tmp_path, shape, orders):
    """Every entry - sum W r^2, the projection of W m r onto the orders < k, the projection of W m^2 onto the orders
    < 2 k - 1 - within bias64.terms64's bound 2 (N + 3) 2^-53 sum |term| of the restatement on the same float32 inputs:
    without weights, with g and u along each slice axis, with either alone, always with zeros in x.  Two runs agree bit
    for bit, every entry is written, and the objective-only form gives the full form's objective bit for bit."""
    res = _kernels(tmp_path)
    key = 'x'.join(map(str, shape))
    inp = case_inputs(shape, orders)
    for arm, axis in ARMS:
        g = inp['g'] if 'g' in arm else None
        u = inp['u'][axis] if 'u' in arm else None
        want, bound = bias64.terms64(inp['x'], inp['mu'], inp['b'], g, u, axis, orders)
        got = res['%s/%s%d/run0' % (key, arm, axis)]
        assert got.shape == want.shape and np.isfinite(got).all(), (key, arm, axis)
        assert np.array_equal(got, res['%s/%s%d/run1' % (key, arm, axis)]), (key, arm, axis, 'two runs differ')
        assert np.array_equal(got[:1], res['%s/%s%d/obj' % (key, arm, axis)]), (key, arm, axis, 'objective alone')
        err = np.abs(got - want)
        worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print('bias terms %-10s %s/%d: worst err / bound %.3g' % (key, arm, axis, worst), flush=True)
        assert (err <= bound).all(), (key, arm, axis, int(np.argmax(err - bound)), float(err.max()))
    if np.prod(shape) > 1:  # (the weights did something)
        assert res['%s/none2/run0' % key][0] != res['%s/gu2/run0' % key][0]


# ---- (3) one step of the rule on the device ----------------------------------------------------------------------------
def _step_structs(dev):
    import unires_amd as U
    from unires_amd.run import _init_bias
    shape = (12, 10, 9)
    rng = np.random.default_rng(21)
    mu = (80.0 + 40.0 * rng.random(shape)).astype(np.float32)
    planted = np.zeros((3, 3, 3))
    planted[0, 0, 0], planted[1, 0, 0], planted[0, 2, 1], planted[2, 1, 0] = 0.05, 0.15, -0.1, 0.08
    x = (mu * np.exp(bias64.beta64(planted, shape)) + 3.0 * rng.standard_normal(shape)).astype(np.float32)
    x[rng.random(shape) < 0.05] = 0
    g, u = rng.random(shape).astype(np.float32), rng.random(shape[2]).astype(np.float32)
    xn = U._input(torch.from_numpy(x).to(dev), torch.eye(4, dtype=torch.float64), 1.0 / 9.0)
    xn.po = SimpleNamespace(dim_thick=2)
    xn.weight, xn.slice_w = torch.from_numpy(g).to(dev), torch.from_numpy(u).to(dev)
    sett = U.settings()
    sett.bias, sett.bias_cutoff = True, 8.0  # (orders ceil(24 / 8), ceil(20 / 8), ceil(18 / 8) = 3, 3, 3)
    _init_bias([[xn]], sett, dev)
    return xn, sett, dict(x=x, mu=mu, g=g, u=u, shape=shape)


def test_update_bias_step_against_the_float64_rule(dev):
    """One _update_bias step from c = 0 at fixed mu on 12 x 10 x 9 with g, u and zeros in x, against bias64's step on
    the same float32 inputs (its sums in long double, its line search on bias64.field64).  The same step length is
    accepted, E falls, and the coefficients agree within 8 cond(H) eps ||c||: to first order a solve carries the
    relative perturbation of its matrix and right-hand side times cond(H), eps = ||dG|| / ||gradient|| + ||dH|| / ||H||
    with dG, dH the bounds bias64.terms64 puts on the device's sums (dH assembled like H: 1/8 of eight bounds), cond
    taken from the restatement; the factor 8 is the issue's."""
    from unires_amd._update import _update_bias
    xn, sett, inp = _step_structs(dev)
    shape, tau = inp['shape'], float(xn.tau)
    assert tuple(xn._bias_coef.shape) == (3, 3, 3) and xn._bias_est and float(xn._bias_coef.abs().max()) == 0.0
    lam = xn._bias_lam
    kappa = tau * float((inp['x'].astype(np.float64) ** 2).sum())
    assert abs(xn._bias_kappa - kappa) <= 1e-12 * kappa
    assert np.allclose(lam, bias64.lambda64(shape, (1.0, 1.0, 1.0), (3, 3, 3), kappa, 0.01, 8.0), rtol=1e-12, atol=0)
    assert torch.equal(xn._bias_b.cpu(), torch.ones(shape)) and torch.equal(xn._bias_dat, xn.dat)
    assert torch.equal(xn._bias_weight, xn.weight)  # (c = 0: b = 1, g b^2 = g, x / b = x)
    mu_dev = torch.from_numpy(inp['mu']).to(dev)
    _update_bias([[xn]], [None], sett, raw={(0, 0): mu_dev})
    torch.cuda.synchronize()
    got = xn._bias_coef.numpy()
    E0, E1, s = xn._bias_E
    ones = np.ones(shape, dtype=np.float32)
    want, bound = bias64.terms64(inp['x'], inp['mu'], ones, inp['g'], inp['u'], 2, (3, 3, 3))
    K = 27
    c0 = np.zeros((3, 3, 3))
    delta, grad, H = bias64.step64(c0, want[1:1 + K], want[1 + K:].reshape(5, 5, 5), lam, tau)

    def energy(cand):
        fo = bias64.summands64(inp['x'], inp['mu'], bias64.field64(cand, shape), inp['g'], inp['u'], 2)[0]
        return bias64.energy64(fo.sum(), cand, lam, tau)

    ref, E1r, sr = bias64.line_search64(c0, delta, bias64.energy64(want[0], c0, lam, tau), energy)
    assert s == sr and s > 0, (s, sr)
    assert E1 < E0 and abs(E0 - bias64.energy64(want[0], c0, lam, tau)) <= 1e-12 * E0
    assert abs(E1 - E1r) <= 1e-6 * E1r  # (b may differ by an ulp of float32 at some voxels)
    dG = tau * np.linalg.norm(bound[1:1 + K])
    dH = tau * np.linalg.norm(bias64.hessian_from_projection64(bound[1 + K:].reshape(5, 5, 5), (3, 3, 3)))
    eps = dG / np.linalg.norm(grad) + dH / np.linalg.norm(H)
    cond = np.linalg.cond(H)
    err, tol = np.linalg.norm(got - ref), 8.0 * cond * eps * np.linalg.norm(ref)
    print('bias step: s = %g, E %.6g -> %.6g, cond(H) %.3g, |c - c64| %.3g (tolerance %.3g), |c| %.3g'
          % (s, E0, E1, cond, err, tol, np.linalg.norm(ref)), flush=True)
    assert err <= tol, (err, tol)
    assert got[1, 0, 0] > 0.05 and got[0, 2, 1] < -0.03  # (towards the planted field)
    # the plan's volumes follow in _bias_compose, and only there
    from unires_amd._update import _bias_compose
    assert torch.equal(xn._bias_dat, xn.dat)
    v0 = (xn._bias_weight._version, xn._bias_dat._version)
    _bias_compose([[xn]], sett)
    torch.cuda.synchronize()
    b = xn._bias_b.cpu().numpy()
    assert int(_ulps(b, bias64.field64(got, shape)).max()) <= 1
    wg, wx = bias64.compose32(inp['g'], b, inp['x'])
    assert np.array_equal(xn._bias_weight.cpu().numpy(), wg) and np.array_equal(xn._bias_dat.cpu().numpy(), wx)
    assert xn._bias_weight._version > v0[0] and xn._bias_dat._version > v0[1]
    v1 = (xn._bias_weight._version, xn._bias_dat._version)
    _bias_compose([[xn]], sett)  # (nothing changed: nothing is written)
    assert (xn._bias_weight._version, xn._bias_dat._version) == v1


# ---- (4) the plan ------------------------------------------------------------------------------------------------------
def test_a_plan_with_a_field_has_the_bits_of_the_plan_handed_its_volumes(dev):
    """tests/test_gpu_mask.py's 10 x 9 x 8 two-repeat problem, fixed coefficients on the second repeat: the matvec, the
    right-hand side (assembled and cached) and a 6-iteration tol = 0 CG solve of the plan fetched through the
    observation structs are bit for bit those of a plan whose second repeat was given bias64.compose32's g b^2 through
    set_voxel_weights and x / b for its observation, with a voxel map g and without.  New coefficients: the solve -
    a replay of the captured graph - has the bits of a fresh plan's with the recomposed volumes."""
    import unires_amd as U
    from tests.test_gpu_mask import _small
    from unires_amd._plan import ChannelPlan
    from unires_amd._project import _channel_plan
    from unires_amd._update import _bias_compose, _obs
    from unires_amd.run import _init_bias
    rng = np.random.default_rng(4)
    for with_g in (False, True):
        prob, xg, yg, vx = _small(dev)
        sett = U.settings()
        x1 = xg[0][1]
        shape = tuple(x1.dat.shape)
        g = torch.from_numpy(rng.random(shape).astype(np.float32)).to(dev) if with_g else None
        x1.weight = g
        coefs = [torch.from_numpy(0.2 * rng.standard_normal((2, 2, 2))) for _ in range(2)]
        x1.bias_coef = coefs[0]
        _init_bias(xg, sett, dev)
        assert xg[0][0]._bias_b is None and x1._bias_b is not None and not x1._bias_est
        rho, lam = float(prob['rho']), float(yg[0].lam)
        w, z = prob['w'][0].to(dev), prob['z'][0].to(dev)
        p = torch.from_numpy(rng.random(prob['dim_y']).astype(np.float32)).to(dev)
        reps = [(xn.po, xn.tau) for xn in xg[0]]
        vxl = [float(v) for v in vx]

        def by_hand():
            b = x1._bias_b.cpu().numpy()
            wg, wx = bias64.compose32(None if g is None else g.cpu().numpy(), b, x1.dat.cpu().numpy())
            pl = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
            pl.set_voxel_weights(1, torch.from_numpy(wg).to(dev))
            return pl, [xg[0][0].dat, torch.from_numpy(wx).to(dev)]

        def outputs(pl, dats):
            q = pl.matvec(p, rho, lam)
            b1 = pl.rhs(dats, w, z, rho, lam)
            b2 = torch.empty_like(b1)
            pl.rhs_cached(dats, w, z, rho, lam, out=b2)
            y = prob['y0'][0].to(dev).clone()
            pl.cg(b1, y, rho, lam, max_iter=6, tolerance=0.0)
            torch.cuda.synchronize()
            return q, b1, b2, y

        plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
        assert plan.repeat_info(1)['voxel_weighted'] and not plan.repeat_info(0)['voxel_weighted']
        got = outputs(plan, [_obs(xn, sett) for xn in xg[0]])
        hand, dats = by_hand()
        want = outputs(hand, dats)
        hand.close()
        for a_, b_, what in zip(got, want, ('matvec', 'rhs', 'cached rhs', 'cg')):
            assert torch.equal(a_, b_), (with_g, what)
        plain = ChannelPlan(prob['dim_y'], vxl, reps, prob['method'], prob['do_proj'], device=dev)
        if g is not None:
            plain.set_voxel_weights(1, g)
        assert not torch.equal(plain.matvec(p, rho, lam), got[0])  # (the field did something)
        plain.close()
        # new coefficients: recomposed, the plan fetched again, the captured solve replayed
        x1._bias_coef = coefs[1].clone()
        x1._bias_rev += 1
        _bias_compose(xg, sett)
        plan2 = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
        assert plan2 is plan
        got2 = outputs(plan2, [_obs(xn, sett) for xn in xg[0]])
        hand, dats = by_hand()
        want2 = outputs(hand, dats)
        hand.close()
        for a_, b_, what in zip(got2, want2, ('matvec', 'rhs', 'cached rhs', 'cg')):
            assert torch.equal(a_, b_), (with_g, 'recomposed', what)
        assert not torch.equal(got2[3], got[3])
        plan.close()


# ---- (5) end to end ----------------------------------------------------------------------------------------------------
def _shaded(dev, fixed=False):
    """tests/test_gpu_slice.py's 48 x 48 x 40 phantom with two channels, 3 mm slices, noise sd 2: channel 0 with two
    repeats, thick along z (48, 48, 13) and along y (48, 16, 40) so that together they resolve the phantom, which carry
    opposite planted fields - beta = +-(0.15 phi_1(i) + 0.05 phi_1(j)) on each repeat's own grid, the same function of
    position, b within 0.82 .. 1.22 - and channel 1 with one clean repeat.  bias_cutoff = 40 mm gives every repeat the
    orders (3, 3, 2).  Both repeats get the precision of the noise they were drawn with (make_problem understates the
    second's): the ridge pins the kappa-weighted mean of a channel's log fields to 0 and leaves the rest of a common
    shading to y, so opposite fields are recoverable exactly when the two kappas agree."""
    from tests.helpers import gpu_structs, make_problem
    prob = make_problem(seed=5, dim_y=(48, 48, 40), n_channels=2, thick=3, n_repeats=2, rot=0.0, trans=0.0, noise_sd=2.0,
                        thick_axes=None, shift=(0.0, 0.0, 0.0))
    xg, yg, sett = gpu_structs(prob, dev)
    xg[1] = xg[1][:1]
    xg[0][1].tau = xg[0][0].tau
    planted = np.zeros((3, 3, 2))
    planted[1, 0, 0], planted[0, 1, 0] = 0.15, 0.05
    fields = [np.exp(bias64.beta64(sgn * planted, tuple(xn.dat.shape))).astype(np.float32)
              for sgn, xn in zip((1.0, -1.0), xg[0])]
    assert [tuple(xn.dat.shape) for xn in xg[0]] == [(48, 48, 13), (48, 16, 40)]
    for xn, f in zip(xg[0], fields):
        xn.dat = xn.dat * torch.from_numpy(f).to(dev)
    for yc in yg:
        yc.lam0 = float(yc.lam) / 4.0
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 14, 1e-4, 4.0, 0
    sett.cgs_max_iter, sett.cgs_tol = 20, 0.0
    sett.clean_fov = False
    sett.bias_cutoff = 40.0
    return prob, xg, yg, sett, planted, fields


def test_fit_corrects_shading(dev, monkeypatch):
    """fit() for 14 ADMM iterations with sett.bias off and on, on the same data.  With it on: (a) no bias step raises
    its objective (every (E before, E after) pair of every repeat and iteration, recorded around _update_bias); (b) the
    log ratio of the two recovered fields of channel 0, both synthesised on the reconstruction's grid, correlates with
    the planted one (> 0.9); (c) the RMS error of
    channel 0 against the phantom is lower than with it off; (d) info['bias'] holds one CPU float64 (3, 3, 2) tensor
    per repeat, None with it off, and obj is (14, 3) with obj[:, 0] = obj[:, 1] + obj[:, 2].

    Observed on an MI355X: RMSE of channel 0 8.018 off, 6.344 on; recovered c[1,0,0] +0.1470 / -0.1449 for planted
    +-0.15; correlation 1.0000; 42 steps, none raised E.  (A first form of the phantom - both repeats thick along z, the
    second repeat's tau understated by 1.69 - gave 22.570 off against 22.716 on, with the same correlation: DESIGN.md
    8.16 says why that phantom cannot show the difference.)"""
    import unires_amd as U
    from unires_amd import _update
    steps = []
    inner = _update._update_bias

    def recording(x, y, sett, raw=None):
        out = inner(x, y, sett, raw)
        steps.extend(xn._bias_E for xc in x for xn in xc if getattr(xn, '_bias_est', False))
        return out

    monkeypatch.setattr(_update, '_update_bias', recording)
    out, infos = {}, {}
    for arm in ('off', 'on'):
        prob, xg, yg, sett, planted, fields = _shaded(dev)
        sett.bias = arm == 'on'
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 14
        out[arm], infos[arm] = dat.cpu(), info
    truth = prob['truth']
    rmse = {arm: [float(((out[arm][..., c].double() - truth[c].double()) ** 2).mean().sqrt()) for c in range(2)]
            for arm in out}
    print('fit with shading: RMSE of channel 0 off %.3f on %.3f; channel 1 off %.3f on %.3f'
          % (rmse['off'][0], rmse['on'][0], rmse['off'][1], rmse['on'][1]), flush=True)
    # (d)
    assert infos['off']['bias'] == [[None, None], [None]]
    cs = infos['on']['bias']
    assert [len(c) for c in cs] == [2, 1]
    assert all(t.device.type == 'cpu' and t.dtype == torch.float64 and tuple(t.shape) == (3, 3, 2) for c in cs for t in c)
    for arm in infos:
        obj = infos[arm]['obj']
        assert tuple(obj.shape) == (14, 3) and bool(torch.isfinite(obj).all())
        assert torch.allclose(obj[:, 0], obj[:, 1] + obj[:, 2], rtol=1e-12, atol=0.0)
    # (a)
    assert len(steps) == 14 * 3
    assert all(E1 <= E0 for E0, E1, _ in steps), [s for s in steps if s[1] > s[0]]
    assert sum(1 for _, _, s in steps if s > 0) >= 14
    # (b)
    # (the two repeats have grids of their own over one field of view: both fields are synthesised on the reconstruction's)
    shape = tuple(prob['dim_y'])
    rec = [U.bias_field(cs[0][n], shape, device=dev).cpu().double().log().numpy() for n in range(2)]
    want = 2.0 * bias64.beta64(planted, shape)
    corr = float(np.corrcoef((rec[0] - rec[1]).ravel(), want.ravel())[0, 1])
    print('  recovered coefficients: c[1,0,0] %.4f / %.4f (planted +-0.15), c[0,1,0] %.4f / %.4f (planted +-0.05), '
          'c[0,0,0] %.4f / %.4f; correlation of the log ratio %.4f; the clean channel |c| <= %.4f'
          % (cs[0][0][1, 0, 0], cs[0][1][1, 0, 0], cs[0][0][0, 1, 0], cs[0][1][0, 1, 0], cs[0][0][0, 0, 0],
             cs[0][1][0, 0, 0], corr, float(cs[1][0].abs().max())), flush=True)
    assert corr > 0.9
    # (c)
    assert rmse['on'][0] < rmse['off'][0]


# ---- (6) fixed coefficients --------------------------------------------------------------------------------------------
def test_fixed_coefficients_come_back_unchanged(dev):
    """_input.bias_coef equal to the planted coefficients, sett.bias off, three iterations: info['bias'] returns them
    bit for bit (a copy: not the user's tensor), the other repeats have None, and the reconstruction differs from the
    run without them.  With sett.bias on as well they still come back unchanged, and the other repeats are estimated."""
    import unires_amd as U
    res = {}
    for arm in ('none', 'fixed', 'fixed+est'):
        prob, xg, yg, sett, planted, _ = _shaded(dev)
        sett.max_iter = 3
        given = [torch.from_numpy(sgn * planted) for sgn in (1.0, -1.0)]
        if arm != 'none':
            xg[0][0].bias_coef = given[0]
        sett.bias = arm == 'fixed+est'
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        res[arm] = (dat.cpu(), info['bias'])
        if arm != 'none':
            assert xg[0][0].bias_coef is given[0] and torch.equal(given[0], torch.from_numpy(planted))
            got = info['bias'][0][0]
            assert torch.equal(got, given[0]) and got.data_ptr() != given[0].data_ptr()
    assert res['none'][1] == [[None, None], [None]]
    assert res['fixed'][1][0][1] is None and res['fixed'][1][1][0] is None
    assert not torch.equal(res['fixed'][0], res['none'][0])
    est = res['fixed+est'][1]
    assert float(est[0][1].abs().max()) > 0 and est[1][0] is not None


# ---- (7) with both robust rules, mask_zeros and channel streams ----------------------------------------------------------
def test_bias_with_both_robust_rules_and_mask_zeros_on_channel_streams(dev):
    """Three channels of two repeats on streams of their own, sett.bias with sett.slice_robust, sett.voxel_robust
    (voxel_scale = 'mad') and sett.mask_zeros, a zero-filled corner and a +-15 % ramp in every channel's first repeat,
    three ADMM iterations through fit() on fresh structs, twice: it finishes, everything is finite, and the two runs
    agree bit for bit - in y, the coefficients and the weights.  The fields move: the run with sett.bias off differs."""
    import unires_amd as U
    from tests.helpers import gpu_structs, make_problem
    prob = make_problem(seed=7, dim_y=(40, 36, 33), n_channels=3, n_repeats=2, thick=3, rot=0.08, trans=1.0)

    def run(bias=True):
        xg, yg, sett = gpu_structs(prob, dev)
        for xc in xg:
            xc[0].dat[:4, :4, :2] = 0
            n0 = int(xc[0].dat.shape[0])
            ramp = torch.linspace(0.85, 1.15, n0, device=dev).reshape(n0, 1, 1)
            xc[0].dat *= ramp
        for yc in yg:
            yc.lam0 = float(yc.lam)
        sett.channel_streams = True
        sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 3, 1e-4, 1.0, 0
        sett.cgs_max_iter, sett.cgs_tol = 8, 0.0
        sett.clean_fov = False
        sett.bias, sett.bias_cutoff = bias, 30.0
        sett.slice_robust, sett.voxel_robust, sett.voxel_scale, sett.mask_zeros = True, True, 'mad', True
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 3
        return dat.cpu(), info

    a, ia = run()
    b, ib = run()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(ia['obj']).all())
    assert torch.equal(a, b)
    for c in range(3):
        assert bool(torch.isfinite(ia['bias'][c][0]).all()) and max(ia['bias'][c][0].shape) > 1
        assert torch.equal(ia['bias'][c][0], ib['bias'][c][0]), c
        assert torch.equal(ia['slice_w'][c][0], ib['slice_w'][c][0]), c
        assert torch.equal(ia['voxel_w'][c][0], ib['voxel_w'][c][0]), c
        assert float(ia['bias'][c][0].abs().max()) > 0.005, c
    plain, _ = run(bias=False)
    assert not torch.equal(plain, a)
