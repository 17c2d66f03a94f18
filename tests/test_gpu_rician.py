"""The Rician data term on the GPU (sett.noise_model = 'rician'): a non-CT repeat's voxel term is
W [1/2 tau (x - mu)^2 + c(tau x mu)], mu = e . A y, and every y-update is the Gaussian one on the effective observation
x R(tau x mu) of the previous y (the first on x itself).

(1) unires_rician_terms against float64; (2) the first Rician iteration is the Gaussian one; (3) exact MM descent at
10 x 9 x 8 with dense-accurate solves; (4) fit() removes the bias of dark regions; (5) with both robust rules, a CT
repeat and the channels on streams of their own.

The reference has no counterpart: the float64 side is tests/rician64.py (torch.special's i0e / i1e) on tests/ref64.py.
Children are started the way tests/test_gpu_gain.py starts them (tests/test_gpu_mask.py's ``_run``).

Tests (1) - (4) fail on the commit before the feature: the library has no ``unires_rician_terms``, the settings no
``noise_model``, and nothing removes the bias.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import rician64
from tests.test_gpu_mask import GATE, _dense, _run
from tests.test_gpu_slice import SUM_SHAPES, _phantom, _small_clean, sums_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ('none', 'g', 'e', 'ge', '01')
FORMS = ('xt', 'sums', 'both')
TAU = 2.5e-4  # sums_inputs' x and ay are about 100 +- 50: z = tau x ay lies on both sides of the branch point 3.75
PLANTED_SHAPE = (6, 5, 67)


def terms_weights(shape, axis, arm):
    """(g, e) float32 CPU or None each for an arm of (1): g generic in [0, 1] ('01': draws from {0, 1}), e generic in
    [0.5, 2]."""
    from tests import gain64
    gen = torch.Generator().manual_seed(67 + axis + sum(shape))
    g = torch.rand(shape, generator=gen).float()
    if arm == '01':
        return (g < 0.7).float(), None
    return (g if 'g' in arm else None), (gain64.gains(shape[axis], 'generic') if 'e' in arm else None)


def planted_inputs():
    """(x, ay, tau): x = 0, ay = 0, ay < 0, z = tau x ay at, just below and just above the branch point, tiny and
    huge z, cycled through a volume no extent of which is a multiple of the wave."""
    n = int(np.prod(PLANTED_SHAPE))
    xs = torch.tensor([1.5, 0.0, 1.5, 1.5, 3.0, 1.5, 1e-15, 1.5e3, 0.75, 1.5, 2.0, 0.0])
    ays = torch.tensor([2.5, 2.5, 0.0, -2.5, 1.2499999, 2.5000002, 1e-15, 1.5e3, -5.0000005, 2.4999998, -0.0, -1.0])
    i = torch.arange(n)
    return xs[i % 12].reshape(PLANTED_SHAPE).float(), ays[(i + i // 12) % 12].reshape(PLANTED_SHAPE).float(), 1.0


def _cases():
    """(key, shape, axis, arm, x, ay, g, e, tau) of (1)."""
    for shape, axis in SUM_SHAPES:
        x, ay = sums_inputs(shape, axis)
        for arm in ARMS:
            g, e = terms_weights(shape, axis, arm)
            yield 'x'.join(map(str, shape)) + '/%d/%s' % (axis, arm), shape, axis, arm, x, ay, g, e, TAU
    x, ay, tau = planted_inputs()
    for axis in range(3):
        for arm in ('none', 'ge'):
            g, e = terms_weights(PLANTED_SHAPE, axis, arm)
            yield 'planted/%d/%s' % (axis, arm), PLANTED_SHAPE, axis, arm, x, ay, g, e, tau


# ---- (1) unires_rician_terms ---------------------------------------------------------------------------------------------
_TERMS_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_rician import FORMS, _cases
from tests.test_gpu_slice import sums_inputs
from unires_amd import _lib
from unires_amd._lib import i3
lib, out, res = _lib.load(), sys.argv[1], {}
P = lambda t: None if t is None else t.data_ptr()
D = lambda t: None if t is None else t.to('cuda:0')
for key, shape, axis, arm, x, ay, g, e, tau in _cases():
    x, ay, g, e = D(x), D(ay), D(g), D(e)
    S = shape[axis]
    for form in FORMS:
        for run in (0, 1):
            xt = torch.full(shape, float('nan'), device='cuda:0') if form != 'sums' else None
            L = torch.full((S,), float('nan'), dtype=torch.float64, device='cuda:0') if form != 'xt' else None
            rc = lib.unires_rician_terms(P(x), P(ay), P(g), P(e), i3(shape), axis, tau, P(xt), P(L), None)
            assert rc == 0, (key, form, rc)
            torch.cuda.synchronize()
            if xt is not None:
                res['%%s/%%s/xt%%d' %% (key, form, run)] = xt.cpu().numpy()
            if L is not None:
                res['%%s/%%s/L%%d' %% (key, form, run)] = L.cpu().numpy()
# in place on ay
x, ay = (t.to('cuda:0') for t in sums_inputs((41, 38, 60), 1))
keep = ay.clone()
want = torch.empty_like(ay)
assert lib.unires_rician_terms(P(x), P(ay), None, None, i3(ay.shape), 1, %(tau)r, P(want), None, None) == 0
assert lib.unires_rician_terms(P(x), P(ay), None, None, i3(ay.shape), 1, %(tau)r, P(ay), None, None) == 0
torch.cuda.synchronize()
res['inplace'] = np.array(int(torch.equal(ay, want) and not torch.equal(ay, keep)))
# status codes: unires_slice_sums' for the same mistakes; nothing to write, or xt == x: the invalid-argument code
x, ay = (t.to('cuda:0') for t in sums_inputs((5, 7, 6), 1))
o1, o2 = torch.zeros(7, dtype=torch.float64, device='cuda:0'), torch.zeros(14, dtype=torch.float64, device='cuda:0')
codes = []
for bad in ('x', 'ay', 'axis-', 'axis+', 'dim0'):
    a = dict(x=x.data_ptr(), ay=ay.data_ptr(), dim=i3((5, 7, 6)), axis=1)
    if bad in ('x', 'ay'):
        a[bad] = None
    if bad.startswith('axis'):
        a['axis'] = -1 if bad == 'axis-' else 3
    if bad == 'dim0':
        a['dim'] = i3((5, 0, 6))
    mine = lib.unires_rician_terms(a['x'], a['ay'], None, None, a['dim'], a['axis'], 1.0, None, o1.data_ptr(), None)
    theirs = lib.unires_slice_sums(a['x'], a['ay'], a['dim'], a['axis'], o2.data_ptr(), None)
    codes.append((mine, theirs))
res['codes'] = np.array(codes)
arg = lib.unires_slice_sums(x.data_ptr(), ay.data_ptr(), i3((5, 7, 6)), 3, o2.data_ptr(), None)
res['arg'] = np.array([arg,
                       lib.unires_rician_terms(x.data_ptr(), ay.data_ptr(), None, None, i3((5, 7, 6)), 1, 1.0, None, None, None),
                       lib.unires_rician_terms(x.data_ptr(), ay.data_ptr(), None, None, i3((5, 7, 6)), 1, 1.0, x.data_ptr(),
                                               o1.data_ptr(), None)])
np.savez(out, **res)
'''


def test_rician_terms_against_float64(tmp_path):
    """Over SUM_SHAPES x the arms {none, g, e, g + e, 0 / 1 g} x the forms {xt, sums, both}, and the planted input along
    every axis.  x~: every voxel within (2e-6 + 4 2^-24) |x~64| + 2^-120 (R's cap; three roundings of z, where R's
    elasticity is at most 1; the final product), exactly +0 where x == 0.  L: every entry within the accumulation bound
    plus sum g 1e-6 (1 + |c64|), exactly 0 for the all-zero slice.  Two runs the same bits; the forms agree bit for bit
    on what they share; nothing is left unwritten (the outputs start as NaN); the status codes."""
    res = _run(tmp_path, 'rician_terms', _TERMS_CHILD % dict(root=ROOT, tau=TAU), timeout=300)
    worst_x = worst_l = 0.0
    for key, shape, axis, arm, x, ay, g, e, tau in _cases():
        x, ay = x.numpy(), ay.numpy()
        gn, en = (None if t is None else t.numpy() for t in (g, e))
        xt64, c64 = rician64.terms64(x, ay, en, tau, axis)
        S = shape[axis]
        xt, L = res['%s/both/xt0' % key], res['%s/both/L0' % key]
        for form in FORMS:
            for run in (0, 1):
                if form != 'sums':
                    assert np.array_equal(res['%s/%s/xt%d' % (key, form, run)].view(np.uint32), xt.view(np.uint32)), (key, form, run)
                if form != 'xt':
                    assert np.array_equal(res['%s/%s/L%d' % (key, form, run)].view(np.uint64), L.view(np.uint64)), (key, form, run)
        assert xt.shape == tuple(shape) and np.isfinite(xt).all(), key
        assert L.shape == (S,) and np.isfinite(L).all(), key
        tol = (2e-6 + 4 * 2.0 ** -24) * np.abs(xt64) + 2.0 ** -120
        err = np.abs(xt.astype(np.float64) - xt64)
        worst_x = max(worst_x, float((err / tol).max()))
        assert (err <= tol).all(), (key, 'xt', int(np.argmax(err / tol)), float((err / tol).max()))
        zero = x == 0
        assert (xt[zero] == 0).all() and not np.signbit(xt[zero]).any(), (key, 'x == 0')
        want, acc, _ = rician64.sums64(c64, gn, axis)
        cap = rician64.sums64(1e-6 * (1.0 + np.abs(c64)), gn, axis)[0]
        lerr = np.abs(L - want)
        lrat = lerr / np.maximum(acc + cap, 1e-300)
        worst_l = max(worst_l, float(lrat.max()))
        assert (lerr <= acc + cap).all(), (key, 'L', int(np.argmax(lrat)), float(lrat.max()))
        if not key.startswith('planted'):
            assert L[S // 2] == 0.0, (key, 'the all-zero slice')
    print('rician terms: worst x~ err / tol %.3f, worst L err / bound %.3f' % (worst_x, worst_l), flush=True)
    # the planted input holds what it says
    x, ay, tau = planted_inputs()
    z = rician64.z32(x.numpy(), ay.numpy(), None, tau)[1]
    assert (x == 0).any() and (ay == 0).any() and (ay < 0).any()
    assert ((z > 3.7) & (z <= 3.75)).any() and ((z > 3.75) & (z < 3.8)).any() and (z < -3.75).any() and (z > 1e6).any()
    assert int(res['inplace']) == 1
    codes = res['codes']
    assert (codes[:, 0] == codes[:, 1]).all() and (codes[:, 0] != 0).all(), codes
    assert res['arg'][0] != 0 and (res['arg'][1:] == res['arg'][0]).all(), res['arg']


# ---- (2) the first Rician iteration is the Gaussian one --------------------------------------------------------------------
def _magnitude(xg):
    """The helpers' observations carry Gaussian noise: their magnitudes, for both models alike."""
    for xc in xg:
        for xn in xc:
            xn.dat = xn.dat.abs()
    return xg


def _fit_settings(sett, yg, max_iter, cg_iter):
    for yc in yg:
        yc.lam0 = float(yc.lam)
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = max_iter, 1e-4, 1.0, 0
    sett.cgs_max_iter, sett.cgs_tol = cg_iter, 0.0
    sett.clean_fov = False
    return sett


def _correction64(xg, yg, sett):
    """(sum of the repeats' sum_s L_s, its bound) from rician64 on the device's own A y."""
    import unires_amd as U
    from unires_amd._project import _slice_axis
    tot = bound = 0.0
    for n, xn in enumerate(xg[0]):
        Ay = U._proj('A', yg[0].dat, xg[0], yg[0], n=n, method=sett.method, do=sett.do_proj)
        e = getattr(xn, 'slice_gain', None)
        a = _slice_axis(xn)
        _, c64 = rician64.terms64(xn.dat.cpu().numpy(), Ay.cpu().numpy(), None if e is None else e.cpu().numpy(),
                                  float(xn.tau), a)
        want, acc, _ = rician64.sums64(c64, None, a)
        cap = rician64.sums64(1e-6 * (1.0 + np.abs(c64)), None, a)[0]
        tot += math.fsum(want.tolist())
        bound += math.fsum((acc + cap).tolist())
    return tot, bound


@pytest.mark.parametrize('which', ['small', 'phantom'])
def test_the_first_rician_iteration_is_the_gaussian_one(dev, which):
    """max_iter = 1 on the 10 x 9 x 8 two-repeat problem and on the thick-slice 48 x 48 x 40 phantom: y has the same
    bits under both models, obj[0, 2] too, and obj[0, 1] differs by the repeats' sum_s L_s of rician64 within (1)'s
    bound (and a few roundings of the float64 additions)."""
    import unires_amd as U
    out = {}
    for model in ('gaussian', 'rician'):
        if which == 'small':
            prob, xg, yg, vx, a, S = _small_clean(dev)
            from tests.helpers import gpu_structs
            sett = gpu_structs(prob, dev)[2]
        else:
            prob, (xg, yg, sett) = _phantom(dev)
        _magnitude(xg)
        _fit_settings(sett, yg, 1, 12)
        sett.noise_model = model
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 1
        out[model] = (dat.cpu(), info['obj'], xg, yg, sett)
    yg_, yr_ = out['gaussian'][0], out['rician'][0]
    assert torch.equal(yg_, yr_)
    og, orr = out['gaussian'][1], out['rician'][1]
    assert float(og[0, 2]) == float(orr[0, 2])
    assert float(orr[0, 0]) == float(orr[0, 1]) + float(orr[0, 2])
    _, _, xg, yg, sett = out['rician']
    for xn in xg[0]:  # the effective observation of the second y-update is in place, and is not x
        assert xn._rician_dat is not None and not torch.equal(xn._rician_dat, xn.dat)
        assert bool((xn._rician_dat.abs() <= xn.dat).all())
    assert all(getattr(xn, '_rician_dat', None) is None for xn in out['gaussian'][2][0])
    want, bound = _correction64(xg, yg, sett)
    got = float(orr[0, 1]) - float(og[0, 1])
    slack = 8 * 2.0 ** -53 * abs(float(orr[0, 1]))
    print('%s: obj[0, 1] gaussian %.6f rician %.6f, correction %.9g (float64 %.9g, bound %.3g)'
          % (which, float(og[0, 1]), float(orr[0, 1]), got, want, bound + slack), flush=True)
    assert want > 0
    assert abs(got - want) <= bound + slack


# ---- (3) exact MM descent ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weighted', [False, True])
def test_mm_steps_with_dense_accurate_solves_descend_the_rician_objective(dev, weighted):
    """10 x 9 x 8, two repeats, fixed z, w, rho; Rician data planted from A y* at 1 - 3 sigma, the first third of the
    second repeat's slices zero.  The Gaussian solve, then six outer steps - x~ from the current y, plan.rhs + plan.cg
    run to the dense-solve gate.  F(y) = sum W [1/2 tau (x - e A y)^2 + c] + 1/2 rho |lam D y - z + w / rho|^2 in float64
    from ref64.Operator64 is non-increasing from step to step within 1e-6 |F| and ends below its value at the Gaussian
    solution.  Once without weights; once with slice and voxel weights and a user gain on the second repeat."""
    from tests import diff64, gain64, ref64, slice64, voxel64
    from tests.helpers import oracle_structs
    from unires_amd._project import _channel_plan
    from unires_amd._update import _rician_terms
    from unires_amd.struct import settings
    prob, xg, yg, vx, a, S = _small_clean(dev)
    xs, ys = oracle_structs(prob)
    dim = prob['dim_y']
    ny = int(np.prod(dim))
    rho, lam = ref64._f32(prob['rho']), ref64._f32(ys[0].lam)
    A = [_dense(ref64.Operator64(xn.po, prob['method'])) for xn in xs[0]]
    taus = [ref64._f32(xn.tau) for xn in xs[0]]
    gen = torch.Generator().manual_seed(77)
    truth = prob['truth'][0].double().numpy().reshape(-1)
    ystar = truth * (2.0 * taus[0] ** -0.5 / truth.mean())
    W, E = [], []
    for n, xn in enumerate(xg[0]):
        shape = tuple(xn.dat.shape)
        clean = torch.from_numpy((A[n] @ ystar).reshape(shape))
        dat = rician64.rice(clean, taus[n] ** -0.5, shape, gen).float()
        if n == 1:
            dat[:, :, :max(1, shape[2] // 3)] = 0.0
        xn.dat = dat.to(dev)
        w_n, e_n = np.ones(shape), np.ones(shape)
        if weighted and n == 1:
            u, g, e = slice64.weights(S, 'ramp'), voxel64.weights(shape, 'ramp'), gain64.gains(S, 'generic')
            xn.slice_w, xn.weight, xn.slice_gain = u.to(dev), g.to(dev), e.to(dev)
            w_n = slice64.spread(u, shape, a).double().numpy() * g.double().numpy()
            e_n = slice64.spread(e, shape, a).double().numpy()
        W.append(w_n.reshape(-1))
        E.append(e_n.reshape(-1))
    X = [xn.dat.cpu().double().numpy().reshape(-1) for xn in xg[0]]
    DtD = diff64.dense_dtd(dim, [float(v) for v in vx], 'forward')
    Reg = rho * lam * lam * DtD
    Sys = Reg.copy()
    for n in range(2):
        Sys = Sys + taus[n] * (A[n].T @ ((W[n] * E[n] * E[n])[:, None] * A[n]))
    sk = float(np.sqrt(np.linalg.cond(Sys)))
    n_it = int(np.ceil(np.log(0.5e-6) / np.log((sk - 1.0) / (sk + 1.0))))
    z, w = prob['z'][0].to(dev), prob['w'][0].to(dev)
    sett = settings()
    sett.device, sett.method, sett.do_proj, sett.noise_model = dev, prob['method'], prob['do_proj'], 'rician'
    plan = _channel_plan(xg[0], yg[0], prob['method'], prob['do_proj'], vx, weights=True)
    # the regulariser's linear term as the plan forms it: b = -lam D^T (w - rho z) = rho lam D^T (z - w / rho)
    b_reg = plan.rhs([torch.zeros_like(xn.dat) for xn in xg[0]], w, z, rho, lam).cpu().double().numpy().reshape(-1)
    const = 0.5 * rho * float(((prob['z'][0].double() - prob['w'][0].double() / rho) ** 2).sum())

    def F(y):
        y = y.cpu().double().numpy().reshape(-1)
        data = 0.0
        for n in range(2):
            mu = E[n] * (A[n] @ y)
            data += float((W[n] * rician64.nll64(X[n], mu, taus[n])).sum())
        return data + 0.5 * float(y @ Reg @ y) - float(y @ b_reg) + const

    y = yg[0].dat
    y.zero_()
    Fs = []
    for step in range(7):
        if step > 0:
            _rician_terms(xg, yg, sett, sums=False)
        obs = [xn.dat if step == 0 else xn._rician_dat for xn in xg[0]]
        b = plan.rhs(obs, w, z, rho, lam)
        plan.cg(b, y, rho, lam, max_iter=n_it, tolerance=0.0)
        torch.cuda.synchronize()
        Fs.append(F(y))
    print('MM descent (%s): %d CG iterations per solve; F at the Gaussian solution %.6f, then %s'
          % ('weighted' if weighted else 'plain', n_it, Fs[0], ['%.6f' % v for v in Fs[1:]]), flush=True)
    for before, after in zip(Fs[:-1], Fs[1:]):
        assert after <= before + 1e-6 * abs(before), Fs
    assert Fs[-1] < Fs[0] - 1e-6 * abs(Fs[0]), Fs
    assert GATE == 1e-4  # (the dense-solve gate n_it is sized for)
    plan.close()


# ---- (4) end to end: the bias of dark regions ----------------------------------------------------------------------------
SIGMA = 5.0
LEVELS = (0.0, 1.0, 2.0, 8.0)  # slabs of 12 voxels along x, in units of sigma
LAM = 0.3  # about 4 / mean(truth), helpers.make_problem's rule: lam / tau_eff is 1.5 - 2 sigma_eff, a flat interior


def _slab_problem(dev, regime):
    """A 48 x 48 x 40 piecewise-constant phantom - slabs of 0, 1, 2 and 8 sigma along x - seen through the operators of
    ``_phantom`` (two repeats with 3 mm slices along z and along y) or of the denoising regime (one repeat), with
    seeded Rician noise of sigma = 5 and tau = 1 / sigma^2."""
    import unires_amd as U
    from tests.helpers import gpu_structs, make_problem
    if regime == 'sr':
        prob, (xg, yg, sett) = _phantom(dev)
    else:
        prob = make_problem(seed=5, dim_y=(48, 48, 40), regime='dn', n_repeats=1, rot=0.0, trans=0.0, noise_sd=SIGMA,
                            shift=(0.0, 0.0, 0.0))
        xg, yg, sett = gpu_structs(prob, dev)
    truth = torch.zeros(prob['dim_y'])
    for k, lev in enumerate(LEVELS):
        truth[12 * k:12 * (k + 1)] = lev * SIGMA
    gen = torch.Generator().manual_seed(101)
    for n, xn in enumerate(xg[0]):
        clean = U._proj('A', truth.to(dev), xg[0], yg[0], n=n, method=sett.method, do=sett.do_proj).cpu().double()
        xn.dat = rician64.rice(clean.clamp(min=0.0), SIGMA, tuple(clean.shape), gen).float().to(dev)
        xn.tau = 1.0 / SIGMA ** 2
    yg[0].dat.zero_()
    yg[0].lam = LAM
    return prob, xg, yg, sett, truth


@pytest.mark.parametrize('regime', ['sr', 'dn'])
def test_fit_removes_the_bias_of_dark_regions(dev, regime):
    """30 ADMM iterations of 10 CG iterations under both models.  Over the slab interiors, eroded by the slice
    thickness (3 voxels): |mean(y) - truth| is smaller under 'rician' than under 'gaussian' in the 0, 1 sigma and
    2 sigma slabs, and in the 1 sigma slab less than half of it.  obj is (30, 3) with obj[:, 0] = obj[:, 1] + obj[:, 2].

    Observed values: DESIGN.md 8.14 (the test prints them)."""
    import unires_amd as U
    bias, flat = {}, {}
    for model in ('gaussian', 'rician'):
        prob, xg, yg, sett, truth = _slab_problem(dev, regime)
        _fit_settings(sett, yg, 30, 10)
        sett.noise_model = model
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 30
        obj = info['obj']
        assert tuple(obj.shape) == (30, 3) and obj.dtype == torch.float64 and bool(torch.isfinite(obj).all())
        assert torch.allclose(obj[:, 0], obj[:, 1] + obj[:, 2], rtol=1e-12, atol=0.0)
        y = dat[..., 0].cpu().double()
        for k, lev in enumerate(LEVELS):
            inner = y[12 * k + 3:12 * (k + 1) - 3, 3:-3, 3:-3]
            bias[(model, lev)] = abs(float(inner.mean()) - lev * SIGMA) / SIGMA
            flat[(model, lev)] = float(inner.std()) / SIGMA
    for lev in LEVELS:
        print('%s slab %g sigma: |bias| gaussian %.3f rician %.3f sigma; interior std %.3f / %.3f sigma'
              % (regime, lev, bias[('gaussian', lev)], bias[('rician', lev)], flat[('gaussian', lev)],
                 flat[('rician', lev)]), flush=True)
    for lev in (0.0, 1.0, 2.0):
        assert bias[('rician', lev)] < bias[('gaussian', lev)], (regime, lev, bias)
    assert bias[('rician', 1.0)] < 0.5 * bias[('gaussian', 1.0)], (regime, bias)


# ---- (5) with the rules, a CT repeat and channel streams --------------------------------------------------------------------
def test_rician_with_both_robust_rules_a_ct_repeat_and_channel_streams(dev):
    """Three channels under 'rician' with sett.slice_robust and sett.voxel_robust, the third channel's repeat CT, three
    ADMM iterations through fit(): the channels on streams of their own against one channel after the other, on fresh
    structs each time - the same bits in y and in both kinds of weights.  The CT repeat keeps ``_rician_dat`` unset,
    keeps its negative values, and adds to the objective what it adds under 'gaussian', bit for bit; the model does
    something: the Gaussian run differs."""
    import unires_amd as U
    from tests.helpers import gpu_structs, make_problem, rel_err
    from unires_amd._update import _compute_nll, _obs, _rician_terms
    prob = make_problem(seed=7, dim_y=(40, 36, 33), n_channels=3, thick=3, rot=0.08, trans=1.0, noise_sd=150.0)

    def run(streams, model='rician'):
        xg, yg, sett = gpu_structs(prob, dev)
        _magnitude(xg[:2])
        xg[2][0].ct = True
        _fit_settings(sett, yg, 3, 8)
        sett.channel_streams = streams
        sett.slice_robust, sett.voxel_robust = True, True
        sett.noise_model = model
        dat, _, _, info = U.fit(xg, yg, sett)
        torch.cuda.synchronize()
        assert info['n_iter'] == 3
        return dat.cpu(), info, xg, yg, sett

    serial, si, xg, yg, sett = run(False)
    assert bool((xg[2][0].dat < 0).any())
    assert xg[2][0]._rician_dat is None and _obs(xg[2][0], sett) is xg[2][0].dat
    assert all(xg[c][0]._rician_dat is not None and _obs(xg[c][0], sett) is xg[c][0]._rician_dat for c in range(2))
    assert sorted(_rician_terms(xg, yg, sett, write=False)) == [(0, 0), (1, 0)]
    # the CT repeat's data term on its own, at the final y, under both models
    vals = []
    for model in ('rician', 'gaussian'):
        sett.noise_model = model
        vals.append(float(_compute_nll([xg[2]], [yg[2]], sett, 1.0)[1]))
    sett.noise_model = 'rician'
    assert vals[0] == vals[1] and vals[0] > 0
    for attempt in range(2):
        side, pi, _, _, _ = run(True)
        print('channel streams: attempt %d rel. difference %.3g' % (attempt, rel_err(side, serial)), flush=True)
        assert torch.equal(side, serial), (attempt, rel_err(side, serial))
        for c in range(3):
            assert torch.equal(pi['slice_w'][c][0], si['slice_w'][c][0]), (attempt, c)
            assert torch.equal(pi['voxel_w'][c][0].cpu(), si['voxel_w'][c][0].cpu()), (attempt, c)
    obj = si['obj']
    assert torch.allclose(obj[:, 0], obj[:, 1] + obj[:, 2], rtol=1e-12, atol=0.0)
    plain = run(True, model='gaussian')[0]
    assert rel_err(plain, serial) > 1e-4
