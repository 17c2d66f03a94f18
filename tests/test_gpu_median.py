"""Exact medians on the GPU: ``unires_median_absres``, ``unires_median_hh`` and ``unires_voxel_huber_dev``
bit for bit against tests/median64.py (the count N exact), then ``init()`` with ``sett.noise_est = 'mad'`` and ``fit()``
with ``sett.voxel_scale = 'mad'`` against the restated chains.

(1) the kernels on their own, in one child process (tests/test_gpu_mask.py's ``_run``: under a time limit, nothing more
on the GPU after a child that exited non-zero or timed out); (2) init(); (3) fit() on tests/test_gpu_voxel.py's phantom
with a planted box.

Every median is an integer-count radix select: there is no tolerance anywhere in (1), and none on sd, tau, the weights
or the reported scale in (2) and (3); mu is a float64 sum in torch's order against numpy's, 1e-6 relative.

Every test of this file fails on the commit before the feature: the library has none of the three symbols, ``stats`` no
``median_hh``, and ``settings`` neither ``noise_est`` nor ``voxel_scale``.
"""
import os

import numpy as np
import pytest
import torch

from tests import median64 as M
from tests.test_gpu_mask import _run
from tests.test_gpu_voxel import BOX, HUBER_C, HUBER_SHAPES, NOISE_SD, huber_inputs
from tests.test_median import value_sets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)

# ---- (1) the kernels on their own ---------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257)
# (n, every pointer one float past a 16-byte boundary): 1027 - a tail after the 16-byte groups, or all of it voxel by
# voxel; 40003 - 10 workgroups of 256 threads, two groups in flight each: more than one sweep of the grid, and a tail
LONG = ((1027, False), (1027, True), (40003, False), (40003, True))
ELIGIBILITY = ('plain', 'x0', 'p0', 'nonfinite', 'none')
# (shape, axis): one cell; no cell; every axis; odd sizes over more than one workgroup; the phantom's size
HH_CASES = [((2, 2, 1), 2), ((1, 5, 4), 2), ((5, 1, 4), 0), ((3, 4, 5), 0), ((3, 4, 5), 1), ((3, 4, 5), 2), ((67, 3, 65), 1),
            ((9, 70, 3), 2), ((48, 48, 40), 2)]
HH_VARIANTS = ('plain', 'zeros', 'weight', 'ct', 'neg')


def absres_inputs(n, values, elig):
    """(x, ay, prior or None) whose eligible residuals are the magnitudes of value set ``values``: x = v, ay = 0 where
    v != 0 and x = ay = 1 (an exact zero residual of a voxel that is not missing) where v == 0; then ``elig``: 'x0' -
    x == 0 on 30 %; 'p0' - a prior with zeros on 30 %; 'nonfinite' - inf / nan planted in ay; 'none' - a zero prior."""
    v = value_sets(n)[values]
    rng = np.random.RandomState(7 * n + len(values) + len(elig))
    x = np.where(v != 0, v, np.float32(1.0)).astype(np.float32)
    ay = np.where(v != 0, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    prior = None
    if elig == 'x0':
        x[rng.rand(n) < 0.3] = 0.0
    elif elig == 'p0':
        prior = np.where(rng.rand(n) < 0.3, 0.0, rng.rand(n) + 0.01).astype(np.float32)
    elif elig == 'nonfinite':
        bad = rng.rand(n) < 0.2
        ay[bad] = np.where(rng.rand(int(bad.sum())) < 0.5, np.inf, np.nan)
    elif elig == 'none':
        prior = np.zeros(n, np.float32)
    return x, ay, prior


def absres_cases():
    out = [(n, False, values, elig) for n in SIZES for values in ('equal', 'ulp', 'exponents', 'subnormal', 'normal')
           for elig in ELIGIBILITY]
    out += [(n, off, values, elig) for n, off in LONG for values in ('ulp', 'normal', 'subnormal') for elig in ('plain', 'p0', 'x0')]
    return out


def hh_inputs(shape, variant):
    """(dat, ct, w or None): positive values around 60; 'zeros' - 10 % exact zeros; 'weight' - a map with zeros on 15 %;
    'ct' - values of both signs with zeros, read as CT; 'neg' - the same read as not CT (a negative voxel is out)."""
    rng = np.random.RandomState(sum(shape) + len(variant))
    dat = (60.0 + 9.0 * rng.standard_normal(shape)).astype(np.float32)
    ct, w = False, None
    if variant == 'zeros':
        dat[rng.rand(*shape) < 0.1] = 0.0
    elif variant == 'weight':
        w = np.where(rng.rand(*shape) < 0.15, 0.0, rng.rand(*shape) + 0.05).astype(np.float32)
    elif variant in ('ct', 'neg'):
        dat = (25.0 * rng.standard_normal(shape)).astype(np.float32)
        dat[rng.rand(*shape) < 0.05] = 0.0
        ct = variant == 'ct'
    return dat, ct, w


_KERNEL_CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.test_gpu_median import HH_CASES, HH_VARIANTS, absres_cases, absres_inputs, hh_inputs
from tests.test_gpu_voxel import HUBER_C, HUBER_SHAPES, huber_inputs
from unires_amd import _lib, stats
from unires_amd._lib import check
lib, out, res = _lib.load(), sys.argv[1], {}
dev = torch.device('cuda:0')
P = lambda t: None if t is None else t.data_ptr()


def put(a, off):
    """``a`` on the device, on a 16-byte boundary or (off) one float past one."""
    if a is None:
        return None
    buf = torch.zeros(a.size + 8, device=dev)
    t = buf[1:1 + a.size] if off else buf[4:4 + a.size]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() %% 16 == (4 if off else 0)
    return t


work = stats.median_work(dev)
work.fill_(-1)  # (the entry points clear it themselves)
for n, off, values, elig in absres_cases():
    x, ay, prior = (put(a, off) for a in absres_inputs(n, values, elig))
    key = 'absres/%%d/%%d/%%s/%%s' %% (n, off, values, elig)
    r0 = stats.median_absres(x, ay, prior, work=work).cpu().numpy()
    r1 = stats.median_absres(x, ay, prior).cpu().numpy()  # a second run, a fresh scratch: the same bits
    assert np.array_equal(r0.view(np.int64), r1.view(np.int64)), key
    res[key] = r0
for shape, axis in HH_CASES:
    for variant in HH_VARIANTS:
        dat, ct, w = hh_inputs(shape, variant)
        d = torch.from_numpy(dat).to(dev)
        g = None if w is None else torch.from_numpy(w).to(dev)
        key = 'hh/%%s/%%d/%%s' %% ('x'.join(map(str, shape)), axis, variant)
        r0 = stats.median_hh(d, axis, ct, g, work=work).cpu().numpy()
        r1 = stats.median_hh(d, axis, ct, g, work=work).cpu().numpy()
        assert np.array_equal(r0.view(np.int64), r1.view(np.int64)), key
        res[key] = r0
# argument checks: nothing is launched
out2 = torch.zeros(2, dtype=torch.float64, device=dev)
x = torch.ones(8, device=dev)
i3 = _lib.i3
assert lib.unires_median_absres(P(x), P(x), None, 2 ** 32, P(work), P(out2), None) == 3
assert lib.unires_median_absres(None, P(x), None, 8, P(work), P(out2), None) == 3
assert lib.unires_median_absres(P(x), P(x), None, 8, None, P(out2), None) == 3
assert lib.unires_median_absres(P(x), P(x), None, 8, P(work), None, None) == 3
assert lib.unires_median_hh(P(x), i3((2, 2, 2)), 3, 0, None, P(work), P(out2), None) == 3
assert lib.unires_median_hh(P(x), i3((2, 2, 2)), -1, 0, None, P(work), P(out2), None) == 3
assert lib.unires_median_hh(None, i3((2, 2, 2)), 0, 0, None, P(work), P(out2), None) == 3
assert lib.unires_median_hh(P(x), i3((2, 2, 2)), 0, 0, None, None, P(out2), None) == 3
assert lib.unires_median_hh(P(x), i3((65535, 65537, 2)), 2, 0, None, P(work), P(out2), None) == 3  # more than 2^32 - 1 cells
# the Huber rule with its threshold on the device
for shape in HUBER_SHAPES:
    x, ay, prior = (t.to(dev) for t in huber_inputs(shape))
    key = 'huber/' + 'x'.join(map(str, shape))
    scale = torch.tensor([HUBER_C, 123.0], dtype=torch.float64, device=dev)
    zero = torch.zeros(2, dtype=torch.float64, device=dev)
    for name, pr in (('plain', None), ('prior', prior)):
        want = torch.full(shape, float('nan'), device=dev)
        check(lib.unires_voxel_huber(P(x), P(ay), P(pr), HUBER_C, x.numel(), P(want), None))
        g = torch.full(shape, float('nan'), device=dev)
        check(lib.unires_voxel_huber_dev(P(x), P(ay), P(pr), P(scale), 1.0, x.numel(), P(g), None))
        torch.cuda.synchronize()
        res[key + '/' + name], res[key + '/' + name + '/want'] = g.cpu().numpy(), want.cpu().numpy()
        g = torch.full(shape, float('nan'), device=dev)
        check(lib.unires_voxel_huber_dev(P(x), P(ay), P(pr), P(zero), 1.0, x.numel(), P(g), None))
        res[key + '/' + name + '/c0'] = g.cpu().numpy()
    g = prior.clone()  # in place on the prior
    check(lib.unires_voxel_huber_dev(P(x), P(ay), P(g), P(scale), 1.0, x.numel(), P(g), None))
    res[key + '/inplace'] = g.cpu().numpy()
    g = prior.clone()
    check(lib.unires_voxel_huber_dev(P(x), P(ay), P(g), P(zero), 1.0, x.numel(), P(g), None))
    res[key + '/inplace/c0'] = g.cpu().numpy()
    # a multiplier: c = fl32(mult (float) scale)
    g = torch.full(shape, float('nan'), device=dev)
    check(lib.unires_voxel_huber_dev(P(x), P(ay), P(prior), P(scale), 0.7, x.numel(), P(g), None))
    res[key + '/mult'] = g.cpu().numpy()
    assert lib.unires_voxel_huber_dev(P(x), P(ay), None, P(scale), 0.0, x.numel(), P(g), None) == 3
    assert lib.unires_voxel_huber_dev(P(x), P(ay), None, None, 1.0, x.numel(), P(g), None) == 1
torch.cuda.synchronize()
np.savez(out, **res)
'''


@pytest.fixture(scope='module')
def kernels(dev, tmp_path_factory):
    return _run(tmp_path_factory.mktemp('median_kernels'), 'kernels', _KERNEL_CHILD % dict(root=ROOT))


def _same(got, want, key):
    med, N = want
    assert got.shape == (2,) and got[1] == float(N), (key, 'N', got, want)
    assert got[0] == float(np.float32(got[0])), (key, 'the median is not a float32 value')
    assert bits(got[0]) == bits(med), (key, 'median', got, want)


@pytest.mark.parametrize('n', SIZES + tuple(sorted({n for n, _ in LONG})))
def test_median_absres_bit_for_bit(kernels, n):
    """Every value set and eligibility case at this n: the median's bits and N exact; two runs the same bits (asserted
    in the child).  Nothing eligible gives (0, 0)."""
    cases = [c for c in absres_cases() if c[0] == n]
    assert cases
    decided = 0
    for _, off, values, elig in cases:
        x, ay, prior = absres_inputs(n, values, elig)
        want = M.median_absres(x, ay, prior)
        key = 'absres/%d/%d/%s/%s' % (n, off, values, elig)
        _same(kernels[key], want, key)
        if elig == 'none':
            assert want == (0.0, 0) and kernels[key][0] == 0.0
        decided += want[1] > 0
    assert decided >= len(cases) // 2


@pytest.mark.parametrize('shape, axis', HH_CASES)
def test_median_hh_bit_for_bit(kernels, shape, axis):
    cells = int(np.prod([s - (a != axis) for a, s in enumerate(shape)]))
    for variant in HH_VARIANTS:
        dat, ct, w = hh_inputs(shape, variant)
        want = M.median_hh(dat, axis, ct, w)
        key = 'hh/%s/%d/%s' % ('x'.join(map(str, shape)), axis, variant)
        _same(kernels[key], want, key)
        if variant == 'plain':
            assert want[1] == cells, (key, 'every cell is complete')
        elif cells >= 24 and variant in ('zeros', 'weight'):
            assert 0 < want[1] < cells, (key, 'planted voxels remove cells')
    if cells == 0:
        assert all(kernels['hh/%s/%d/%s' % ('x'.join(map(str, shape)), axis, v)].tolist() == [0.0, 0.0] for v in HH_VARIANTS)


@pytest.mark.parametrize('shape', HUBER_SHAPES)
def test_huber_rule_with_the_threshold_on_the_device(kernels, shape):
    """scale_dev = [c], mult = 1: the bits of unires_voxel_huber(c) - and of tests/voxel64.huber64 - without and with a
    prior and in place; c == 0: the prior (ones without one); mult = 0.7: the rule at fl32(0.7f (float) c)."""
    from tests import voxel64
    x, ay, prior = (t.numpy() for t in huber_inputs(shape))
    key = 'huber/' + 'x'.join(map(str, shape))
    for name, pr in (('plain', None), ('prior', prior)):
        assert np.array_equal(bits(kernels[key + '/' + name]), bits(kernels[key + '/' + name + '/want'])), (key, name)
        assert np.array_equal(bits(kernels[key + '/' + name]), bits(voxel64.huber64(x, ay, pr, HUBER_C))), (key, name)
        assert np.array_equal(bits(kernels[key + '/' + name + '/c0']), bits(np.ones(shape, np.float32) if pr is None else pr))
    assert np.array_equal(bits(kernels[key + '/inplace']), bits(voxel64.huber64(x, ay, prior, HUBER_C))), key
    assert np.array_equal(bits(kernels[key + '/inplace/c0']), bits(prior)), key
    c = np.float32(np.float32(0.7) * np.float32(HUBER_C))
    assert np.array_equal(bits(kernels[key + '/mult']), bits(voxel64.huber64(x, ay, prior, c))), key


# ---- (2) init() ---------------------------------------------------------------------------------------------------------
PHANTOM_MAT = np.diag([1.0, 1.0, 3.0, 1.0])  # thick along z: the Haar detail is taken in the (x, y) planes


def _hyper(dat, dev, mat=PHANTOM_MAT, weight=None, **fields):
    import unires_amd as U
    xn = U._input(torch.from_numpy(dat).to(dev), torch.from_numpy(np.asarray(mat, np.float64)))
    xn.weight = None if weight is None else torch.from_numpy(weight).to(dev)
    sett = U.settings()
    for k, v in fields.items():
        if v is None:
            delattr(sett, k)
        else:
            setattr(sett, k, v)
    U._estimate_hyperpar([[xn]], sett)
    return xn


def _check_mad(xn, dat, axis, ct=False, w=None):
    med, N = M.median_hh(dat, axis, ct, w)
    sd = M.sd_of(med)
    assert N > 0 and xn.sd.dtype == torch.float32 and not xn.sd.is_cuda
    assert bits(float(xn.sd)) == bits(sd), (float(xn.sd), sd)
    assert bits(float(xn.tau)) == bits(M.tau_of(sd)), (float(xn.tau), M.tau_of(sd))
    mu = M.mu_of(dat, ct, w)
    assert abs(float(xn.mu) - mu) <= 1e-6 * mu, (float(xn.mu), mu)
    return float(sd)


def test_init_with_the_mad_noise_estimate(dev):
    """init() on the background-free phantom with noise_est = 'mad': sd and tau bit for bit and mu to 1e-6 against the
    restatement, sd within 15 % of the planted 20 where the mixture rule (the default, and 'mixture' set by name: the
    bits of a settings object without the field) is off by more than a factor of 2.  The thick axis comes from the
    observation's affine.  With voxel_init and a map: the restatement with the map.  A noise-free volume is a ValueError."""
    import unires_amd as U
    dat = M.phantom(20.0)
    sett = U.settings()
    sett.device, sett.max_iter, sett.vx, sett.write_out, sett.noise_est = dev, 3, 0, False, 'mad'
    x, _, _ = U.init([[torch.from_numpy(dat).to(dev), torch.from_numpy(PHANTOM_MAT)]], sett)
    sd = _check_mad(x[0][0], dat, 2)
    assert abs(sd - 20.0) <= 0.15 * 20.0
    # stats.estimate_noise_mad, the call for one volume: (sd, N) of the restatement, with and without a map
    from unires_amd import stats
    wmap = np.ones(dat.shape, np.float32)
    wmap[5:20, :, 8:30] = 0.0
    for w in (None, wmap):
        got_sd, got_n = stats.estimate_noise_mad(torch.from_numpy(dat).to(dev), 2, False,
                                                 None if w is None else torch.from_numpy(w).to(dev))
        med, N = M.median_hh(dat, 2, False, w)
        assert got_n == N and got_sd.dtype == torch.float32 and not got_sd.is_cuda
        assert bits(float(got_sd)) == bits(M.sd_of(med)), (float(got_sd), M.sd_of(med))
    default, named = _hyper(dat, dev, noise_est=None), _hyper(dat, dev, noise_est='mixture')
    for f in ('sd', 'tau', 'mu'):
        assert bits(float(getattr(default, f))) == bits(float(getattr(named, f))), f
    print("init() sd: planted 20, 'mad' %.3f, 'mixture' %.3f" % (sd, float(default.sd)), flush=True)
    assert float(default.sd) > 2.0 * 20.0
    # the thick axis from the affine: the first of the largest voxel sizes
    for mat, axis in ((np.diag([3.0, 1.0, 1.0, 1.0]), 0), (np.diag([1.0, 2.0, 1.0, 1.0]), 1), (np.eye(4), 0)):
        _check_mad(_hyper(dat, dev, mat=mat, noise_est='mad'), dat, axis)
    # a weight map: ignored without voxel_init, the restatement's with it
    w = np.ones(dat.shape, np.float32)
    w[10:30, 12:36, :] = 0.0
    _check_mad(_hyper(dat, dev, weight=w, noise_est='mad'), dat, 2)
    got = _check_mad(_hyper(dat, dev, weight=w, noise_est='mad', voxel_init=True), dat, 2, w=w)
    assert got != sd
    # CT: negative voxels count
    ct = (dat - 300.0 * (dat != 0)).astype(np.float32)
    xn = U._input(torch.from_numpy(ct).to(dev), torch.from_numpy(PHANTOM_MAT))
    xn.ct = True
    sett = U.settings()
    sett.noise_est = 'mad'
    U._estimate_hyperpar([[xn]], sett)
    _check_mad(xn, ct, 2, ct=True)
    # nothing to estimate from
    flat = np.where(dat != 0, np.float32(100.0), np.float32(0.0)).astype(np.float32)
    with pytest.raises(ValueError, match='channel 0, repeat 0.*zero median'):
        _hyper(flat, dev, noise_est='mad')
    with pytest.raises(ValueError, match='channel 0, repeat 0.*no 2 x 2'):
        _hyper(np.zeros((8, 8, 8), np.float32), dev, noise_est='mad')
    sett = U.settings()
    sett.device, sett.noise_est = dev, 'median'
    with pytest.raises(ValueError, match='noise_est'):
        U.init([[torch.from_numpy(dat).to(dev), torch.from_numpy(PHANTOM_MAT)]], sett)


# ---- (3) fit() ----------------------------------------------------------------------------------------------------------
def _fit(dev, n_iter, **fields):
    """tests/test_gpu_voxel.py's robust arm: the 48 x 48 x 40 phantom, two repeats with 3 mm slices, a box of the second
    repeat's voxels raised by 20 noise standard deviations, sett.voxel_robust."""
    import unires_amd as U
    from tests.test_gpu_slice import _phantom
    _, (xg, yg, sett) = _phantom(dev, NOISE_SD)
    xg[0][1].dat[BOX] += 20.0 * NOISE_SD
    yg[0].lam0 = float(yg[0].lam) / 4.0
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = n_iter, 1e-4, 4.0, 0
    sett.cgs_max_iter, sett.cgs_tol = 20, 0.0
    sett.clean_fov = False
    sett.voxel_robust = True
    for k, v in fields.items():
        if v is None:
            if hasattr(sett, k):
                delattr(sett, k)
        else:
            setattr(sett, k, v)
    dat, _, _, info = U.fit(xg, yg, sett)
    torch.cuda.synchronize()
    assert info['n_iter'] == n_iter
    return dat[..., 0].cpu(), info, (xg, yg, sett)


def _restated_weights(structs, n):
    """(weights, 1.4826 med, N) the restated chain gives repeat n from the A y of the fit's last iterate."""
    import unires_amd as U
    from tests import voxel64
    xg, yg, sett = structs
    Ay = U._proj('A', yg[0].dat, xg[0], yg[0], n=n, method=sett.method, do=sett.do_proj).cpu().numpy()
    x = xg[0][n].dat.cpu().numpy()
    med, N = M.median_absres(x, Ay)
    return voxel64.huber64(x, Ay, None, M.threshold(med, sett.voxel_k)), np.float32(M.MAD_TO_SD * med), N


def test_fit_with_the_mad_scale_after_one_iteration(dev):
    """One ADMM iteration: each repeat's weights are the Huber rule at c = fl32(fl32(k) 1.4826) median|x - A y| of the
    restatement, bit for bit, and info['voxel_scale'] is fl32(1.4826 med), a float32 CPU scalar."""
    _, info, structs = _fit(dev, 1, voxel_scale='mad')
    assert len(info['voxel_scale']) == 1 and len(info['voxel_scale'][0]) == 2
    for n in range(2):
        want, scale, N = _restated_weights(structs, n)
        got = info['voxel_w'][0][n].cpu().numpy()
        assert N == int((structs[0][0][n].dat != 0).sum()) > 0 and (want < 1.0).any() and (want == 1.0).any()
        assert np.array_equal(bits(got), bits(want)), (n, int((bits(got) != bits(want)).sum()))
        s = info['voxel_scale'][0][n]
        assert torch.is_tensor(s) and s.dtype == torch.float32 and not s.is_cuda and s.dim() == 0
        assert bits(float(s)) == bits(scale), (n, float(s), scale)
        print('one iteration, repeat %d: scale %.4f (noise sd %.4f)' % (n, float(s), float(structs[0][0][n].tau) ** -0.5), flush=True)


def test_fit_with_the_mad_scale_rejects_the_planted_box(dev):
    """The full fit (12 ADMM iterations), twice: the same bits; the mean weight inside the planted box is below 1/2, at
    least 95 % of the voxels outside it have weight exactly 1 (k = 3 and Gaussian residuals: 99.7 %; the cap leaves room
    for edges) - of the restated chain too, whose bits the weights are."""
    dat, info, structs = _fit(dev, 12, voxel_scale='mad')
    dat2, info2, _ = _fit(dev, 12, voxel_scale='mad')
    assert torch.equal(dat.view(torch.int32), dat2.view(torch.int32))
    planted = np.zeros((48, 16, 40), bool)
    planted[BOX] = True
    for n in range(2):
        got = info['voxel_w'][0][n].cpu().numpy()
        assert np.array_equal(bits(got), bits(info2['voxel_w'][0][n].cpu().numpy())), n
        assert bits(float(info['voxel_scale'][0][n])) == bits(float(info2['voxel_scale'][0][n])), n
        want, scale, _ = _restated_weights(structs, n)
        assert np.array_equal(bits(got), bits(want)), n
        assert bits(float(info['voxel_scale'][0][n])) == bits(scale), n
        clean = ~planted if n == 1 else np.ones(got.shape, bool)
        share, share_want = float((got[clean] == 1.0).mean()), float((want[clean] == 1.0).mean())
        print('full fit, repeat %d: scale %.4f, weight exactly 1 on %.4f of the clean voxels (restated %.4f)'
              % (n, float(info['voxel_scale'][0][n]), share, share_want), flush=True)
        assert share_want >= 0.95 and share >= 0.95
    inside = float(info['voxel_w'][0][1].cpu().numpy()[planted].mean())
    print('  mean weight inside the planted box %.4f' % inside, flush=True)
    assert inside < 0.5


def test_fit_with_the_noise_scale_is_the_fit_without_the_field(dev):
    """voxel_scale = 'noise' against a settings object that has no such field: the reconstruction's and the weights' bits,
    and info['voxel_scale'] all None; a name that is not built is refused."""
    import unires_amd as U
    dat, info, structs = _fit(dev, 3, voxel_scale='noise')
    dat0, info0, _ = _fit(dev, 3, voxel_scale=None)
    assert torch.equal(dat.view(torch.int32), dat0.view(torch.int32))
    for n in range(2):
        assert torch.equal(info['voxel_w'][0][n].view(torch.int32), info0['voxel_w'][0][n].view(torch.int32))
    assert info['voxel_scale'] == [[None, None]] and info0['voxel_scale'] == [[None, None]]
    mad, _, _ = _fit(dev, 3, voxel_scale='mad')
    assert not torch.equal(mad, dat)
    xg, yg, sett = structs
    sett.voxel_scale = 'sigma'
    with pytest.raises(ValueError, match='voxel_scale'):
        U.fit(xg, yg, sett)
