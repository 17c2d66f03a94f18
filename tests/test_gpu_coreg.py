"""Coregistration on the GPU: quantisation and joint histograms bit for bit against the
NumPy restatement, costs to 1e-12, the same Powell search from GPU and restatement costs, planted
rigid misalignments recovered by _init_reg, and an end-to-end fit()."""
import numpy as np
import pytest
import torch

from tests import coreg_phantom as P
from tests import coreg_restated as R

pytestmark = pytest.mark.gpu


def _vol(shape, seed, smooth=True):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g) * 1000.0
    if smooth:
        v = torch.nn.functional.avg_pool3d(v[None, None], 3, 1, 1)[0, 0]
    return v.contiguous()


def _u8(shape, seed, dev):
    u = R.quantise(_vol(shape, seed).numpy())[0]
    return u, torch.from_numpy(u).to(dev)


def test_quantisation_bit_for_bit(dev):
    from unires_amd import preproc
    vols = [_vol((37, 41, 29), 1), _vol((64, 64, 64), 2, smooth=False), _vol((40, 33, 9), 3)]
    vols[0][0, 0, :3] = 5e5
    vols[1][1, 2, 3], vols[1][4, 5, 6], vols[1][7, 8, 9] = float('nan'), float('inf'), -float('inf')
    vols[2][:, :, 0] = -200.0
    outs, counts, params = preproc.coreg_quantise([v.to(dev) for v in vols])
    for v, u, c, prm in zip(vols, outs, counts.cpu().numpy(), params.cpu().numpy()):
        ru, rc, (mn, mxa, mx, scale) = R.quantise(v.numpy())
        assert u.cpu().numpy().tobytes() == ru.tobytes()
        assert (c.astype(np.int64) == rc).all()
        assert np.float32(prm[0]) == mn and np.float32(prm[1]) == mxa and np.float32(prm[2]) == mx
        assert np.float32(prm[3]) == scale and prm[4] == 0


def test_quantisation_errors(dev):
    from unires_amd import preproc
    with pytest.raises(ValueError, match='constant'):
        preproc.coreg_quantise([_vol((8, 8, 8), 1).to(dev), torch.full((8, 8, 8), 7.0, device=dev)])
    with pytest.raises(ValueError, match='no finite'):
        preproc.coreg_quantise([torch.full((8, 8, 8), float('nan'), device=dev)])


def _rot(a, b, c):
    from unires_amd._rigid import _expm, affine_basis
    return _expm(np.array([0, 0, 0, a, b, c]), affine_basis()).numpy()


def _cases(dev):
    Gn, G = _u8((40, 36, 32), 11, dev)
    Fn, F = _u8((38, 40, 30), 12, dev)
    Tn, T = _u8((40, 36, 8), 13, dev)        # thick along z
    I = np.eye(4)
    sh = np.eye(4)
    sh[:3, 3] = [0.37, -0.61, 0.25]
    rot = _rot(0.05, -0.03, 0.08)
    rot[:3, 3] = [1.0, -2.0, 0.5]
    thick = np.diag([1.0, 1.0, 0.25, 1.0])    # G voxel (z at 1) -> thick voxel (z at 4)
    edge = np.eye(4)
    edge[:3, 3] = [-2.0, 4.0, -2.0]           # puts G's faces on F's
    m = lambda a: a[:3, :].astype(np.float32).reshape(-1)  # noqa: E731
    one = np.ones(3, np.float32)
    # a large zero background (the (0, 0) / (0, 1) register counters): the volumes zero-padded
    Zg, Zf = np.zeros((48, 44, 40), np.uint8), np.zeros((46, 48, 38), np.uint8)
    Zg[4:44, 4:40, 4:36] = Gn
    Zf[4:42, 4:44, 4:34] = Fn
    Zg[Zg == 1] = 0
    return [
        ('zero_background', (Zg, torch.from_numpy(Zg).to(dev)), (Zf, torch.from_numpy(Zf).to(dev)), m(sh), one),
        ('identity', (Gn, G), (Fn, F), m(I), one),
        ('subvoxel_shift', (Gn, G), (Fn, F), m(sh), one),
        ('rotation', (Gn, G), (Fn, F), m(rot), np.array([1.5, 1.5, 1.5], np.float32)),
        ('thick_moving', (Gn, G), (Tn, T), m(thick @ rot), one),
        ('thick_fixed_step_below_1', (Tn, T), (Fn, F), m(np.linalg.inv(thick)), np.array([1, 1, 0.25], np.float32)),
        ('step_below_1', (Gn, G), (Fn, F), m(sh), np.array([0.5, 0.75, 0.6], np.float32)),
        ('fov_edge', (Gn, G), (Fn, F), m(edge), one),
    ]


def test_histograms_bit_for_bit_and_batched(dev):
    from unires_amd import preproc
    cases = _cases(dev)
    jobs = [(g[1], f[1], M, s) for _, g, f, M, s in cases]
    batched = preproc.coreg_hist(jobs).cpu().numpy()
    for k, (name, g, f, M, s) in enumerate(cases):
        ref = R.hist(g[0], f[0], M, s)
        one = preproc.coreg_hist([jobs[k]]).cpu().numpy()[0]
        assert one.astype(np.uint64).tobytes() == ref.tobytes(), name
        assert batched[k].tobytes() == one.tobytes(), name
        assert ref.sum() % 65536 == 0 and ref.sum() > 0, name
        if name == 'zero_background':
            assert ref[0, 0] > ref.sum() // 4 and ref[0, 1] > 0


def test_histogram_counts_every_point_once(dev):
    from unires_amd import preproc
    _, G = _u8((50, 50, 50), 3, dev)
    h = preproc.coreg_hist([(G, G, np.eye(4)[:3].astype(np.float32).reshape(-1), np.ones(3, np.float32))])
    # identity map, step 1: every jittered point of the 50^3 grid inside [0, 49] is kept
    T = R.jitter_table()
    p = np.arange(50 ** 3)
    inside = np.ones(p.shape, bool)
    for d in range(3):
        i = [p // 2500, (p // 50) % 50, p % 50][d]
        inside &= (i.astype(np.float32) + T[(3 * (p % 97) + d) % 97]) <= 49
    assert int(h.sum()) == int(inside.sum()) * 65536


@pytest.mark.parametrize('cost_fun', ['nmi', 'mi', 'ecc'])
def test_costs_match_restatement(dev, cost_fun):
    from unires_amd import preproc
    cases = _cases(dev)
    jobs = [(g[1], f[1], M, s) for _, g, f, M, s in cases]
    H = preproc.coreg_hist(jobs)
    for fwhm in (7.0, 0.0, 2.3):
        got = preproc.coreg_cost(H, cost_fun, fwhm).cpu().numpy()
        for k in range(len(cases)):
            want = R.cost(H[k].cpu().numpy(), cost_fun, fwhm)
            assert abs(got[k] - want) <= 1e-12 * abs(want), (cases[k][0], fwhm, got[k], want)
    with pytest.raises(NotImplementedError):
        preproc.coreg_cost(H, 'njtv')


def _pair(dev, dim=(48, 48, 48), vx=(3.0, 3.0, 3.0), seed=0):
    g, mg = P.observation(dim, vx, 0, 1, dev)
    f, mf = P.observation(dim, vx, 1, 2, dev)
    Pl = P.random_rigid(np.random.default_rng(seed))
    return [[g, torch.from_numpy(mg)], [f, torch.from_numpy(Pl @ mf)]], Pl, mf


def test_same_search_from_gpu_and_restatement_costs(dev):
    from unires_amd import preproc
    from unires_amd._rigid import _expm, affine_basis
    from unires_amd.spatial import _m12
    imgs, Pl, mf = _pair(dev)
    q, mat_a = preproc.affine_align(imgs, samp=3, device=dev)
    G = R.quantise(imgs[0][0].cpu().numpy())[0]
    F = R.quantise(imgs[1][0].cpu().numpy())[0]
    B = affine_basis()
    step = np.ones(3, np.float32)

    def ev(reqs):
        return [R.cost(R.hist(G, F, _m12(preproc.voxel_map(x, B, imgs[1][1].numpy(), imgs[0][1].numpy())), step))
                for _, x in reqs]
    (res,), _ = preproc.lockstep([preproc.powell(np.zeros(6))], ev)
    ref = _expm(res[0], B)
    assert torch.allclose(mat_a[1], ref, atol=1e-6, rtol=0), (mat_a[1], ref)
    assert torch.equal(mat_a[0], torch.eye(4, dtype=torch.float64))
    assert P.rms_mm(np.linalg.solve(mat_a[1].numpy(), imgs[1][1].numpy()), mf, (48, 48, 48)) < 0.3


def _subject(dev, dim, vx, thick_axes, trans, rot, seed, scale=1.0, **kw):
    """Three contrasts of one anatomy; observation i is thick (4 mm) along thick_axes[i] (None: not);
    every observation but the first carries a planted rigid in its header."""
    import unires_amd as U
    rng = np.random.default_rng(seed)
    x, truth = [], []
    for c, ax in enumerate(thick_axes):
        v = list(vx)
        d = list(dim)
        if ax is not None:
            v[ax] = 4.0
            d[ax] = int(round(dim[ax] * vx[ax] / 4.0))
        dat, mat = P.observation(tuple(d), tuple(v), c, 100 + seed + c, dev, sub_axis=ax, scale=scale, **kw)
        Pl = np.eye(4) if c == 0 else P.random_rigid(rng, trans, rot)
        xn = U._input(dat, torch.from_numpy(Pl @ mat))
        x.append([xn])
        truth.append((mat, tuple(d)))
    return x, truth


def _recover(dev, dim, vx, thick_axes, trans, rot, seed, scale=1.0, coreg_params=None, **kw):
    import unires_amd as U
    x, truth = _subject(dev, dim, vx, thick_axes, trans, rot, seed, scale, **kw)
    sett = U.settings()
    sett.device = dev
    if coreg_params:
        sett.coreg_params = dict(sett.coreg_params, **coreg_params)
    U._init_reg(x, sett)
    errs = [P.rms_mm(x[c][0].mat.cpu().numpy(), truth[c][0], truth[c][1], scale=scale) for c in range(len(x))]
    return errs, sett, x


def _check(errs, thick_axes):
    assert errs[0] == 0.0
    for e, ax in zip(errs[1:], thick_axes[1:]):
        assert e <= (0.5 if ax is not None else 0.3), errs


@pytest.mark.parametrize('seed', [0, 1])
def test_init_reg_recovers_planted_rigids_96(dev, seed):
    axes = (None, None, 2)
    errs, sett, x = _recover(dev, (96, 96, 96), (1.0, 1.0, 1.0), axes, 5.0, 0.1, seed, scale=0.6)
    _check(errs, axes)
    assert sett.mat_coreg.shape == (3, 4, 4) and sett.mat_coreg.dtype == torch.float64
    assert all(torch.equal(xn.rigid_q.cpu(), torch.zeros(6, dtype=torch.float64)) for xc in x for xn in xc)


def test_init_reg_recovers_demo_sized_misalignment_96(dev):
    # the demo's +-10 mm / +-0.2 rad, default parameters (samp = 1)
    axes = (None, None, 2)
    errs, _, _ = _recover(dev, (96, 96, 96), (1.0, 1.0, 1.0), axes, 10.0, 0.2, 5, scale=0.6)
    _check(errs, axes)


@pytest.mark.parametrize('axes', [(2, None, 1), (0, 1, 2)])
def test_init_reg_recovers_with_a_thick_fixed_image_96(dev, axes):
    # the fixed image in 4 mm slices: sampling steps below one voxel along its thick axis
    errs, _, _ = _recover(dev, (96, 96, 96), (1.0, 1.0, 1.0), axes, 5.0, 0.1, 0, scale=0.6)
    _check(errs, axes)


@pytest.mark.slow
@pytest.mark.parametrize('axes', [(None, None, 2), (0, 1, 2)])
def test_init_reg_recovers_planted_rigids_demo_shape(dev, axes):
    # 181 x 217 x 181: one observation in 4 mm slices, and the demo's 4 mm slices along x, y and z
    errs, _, _ = _recover(dev, (181, 217, 181), (1.0, 1.0, 1.0), axes, 5.0, 0.1, 3)
    _check(errs, axes)


def test_reproducible(dev):
    from unires_amd import preproc
    imgs, _, _ = _pair(dev, seed=4)
    a = preproc.affine_align(imgs, samp=3, device=dev)[1]
    b = preproc.affine_align(imgs, samp=3, device=dev)[1]
    assert a.numpy().tobytes() == b.numpy().tobytes()


def test_coarse_to_fine_levels(dev):
    from unires_amd import preproc
    imgs, Pl, mf = _pair(dev, dim=(64, 64, 64), vx=(2.0, 2.0, 2.0), seed=6)
    _, mat_a = preproc.affine_align(imgs, samp=(6, 4, 2), device=dev)
    assert P.rms_mm(np.linalg.solve(mat_a[1].numpy(), imgs[1][1].numpy()), mf, (64, 64, 64)) < 0.5


def test_end_to_end_read_estimate_coreg_fit(dev):
    import unires_amd as U
    dim_y, vx_y = (64, 64, 64), (1.0, 1.0, 1.0)
    scale = 0.4
    obs, truth_y = [], []
    rng = np.random.default_rng(9)
    for c, ax in enumerate((None, 2)):
        v = [1.0, 1.0, 1.0]
        d = list(dim_y)
        if ax is not None:
            v[ax], d[ax] = 3.0, dim_y[ax] // 3
        dat, mat = P.observation(tuple(d), tuple(v), c, 40 + c, dev, sub_axis=ax, sub=3, scale=scale)
        Pl = np.eye(4) if c == 0 else P.random_rigid(rng)
        obs.append((dat.cpu(), Pl @ mat, mat))
        truth_y.append(P.observation(dim_y, vx_y, c, 0, dev, noise=0.0, scale=scale)[0])
    mat_y = torch.from_numpy(P.true_mat(dim_y, vx_y))

    def run(which):
        x = []
        for dat, mat_given, mat_true in obs:
            dat, dim, mat, _, _, _, _, ct = U._read_image([dat, mat_true if which == 'true' else mat_given], device=dev)
            xn = U._input(dat, mat)
            xn.ct = ct
            x.append([xn])
        sett = U.settings()
        sett.device, sett.method, sett.do_proj = dev, 'super-resolution', True
        U._estimate_hyperpar(x, sett)
        sett.do_coreg = which == 'coreg'
        U._init_reg(x, sett)
        for xc in x:
            xc[0].po = U._proj_info(dim_y, mat_y, xc[0].dim, xc[0].mat, device=dev)
        y = [U._output(torch.zeros(dim_y, device=dev), mat_y) for _ in x]
        U._init_y_dat(x, y, sett)
        U._init_lam(x, y, sett)
        sett.max_iter, sett.sched_num = 8, 1
        dat_y, _, _, _ = U.fit(x, y, sett)
        return float((dat_y[..., 1].reshape(dim_y) - truth_y[1]).norm() / truth_y[1].norm())
    e_none, e_coreg, e_true = run('none'), run('coreg'), run('true')
    assert e_coreg < 0.7 * e_none, (e_none, e_coreg, e_true)
    assert e_coreg < 1.1 * e_true, (e_none, e_coreg, e_true)
