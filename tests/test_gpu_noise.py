"""The noise / intensity hyper-parameter estimator on the GPU (noise.hip: k_noise_range, k_noise_hist,
k_noise_fit) against its float64 restatement (tests/noise_restated.py): histograms bit for
bit, fits to 1e-6 at the GPU's own M-step count, batching, recovery of planted noise, errors, and the
path _read_image -> _estimate_hyperpar -> _init_lam -> fit()."""
import math

import numpy as np
import pytest
import torch

from tests import noise_restated as R

pytestmark = pytest.mark.gpu
SD = 75.0


def _gpu_hist(vols, cts, dev):
    from unires_amd import stats as S
    counts, rng = S.noise_hist([torch.as_tensor(v).to(dev) for v in vols], cts)
    return counts.cpu().numpy().astype(np.int64), rng.cpu().numpy()


def _check_hist(vols, cts, dev):
    counts, rng = _gpu_hist(vols, cts, dev)
    for o, (v, ct) in enumerate(zip(vols, cts)):
        want, (mn, mx) = R.histogram(torch.as_tensor(v).cpu().numpy(), ct)
        assert rng[o, 0].tobytes() == np.float32(mn).tobytes(), o
        assert rng[o, 1].tobytes() == np.float32(mx).tobytes(), o
        if want is None:
            assert not counts[o].any()
        else:
            np.testing.assert_array_equal(counts[o], want, err_msg='observation %d' % o)
    return counts, rng


def _messy(shape, seed):
    """Gaussian values around 0 with NaN, +-Inf, +-0 and repeated values sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g) * 100.0
    flat = v.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)
    k = max(flat.numel() // 50, 1)
    flat[idx[:k]] = float('nan')
    flat[idx[k:2 * k]] = float('inf')
    flat[idx[2 * k:3 * k]] = -float('inf')
    flat[idx[3 * k:4 * k]] = 0.0
    flat[idx[4 * k:5 * k]] = -0.0
    flat[idx[5 * k:6 * k]] = 17.25
    return v


@pytest.mark.parametrize('ct', [False, True])
def test_histogram_odd_sizes_and_special_values(dev, ct):
    shapes = [(7,), (1023,), (1025,), (12345,), (37, 41, 43), (3, 1, 5)]
    vols = [_messy(s, i) for i, s in enumerate(shapes)]
    _check_hist(vols, [ct] * len(vols), dev)


def test_histogram_unaligned_start(dev):
    v = _messy((64, 33, 17), 5).view(-1).to(dev)  # sliced on the device: starts off 16-byte alignment
    _check_hist([v[1:], v[2:-3], v[3:]], [False, True, False], dev)


def test_histogram_values_on_bin_edges(dev):
    # mn = 1, mx = 5: every 1 + 4 k / 1024 is a bin edge, exact in float32; mx lands in the last bin
    edges = (1.0 + 4.0 * torch.arange(1025, dtype=torch.float64) / 1024).float()
    v = torch.cat([edges, edges[::3], torch.tensor([5.0, 5.0, 1.0])])
    counts, _ = _check_hist([v], [False], dev)
    assert counts[0, 1023] == 5  # k = 1023, 1024, 1023 again, and the two extra 5.0s


def test_histogram_thick_slice_and_256_cubed(dev):
    g = torch.Generator().manual_seed(7)
    thick = (torch.randn((256, 256, 43), generator=g) * SD + 500.0).abs()
    big = torch.randn((256, 256, 256), generator=g) * SD
    big[64:192, 64:192, 64:192] += 1000.0
    big = big.abs()
    big[:8] = 0.0
    _check_hist([thick, big], [False, False], dev)


def test_histogram_empty_and_constant(dev):
    from unires_amd import stats as S
    vols = [torch.zeros(100), torch.full((50,), 3.0), torch.full((50,), -2.0), torch.full((9,), float('nan'))]
    counts, rng = _check_hist(vols, [False, False, False, True], dev)
    out = S.noise_fit(torch.as_tensor(counts, dtype=torch.int32).to(dev), torch.as_tensor(rng).to(dev)).cpu()
    assert (out[:, S.MODEL] == -1).all()


# ---- fit ------------------------------------------------------------------------------------------------
def _rician(shape, seed, nu=1000.0, frac=0.4):
    g = torch.Generator().manual_seed(seed)
    loc = torch.where(torch.rand(shape, generator=g) < frac, nu, 0.0)
    re, im = torch.randn(shape, generator=g) * SD, torch.randn(shape, generator=g) * SD
    return torch.sqrt((loc + re) ** 2 + im ** 2)


def _ct(shape, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.where(torch.rand(shape, generator=g) < 0.5, -1000.0, 40.0)
    return v + torch.randn(shape, generator=g) * 20.0


def _close(a, b, scale, rel=1e-6):
    return abs(a - b) <= rel * max(abs(b), scale)


def _check_fit(row, counts, mn, mx):
    from unires_amd import stats as S
    free = R.fit(counts, mn, mx)
    n = int(row[S.ITERS])
    assert abs(free['iters'] - n) <= 1, (free['iters'], n)
    r = R.fit(counts, mn, mx, max_iter=n, stop=False)
    scale = float(np.max(r['sig']))
    assert int(row[S.MODEL]) == int(r['gmm'])
    for k in range(2):
        assert _close(row[S.MG + k], r['mg'][k], 0.0)
        assert _close(row[S.LOC + k], r['loc'][k], scale)
        assert _close(row[S.SIG + k], r['sig'][k], 0.0)
        assert _close(row[S.MEAN + k], r['mean'][k], scale)
    assert _close(row[S.SD], r['sd'], 0.0) and _close(row[S.MU], r['mu'], 0.0)
    assert row[S.SUMH] == counts.sum()
    return r


@pytest.mark.parametrize('kind', ['rice', 'rice_low_snr', 'gauss'])
def test_fit_matches_restatement_at_the_gpu_iteration_count(dev, kind):
    from unires_amd import stats as S
    vol = {'rice': lambda: _rician((100, 100, 100), 1),
           'rice_low_snr': lambda: _rician((100, 100, 100), 2, nu=150.0, frac=0.7),
           'gauss': lambda: _ct((100, 100, 100), 3)}[kind]()
    ct = kind == 'gauss'
    counts, rng = _gpu_hist([vol], [ct], dev)
    out = S.noise_fit(torch.as_tensor(counts, dtype=torch.int32).to(dev), torch.as_tensor(rng).to(dev)).cpu().numpy()
    r = _check_fit(out[0], counts[0], rng[0, 0], rng[0, 1])
    assert r['gmm'] == ct


def _subject(dev):
    import unires_amd as U
    shapes = [[(60, 64, 20), (64, 20, 60)], [(50, 50, 50), (33, 47, 29)], [(40, 40, 16), (48, 40, 12)]]
    x = []
    for c, shp in enumerate(shapes):
        xc = []
        for n, s in enumerate(shp):
            dat = _ct(s, 10 * c + n) if (c, n) == (2, 1) else _rician(s, 10 * c + n, nu=600.0 + 400 * c)
            xn = U._input(dat.to(dev), torch.eye(4, dtype=torch.float64))
            xn.ct = (c, n) == (2, 1)
            xc.append(xn)
        x.append(xc)
    return x


def _bits(x):
    return [(float(xn.sd), float(xn.tau), float(xn.mu)) for xc in x for xn in xc]


def test_batched_subject_same_bits_as_one_at_a_time_and_run_to_run(dev):
    import unires_amd as U
    from unires_amd import stats as S
    x = _subject(dev)
    U._estimate_hyperpar(x, U.settings())
    got = _bits(x)
    assert all(isinstance(xn.tau, torch.Tensor) and xn.tau.dtype == torch.float32 for xc in x for xn in xc)
    again = _subject(dev)
    U._estimate_hyperpar(again, U.settings())
    assert _bits(again) == got
    one = _subject(dev)
    for xc, oc in zip(x, one):
        for xn, on in zip(xc, oc):
            counts, rng = S.noise_hist([on.dat], [on.ct])
            row = S.noise_fit(counts, rng).cpu()[0]
            p_noise, p_fg = S._noise_params(row)
            sd = p_noise['sd'].float()
            assert float(sd) == float(xn.sd) and float(1 / sd ** 2) == float(xn.tau)
            assert float(torch.abs(p_fg['mean'].float() - p_noise['mean'].float())) == float(xn.mu)
    # the restatement end to end (its own stop rule may take one M-step more or fewer: 1e-4)
    for xc in x:
        for xn in xc:
            r = R.estimate(xn.dat.cpu().numpy(), ct=xn.ct)
            assert float(xn.sd) == pytest.approx(r['sd'], rel=1e-4)
    assert x[2][1].sd < 25 and all(abs(float(xn.sd) - SD) < 0.05 * SD for xc in x for xn in xc if not xn.ct)


def _ellipsoid(dim, dev, value=1000.0):
    ax = [torch.linspace(-1, 1, d, device=dev) for d in dim]
    X, Y, Z = torch.meshgrid(*ax, indexing='ij')
    return value * ((X / 0.7) ** 2 + (Y / 0.6) ** 2 + (Z / 0.8) ** 2 < 1).float()


def _thick_obs(truth, dev, thick=3, axis=2, seed=0):
    import unires_amd as U
    dim_y = tuple(truth.shape)
    mat_y = torch.eye(4, dtype=torch.float64)
    scale = [1.0, 1.0, 1.0]
    scale[axis] = float(thick)
    mat_x = torch.diag(torch.tensor(scale + [1.0], dtype=torch.float64))
    dim_x = tuple(int(d // s) for d, s in zip(dim_y, scale))
    po = U._proj_info(dim_y, mat_y, dim_x, mat_x, device=dev)
    clean = U._proj_apply('A', truth[None, None], po, method='super-resolution')[0, 0]
    g = torch.Generator().manual_seed(seed)
    re = torch.randn(clean.shape, generator=g).to(dev) * SD
    im = torch.randn(clean.shape, generator=g).to(dev) * SD
    return torch.sqrt((clean + re) ** 2 + im ** 2), mat_x


def test_recovers_planted_noise_on_thick_slices(dev):
    """sd within 5 % of 75 and mu within 5 % of 1000 - 75 sqrt(pi / 2): mu is |mean_fg - mean_bg| and the
    background class of magnitude data has the Rayleigh mean.  The issue's 3 % of 75 and of 1000 were
    unmeasured; on this phantom the float64 restatement gives sd ~77.4 (partial-volume slices fill the
    gap between the classes) and mu ~886, so the bounds are set from what it achieves."""
    from unires_amd import stats as S
    dat, _ = _thick_obs(_ellipsoid((96, 96, 96), dev), dev)
    prm_noise, prm_fg = S.estimate_noise(dat)
    r = R.estimate(dat.cpu().numpy(), ct=False)
    assert float(prm_noise['sd']) == pytest.approx(r['sd'], rel=1e-4)
    assert float(prm_fg['mean']) == pytest.approx(r['mean'].max(), rel=1e-4)
    assert float(prm_noise['sd']) == pytest.approx(SD, rel=0.05)
    mu = float(prm_fg['mean'] - prm_noise['mean'])
    assert mu == pytest.approx(1000.0 - SD * math.sqrt(math.pi / 2), rel=0.05)


def test_ct_like_data_takes_the_gaussian_path(dev):
    import unires_amd as U
    from unires_amd import stats as S
    truth = _ellipsoid((64, 64, 64), dev, 1040.0) - 1000.0  # air -1000, body 40
    g = torch.Generator().manual_seed(9)
    dat = truth + (torch.randn(truth.shape, generator=g) * 20.0).to(dev)
    counts, rng = S.noise_hist([dat], [True])
    row = S.noise_fit(counts, rng).cpu().numpy()[0]
    assert row[S.MODEL] == 1
    _check_fit(row, counts.cpu().numpy()[0].astype(np.int64), rng.cpu()[0, 0].item(), rng.cpu()[0, 1].item())
    xn = U._input(dat, torch.eye(4, dtype=torch.float64))
    xn.ct = True
    U._estimate_hyperpar([[xn]], U.settings())
    assert float(xn.sd) == pytest.approx(20.0, rel=0.03) and float(xn.mu) == pytest.approx(1040.0, rel=0.03)


def test_estimate_noise_ignores_non_finite_values(dev):
    from unires_amd import stats as S
    clean = _rician((40, 40, 40), 4)
    messy = clean.clone().view(-1)
    messy[::97] = float('nan')
    messy[1::101] = float('inf')
    messy[2::103] = -float('inf')
    keep = torch.isfinite(messy)
    a = S.estimate_noise(messy.view(40, 40, 40).to(dev))
    b = S.estimate_noise(messy[keep].to(dev))
    for pa, pb in zip(a, b):
        assert torch.equal(pa['sd'], pb['sd']) and torch.equal(pa['mean'], pb['mean'])
    r = R.estimate(messy.numpy(), ct=True)
    assert float(a[0]['sd']) == pytest.approx(r['sd'], rel=1e-4)


def test_errors_name_the_observation(dev):
    import unires_amd as U
    from unires_amd import stats as S
    x = _subject(dev)
    x[1][1].dat = torch.zeros_like(x[1][1].dat)
    with pytest.raises(ValueError, match='channel 1, repeat 1'):
        U._estimate_hyperpar(x, U.settings())
    x = _subject(dev)
    x[0][1].dat = torch.full_like(x[0][1].dat, 12.5)
    with pytest.raises(ValueError, match='channel 0, repeat 1'):
        U._estimate_hyperpar(x, U.settings())
    x = _subject(dev)
    x[2][0].dat = -x[2][0].dat  # not CT: nothing >= 0 is left
    with pytest.raises(ValueError, match='channel 2, repeat 0'):
        U._estimate_hyperpar(x, U.settings())
    with pytest.raises(ValueError):
        S.estimate_noise(torch.zeros(10, device=dev))
    with pytest.raises(ValueError):
        S.estimate_noise(torch.full((10,), -4.0, device=dev))


def test_end_to_end_read_estimate_fit(dev):
    import unires_amd as U
    dim_y = (96, 96, 96)
    g = torch.Generator().manual_seed(11)
    import workloads
    truth = workloads.phantom(dim_y, g, dev) * 1000.0
    x = [[]]
    for n, axis in enumerate((2, 0)):
        dat, mat_x = _thick_obs(truth, dev, axis=axis, seed=20 + n)
        dat, dim, mat, _, _, _, _, ct = U._read_image([dat.cpu(), mat_x], device=dev)
        xn = U._input(dat, mat)
        xn.ct = ct
        x[0].append(xn)
    sett = U.settings()
    sett.device, sett.method, sett.do_proj = dev, 'super-resolution', True
    U._estimate_hyperpar(x, sett)
    mat_y = torch.eye(4, dtype=torch.float64)
    for xn in x[0]:
        assert abs(float(xn.sd) - SD) < 0.1 * SD
        xn.po = U._proj_info(dim_y, mat_y, xn.dim, xn.mat, device=dev)
    y = [U._output(torch.zeros(dim_y, device=dev), mat_y)]
    U._init_y_dat(x, y, sett)
    U._init_lam(x, y, sett)
    assert 0 < float(y[0].lam0) < 1e-2
    y0 = y[0].dat.clone()
    sett.max_iter, sett.sched_num = 6, 1
    dat_y, _, _, info = U.fit(x, y, sett)
    obj = info['obj'][:, 0].cpu()
    obj = obj[obj != 0]
    assert len(obj) >= 2 and float(obj[-1]) < float(obj[0])
    err0 = float((y0 - truth).norm())
    err = float((dat_y.reshape(dim_y) - truth).norm())
    assert err < err0, (err, err0)
