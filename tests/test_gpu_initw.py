"""Voxel weight maps in init() on the GPU: unires_noise_hist_g, unires_coreg_quantise_m,
unires_coreg_cellmask, unires_coreg_hist_m and unires_pull3d_support bit for bit against tests/initw_restated.py and
against the unmasked entries on compacted / all-usable data, "a voxel outside the support changes no bit", and the
three steps of init() end to end: noise, coregistration with a planted defect, init() / preproc()."""
import numpy as np
import pytest
import torch

from tests import coreg_phantom as P
from tests import coreg_restated as CR
from tests import initw_restated as W
from tests import voxel64
from tests.test_initw import MARGIN, DEFECT_DIM, DEFECT_SCALE, defect_pair

pytestmark = pytest.mark.gpu


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _map(shape, pattern):
    if pattern == 'binary':
        return (voxel64.weights(shape, 'pow2', seed=23) > 0.25).float()
    return voxel64.weights(shape, pattern)


def _vals(shape, seed, ct):
    """Values with NaN, +-Inf, +-0 and repeats sprinkled in; magnitudes for non-CT with some negatives left."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g) * 100.0 + (0.0 if ct else 60.0)
    flat = v.view(-1)
    n = flat.numel()
    if n >= 50:
        idx = torch.randperm(n, generator=g)
        k = n // 50
        for j, val in enumerate((float('nan'), float('inf'), -float('inf'), 0.0, -0.0, 17.25)):
            flat[idx[j * k:(j + 1) * k]] = val
    return v


# ---- unires_noise_hist_g -------------------------------------------------------------------------------------------
NOISE_SHAPES = [(1,), (3,), (4,), (5,), (1023,), (1025,), (4099,), (33, 20, 17)]


def _hist(vols, cts, ws, dev):
    from unires_amd import stats as S
    counts, rng = S.noise_hist([v.to(dev) for v in vols], cts, None if ws is None else [None if w is None else w.to(dev) for w in ws])
    return counts.cpu().numpy(), rng.cpu().numpy()


def _check_restated(counts, rng, vols, cts, ws):
    for o, (v, ct, w) in enumerate(zip(vols, cts, ws)):
        want, (mn, mx) = W.histogram(v.cpu().numpy(), ct, None if w is None else w.cpu().numpy())
        assert rng[o, 0].tobytes() == np.float32(mn).tobytes() and rng[o, 1].tobytes() == np.float32(mx).tobytes(), o
        if want is None:
            assert not counts[o].any(), o
        else:
            np.testing.assert_array_equal(counts[o].astype(np.int64), want, err_msg='observation %d' % o)


@pytest.mark.parametrize('form', ['0', '1'])
@pytest.mark.parametrize('pattern', ['pow2', 'ramp', 'binary'])
@pytest.mark.parametrize('ct', [False, True])
def test_noise_hist_g_bit_for_bit(dev, monkeypatch, ct, pattern, form):
    monkeypatch.setenv('UNIRES_NOISE_HIST_FORM', form)  # (read by the library at every call)
    vols = [_vals(s, 3 + i, ct) for i, s in enumerate(NOISE_SHAPES)]
    ws = [_map(s, pattern) for s in NOISE_SHAPES]
    cts = [ct] * len(vols)
    counts, rng = _hist(vols, cts, ws, dev)
    _check_restated(counts, rng, vols, cts, ws)
    # ... the unmasked entry on the compacted usable voxels (an empty compaction: a lone 0, which selects nothing)
    comp = [v.reshape(-1)[w.reshape(-1) > 0] for v, w in zip(vols, ws)]
    comp = [c if c.numel() else torch.zeros(1) for c in comp]
    c2, r2 = _hist(comp, cts, None, dev)
    assert counts.tobytes() == c2.tobytes() and rng.tobytes() == r2.tobytes()
    # ... unusable voxels changed: no bit moves; and run to run
    for bad in (1e30, float('nan'), -1.0):
        corrupt = [torch.where(w > 0, v, torch.full_like(v, bad)) for v, w in zip(vols, ws)]
        c3, r3 = _hist(corrupt, cts, ws, dev)
        assert counts.tobytes() == c3.tobytes() and rng.tobytes() == r3.tobytes(), bad
    c4, r4 = _hist(vols, cts, ws, dev)
    assert counts.tobytes() == c4.tobytes() and rng.tobytes() == r4.tobytes()
    # ... an all-positive map: the bits of unires_noise_hist
    c5, r5 = _hist(vols, cts, [0.5 + _map(s, 'ramp') for s in NOISE_SHAPES], dev)
    c6, r6 = _hist(vols, cts, None, dev)
    assert c5.tobytes() == c6.tobytes() and r5.tobytes() == r6.tobytes()


@pytest.mark.parametrize('off_v,off_w', [(1, 0), (0, 1), (1, 1), (2, 3), (0, 0)])
def test_noise_hist_g_unaligned_data_or_map(dev, off_v, off_w):
    from unires_amd import stats as S
    n = 33 * 20 * 17
    v = _vals((n + 4,), 11, False).to(dev)
    w = _map((n + 4,), 'pow2').to(dev)
    dv, dw = v[off_v:off_v + n], w[off_w:off_w + n]   # sliced on the device: off 16-byte alignment
    assert dv.data_ptr() % 16 == 4 * off_v % 16 and dw.data_ptr() % 16 == 4 * off_w % 16
    counts, rng = S.noise_hist([dv], [False], [dw])
    _check_restated(counts.cpu().numpy(), rng.cpu().numpy(), [dv], [False], [dw])


def test_noise_hist_g_mixed_maps_and_more_than_one_chunk(dev):
    shapes = [(33, 20, 17), (1025,), (40, 9, 7)]
    vols = [_vals(s, 20 + i, i == 1) for i, s in enumerate(shapes)]
    ws = [_map(shapes[0], 'ramp'), None, _map(shapes[2], 'pow2')]
    cts = [False, True, False]
    counts, rng = _hist(vols, cts, ws, dev)
    _check_restated(counts, rng, vols, cts, ws)
    # 35 observations: more than kNoiseMaxObs = 32 in one call, maps on two of every three
    many = [_vals((257 + 3 * i,), 40 + i, i % 2 == 0) for i in range(35)]
    wm = [None if i % 3 == 1 else _map((257 + 3 * i,), 'pow2' if i % 3 else 'ramp') for i in range(35)]
    cm = [i % 2 == 0 for i in range(35)]
    counts, rng = _hist(many, cm, wm, dev)
    _check_restated(counts, rng, many, cm, wm)


def test_noise_hist_g_all_zero_map(dev):
    import unires_amd as U
    v = _vals((33, 20, 17), 5, False)
    counts, rng = _hist([v], [False], [torch.zeros_like(v)], dev)
    assert not rng[0, 1] > rng[0, 0] and not counts.any()
    xn = U._input(v.to(dev), torch.eye(4, dtype=torch.float64))
    xn.weight = torch.zeros_like(xn.dat)
    sett = U.settings()
    sett.voxel_init = True
    with pytest.raises(ValueError, match='channel 0, repeat 0.*weight > 0'):
        U._estimate_hyperpar([[xn]], sett)


# ---- unires_coreg_quantise_m / unires_coreg_cellmask ---------------------------------------------------------------
def _mask(shape, seed, p=0.8):
    m = (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)
    m[0, 0, 0] = m[-1, -1, -1] = 1
    return m


def _fvol(shape, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g) * 1000.0
    v[0, 0, 0], v[-1, -1, -1] = 3.0, 900.0
    return v.contiguous()


Q_SHAPES = [(2, 2, 2), (5, 7, 6), (33, 20, 17)]


def test_quantise_m_bit_for_bit(dev):
    from unires_amd import preproc
    vols = [_fvol(s, 30 + i) for i, s in enumerate(Q_SHAPES)]
    vols[2][1, 2, 3], vols[2][4, 5, 6] = float('nan'), float('inf')
    vols[1][1, 1, 1] = 5e5   # an outlier, masked below: the robust maximum must not see it
    masks = [_mask(s, 40 + i) for i, s in enumerate(Q_SHAPES)]
    masks[1][1, 1, 1] = 0
    dm = [torch.from_numpy(m).to(dev) for m in masks]
    outs, counts, params = preproc.coreg_quantise([v.to(dev) for v in vols], dm)
    for v, m, u, c, prm in zip(vols, masks, outs, counts.cpu().numpy(), params.cpu().numpy()):
        ru, rc, (mn, mxa, mx, scale) = W.quantise(v.numpy(), m)
        assert u.cpu().numpy().tobytes() == ru.tobytes()
        assert (c.astype(np.int64) == rc).all()
        assert [np.float32(p) for p in prm[:4]] == [mn, mxa, mx, scale] and prm[4] == 0
    assert float(params[1, 1]) < 1001.0
    # params: those of the unmasked entry on the compacted usable voxels
    comp = [v.reshape(-1)[torch.from_numpy(m.reshape(-1) != 0)].reshape(-1, 1, 1).to(dev) for v, m in zip(vols, masks)]
    _, c2, p2 = preproc.coreg_quantise(comp)
    assert _bytes(params[:, :5]) == _bytes(p2[:, :5]) and _bytes(counts) == _bytes(c2)
    # all-ones masks: the bits of the unmasked entry
    o3, c3, p3 = preproc.coreg_quantise([v.to(dev) for v in vols], [torch.ones_like(m) for m in dm])
    o4, c4, p4 = preproc.coreg_quantise([v.to(dev) for v in vols])
    assert _bytes(c3) == _bytes(c4) and _bytes(p3[:, :5]) == _bytes(p4[:, :5])
    assert all(_bytes(a) == _bytes(b) for a, b in zip(o3, o4))
    # unusable voxels corrupted: no parameter moves
    for bad in (1e30, float('nan'), -1e6):
        corrupt = [torch.where(torch.from_numpy(m != 0), v, torch.full_like(v, bad)).to(dev) for v, m in zip(vols, masks)]
        _, c5, p5 = preproc.coreg_quantise(corrupt, dm)
        assert _bytes(c5) == _bytes(counts) and _bytes(p5[:, :5]) == _bytes(params[:, :5]), bad
    # mixed NULL / non-NULL masks in one call
    o6, c6, p6 = preproc.coreg_quantise([v.to(dev) for v in vols], [dm[0], None, dm[2]])
    assert _bytes(p6[0, :5]) == _bytes(params[0, :5]) and _bytes(p6[2, :5]) == _bytes(params[2, :5])
    assert _bytes(p6[1, :5]) == _bytes(p4[1, :5]) and _bytes(o6[1]) == _bytes(o4[1]) and _bytes(o6[2]) == _bytes(outs[2])
    with pytest.raises(ValueError, match='no finite usable'):
        preproc.coreg_quantise([vols[1].to(dev)], [torch.zeros_like(dm[1])])
    only = torch.zeros_like(dm[1])
    only[0, 0, 0] = 1
    with pytest.raises(ValueError, match='constant'):
        preproc.coreg_quantise([vols[1].to(dev)], [only])


@pytest.mark.parametrize('shape', [(2, 2, 2), (3, 4, 5), (33, 20, 17)])
def test_cellmask_bit_for_bit(dev, shape):
    from unires_amd import preproc
    for seed, p in ((0, 0.9), (1, 0.6), (2, 1.0)):
        m = _mask(shape, seed, p)
        got = preproc.coreg_cellmask(torch.from_numpy(m).to(dev)).cpu().numpy()
        want = W.cellmask(m)
        d = W.defined(shape)
        assert got.dtype == np.uint8 and (got[d] == want[d]).all()
        assert not got[~d].any()


# ---- unires_coreg_hist_m -------------------------------------------------------------------------------------------
def _u8(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g) * 1000.0
    v = torch.nn.functional.avg_pool3d(v[None, None], 3, 1, 1)[0, 0]
    u = CR.quantise(v.contiguous().numpy())[0]
    return u, torch.from_numpy(u).to(dev)


def _rot(a, b, c):
    from unires_amd._rigid import _expm, affine_basis
    return _expm(np.array([0, 0, 0, a, b, c]), affine_basis()).numpy()


_CASES = {}


def _cases(dev):
    """The geometries of tests/test_gpu_coreg.py restated, (2,2,2) against (2,2,2), and jobs of several chunks
    (zero_background 84 480, step_below_1 193 000 sample points > 64 512), each with voxel supports and cell supports."""
    if _CASES:
        return _CASES['v']
    Gn, G = _u8((40, 36, 32), 11, dev)
    Fn, F = _u8((38, 40, 30), 12, dev)
    Tn, T = _u8((40, 36, 8), 13, dev)
    rng = np.random.default_rng(14)
    An, Bn = rng.integers(0, 256, (2, 2, 2)).astype(np.uint8), rng.integers(0, 256, (2, 2, 2)).astype(np.uint8)
    A, B = torch.from_numpy(An).to(dev), torch.from_numpy(Bn).to(dev)
    I = np.eye(4)
    sh = np.eye(4)
    sh[:3, 3] = [0.37, -0.61, 0.25]
    rot = _rot(0.05, -0.03, 0.08)
    rot[:3, 3] = [1.0, -2.0, 0.5]
    thick = np.diag([1.0, 1.0, 0.25, 1.0])
    edge = np.eye(4)
    edge[:3, 3] = [-2.0, 4.0, -2.0]
    tiny = np.eye(4)
    tiny[:3, 3] = [0.1, -0.05, 0.2]
    m = lambda a: a[:3, :].astype(np.float32).reshape(-1)  # noqa: E731
    one = np.ones(3, np.float32)
    Zg, Zf = np.zeros((48, 44, 40), np.uint8), np.zeros((46, 48, 38), np.uint8)
    Zg[4:44, 4:40, 4:36] = Gn
    Zf[4:42, 4:44, 4:34] = Fn
    Zg[Zg == 1] = 0
    geo = [
        ('zero_background', (Zg, torch.from_numpy(Zg).to(dev)), (Zf, torch.from_numpy(Zf).to(dev)), m(sh), one),
        ('identity', (Gn, G), (Fn, F), m(I), one),
        ('subvoxel_shift', (Gn, G), (Fn, F), m(sh), one),
        ('rotation', (Gn, G), (Fn, F), m(rot), np.array([1.5, 1.5, 1.5], np.float32)),
        ('thick_moving', (Gn, G), (Tn, T), m(thick @ rot), one),
        ('thick_fixed_step_below_1', (Tn, T), (Fn, F), m(np.linalg.inv(thick)), np.array([1, 1, 0.25], np.float32)),
        ('step_below_1', (Gn, G), (Fn, F), m(sh), np.array([0.5, 0.75, 0.6], np.float32)),
        ('fov_edge', (Gn, G), (Fn, F), m(edge), one),
        ('two_cubed', (An, A), (Bn, B), m(tiny), np.array([0.25, 0.25, 0.25], np.float32)),
    ]
    out = []
    for k, (name, g, f, M, s) in enumerate(geo):
        p = 1.0 if name == 'two_cubed' else 0.97
        vg, vf = _mask(g[0].shape, 60 + k, p), _mask(f[0].shape, 80 + k, p)   # voxel supports
        cg, cf = W.cellmask(vg), W.cellmask(vf)
        out.append(dict(name=name, G=g, F=f, M=M, s=s, vG=vg, vF=vf, cG=cg, cF=cf, full=int(CR.hist(g[0], f[0], M, s).sum()),
                        dG=torch.from_numpy(cg).to(dev), dF=torch.from_numpy(cf).to(dev)))
    _CASES['v'] = out
    return out


@pytest.mark.parametrize('which', ['G', 'F', 'both', 'none'])
def test_hist_m_bit_for_bit_and_batched(dev, which):
    from unires_amd import preproc
    cases = _cases(dev)
    useG, useF = which in ('G', 'both'), which in ('F', 'both')
    jobs = [(c['G'][1], c['F'][1], c['M'], c['s'], c['dG'] if useG else None, c['dF'] if useF else None) for c in cases]
    batched = preproc.coreg_hist(jobs).cpu().numpy()
    again = preproc.coreg_hist(jobs).cpu().numpy()
    assert batched.tobytes() == again.tobytes()
    some = False
    for k, c in enumerate(cases):
        ref, kept = W.hist(c['G'][0], c['F'][0], c['M'], c['s'], c['cG'] if useG else None, c['cF'] if useF else None,
                           return_kept=True)
        one = preproc.coreg_hist([jobs[k]]).cpu().numpy()[0]
        assert one.astype(np.uint64).tobytes() == ref.tobytes(), c['name']
        assert batched[k].tobytes() == one.tobytes(), c['name']
        assert int(one.sum()) == 65536 * kept, c['name']
        full = c['full']
        assert int(one.sum()) <= full and (which != 'none' or int(one.sum()) == full)
        some = some or int(one.sum()) < full
    assert some == (which != 'none')


def test_hist_m_all_ones_masks_give_the_unmasked_bits(dev):
    from unires_amd import preproc
    cases = _cases(dev)
    plain = preproc.coreg_hist([(c['G'][1], c['F'][1], c['M'], c['s']) for c in cases])
    ones = preproc.coreg_hist([(c['G'][1], c['F'][1], c['M'], c['s'], torch.ones_like(c['dG']), torch.ones_like(c['dF']))
                               for c in cases])
    half = preproc.coreg_hist([(c['G'][1], c['F'][1], c['M'], c['s'], torch.ones_like(c['dG']), None) for c in cases])
    assert _bytes(plain) == _bytes(ones) == _bytes(half)
    # NULL / NULL through the masked entry itself (the Python wrapper takes the unmasked entry for such jobs)
    import ctypes as C
    from unires_amd import _lib
    from unires_amd._ops import _stream
    n = len(cases)
    arr = (preproc.JobM * n)(*[preproc._job(c['G'][1], c['F'][1], c['M'], c['s'], None, None, cls=preproc.JobM) for c in cases])
    hist = torch.empty((n, 256, 256), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().unires_coreg_hist_m(n, arr, C.c_void_p(hist.data_ptr()), _stream()))
    assert _bytes(hist) == _bytes(plain)


def test_hist_m_never_reads_a_voxel_outside_the_support(dev):
    from unires_amd import preproc
    cases = _cases(dev)
    clean = preproc.coreg_hist([(c['G'][1], c['F'][1], c['M'], c['s'], c['dG'], c['dF']) for c in cases])
    jobs = []
    for c in cases:
        Gc, Fc = c['G'][0].copy(), c['F'][0].copy()
        Gc[c['vG'] == 0] = 255
        Fc[c['vF'] == 0] = 255
        jobs.append((torch.from_numpy(Gc).to(dev), torch.from_numpy(Fc).to(dev), c['M'], c['s'], c['dG'], c['dF']))
    assert _bytes(preproc.coreg_hist(jobs)) == _bytes(clean)


def test_hist_m_counts_a_point_outside_f_under_a_zero_mf(dev):
    from unires_amd import preproc
    c = [k for k in _cases(dev) if k['name'] == 'fov_edge'][0]
    zero = torch.zeros_like(c['dF'])
    H = preproc.coreg_hist([(c['G'][1], c['F'][1], c['M'], c['s'], None, zero)]).cpu().numpy()[0]
    ref, kept = W.hist(c['G'][0], c['F'][0], c['M'], c['s'], None, np.zeros_like(c['cF']), return_kept=True)
    assert H.astype(np.uint64).tobytes() == ref.tobytes()
    assert kept > 0 and int(H[:, 0].sum()) == 65536 * kept and not H[:, 1:].any()   # only the points outside F, f = 0


# ---- unires_pull3d_support -----------------------------------------------------------------------------------------
def _m12(A):
    return np.asarray(A, dtype=np.float64)[:3].astype(np.float32).reshape(-1)


def _exact_geometries():
    I = np.eye(4)
    tr = np.eye(4)
    tr[:3, 3] = [2.0, -1.0, 3.0]
    half = np.diag([0.5, 0.5, 0.5, 1.0])          # a grid twice as fine: half-integer coordinates
    dbl = np.diag([2.0, 2.0, 2.0, 1.0])
    big = np.eye(4)
    big[:3, 3] = [-3.0, -2.0, -4.0]               # the grid starts outside the source on every side
    return [('identity', (9, 8, 7), I, (9, 8, 7)), ('translation', (9, 8, 7), tr, (9, 8, 7)),
            ('ratio_2_fine', (9, 8, 7), half, (17, 15, 13)), ('ratio_2_coarse', (9, 8, 7), dbl, (5, 4, 4)),
            ('larger_grid', (9, 8, 7), big, (16, 13, 16)), ('one_voxel', (1, 1, 1), I, (3, 2, 2)),
            ('one_voxel_shifted', (1, 1, 1), big, (5, 4, 6)), ('one_slice', (9, 8, 1), I, (9, 8, 2)),
            ('long_row', (4, 3, 200), I, (4, 3, 200)), ('row_100', (3, 3, 100), I, (3, 3, 100)),
            ('row_181', (3, 3, 181), tr, (3, 3, 181))]


@pytest.mark.parametrize('name,sdim,A,gdim', _exact_geometries(), ids=[g[0] for g in _exact_geometries()])
def test_pull_support_exact_geometries(dev, name, sdim, A, gdim):
    from unires_amd import _ops
    for pattern in ('pow2', 'ones', 'zeros'):
        g = _map(sdim, pattern)
        got = _ops.pull_support(g.to(dev), _m12(A), gdim)
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(gdim)
        want, _ = W.support(g.numpy(), _m12(A), gdim)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (name, pattern)
        if pattern == 'zeros':
            assert not got.any()


def test_pull_support_general_rigid(dev):
    from unires_amd import _ops
    from unires_amd._rigid import _expm, affine_basis
    sdim, gdim = (24, 20, 18), (30, 28, 26)
    R = _expm(np.array([2.3, -1.7, 2.9, 0.08, -0.06, 0.1]), affine_basis()).numpy()
    cs, cg = np.eye(4), np.eye(4)
    cs[:3, 3] = (np.asarray(sdim) - 1) / 2.0
    cg[:3, 3] = -(np.asarray(gdim) - 1) / 2.0
    M = _m12(cs @ R @ cg)                          # grid voxel -> source voxel, about the centres
    g = _map(sdim, 'binary')
    g = torch.where(torch.rand(sdim, generator=torch.Generator().manual_seed(2)) < 0.9, torch.ones(sdim), g)
    want, flag = W.support(g.numpy(), M, gdim)
    share = float(flag.mean())
    assert share < 0.005, share                    # the restatement alone: few near ties under this rigid
    got = _ops.pull_support(g.to(dev), M, gdim).cpu().numpy()
    differ = got != want
    assert not (differ & ~flag).any(), int((differ & ~flag).sum())
    assert 0.05 < got.mean() < 0.95
    # where the support is 1 the pull reads no unusable voxel: corrupting them moves no bit
    dat = _fvol(sdim, 9)
    clean = _ops.pull_affine(dat.to(dev), M, gdim).cpu().numpy()
    sup = got != 0
    for bad in (1e30, -777.0):
        corrupt = torch.where(g > 0, dat, torch.full_like(dat, bad))
        out = _ops.pull_affine(corrupt.to(dev), M, gdim).cpu().numpy()
        assert out[sup].tobytes() == clean[sup].tobytes(), bad
        assert (out != clean).any()


# ---- end to end: noise ---------------------------------------------------------------------------------------------
def test_estimate_hyperpar_with_a_masked_defect(dev):
    """48^3 phantom with a 6 x 6 x 6 block at 100 x the foreground maximum.  With the block as a 0-weight map and
    voxel_init on: the bits of sd, tau, mu of the volume with the block's voxels removed.  Off: today's unmasked bits,
    which differ - this fails without the feature."""
    import unires_amd as U
    from unires_amd import stats as S
    dat, mat = P.observation((48, 48, 48), (3.0, 3.0, 3.0), 0, 7, dev, rician=True)
    dat = dat.clone()
    dat[20:26, 22:28, 18:24] = 100.0 * float(max(P.CONTRASTS[0]))
    w = torch.ones_like(dat)
    w[20:26, 22:28, 18:24] = 0.0

    def run(on):
        xn = U._input(dat, torch.from_numpy(mat))
        xn.weight = w
        sett = U.settings()
        sett.voxel_init = on
        U._estimate_hyperpar([[xn]], sett)
        return float(xn.sd), float(xn.tau), float(xn.mu)

    def direct(vol):
        counts, rng = S.noise_hist([vol], [False])
        noise, fg = S._noise_params(S.noise_fit(counts, rng).cpu()[0])
        sd = noise['sd'].float()
        return float(sd), float(1 / sd ** 2), float(torch.abs(fg['mean'].float() - noise['mean'].float()))
    masked, off = run(True), run(False)
    print('sd, tau, mu masked %r unmasked %r' % (masked, off))
    assert masked == direct(dat[w > 0])
    assert off == direct(dat)
    assert masked != off


# ---- end to end: coregistration ------------------------------------------------------------------------------------
def test_affine_align_with_a_masked_defect(dev):
    """Clean data, defect with its mask, defect without, with the default coreg_params: the masked search comes within
    the clean search's error + 0.1 mm, the unmasked one is worse (DESIGN 8.10 records the errors)."""
    import unires_amd as U
    from unires_amd import preproc
    clean, bad, w, mf = defect_pair(dev)
    prm = U.settings().coreg_params

    def err(imgs, weights=None):
        mat_a = preproc.affine_align(imgs, **prm, device=dev, weights=weights)[1]
        return P.rms_mm(np.linalg.solve(mat_a[1].numpy(), imgs[1][1].numpy()), mf, DEFECT_DIM, scale=DEFECT_SCALE)
    e_clean, e_mask, e_raw = err(clean), err(bad, [None, w]), err(bad)
    print('gpu rms mm: clean %.4f masked %.4f unmasked %.4f' % (e_clean, e_mask, e_raw))
    assert e_clean < 0.3
    assert e_mask <= e_clean + MARGIN, (e_clean, e_mask, e_raw)
    assert e_raw > e_mask, (e_clean, e_mask, e_raw)
    assert err(clean, [None, None]) == e_clean    # no map: the unmasked path


def test_affine_align_erodes_the_support_where_it_smooths(dev):
    """samp above the voxel size: the level volumes are smoothed, and the supports eroded by the tap radius - corrupting
    the 0-weight voxels then moves no bit of the result."""
    from unires_amd import preproc
    clean, bad, w, mf = defect_pair(dev)
    a = preproc.affine_align(bad, samp=2, device=dev, weights=[None, w])[0]
    worse = [bad[0], [torch.where(w > 0, bad[1][0], torch.full_like(w, -5e4)), bad[1][1]]]
    b = preproc.affine_align(worse, samp=2, device=dev, weights=[None, w])[0]
    assert a.numpy().tobytes() == b.numpy().tobytes()
    R = [(t.size - 1) // 2 for t in preproc._level_taps((1.0, 1.0, 1.0), 2.0)]
    assert min(R) >= 1
    sup = preproc._level_support(w, (1.0, 1.0, 1.0), 2.0).cpu().numpy()
    assert (sup != 0).tobytes() == W.erode(w.cpu().numpy() > 0, R).tobytes()


# ---- end to end: init() / preproc() --------------------------------------------------------------------------------
IDIM, IVX, ISCALE = (32, 32, 32), (2.0, 2.0, 2.0), 0.45


def _init_subject(dev):
    """Channel 0: one repeat; channel 1: two repeats, the second under a planted rigid and with a defect block that
    its map gives weight 0."""
    rng = np.random.default_rng(3)
    mat = P.true_mat(IDIM, IVX)
    d0 = P.observation(IDIM, IVX, 0, 70, dev, scale=ISCALE, rician=True)[0]
    d1 = P.observation(IDIM, IVX, 1, 71, dev, scale=ISCALE, rician=True)[0]
    d2 = P.observation(IDIM, IVX, 1, 72, dev, scale=ISCALE, rician=True)[0].clone()
    sl = (slice(8, 14), slice(10, 16), slice(12, 18))
    d2[sl] = 100.0 * float(max(P.CONTRASTS[1]))
    w = torch.ones(IDIM, device=dev)
    w[sl] = 0.0
    Pl = P.random_rigid(rng, 3.0, 0.05)
    mats = [torch.from_numpy(mat), torch.from_numpy(mat), torch.from_numpy(Pl @ mat)]
    return [d0, d1, d2], mats, w


def _data(dats, mats):
    return [[dats[0].clone(), mats[0]], [[dats[1].clone(), mats[1]], [dats[2].clone(), mats[2]]]]


def _sett(dev, weight, on):
    import unires_amd as U
    s = U.settings()
    s.device, s.max_iter, s.vx, s.write_out, s.weight, s.voxel_init = dev, 3, 0, False, weight, on
    s.cgs_max_iter, s.cgs_tol = 5, 0.0
    return s


def _by_hand(dats, mats, w, dev, on):
    """The steps of init() chained by hand from the op-level calls; ``on``: with the map of repeat (1, 1)."""
    import unires_amd as U
    from unires_amd import _core, _ops, preproc, stats as S
    from unires_amd.spatial import _m12 as m12
    sett = _sett(dev, None, on)
    x = _core._read_data(_data(dats, mats), sett)
    gs = [None, None, w.float().contiguous() if on else None]
    flat = [xn for xc in x for xn in xc]
    counts, rng = S.noise_hist([xn.dat for xn in flat], [bool(xn.ct) for xn in flat], gs if on else None)
    for xn, row in zip(flat, S.noise_fit(counts, rng).cpu()):
        noise, fg = S._noise_params(row)
        xn.sd = noise['sd'].float()
        xn.tau = 1 / xn.sd ** 2
        xn.mu = torch.abs(fg['mean'].float() - noise['mean'].float())
    from unires_amd._rigid import affine_basis
    sett.rigid_basis = affine_basis(group='SE', dtype=torch.float64)
    kw = dict(weights=gs) if on else {}
    mat_a = preproc.affine_align([[xn.dat, xn.mat] for xn in flat], **sett.coreg_params, fix=sett.fix, device=dev, **kw)[1]
    sett.mat_coreg = mat_a
    for i, xn in enumerate(flat):
        m = torch.as_tensor(xn.mat, dtype=torch.float64)
        xn.mat = torch.linalg.solve(mat_a[i].to(m), m)
        xn.rigid_q = torch.zeros(6, device=dev, dtype=torch.float64)
    y, sett = _core._format_y(x, sett)
    x = _core._proj_info_add(x, y, sett)
    dim_y = tuple(y[0].dim)
    mat_y = torch.as_tensor(y[0].mat).detach().to('cpu', torch.float64)
    i = 0
    for c in range(len(x)):
        tot, sm = 0, 0
        for xn in x[c]:
            M = m12(torch.linalg.solve(torch.as_tensor(xn.mat).detach().to('cpu', torch.float64), mat_y))
            use = xn.dat if gs[i] is None else xn.dat[gs[i] > 0]
            res = _ops.pull_affine(xn.dat, M, dim_y).clamp(float(use.min()), float(use.max()))
            if gs[i] is not None:
                res = res * (_ops.pull_support(gs[i], M, dim_y) != 0)
            tot, sm = tot + res, sm + (res > 0).float()
            i += 1
        y[c].dat = tot / sm.clamp(min=1)
    return x, y, sett


def _compare(x, y, sett, xh, yh, sh):
    for c in range(len(x)):
        for a, b in zip(x[c], xh[c]):
            for k in ('tau', 'mu', 'mat', 'rigid_q'):
                va, vb = torch.as_tensor(getattr(a, k)).cpu(), torch.as_tensor(getattr(b, k)).cpu()
                assert va.dtype == vb.dtype and torch.equal(va, vb), (c, k)
        assert torch.equal(torch.as_tensor(y[c].lam0), torch.as_tensor(yh[c].lam0)), c
        assert tuple(y[c].dim) == tuple(yh[c].dim) and torch.equal(y[c].dat, yh[c].dat), c
    assert torch.equal(sett.mat_coreg, sh.mat_coreg)


@pytest.mark.parametrize('on', [True, False])
def test_init_equals_the_steps_chained_by_hand(dev, on):
    import unires_amd as U
    dats, mats, w = _init_subject(dev)
    x, y, sett = U.init(_data(dats, mats), _sett(dev, [None, [None, w.cpu().double()]], on))
    xh, yh, sh = _by_hand(dats, mats, w, dev, on)
    _compare(x, y, sett, xh, yh, sh)
    assert x[1][1].weight is not None and x[1][0].weight is None
    if on:
        assert x[1][1].weight.dtype == torch.float32 and x[1][1].weight.is_cuda and x[1][1].weight.is_contiguous()
    else:  # off: what init() gives without any map - the parent's behaviour
        x0, y0, s0 = U.init(_data(dats, mats), _sett(dev, None, False))
        _compare(x, y, sett, x0, y0, s0)


def test_init_ignores_what_the_zero_weight_voxels_hold_and_preproc_runs(dev):
    import unires_amd as U
    from unires_amd.run import preproc
    dats, mats, w = _init_subject(dev)
    weight = [None, [None, w]]
    x, y, sett = U.init(_data(dats, mats), _sett(dev, weight, True))
    worse = list(dats)
    worse[2] = torch.where(w > 0, dats[2], torch.full_like(w, 7e6))
    x2, y2, sett2 = U.init(_data(worse, mats), _sett(dev, weight, True))
    _compare(x, y, sett, x2, y2, sett2)
    x3, y3, sett3 = U.init(_data(dats, mats), _sett(dev, weight, False))
    assert not torch.equal(x3[1][1].tau, x[1][1].tau) and not torch.equal(y3[1].dat, y[1].dat)
    dat_y, mat_y, _ = preproc(_data(dats, mats), _sett(dev, weight, True))
    assert dat_y.shape[-1] == 2 and bool(torch.isfinite(dat_y).all())
    assert float(dat_y[..., 1].max()) < 2.0 * float(max(P.CONTRASTS[1]))   # the defect did not reach the reconstruction

    def bad(value):
        g = w.clone()
        g[3, 4, 5] = value
        return _sett(dev, [None, [None, g]], True)
    for value in (-0.5, float('nan')):
        with pytest.raises(ValueError, match='channel 1, repeat 1'):
            U.init(_data(dats, mats), bad(value))
