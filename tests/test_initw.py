"""Voxel weight maps in init(), the part that needs no GPU: the restatement (tests/initw_restated.py)
against brute force and against the unmasked restatements it extends, the switch (off: ``xn.weight`` is never touched),
validation by name, the C surface, and the planted-defect coregistration searches on the restatement whose errors
DESIGN 8.10 records."""
import os
import re

import numpy as np
import pytest
import torch

from tests import coreg_phantom as P
from tests import coreg_restated as CR
from tests import initw_restated as W
from tests import noise_restated as NR
from tests import voxel64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('unires_noise_hist_g', 'unires_coreg_quantise_m', 'unires_coreg_cellmask', 'unires_coreg_hist_m',
               'unires_pull3d_support')


def _mask(shape, seed, p=0.8):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


# ---- the restatement against brute force -------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 2, 2), (3, 4, 5), (5, 7, 6)])
def test_cellmask_against_an_eight_fold_loop(shape):
    for seed, p in ((0, 0.9), (1, 0.6), (2, 1.0)):
        m = _mask(shape, seed, p)
        want = np.zeros(shape, np.uint8)
        for i0 in range(shape[0] - 1):
            for i1 in range(shape[1] - 1):
                for i2 in range(shape[2] - 1):
                    ok = True
                    for o0 in (0, 1):
                        for o1 in (0, 1):
                            for o2 in (0, 1):
                                ok = ok and bool(m[i0 + o0, i1 + o1, i2 + o2])
                    want[i0, i1, i2] = ok
        got = W.cellmask(m)
        assert got.dtype == np.uint8 and (got == want).all()
        assert not got[~W.defined(shape)].any()


@pytest.mark.parametrize('radius', [(1, 0, 0), (0, 2, 0), (0, 0, 3), (2, 1, 3), (9, 0, 0)])
def test_erosion_against_a_loop(radius):
    shape = (6, 7, 8)
    m = _mask(shape, 3, 0.93).astype(bool)
    want = np.ones(shape, bool)
    for i in np.ndindex(*shape):
        # one axis after the other == a box: no unusable voxel within +-R_d along every axis, inside the volume
        lo = [max(0, i[d] - radius[d]) for d in range(3)]
        hi = [min(shape[d], i[d] + radius[d] + 1) for d in range(3)]
        want[i] = m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].all()
    assert (W.erode(m, radius) == want).all()
    # the package's device pass (torch ops) is the same integer rule
    from unires_amd import preproc
    got = preproc.erode_support(torch.from_numpy(m), radius).numpy()
    assert (got == want).all()
    assert (W.erode(np.ones(shape, bool), radius)).all()   # beyond the volume's end counts as usable


def _u8(shape, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g) * 1000.0
    v = torch.nn.functional.avg_pool3d(v[None, None], 3, 1, 1)[0, 0]
    return CR.quantise(v.numpy())[0]


def test_masked_hist_with_all_ones_masks_is_the_unmasked_restatement():
    G, F = _u8((14, 12, 10), 1), _u8((12, 13, 9), 2)
    M = np.eye(4)
    M[:3, 3] = [0.37, -0.61, 0.25]
    M = M[:3].astype(np.float32).reshape(-1)
    s = np.array([1.0, 0.75, 1.5], np.float32)
    ref = CR.hist(G, F, M, s)
    oneG, oneF = W.cellmask(np.ones(G.shape, np.uint8)), W.cellmask(np.ones(F.shape, np.uint8))
    for mG, mF in ((None, None), (oneG, None), (None, oneF), (oneG, oneF)):
        H, kept = W.hist(G, F, M, s, mG, mF, return_kept=True)
        assert H.tobytes() == ref.tobytes() and kept * 65536 == int(ref.sum())
    # and a real mask removes whole points: the total stays a multiple of 65536 and drops
    H, kept = W.hist(G, F, M, s, W.cellmask(_mask(G.shape, 5)), W.cellmask(_mask(F.shape, 6)), return_kept=True)
    assert int(H.sum()) == kept * 65536 and 0 < kept * 65536 < int(ref.sum())


@pytest.mark.parametrize('ct', [False, True])
@pytest.mark.parametrize('pattern', ['pow2', 'ramp'])
def test_masked_histogram_is_the_histogram_of_the_compacted_usable_voxels(ct, pattern):
    g = torch.Generator().manual_seed(4)
    v = (torch.randn((9, 8, 7), generator=g) * 100.0).numpy()
    v.ravel()[::13] = np.nan
    v.ravel()[1::17] = 0.0
    w = voxel64.weights(v.shape, pattern).numpy()
    counts, (mn, mx) = W.histogram(v, ct, w)
    want, (wmn, wmx) = NR.histogram(v.ravel()[w.ravel() > 0], ct)
    assert (counts == want).all() and mn == wmn and mx == wmx
    assert (W.select(v, ct, w) == NR.select(v.ravel()[w.ravel() > 0], ct)).all()
    none, (lo, hi) = W.histogram(v, ct, np.zeros_like(w))
    assert none is None and not hi > lo


def test_masked_quantise_reads_only_usable_voxels_for_its_parameters():
    g = torch.Generator().manual_seed(7)
    v = (torch.rand((6, 7, 5), generator=g) * 1000.0).numpy()
    m = _mask(v.shape, 8)
    u, counts, prm = W.quantise(v, m)
    _, wcounts, wprm = CR.quantise(v.ravel()[m.ravel() != 0].reshape(-1, 1, 1))
    assert prm == wprm and (counts == wcounts).all()
    bad = v.copy()
    bad[m == 0] = 1e30
    assert W.quantise(bad, m)[2] == prm
    one = W.quantise(v, np.ones_like(m))
    ref = CR.quantise(v)
    assert one[0].tobytes() == ref[0].tobytes() and one[2] == ref[2]
    with pytest.raises(ValueError):
        W.quantise(v, np.zeros_like(m))


def test_support_restatement_on_exact_geometries():
    g = voxel64.weights((5, 6, 7), 'pow2').numpy()
    use = g > 0
    eye = np.eye(4)[:3].astype(np.float32).reshape(-1)
    s, flag = W.support(g, eye, g.shape)
    # integer coordinates: the corners are the voxel and its upper neighbours that exist (they decide at weight 0 too)
    want = np.zeros(g.shape, bool)
    for i in np.ndindex(*g.shape):
        want[i] = use[i[0]:i[0] + 2, i[1]:i[1] + 2, i[2]:i[2] + 2].all()
    assert (s == want).all() and flag.all()    # every voxel is a near tie by definition
    sh = np.eye(4)
    sh[:3, 3] = [0.5, 0.5, 0.5]
    s, flag = W.support(g, sh[:3].astype(np.float32).reshape(-1), g.shape)
    cell = W.cellmask(use.astype(np.uint8))
    assert (s[:-1, :-1, :-1] == cell[:-1, :-1, :-1]).all() and not flag.any()
    assert not s[-1].any() and not s[:, -1].any() and not s[:, :, -1].any()   # half a voxel beyond the last plane: out of the FOV
    far = np.eye(4)
    far[:3, 3] = [-1.0, 2.0, 40.0]
    s, _ = W.support(np.ones((5, 6, 7), np.float32), far[:3].astype(np.float32).reshape(-1), (3, 3, 3))
    assert not s.any()


# ---- the switch --------------------------------------------------------------------------------------------------
class _Boom:
    """A weight map that raises on any use."""

    def _boom(self, *a, **k):
        raise AssertionError('xn.weight was touched with sett.voxel_init off')
    __getattr__ = __gt__ = __array__ = __len__ = __iter__ = __getitem__ = __bool__ = _boom


def _guarded_input(dat, mat):
    import unires_amd as U

    class Guarded(U._input):
        seen = 0

        @property
        def weight(self):
            type(self).seen += 1
            raise AssertionError('xn.weight was read with sett.voxel_init off')

        @weight.setter
        def weight(self, v):
            pass
    xn = Guarded(dat, mat)
    xn.ct = False
    return xn


def _fake_steps(monkeypatch, seen):
    from unires_amd import _ops, preproc, stats

    def noise_hist(dats, cts, weights=None):
        seen['noise'] = weights
        return torch.zeros((len(dats), 1024), dtype=torch.int32), torch.zeros((len(dats), 2))

    def noise_fit(counts, rng):
        rows = torch.zeros((counts.shape[0], stats.NOUT), dtype=torch.float64)
        rows[:, stats.SIG], rows[:, stats.SIG + 1], rows[:, stats.MEAN + 1] = 2.0, 3.0, 10.0
        return rows

    def affine_align(imgs, **kw):
        seen['coreg'] = kw.get('weights', 'absent')
        return None, torch.stack([torch.eye(4, dtype=torch.float64)] * len(imgs))

    def pull_affine(dat, M, gdim, **kw):
        return torch.ones(tuple(gdim))

    def pull_support(g, M, gdim, **kw):
        seen['pull'] = g
        return torch.ones(tuple(gdim), dtype=torch.uint8)
    monkeypatch.setattr(stats, 'noise_hist', noise_hist)
    monkeypatch.setattr(stats, 'noise_fit', noise_fit)
    monkeypatch.setattr(preproc, 'affine_align', affine_align)
    monkeypatch.setattr(_ops, 'pull_affine', pull_affine)
    monkeypatch.setattr(_ops, 'pull_support', pull_support)


def test_with_voxel_init_off_the_three_steps_never_touch_the_weight(monkeypatch):
    import unires_amd as U
    seen = {}
    _fake_steps(monkeypatch, seen)
    eye = torch.eye(4, dtype=torch.float64)
    for sett in (U.settings(), None):
        x = [[_guarded_input(torch.rand(4, 5, 6), eye), _guarded_input(torch.rand(4, 5, 6), eye)]]
        if sett is not None:
            assert sett.voxel_init is False
            sett.device = 'cpu'
            U._estimate_hyperpar(x, sett)
            U._init_reg(x, sett)
            assert seen['noise'] is None or all(w is None for w in seen['noise'])
            assert seen['coreg'] == 'absent'
        y = [U._output(torch.zeros(4, 5, 6), eye)]
        U._init_y_dat(x, y, sett)
        assert 'pull' not in seen and type(x[0][0]).seen == 0
    # a plain struct carrying a map that raises on any use
    xn = U._input(torch.rand(4, 5, 6), eye)
    xn.ct, xn.weight = False, _Boom()
    sett = U.settings()
    sett.device = 'cpu'
    U._estimate_hyperpar([[xn], [xn]], sett)
    U._init_reg([[xn], [xn]], sett)
    U._init_y_dat([[xn]], [U._output(torch.zeros(4, 5, 6), eye)], sett)


def test_with_voxel_init_on_the_three_steps_hand_the_map_on(monkeypatch):
    import unires_amd as U
    seen = {}
    _fake_steps(monkeypatch, seen)
    eye = torch.eye(4, dtype=torch.float64)
    a, b = U._input(torch.rand(4, 5, 6), eye), U._input(torch.rand(4, 5, 6), eye)
    a.ct = b.ct = False
    b.weight = torch.ones(4, 5, 6)
    sett = U.settings()
    sett.device, sett.voxel_init = 'cpu', True
    x = [[a, b]]
    U._estimate_hyperpar(x, sett)
    assert seen['noise'][0] is None and seen['noise'][1] is b.weight
    U._init_reg(x, sett)
    assert seen['coreg'][0] is None and seen['coreg'][1] is b.weight
    U._init_y_dat(x, [U._output(torch.zeros(4, 5, 6), eye)], sett)
    assert seen['pull'] is b.weight


def test_an_observation_without_usable_voxels_is_named_with_its_weight(monkeypatch):
    import unires_amd as U
    from unires_amd import stats
    seen = {}
    _fake_steps(monkeypatch, seen)
    monkeypatch.setattr(stats, 'noise_fit', lambda counts, rng: torch.full((counts.shape[0], stats.NOUT), -1.0,
                                                                          dtype=torch.float64))
    xn = U._input(torch.rand(4, 5, 6), torch.eye(4, dtype=torch.float64))
    xn.ct, xn.weight = False, torch.zeros(4, 5, 6)
    sett = U.settings()
    sett.voxel_init = True
    with pytest.raises(ValueError, match=r'channel 0, repeat 0 .*weight > 0'):
        U._estimate_hyperpar([[xn]], sett)
    sett.voxel_init = False
    with pytest.raises(ValueError) as e:
        U._estimate_hyperpar([[xn]], sett)
    assert 'weight > 0' not in str(e.value)


# ---- validation, plumbing ----------------------------------------------------------------------------------------
def test_validation_errors_name_channel_and_repeat():
    import unires_amd as U
    from unires_amd._core import _check_init_weights
    eye = torch.eye(4, dtype=torch.float64)

    def subject():
        return [[U._input(torch.rand(3, 4, 5), eye)], [U._input(torch.rand(3, 4, 5), eye), U._input(torch.rand(3, 4, 5), eye)]]
    sett = U.settings()
    sett.voxel_init = True
    for bad in (-1.0, float('nan'), float('inf')):
        x = subject()
        x[1][1].weight = torch.ones(3, 4, 5)
        x[1][1].weight[1, 2, 3] = bad
        with pytest.raises(ValueError, match='channel 1, repeat 1'):
            _check_init_weights(x, sett)
    x = subject()
    x[1][0].weight = torch.ones(3, 4, 6)
    with pytest.raises(ValueError, match='channel 1, repeat 0'):
        _check_init_weights(x, sett)
    x = subject()
    x[0][0].weight = np.ones((3, 4, 5), np.float64)[:, ::1, :] * 2
    x[1][1].weight = torch.ones(5, 4, 3, dtype=torch.float64).permute(2, 1, 0)
    _check_init_weights(x, sett)
    for xn in (x[0][0], x[1][1]):
        assert xn.weight.dtype == torch.float32 and xn.weight.is_contiguous() and xn.weight.device == xn.dat.device
    assert x[1][0].weight is None
    sett.voxel_init = False
    x = subject()
    x[0][0].weight = _Boom()
    _check_init_weights(x, sett)


def test_settings_default_and_the_c_surface():
    import unires_amd as U
    from unires_amd import _lib
    assert U.settings().voxel_init is False
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    declared = set(re.findall(r'\b(unires_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert 'unires_coreg_job_m_t' in hdr
    assert re.search(r'#define\s+UNIRES_HIP_ABI_VERSION\s+1\b', hdr)


def test_new_symbols_are_exported(lib):
    assert lib.unires_abi_version() == 1
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None


def test_job_struct_layout_extends_the_unmasked_job():
    from unires_amd import preproc
    assert preproc.JobM.mG.offset >= preproc.Job.step.offset + preproc.Job.step.size
    for f, _ in preproc.Job._fields_:
        assert getattr(preproc.JobM, f).offset == getattr(preproc.Job, f).offset
    assert preproc.JobM.mF.offset == preproc.JobM.mG.offset + 8


# ---- planted-defect searches on the restatement ------------------------------------------------------------------
DEFECT_DIM, DEFECT_VX, DEFECT_SCALE = (48, 48, 48), (1.0, 1.0, 1.0), 0.3
DEFECT_LO, DEFECT_SIZE, DEFECT_GAIN, DEFECT_SEED = (6, 8, 28), 8, 100.0, 0
MARGIN = 0.1  # mm: a third of the 0.3 mm tests/test_gpu_coreg.py allows at 1 mm voxels


def defect_pair(dev):
    """Two contrasts of the phantom at 48^3, the moving one under a planted rigid; (imgs clean, imgs with a bright
    block fixed in the moving image's voxel coordinates, its 0-weight map, true moving matrix)."""
    g, mg = P.observation(DEFECT_DIM, DEFECT_VX, 0, 1, dev, scale=DEFECT_SCALE)
    f, mf = P.observation(DEFECT_DIM, DEFECT_VX, 1, 2, dev, scale=DEFECT_SCALE)
    Pl = P.random_rigid(np.random.default_rng(DEFECT_SEED))
    fd = f.clone()
    sl = tuple(slice(a, a + DEFECT_SIZE) for a in DEFECT_LO)
    fd[sl] = DEFECT_GAIN * float(max(P.CONTRASTS[1]))
    w = torch.ones(DEFECT_DIM, dtype=torch.float32, device=f.device)
    w[sl] = 0.0
    mats = [torch.from_numpy(mg), torch.from_numpy(Pl @ mf)]
    return [[g, mats[0]], [f, mats[1]]], [[g, mats[0]], [fd, mats[1]]], w, mf


def _restated_search(imgs, w=None):
    from unires_amd import preproc
    from unires_amd._rigid import _expm, affine_basis
    from unires_amd.spatial import _m12
    B = affine_basis()
    Gv, Fv = imgs[0][0].cpu().numpy(), imgs[1][0].cpu().numpy()
    mask = None if w is None else (w.cpu().numpy() > 0).astype(np.uint8)
    G, F = CR.quantise(Gv)[0], W.quantise(Fv, mask)[0]
    mF = None if mask is None else W.cellmask(mask)
    step = (1.0 / np.asarray(DEFECT_VX)).astype(np.float32)  # the default coreg_params: samp = 1 mm
    m_fix, m_mov = imgs[0][1].numpy(), imgs[1][1].numpy()

    def ev(reqs):
        return [CR.cost(W.hist(G, F, _m12(preproc.voxel_map(x, B, m_mov, m_fix)), step, None, mF)) for _, x in reqs]
    (res,), _ = preproc.lockstep([preproc.powell(np.zeros(6))], ev)
    return np.linalg.solve(_expm(res[0], B).numpy(), m_mov)


def test_planted_defect_searches_on_the_restatement():
    """Clean data; defect with its mask; defect without.  The masked search must come within the clean search's error
    plus 0.1 mm, and the unmasked one must be worse than the masked one by at least twice that margin: the block is
    sized so that the restatement shows it (DESIGN 8.10 records the three errors)."""
    clean, bad, w, mf = defect_pair('cpu')
    e_clean = P.rms_mm(_restated_search(clean), mf, DEFECT_DIM, scale=DEFECT_SCALE)
    e_mask = P.rms_mm(_restated_search(bad, w), mf, DEFECT_DIM, scale=DEFECT_SCALE)
    e_raw = P.rms_mm(_restated_search(bad), mf, DEFECT_DIM, scale=DEFECT_SCALE)
    print('restatement rms mm: clean %.4f masked %.4f unmasked %.4f' % (e_clean, e_mask, e_raw))
    assert e_mask <= e_clean + MARGIN, (e_clean, e_mask, e_raw)
    assert e_raw >= e_mask + 2 * MARGIN, (e_clean, e_mask, e_raw)
