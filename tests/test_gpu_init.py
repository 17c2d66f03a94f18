"""init() / preproc() on the GPU: init() against the same steps chained by hand, bit for
bit; the reconstruction of a misaligned two-contrast subject from files; the written files; the
demo's call shape; the input forms; max_iter = 0; reproducibility; the full demo size."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import coreg_phantom as P

pytestmark = pytest.mark.gpu

DIM, VX, SCALE = (64, 64, 64), (1.0, 1.0, 1.0), 0.4


def _subject(dev, seed=9):
    """The two-channel 64^3 subject of tests/test_gpu_coreg.py's end-to-end test: contrast 0 at 1 mm,
    contrast 1 in 3 mm slices along z with a planted rigid in its header.  (dat, given mat, true mat)."""
    obs, rng = [], np.random.default_rng(seed)
    for c, ax in enumerate((None, 2)):
        v, d = [1.0, 1.0, 1.0], list(DIM)
        if ax is not None:
            v[ax], d[ax] = 3.0, DIM[ax] // 3
        dat, mat = P.observation(tuple(d), tuple(v), c, 40 + c, dev, sub_axis=ax, sub=3, scale=SCALE)
        Pl = np.eye(4) if c == 0 else P.random_rigid(rng)
        obs.append((dat.cpu(), Pl @ mat, mat))
    return obs


def _write_subject(obs, folder, which='given'):
    from unires_amd import nifti
    os.makedirs(str(folder), exist_ok=True)
    paths = []
    for c, (dat, given, true) in enumerate(obs):
        paths.append(os.path.join(str(folder), 'sub-01_c%d.nii.gz' % c))
        nifti.write(paths[-1], dat.numpy(), given if which == 'given' else true)
    return paths


def _truth(mat_y, dim_y, contrast, dev):
    """The phantom, noise-free, at the voxel centres of the grid (mat_y, dim_y)."""
    ax = [torch.arange(n, dtype=torch.float32, device=dev) for n in dim_y]
    ijk = torch.stack(torch.meshgrid(*ax, indexing='ij'), -1)
    m = torch.as_tensor(mat_y, dtype=torch.float64).cpu()
    w = ijk @ m[:3, :3].T.float().to(dev) + m[:3, 3].float().to(dev)
    return torch.tensor(P.CONTRASTS[contrast], dtype=torch.float32, device=dev)[P.labels(w, SCALE)]


def _sett(dev, **kw):
    import unires_amd as U
    sett = U.settings()
    sett.device = dev
    for k, v in kw.items():
        setattr(sett, k, v)
    return sett


def _by_hand(data, dev, grid=None, label=None, **kw):
    """The steps of init() chained by hand on one observation per channel.  ``grid``: (mat_y, dim_y),
    else _format_y's; the regime is set by hand."""
    import unires_amd as U
    sett = _sett(dev, **kw)
    x = []
    for d in data:
        dat, dim, mat, fname, direc, nam, file, ct = U._read_image(d, device=dev)
        xn = U._input(dat, mat)
        xn.ct, xn.fname, xn.direc, xn.nam, xn.file = ct, fname, direc, nam, file
        x.append([xn])
    if label is not None:
        U._read_label(x[0][0], label, sett)
    if sett.max_iter > 0:
        U._estimate_hyperpar(x, sett)
    U._init_reg(x, sett)
    if grid is None:
        y0, _ = U._format_y(x, _sett(dev, **kw))
        grid = (y0[0].mat, y0[0].dim)
    mat_y, dim_y = grid
    sett.method, sett.do_proj = kw.get('method', 'super-resolution'), kw.get('do_proj', True)
    for xc in x:
        xc[0].po = U._proj_info(dim_y, mat_y, xc[0].dim, xc[0].mat, prof_ip=sett.profile_ip, prof_tp=sett.profile_tp,
                                gap=sett.gap, device=dev, ratio_tol=U._core.RATIO_TOL)  # (the ceil of _proj_info_add)
    y = [U._output(torch.zeros(dim_y, device=dev), mat_y) for _ in x]
    U._init_y_dat(x, y, sett)
    U._init_lam(x, y, sett)
    U._init_y_label(x, y, sett)
    return x, y, sett


def _same(a, b, what):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), what


def _same_structs(x, y, sett, xh, yh, sh):
    assert (sett.method, sett.do_proj) == (sh.method, sh.do_proj)
    for c in range(len(x)):
        a, b = x[c][0], xh[c][0]
        _same(a.dat, b.dat, 'dat')
        _same(a.mat, b.mat, 'mat')
        _same(a.tau, b.tau, 'tau')
        _same(a.mu, b.mu, 'mu')
        _same(a.rigid_q, b.rigid_q, 'rigid_q')
        assert tuple(a.dim) == tuple(b.dim)
        for k in ('dim_x', 'dim_y', 'dim_yx', 'ratio', 'dim_thick'):
            assert getattr(a.po, k) == getattr(b.po, k), k
        for k in ('mat_x', 'mat_y', 'mat_yx', 'vx_x', 'vx_y', 'smo_ker', 'rigid', 'scl'):
            _same(getattr(a.po, k), getattr(b.po, k), 'po.' + k)
        for k1, k2 in zip(a.po.smo_ker_1d, b.po.smo_ker_1d):
            _same(k1, k2, 'po.smo_ker_1d')
        _same(y[c].dat, yh[c].dat, 'y.dat')
        _same(y[c].mat, yh[c].mat, 'y.mat')
        _same(y[c].lam0, yh[c].lam0, 'lam0')
        assert tuple(y[c].dim) == tuple(yh[c].dim)
        assert (y[c].label is None) == (yh[c].label is None)
        if y[c].label is not None:
            _same(y[c].label, yh[c].label, 'y.label')


@pytest.mark.parametrize('with_label', [False, True])
def test_init_equals_the_steps_chained_by_hand(dev, tmp_path, with_label):
    import unires_amd as U
    from unires_amd import nifti
    obs = _subject(dev)
    paths = _write_subject(obs, tmp_path)
    kw, lab = {}, None
    if with_label:
        lab = str(tmp_path / 'label.nii.gz')
        w = _truth(obs[0][2], DIM, 0, dev)
        nifti.write(lab, (w > 500).float().cpu().numpy() * 3.0 + (w > 1000).float().cpu().numpy() * 4.0, obs[0][1])
        kw = dict(label=(lab, (0, 0)))
    x, y, sett = U.init(paths, _sett(dev, **kw))
    xh, yh, sh = _by_hand(paths, dev, label=lab)
    assert sett.method == 'super-resolution' and sett.do_proj is True and sett.clean_fov is False
    assert x[1][0].nam == 'sub-01_c1.nii.gz' and x[1][0].direc == str(tmp_path)
    _same_structs(x, y, sett, xh, yh, sh)
    if with_label:
        assert y[0].label is not None and sorted(y[0].label.unique().tolist()) == [0.0, 3.0, 7.0] and y[1].label is None
    # the mean space covers both observations at 1 mm
    assert float((U.spatial.voxel_size(y[0].mat) - 1).abs().max()) < 1e-9 and all(58 <= d <= 80 for d in y[0].dim)


def _rel(dat, truth):
    return float((dat - truth).norm() / truth.norm())


def test_preproc_reconstructs_a_misaligned_subject_from_files(dev, tmp_path):
    import unires_amd as U
    from unires_amd.run import preproc
    obs = _subject(dev)
    kw = dict(max_iter=8, sched_num=1)
    dat_y, mat_y, pth_y = preproc(_write_subject(obs, tmp_path / 'coreg'), _sett(dev, **kw))
    dim_y = tuple(dat_y.shape[:3])
    e_coreg = _rel(dat_y[..., 1], _truth(mat_y, dim_y, 1, dev))
    assert [os.path.basename(p) for p in pth_y] == ['u_sub-01_c0.nii.gz', 'u_sub-01_c1.nii.gz'] and all(os.path.isfile(p) for p in pth_y)
    # the same steps by hand with the true headers, on the same grid
    x, y, sett = _by_hand(_write_subject(obs, tmp_path / 'true', 'true'), dev, grid=(mat_y, dim_y), do_coreg=False, **kw)
    U.fit(x, y, sett)
    dat_t = U._write_data(x, y, _sett(dev, write_out=False))[0]
    e_true = _rel(dat_t[..., 1], _truth(mat_y, dim_y, 1, dev))
    # and preproc() without coregistration (on its own mean space)
    dat_n, mat_n, _ = preproc(_write_subject(obs, tmp_path / 'none'), _sett(dev, do_coreg=False, **kw))
    e_none = _rel(dat_n[..., 1], _truth(mat_n, tuple(dat_n.shape[:3]), 1, dev))
    print('relative error of channel 1: coreg %.4f, true headers %.4f, no coreg %.4f' % (e_coreg, e_true, e_none))
    assert e_coreg <= 1.1 * e_true, (e_none, e_coreg, e_true)
    assert e_coreg < 0.7 * e_none, (e_none, e_coreg, e_true)


def test_written_files(dev, tmp_path):
    from unires_amd import nifti
    from unires_amd.run import preproc
    obs = _subject(dev)
    paths = _write_subject(obs, tmp_path / 'in')
    fast = dict(max_iter=0, do_coreg=False)
    before = set(glob.glob(str(tmp_path / '**' / '*'), recursive=True))
    dat_y, mat_y, pth_y = preproc(paths, _sett(dev, write_out=False, **fast))
    assert pth_y == [] and set(glob.glob(str(tmp_path / '**' / '*'), recursive=True)) == before
    for kw, names, folder in ((dict(), ['u_sub-01_c0.nii.gz', 'u_sub-01_c1.nii.gz'], tmp_path / 'in'),
                              (dict(prefix='sr_', dir_out=str(tmp_path / 'out' / 'a')), ['sr_sub-01_c0.nii.gz', 'sr_sub-01_c1.nii.gz'], tmp_path / 'out' / 'a'),
                              (dict(bids=True, dir_out=str(tmp_path / 'out' / 'b')),
                               ['u_sub-01_space-unires_c0.nii.gz', 'u_sub-01_space-unires_c1.nii.gz'], tmp_path / 'out' / 'b')):
        dat_y, mat_y, pth_y = preproc(paths, _sett(dev, **fast, **kw))
        assert sorted(os.listdir(str(folder)) if kw else [n for n in os.listdir(str(folder)) if n.startswith('u_')]) == names
        assert [os.path.dirname(p) for p in pth_y] == [str(folder)] * 2
        for c, n in enumerate(names):
            vox, aff, _ = nifti.read(os.path.join(str(folder), n))
            assert np.array_equal(vox, dat_y[..., c].cpu().numpy())
            assert np.array_equal(aff, mat_y.numpy().astype(np.float32).astype(np.float64))  # (float32 sform)


def test_demo_call_shape(dev):
    """preproc([[dat, eye(4)]]) with vx = 1 (demos/simple_api_use.py of the reference)."""
    import unires_amd as U
    from unires_amd.run import preproc
    dat = P.observation((48, 56, 40), VX, 0, 3, dev, scale=0.35)[0].abs()
    kw = dict(vx=1.0, write_out=False, reg_scl=1.0, ct=False, max_iter=6)
    x, y, sett = U.init([[dat.clone(), torch.eye(4, device=dev)]], _sett(dev, **kw))
    assert sett.method == 'denoising' and sett.do_proj is False and sett.clean_fov is True and sett.unified_rigid is False
    assert y[0].dim == (48, 56, 40) and torch.equal(y[0].mat, torch.eye(4, dtype=torch.float64))
    y_hat, mat_y, pth_y = preproc([[dat.clone(), torch.eye(4, device=dev)]], _sett(dev, **kw))
    assert pth_y == [] and y_hat.shape == (48, 56, 40, 1) and y_hat.dtype == torch.float32
    # fit() on structs built by hand
    xh, yh, sh = _by_hand([[dat.clone(), torch.eye(4)]], dev, grid=(torch.eye(4, dtype=torch.float64), (48, 56, 40)),
                          method='denoising', do_proj=False, **kw)
    sh.clean_fov = True
    out = U.fit(xh, yh, sh)[0][..., 0]
    out = torch.minimum(torch.maximum(out, dat.min()), dat.max())
    assert torch.equal(y_hat[..., 0], out)
    assert float((y_hat[..., 0] - dat).abs().max()) > 0  # (something was denoised)


def test_input_forms_give_the_same_bits(dev, tmp_path):
    from unires_amd import nifti
    from unires_amd.run import preproc
    dim = (32, 32, 32)
    mat = P.true_mat(dim, (2.0, 2.0, 2.0))  # (exact in the float32 sform of a file)
    dats = [P.observation(dim, (2.0, 2.0, 2.0), c, 60 + c, dev, scale=0.45)[0] for c in range(2)]
    arr = torch.stack(dats, -1)
    p4 = str(tmp_path / 'four.nii.gz')
    nifti.write(p4, arr.cpu().numpy(), mat)
    kw = dict(max_iter=3, vx=0)
    res = {}
    for name, data, extra in (('array', arr.clone(), dict(mat=torch.from_numpy(mat), dir_out=str(tmp_path / 'array'))),
                              ('numpy array', arr.cpu().numpy(), dict(mat=mat, write_out=False)),
                              ('4-D path', p4, dict(dir_out=str(tmp_path / 'path'))),
                              ('pairs', [[d.clone(), torch.from_numpy(mat)] for d in dats], dict(write_out=False))):
        res[name] = preproc(data, _sett(dev, **kw, **extra))
    for name in ('numpy array', '4-D path', 'pairs'):
        assert torch.equal(res[name][0], res['array'][0]) and torch.equal(res[name][1], res['array'][1]), name
    assert res['array'][0].shape == dim + (2,)
    # given as one array with sett.mat: one 4-D file
    assert os.listdir(str(tmp_path / 'array')) == ['u_0.nii.gz'] and res['array'][2] == [str(tmp_path / 'array' / 'u_0.nii.gz')]
    vox = nifti.read(res['array'][2][0])[0]
    assert vox.shape == dim + (2,) and np.array_equal(vox, res['array'][0].cpu().numpy())
    # a 4-D file sets no sett.mat: the reference's _write_data then writes one file per channel
    assert sorted(os.listdir(str(tmp_path / 'path'))) == ['u_0.nii.gz', 'u_1.nii.gz']


def test_max_iter_zero_writes_the_clamped_initial_guess(dev, tmp_path):
    import unires_amd as U
    from unires_amd.run import preproc
    obs = _subject(dev)
    paths = _write_subject(obs, tmp_path)
    x, y, sett = U.init(paths, _sett(dev, max_iter=0))
    assert float(x[0][0].tau) == 1.0 and float(x[0][0].mu) == 1.0  # (no hyper-parameter estimate)
    want = [torch.minimum(torch.maximum(y[c].dat, x[c][0].dat.min()), x[c][0].dat.max()) for c in range(2)]
    dat_y, mat_y, pth_y = preproc(paths, _sett(dev, max_iter=0))
    for c in range(2):
        assert torch.equal(dat_y[..., c], want[c])
    assert torch.equal(mat_y, y[0].mat) and len(pth_y) == 2


def test_preproc_is_reproducible(dev, tmp_path):
    from unires_amd import nifti
    from unires_amd.run import preproc
    obs = _subject(dev)
    out = []
    for tag in ('a', 'b'):
        dat_y, mat_y, pth_y = preproc(_write_subject(obs, tmp_path / tag), _sett(dev, max_iter=4, sched_num=1))
        out.append((dat_y.cpu().numpy().tobytes(), mat_y.numpy().tobytes(), [nifti.read(p)[0].tobytes() for p in pth_y]))
    assert out[0] == out[1]


@pytest.mark.slow
def test_init_at_the_full_demo_size(dev):
    """Three contrasts of 181 x 217 x 181 at 1 mm in 4 mm slices along x, y and z, planted rigids of
    +-5 mm and +-0.1 rad."""
    import unires_amd as U
    from unires_amd._project import _channel_plan
    from tests.test_init import _corner_range
    dim, rng = (181, 217, 181), np.random.default_rng(3)
    data, given = [], []
    for c, ax in enumerate((0, 1, 2)):
        v, d = [1.0, 1.0, 1.0], list(dim)
        v[ax], d[ax] = 4.0, int(round(dim[ax] / 4.0))
        dat, mat = P.observation(tuple(d), tuple(v), c, 103 + c, dev, sub_axis=ax)
        Pl = np.eye(4) if c == 0 else P.random_rigid(rng, 5.0, 0.1)
        data.append([dat, torch.from_numpy(Pl @ mat)])
        given.append((Pl @ mat, d))
    x, y, sett = U.init(data, _sett(dev))
    assert sett.method == 'super-resolution' and sett.do_proj is True
    mats = np.stack([xc[0].mat.cpu().numpy() for xc in x])
    dims = np.array([xc[0].dim for xc in x], dtype=np.float64)
    mat_y, dim_y = y[0].mat.numpy(), np.array(y[0].dim, dtype=np.float64)
    A = mat_y[:3, :3]
    assert np.abs(A.T @ A - np.eye(3)).max() < 1e-9 and np.linalg.det(A) > 0
    lo, hi = _corner_range(mat_y, mats, dims)
    assert (lo >= -1e-9).all() and (hi <= dim_y - 1 + 1e-9).all() and ((dim_y - 1) - (hi - lo) < 2).all()
    for c in range(3):
        assert bool(torch.isfinite(y[c].dat).all()) and float(y[c].dat.max()) > 0
        assert x[c][0].po.ratio == tuple(4 if a == c else 1 for a in range(3)) and x[c][0].po.dim_thick == c
        info = _channel_plan(x[c], y[c], sett.method, sett.do_proj).repeat_info(0)
        assert info['pull2'] and info['splat2_axis'] in (0, 1, 2) and not info['separable'], (c, info)
