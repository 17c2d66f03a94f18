"""init() on the host: properties of the mean space (spatial._mean_space), _format_y / _read_data /
_write_data pinned against the reference's own functions where its sources are at hand, the settings
that are refused, the new settings defaults and the exports."""
import importlib
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import unires_amd
from unires_amd import _core, _math, _util, nifti, spatial, struct
from tests.helpers import SIGNED_PERMS, orient_axes, rigid_matrix


# ---- mean-space properties ------------------------------------------------------------------------
def _subject(seed):
    """2 - 4 observations of roughly 96 x 110 x 90 at 1 mm, about half of them with one axis in 4 mm
    slices, each under a random rigid of +-10 mm and +-0.2 rad."""
    rng = np.random.default_rng(seed)
    mats, dims = [], []
    for _ in range(int(rng.integers(2, 5))):
        dim = np.array([96, 110, 90]) + rng.integers(-6, 7, 3)
        vx = np.ones(3)
        if rng.random() < 0.5:
            ax = int(rng.integers(0, 3))
            vx[ax], dim[ax] = 4.0, dim[ax] // 4
        base = np.diag(list(vx) + [1.0])
        base[:3, 3] = -(dim - 1) / 2.0 * vx
        R = rigid_matrix(rng.uniform(-10, 10, 3).tolist(), rng.uniform(-0.2, 0.2, 3).tolist()).numpy()
        mats.append(R @ base)
        dims.append(dim)
    return np.stack(mats), np.stack(dims).astype(np.float64)


def _corner_range(mat, Mat, Dim):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for m, d in zip(Mat, Dim):
        c = np.array([[i, j, k, 1.0] for i in (0, d[0] - 1) for j in (0, d[1] - 1) for k in (0, d[2] - 1)])
        p = (np.linalg.solve(mat, m) @ c.T)[:3]
        lo, hi = np.minimum(lo, p.min(1)), np.maximum(hi, p.max(1))
    return lo, hi


@pytest.mark.parametrize('seed', range(24))
def test_mean_space_properties(seed):
    Mat, Dim = _subject(seed)
    mat, dim, vx = spatial._mean_space(torch.from_numpy(Mat), torch.from_numpy(Dim), torch.ones(3, dtype=torch.float64))
    assert mat.dtype == dim.dtype == vx.dtype == torch.float64 and mat.shape == (4, 4) and dim.shape == (3,)
    mat, dim = mat.numpy(), dim.numpy()
    assert vx.tolist() == [1.0, 1.0, 1.0] and (dim == np.round(dim)).all()
    A = mat[:3, :3]
    dev = np.abs(A.T @ A - np.eye(3)).max()
    lo, hi = _corner_range(mat, Mat, Dim)
    slack = ((dim - 1) - (hi - lo)).max()
    # the same subject with its observations in reverse order
    m2, d2, _ = spatial._mean_space(Mat[::-1].copy(), Dim[::-1].copy(), 1.0)
    dev_order = np.abs(m2.numpy() - mat).max()
    # one observation stored under a signed axis permutation: every observation under all 48 at the step that
    # undoes the storage (the only place the function reads it, beside the corners) ...
    for k in range(len(Mat)):
        want = spatial._canonical(Mat[k], Dim[k])
        for perm, flip in SIGNED_PERMS:
            d3, m3 = orient_axes(tuple(int(v) for v in Dim[k]), torch.from_numpy(Mat[k]), perm, flip)
            assert np.abs(spatial._canonical(m3.numpy(), np.array(d3, dtype=np.float64)) - want).max() < 1e-9, (k, perm, flip)
    # ... and through the whole function: all 48 on three subjects, two on each of the others (about 0.4 s a call)
    k = seed % len(Mat)
    dev_perm = 0.0
    for perm, flip in (SIGNED_PERMS if seed < 3 else [SIGNED_PERMS[(7 * seed + 3) % 48], SIGNED_PERMS[(11 * seed + 20) % 48]]):
        d3, m3 = orient_axes(tuple(int(v) for v in Dim[k]), torch.from_numpy(Mat[k]), perm, flip)
        Mat3, Dim3 = Mat.copy(), Dim.copy()
        Mat3[k], Dim3[k] = m3.numpy(), d3
        m4, d4, _ = spatial._mean_space(Mat3, Dim3, (1.0, 1.0, 1.0))
        dev_perm = max(dev_perm, np.abs(m4.numpy() - mat).max())
        assert (d4.numpy() == dim).all(), (perm, flip)
    print('seed %d: orthogonality %.3g, slack %.4f, order %.3g, storage %.3g' % (seed, dev, slack, dev_order, dev_perm))
    assert dev < 1e-9 and np.linalg.det(A) > 0
    assert (lo >= -1e-9).all() and (hi <= dim - 1 + 1e-9).all(), (lo, hi, dim)
    assert ((dim - 1) - (hi - lo) < 2).all()  # floor + ceil: less than two voxels to spare per axis
    assert dev_order < 1e-9 and (d2.numpy() == dim).all()
    assert dev_perm < 1e-9


@pytest.mark.parametrize('vx, off, dim', [((0.9, 0.9, 0.9), (-90.3, -126.7, -72.1), (200, 240, 180)),
                                          ((0.4297, 0.4297, 3.3), (-110.0, -110.2, -60.5), (512, 512, 40)),
                                          ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (64, 64, 64)),
                                          ((1.0, 1.0, 4.0), (-90.3, -126.7, -72.1), (181, 217, 45))])
def test_mean_space_of_identical_axial_grids_is_their_grid(vx, off, dim):
    M = np.diag(list(vx) + [1.0])
    M[:3, 3] = off
    for n in (1, 2, 5):
        for v in (None, vx):
            mat, d, v_out = spatial._mean_space(np.stack([M] * n), np.array([dim] * n, dtype=np.float64), v)
            assert np.abs(mat.numpy() - M).max() < 1e-12
            assert tuple(int(a) for a in d.tolist()) == dim
            assert np.abs(v_out.numpy() - np.array(vx)).max() < 1e-12


def test_mean_space_applies_the_voxel_size_and_checks_its_arguments():
    Mat, Dim = _subject(3)
    mat, dim, vx = spatial._mean_space(Mat, Dim, (0.5, 1.0, 2.0))
    assert np.abs(spatial.voxel_size(mat).numpy() - [0.5, 1.0, 2.0]).max() < 1e-12 and vx.tolist() == [0.5, 1.0, 2.0]
    lo, hi = _corner_range(mat.numpy(), Mat, Dim)
    assert (lo >= -1e-9).all() and (hi <= dim.numpy() - 1 + 1e-9).all()
    mat, _, vx = spatial._mean_space(Mat, Dim)  # the mean's own voxel size
    A = mat.numpy()[:3, :3]
    assert (vx.numpy() > 0).all() and np.abs(A.T @ A - np.diag(vx.numpy() ** 2)).max() < 1e-9 and np.linalg.det(A) > 0
    with pytest.raises(ValueError):
        spatial._mean_space(Mat, Dim[:1])


def test_ceil_pow_round_and_affine_matrix_classic():
    t = torch.tensor([1.0, 2.0, 3.0, 5.0, 96.0, 97.0, 128.0, 200.0, 300.0], dtype=torch.float64)
    assert _math.ceil_pow(t, p=2.0, l=2.0).tolist() == [2, 2, 4, 8, 128, 128, 128, 256, 512]
    assert _math.ceil_pow(t, p=2.0, l=3.0).tolist() == [3, 3, 3, 6, 96, 192, 192, 384, 384]
    assert _math.ceil_pow(t, p=2.0, l=3.0, mx=256).tolist() == [3, 3, 3, 6, 96, 192, 192, 256, 256]
    out = _math.ceil_pow(t)
    out[0] = -1.0
    assert t[0] == 1.0  # (a new tensor: the reference writes into the result)
    assert _math.round(torch.tensor([1.23449, -0.0005001, 2.0]), 3).tolist() == pytest.approx([1.234, -0.001, 2.0])
    T = spatial.affine_matrix_classic(torch.tensor([1.0, -2.0, 3.5]))
    assert T.dtype == torch.float64 and T[:3, 3].tolist() == [1.0, -2.0, 3.5] and torch.equal(T[:3, :3], torch.eye(3, dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        spatial.affine_matrix_classic(torch.zeros(6))


# ---- pins against the reference's own code ---------------------------------------------------------
def _raiser(name):
    def f(*a, **k):
        raise AssertionError('placeholder for nitorch.%s called' % name)
    return f


@pytest.fixture(scope='module')
def ref_core():
    """unires/_core.py of the reference, imported as it lies with nitorch bound to the oracle (the shim
    of tests/golden/make_golden_from_reference.py), the names it imports beyond the hot path stubbed,
    and the nitorch functions of this feature bound to this package's; sys.modules / sys.path are
    restored afterwards."""
    G = importlib.import_module('tests.golden.make_golden_from_reference')
    if not os.path.isfile(os.path.join(G.REF, 'unires', '_core.py')):
        pytest.skip('reference sources absent')
    mods, path = dict(sys.modules), list(sys.path)
    try:
        G.install_nitorch_shim()
        extra = {'nitorch.tools': [], 'nitorch.tools.preproc': ['atlas_crop', 'affine_align', 'atlas_align', 'reset_origin'],
                 'nitorch.tools.img_statistics': ['estimate_fwhm', 'estimate_noise'],
                 'nitorch.tools._preproc_fov': ['_bb_atlas'], 'nitorch.tools._preproc_utils': ['_mean_space'],
                 'nitorch.core.constants': ['inf'], 'nitorch.core.utils': ['ceil_pow']}
        for name, attrs in extra.items():
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, _raiser(a))
            sys.modules[name] = m
        for a in ('affine_matrix_classic', 'affine_basis', 'max_bb'):
            setattr(sys.modules['nitorch.spatial'], a, _raiser(a))
        sys.path.insert(0, G.REF)
        for k in [k for k in sys.modules if k == 'unires' or k.startswith('unires.')]:
            del sys.modules[k]
        RC = importlib.import_module('unires._core')
        assert RC.__file__.startswith(G.REF)
        RC._mean_space, RC.voxel_size, RC.affine_matrix_classic = spatial._mean_space, spatial.voxel_size, spatial.affine_matrix_classic
        RC.round, RC.ceil_pow, RC.map, RC.inf = _math.round, _math.ceil_pow, nifti.map_file, math.inf
        RC._read_image, RC._write_image, RC._read_label = _util._read_image, _util._write_image, _util._read_label
        RC.settings = importlib.import_module('unires.struct').settings
        yield RC
    finally:
        for k in [k for k in sys.modules if k not in mods]:
            del sys.modules[k]
        sys.modules.update(mods)
        sys.path[:] = path


def _grid(dim, vx, off=(0.0, 0.0, 0.0), rigid=None):
    m = torch.diag(torch.tensor(list(vx) + [1.0], dtype=torch.float64))
    m[:3, 3] = -(torch.tensor(dim, dtype=torch.float64) - 1) / 2 * torch.tensor(vx, dtype=torch.float64) \
        + torch.tensor(off, dtype=torch.float64)
    return dim, (m if rigid is None else rigid @ m)


def _obs(make, grids, mu=(300.0, 500.0, 700.0, 900.0), ct=()):
    """x[c][n] structs (``make()``: the struct class) of the (dim, mat) grids, one list per channel."""
    x, i = [], 0
    for chan in grids:
        xc = []
        for dim, mat in chan:
            xn = make()
            xn.dat, xn.dim, xn.mat = torch.zeros(1), tuple(dim), mat.clone()
            xn.mu, xn.ct = torch.tensor(mu[i % len(mu)]), i in ct
            xc.append(xn)
            i += 1
        x.append(xc)
    return x


_R1 = rigid_matrix((3.0, -2.0, 1.5), (0.05, -0.03, 0.08))
_R2 = rigid_matrix((-4.0, 1.0, 2.5), (-0.02, 0.06, 0.01))
_G = _grid((40, 44, 36), (1.0, 1.0, 1.0))
FORMAT_CASES = {
    'single image': dict(grids=[[_G]]),
    'single image, vx 0': dict(grids=[[_grid((40, 44, 12), (0.9, 0.9, 3.0))]], vx=0),
    'single image, finer vx': dict(grids=[[_G]], vx=0.5),
    'identical grids': dict(grids=[[_G], [_G]]),
    'identical grids, repeats': dict(grids=[[_G, _G], [_G]], vx=None),
    'identical grids, unified_rigid': dict(grids=[[_G], [_G]], unified_rigid=True),
    'same voxel size, different FOV': dict(grids=[[_G], [_grid((38, 40, 42), (1.0, 1.0, 1.0), (2.0, 0.5, -1.0), _R1)]]),
    'same voxel size, different FOV, scaling asked': dict(grids=[[_G], [_grid((38, 40, 42), (1.0, 1.0, 1.0), rigid=_R2)]],
                                                          scaling=True, vx=(1.0, 1.0, 1.0)),
    'thick slices': dict(grids=[[_grid((40, 44, 9), (1.0, 1.0, 4.0), rigid=_R1)], [_grid((10, 44, 36), (4.0, 1.0, 1.0), rigid=_R2)]],
                         scaling=True),
    'thick slices, vx tuple': dict(grids=[[_grid((40, 44, 9), (1.0, 1.0, 4.0))], [_G]], vx=(1.0, 1.0, 2.0)),
    'thick slices, vx int': dict(grids=[[_grid((40, 44, 9), (1.0, 1.0, 4.0)), _G]], vx=2),
    'same coarse voxels, vx None': dict(grids=[[_grid((20, 22, 18), (2.0, 2.0, 2.0), rigid=_R1)], [_grid((20, 22, 18), (2.0, 2.0, 2.0))]],
                                        vx=None),
    'pow int': dict(grids=[[_G], [_grid((40, 44, 9), (1.0, 1.0, 4.0), rigid=_R1)]], pow=256),
    'pow int, capped': dict(grids=[[_G], [_grid((40, 44, 9), (1.0, 1.0, 4.0), rigid=_R1)]], pow=48),
    'pow int, identical grids': dict(grids=[[_G], [_G]], pow=64),
    'pow tuple': dict(grids=[[_G], [_grid((40, 44, 9), (1.0, 1.0, 4.0), rigid=_R2)]], pow=(64, 48, 33)),
    'single CT': dict(grids=[[_grid((40, 44, 9), (1.0, 1.0, 4.0))]], ct=(0,), scaling=True),
    'CT in super-resolution': dict(grids=[[_grid((40, 44, 9), (1.0, 1.0, 4.0)), _G], [_G]], ct=(0, 2)),
    'CT in denoising': dict(grids=[[_G], [_G]], ct=(1,)),
}


@pytest.mark.parametrize('name', list(FORMAT_CASES))
def test_format_y_pins_reference(ref_core, name):
    case = FORMAT_CASES[name]

    def run(fmt, make, sett):
        sett.device, sett.do_print = 'cpu', 0
        for k in ('vx', 'pow', 'unified_rigid', 'scaling'):
            if k in case:
                setattr(sett, k, case[k])
        x = _obs(make, case['grids'], ct=case.get('ct', ()))
        return fmt(x, sett)
    y_ref, s_ref = run(ref_core._format_y, ref_core._input, ref_core.settings())
    y, s = run(_core._format_y, struct._input, struct.settings())
    for k in ('method', 'do_proj', 'scaling', 'unified_rigid', 'clean_fov'):
        assert getattr(s, k) == getattr(s_ref, k) and type(getattr(s, k)) is type(getattr(s_ref, k)), k
    assert len(y) == len(y_ref)
    for yc, rc in zip(y, y_ref):
        assert tuple(yc.dim) == tuple(rc.dim) and all(isinstance(d, int) for d in yc.dim)
        assert yc.mat.dtype == torch.float64 and float((yc.mat - rc.mat).abs().max()) <= 1e-12
        assert abs(float(yc.lam0) - float(rc.lam0)) <= 1e-12 * abs(float(rc.lam0))
        assert float(yc.lam) == float(yc.lam0)
    print(name, s.method, s.do_proj, y[0].dim)


def test_format_y_regimes():
    # the three operator regimes, and the values the pins above agree on
    def fmt(grids, **kw):
        sett = struct.settings()
        sett.device = 'cpu'
        for k, v in kw.items():
            setattr(sett, k, v)
        y, sett = _core._format_y(_obs(struct._input, grids, **({'ct': kw.pop('ct')} if 'ct' in kw else {})), sett)
        return y, sett
    y, s = fmt([[_G], [_G]])
    assert (s.method, s.do_proj) == ('denoising', False) and y[0].dim == (40, 44, 36) and torch.equal(y[0].mat, _G[1])
    assert float(y[0].lam0) == pytest.approx(math.sqrt(0.5) / 300.0) and float(y[1].lam0) == pytest.approx(math.sqrt(0.5) / 500.0)
    y, s = fmt([[_G]], unified_rigid=True)
    assert s.unified_rigid is False and s.clean_fov is True and s.do_proj is False
    y, s = fmt([[_G], [_grid((38, 40, 42), (1.0, 1.0, 1.0), rigid=_R1)]], scaling=True)
    assert (s.method, s.do_proj, s.scaling) == ('denoising', True, False)
    y, s = fmt([[_G], [_grid((40, 44, 9), (1.0, 1.0, 4.0), rigid=_R1)]], scaling=True)
    assert (s.method, s.do_proj, s.scaling) == ('super-resolution', True, True)
    assert np.abs(spatial.voxel_size(y[0].mat).numpy() - 1).max() < 1e-12
    y, s = fmt([[_G], [_grid((40, 44, 9), (1.0, 1.0, 4.0), rigid=_R1)]], pow=(64, 48, 33))
    assert y[0].dim == (64, 48, 33)
    with pytest.raises(ValueError, match='sett.vx'):
        fmt([[_G], [_grid((40, 44, 9), (1.0, 1.0, 4.0))]], vx=0)


def _files(tmp_path):
    g = torch.Generator().manual_seed(5)
    dats = [torch.rand((7, 6, 5), generator=g) * 100 for _ in range(3)]
    dats[1][0, 0, 0] = float('nan')
    mats = [_grid((7, 6, 5), (1.0, 1.0, 2.0), (0.5, 0.25, -1.0))[1], _grid((7, 6, 5), (1.0, 1.0, 2.0))[1], _G[1]]
    os.makedirs(str(tmp_path / 'in'), exist_ok=True)
    paths = [str(tmp_path / 'in' / ('im%d.nii.gz' % i)) for i in range(3)]
    for p, d, m in zip(paths, dats, mats):
        nifti.write(p, d.numpy(), m.numpy())
    p4 = str(tmp_path / 'in' / 'four.nii')
    nifti.write(p4, torch.stack(dats, -1).numpy(), mats[0].numpy())
    lab = str(tmp_path / 'in' / 'lab.nii.gz')
    nifti.write(lab, (dats[0] > 50).float().numpy(), mats[0].numpy())
    return dats, mats, paths, p4, lab


def _same_x(x, xr):
    assert [len(xc) for xc in x] == [len(xc) for xc in xr]
    for a, b in zip(sum(x, []), sum(xr, [])):
        assert torch.equal(a.dat, b.dat) and a.dat.dtype == torch.float32 and bool(torch.isfinite(a.dat).all())
        assert torch.equal(a.mat, b.mat) and tuple(a.dim) == tuple(b.dim)
        assert (a.fname, a.direc, a.nam, a.ct) == (b.fname, b.direc, b.nam, b.ct)
        assert (a.label is None) == (b.label is None)
        if a.label is not None:
            assert torch.equal(a.label[0], b.label[0])


def test_read_data_pins_reference(ref_core, tmp_path):
    dats, mats, paths, p4, lab = _files(tmp_path)
    pair = [[d.clone(), m.clone()] for d, m in zip(dats, mats)]
    arr = torch.stack(dats, -1)
    forms = {
        'one path': (paths[0], {}), 'list of paths': (paths[:2], {}), 'repeats': ([[paths[0], paths[1]], [paths[2]]], {}),
        'one pair': ([pair[0]], {}), 'pairs': (pair[:2], {}), 'pair repeats': ([[pair[0], pair[1]], [pair[2]]], {}),
        'numpy pairs': ([[dats[0].numpy(), mats[0].numpy()]], {}),
        'array with sett.mat': (arr, dict(mat=mats[0])), 'numpy array with sett.mat': (arr.numpy(), dict(mat=mats[0].numpy())),
        '4-D NIfTI': (p4, {}), 'CT': (paths[:2], dict(ct=True)),
        'label': ([[paths[0], paths[1]], [paths[2]]], dict(label=(lab, (0, 0)))),
        'label on a repeat': ([[paths[1], paths[0]]], dict(label=(lab, (0, 1)))),
    }
    for name, (data, kw) in forms.items():
        def run(read, sett):
            sett.device, sett.do_print = 'cpu', 0
            for k, v in kw.items():
                setattr(sett, k, v)
            return read(data, sett)
        x, xr = run(_core._read_data, struct.settings()), run(ref_core._read_data, ref_core.settings())
        _same_x(x, xr)
        print(name, [[tuple(xn.dim) for xn in xc] for xc in x])
    x = _core._read_data(p4, types.SimpleNamespace(mat=None, device='cpu', ct=False, label=None, do_print=0))
    assert len(x) == 3 and torch.equal(x[2][0].dat, dats[2]) and x[0][0].fname is None
    x = _core._read_data([[paths[0], paths[1]], [paths[2]]], struct_settings_cpu())
    assert x[0][1].nam == 'im1.nii.gz' and x[0][1].direc == str(tmp_path / 'in') and x[0][1].dat[0, 0, 0] == 0
    assert x[1][0].file['dim'] == (7, 6, 5)


def struct_settings_cpu(**kw):
    sett = struct.settings()
    sett.device = 'cpu'
    for k, v in kw.items():
        setattr(sett, k, v)
    return sett


def test_read_data_errors(ref_core, tmp_path):
    dats, mats, paths, p4, lab = _files(tmp_path)
    arr = torch.stack(dats, -1)
    for read, make in ((_core._read_data, struct_settings_cpu), (ref_core._read_data, lambda: _ref_sett(ref_core))):
        with pytest.raises(ValueError, match='Image data given as array, please also provide affine matrix in sett.mat!'):
            read(arr, make())
        with pytest.raises(ValueError, match='Input image dimension required to be 3D, recieved 4D!'):
            read([[arr, mats[0]]], make())
        s = make()
        s.label = (str(tmp_path / 'in' / 'lab_other.nii'), (0, 0))
        nifti.write(s.label[0], np.zeros((7, 6, 4), dtype=np.float32), np.eye(4))
        with pytest.raises(ValueError, match='Incorrect label dimensions.'):
            read([paths[2]], s)


def _ref_sett(ref_core, **kw):
    sett = ref_core.settings()
    sett.device, sett.do_print = 'cpu', 0
    for k, v in kw.items():
        setattr(sett, k, v)
    return sett


def _walk(root):
    return {os.path.join(d, n) for d, _, names in os.walk(str(root)) for n in names}


@pytest.mark.parametrize('case', ['paths', 'pairs', 'array', 'label', 'bids', 'dir_out', 'no write'])
def test_write_data_pins_reference(ref_core, tmp_path, case):
    mat_y = _grid((6, 7, 8), (1.0, 1.0, 1.0), (0.123456789, 2.0, -3.0))[1]
    g = torch.Generator().manual_seed(7)
    recon = [torch.rand((6, 7, 8), generator=g) * 140 - 20 for _ in range(3)]  # (values beyond the observations' range)
    out = {}
    for tag in ('ours', 'ref'):  # each side in a tree of its own with the same inputs
        root = tmp_path / tag
        os.makedirs(str(root))
        dats, mats, paths, p4, lab = _files(root)
        kw, data = {}, [[paths[0], paths[1]], [paths[2]]]
        if case == 'pairs':
            data = [[[dats[0], mats[0]]], [[dats[1], mats[1]]]]
        elif case == 'array':
            data, kw = torch.stack(dats, -1), dict(mat=mats[0])
        elif case == 'label':
            kw = dict(label=(lab, (0, 0)), prefix='v_')
        elif case == 'bids':
            os.rename(paths[0], str(root / 'in' / 'sub-01_T1w.nii.gz'))
            data = [str(root / 'in' / 'sub-01_T1w.nii.gz'), paths[2]]
            kw = dict(bids=True)
        elif case == 'dir_out':
            kw = dict(dir_out=str(root / 'elsewhere' / 'deep'), prefix='den_')
        elif case == 'no write':
            kw = dict(write_out=False)
        if tag == 'ours':
            read, write, sett, outp = _core._read_data, _core._write_data, struct_settings_cpu(**kw), struct._output
        else:
            read, write, sett, outp = ref_core._read_data, ref_core._write_data, _ref_sett(ref_core, **kw), ref_core._output
        before, cwd = _walk(root), os.getcwd()
        os.chdir(str(root))  # ('UniRes-output' is relative)
        try:
            x = read(data, sett)
            y = []
            for c in range(len(x)):
                yc = outp()
                yc.dat, yc.mat, yc.dim = recon[c].clone(), mat_y.clone(), (6, 7, 8)
                yc.label = (recon[c] > 60).float() if (case == 'label' and c == 0) else None
                y.append(yc)
            dat_y, pth_y, label, pth_label = write(x, y, sett)
        finally:
            os.chdir(cwd)
        for c, yc in enumerate(y):  # clamped in place
            assert torch.equal(yc.dat, dat_y[..., c])
        files = {os.path.relpath(p, str(root)): nifti.read(p)[:2] for p in sorted(_walk(root) - before)}
        rel = lambda p: None if p is None else p.replace(str(root), '<root>')  # noqa: E731
        out[tag] = (dat_y, [rel(p) for p in pth_y], label, rel(pth_label), files)
    (dat_y, pth_y, label, pth_label, files), (r_dat, r_pth, r_label, r_pth_label, r_files) = out['ours'], out['ref']
    assert torch.equal(dat_y, r_dat) and dat_y.shape == r_dat.shape and dat_y.dtype == r_dat.dtype
    assert pth_y == r_pth and pth_label == r_pth_label
    assert (label is None) == (r_label is None) and (label is None or torch.equal(label, r_label))
    assert sorted(files) == sorted(r_files), (sorted(files), sorted(r_files))
    for k in files:
        assert np.array_equal(files[k][0], r_files[k][0]) and np.array_equal(files[k][1], r_files[k][1])
    # ... and what those agreeing values are
    assert float(dat_y[..., 0].min()) >= 0.0 and float(dat_y[..., 0].max()) <= 100.0 and float(recon[0].max()) > 100.0
    j = os.path.join
    want = {'paths': [j('in', 'u_im0.nii.gz'), j('in', 'u_im2.nii.gz')],
            'pairs': [j('UniRes-output', 'u_0.nii.gz'), j('UniRes-output', 'u_1.nii.gz')],
            'array': [j('UniRes-output', 'u_0.nii.gz')],
            'label': [j('in', 'v_im0.nii.gz'), j('in', 'v_im2.nii.gz'), j('in', 'v_label_im0.nii.gz')],
            'bids': [j('in', 'u_sub-01_space-unires_T1w.nii.gz'), j('in', 'u_space-unires_im2.nii.gz')],
            'dir_out': [j('elsewhere', 'deep', 'den_im0.nii.gz'), j('elsewhere', 'deep', 'den_im2.nii.gz')],
            'no write': []}[case]
    assert sorted(files) == sorted(want)
    if case == 'no write':
        assert pth_y == [] and dat_y.shape == (6, 7, 8, 2)
    elif case == 'array':
        assert np.array_equal(files[want[0]][0], dat_y.numpy()) and dat_y.shape == (6, 7, 8, 3)
        assert pth_y == [want[0]]
    elif case == 'bids':  # (the reference returns the names from before the tag is added)
        assert pth_y == [j('<root>', 'in', 'u_sub-01_T1w.nii.gz'), j('<root>', 'in', 'u_im2.nii.gz')]
    else:
        assert pth_y == [j('<root>', w) if case != 'pairs' else w for w in want[:2]]
        for c, w in enumerate(want[:2]):
            assert np.array_equal(files[w][0], dat_y[..., c].numpy())
            assert np.abs(files[w][1] - mat_y.numpy()).max() < 1e-6
    if case == 'label':
        assert pth_label == j('<root>', want[2]) and np.array_equal(files[want[2]][0], label.numpy())


# ---- errors, defaults, exports -------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['crop', 'common_output', 'do_atlas_align', 'write_jtv', 'plot_conv', 'show_hyperpar', 'show_jtv'])
def test_settings_that_are_not_built_raise_by_name(name):
    from unires_amd import run
    sett = struct_settings_cpu(**{name: True})
    with pytest.raises(NotImplementedError, match=name):
        run.init([[torch.zeros(4, 4, 4), torch.eye(4)]], sett)
    if name == 'crop':  # (each function refuses the settings it reads)
        with pytest.raises(NotImplementedError, match=name):
            _core._format_y(_obs(struct._input, [[_G]]), struct_settings_cpu(crop=True))
    if name == 'do_atlas_align':
        with pytest.raises(NotImplementedError, match=name):
            _core._init_reg(_obs(struct._input, [[_G]]), struct_settings_cpu(do_atlas_align=True))
    if name == 'write_jtv':
        with pytest.raises(NotImplementedError, match=name):
            _core._write_data(None, None, struct_settings_cpu(write_jtv=True))


def test_ct_with_do_res_origin_is_refused():
    x = _obs(struct._input, [[_G], [_G]], ct=(1,))
    with pytest.raises(NotImplementedError, match='do_res_origin'):
        _core._fix_affine(x, struct_settings_cpu(do_res_origin=True))
    assert _core._fix_affine(x, struct_settings_cpu()) is x
    assert _core._fix_affine(_obs(struct._input, [[_G]]), struct_settings_cpu(do_res_origin=True)) is not None
    from unires_amd import run
    with pytest.raises(NotImplementedError, match='do_res_origin'):
        run.init([[torch.rand(4, 4, 4), torch.eye(4)]], struct_settings_cpu(ct=True, do_res_origin=True, max_iter=0))


def test_new_settings_defaults_equal_the_reference(ref_core):
    s, r = struct.settings(), ref_core.settings()
    for k in ('atlas_rigid', 'bids', 'common_output', 'crop', 'ct', 'dir_out', 'do_res_origin', 'fov', 'mat', 'pow',
              'prefix', 'write_jtv', 'write_out', 'plot_conv', 'show_hyperpar', 'show_jtv'):
        assert getattr(s, k) == getattr(r, k) and type(getattr(s, k)) is type(getattr(r, k)), k
    assert set(vars(r)) <= set(vars(s))  # every field of the reference's settings exists


def test_new_settings_defaults():
    s = struct.settings()
    assert (s.atlas_rigid, s.bids, s.common_output, s.crop, s.ct, s.do_res_origin, s.write_jtv) == (False,) * 7
    assert (s.plot_conv, s.show_hyperpar, s.show_jtv) == (False,) * 3
    assert s.dir_out is None and s.mat is None and s.pow == 0 and s.prefix == 'u_' and s.fov == 'brain' and s.write_out is True
    xn = struct._input()
    assert xn.file is None and xn.fname is None and xn.direc is None and xn.nam is None


def test_exports():
    for name in ('init', '_format_y', '_read_data', '_write_data', '_proj_info_add'):
        assert name in unires_amd.__all__ and callable(getattr(unires_amd, name)), name
    from unires_amd.run import init, preproc
    assert callable(preproc) and unires_amd.init is init
    assert isinstance(unires_amd.preproc, types.ModuleType)  # (the coregistration module keeps its name)
    assert callable(spatial._mean_space) and callable(nifti.map_file)


def test_proj_info_add_ignores_rounding_noise_in_the_voxel_ratio():
    """Against a mean space the voxel ratio of an axis that is not thick is 1 up to the rounding of the 4x4
    algebra (or of a float32 sform): _proj_info_add must not round it up to 2, nor 4 to 5.  _proj_info itself
    keeps the reference's plain ceil unless told otherwise."""
    from unires_amd import _project
    rng = np.random.default_rng(3)
    grids = []
    for ax in range(3):
        v, d = [1.0, 1.0, 1.0], [181, 217, 181]
        v[ax], d[ax] = 4.0, int(round(d[ax] / 4.0))
        R = rigid_matrix(rng.uniform(-5, 5, 3).tolist(), rng.uniform(-0.1, 0.1, 3).tolist())
        grids.append(_grid(tuple(d), tuple(v), rigid=R))
    noisy = 0
    for f32 in (False, True):
        x = _obs(struct._input, [[g] for g in grids])
        sett = struct_settings_cpu(rigid_basis=unires_amd.affine_basis())
        for xc in x:
            xc[0].rigid_q = torch.zeros(6, dtype=torch.float64)
            if f32:
                xc[0].mat = xc[0].mat.float().double()
        y, sett = _core._format_y(x, sett)
        _core._proj_info_add(x, y, sett)
        for ax, xc in enumerate(x):
            assert xc[0].po.ratio == tuple(4 if a == ax else 1 for a in range(3))
            plain = _project._proj_info(y[0].dim, y[0].mat, xc[0].dim, xc[0].mat, device='cpu').ratio
            noisy += plain != xc[0].po.ratio
    assert noisy > 0  # (the case is one where the plain ceil does round noise up)
    # the tolerance is relative: the float32 rounding of a rotated affine scales with the ratio, and a ratio that
    # exceeds an integer by more than the tolerance is rounded up either way; the default is the plain ceil
    R = rigid_matrix((3.0, -2.0, 1.0), (0.07, -0.04, 0.09))
    I = torch.eye(4, dtype=torch.float64)
    for r in (1.0, 4.0, 8.0, 16.0, 31.0):
        for k in range(40):
            Rk = rigid_matrix((k, -2.0 * k, 1.0), (0.07 + 0.01 * k, -0.04, 0.09 - 0.005 * k))
            mat_x = (Rk @ torch.diag(torch.tensor([1.0, 1.0, r, 1.0], dtype=torch.float64))).float().double()
            assert _project._proj_info((8, 8, 8), Rk, (8, 8, 8), mat_x, device='cpu', ratio_tol=_core.RATIO_TOL).ratio == (1, 1, int(r))
    for vx, want, plain in ((1.25, 2, 2), (3.0, 3, 3), (1.00001, 2, 2), (0.7, 1, 1), (2.0000001, 2, 3), (16.001, 17, 17),
                            (16.000001, 16, 17), (1.0 + 1e-5, 2, 2)):
        mat_x = torch.diag(torch.tensor([1.0, 1.0, vx, 1.0], dtype=torch.float64))
        assert _project._proj_info((8, 8, 8), I, (8, 8, 8), mat_x, device='cpu', ratio_tol=_core.RATIO_TOL).ratio == (1, 1, want)
        assert _project._proj_info((8, 8, 8), I, (8, 8, 8), mat_x, device='cpu').ratio == (1, 1, plain)
