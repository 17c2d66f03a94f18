"""Label path on the host: struct / settings defaults, argument errors raised before any device
work, and the restated reference (tests/label_restated.py) pinned against the reference's own
_warp_label / _init_y_label / _resample_inplane where the reference's sources are at hand."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import unires_amd
from unires_amd import _core, _util, nifti, spatial, struct
from tests import label_restated as R


def test_struct_and_settings_defaults():
    assert struct._input().label is None
    assert struct._output().label is None
    s = struct.settings()
    assert s.label is None and s.force_inplane_res is False and s.vx == 1.0
    for name in ('_warp_label', '_init_y_label', '_resample_inplane', '_read_label'):
        assert name in unires_amd.__all__ and callable(getattr(unires_amd, name))


def test_read_label_checks_dimensions(tmp_path):
    pth = str(tmp_path / 'lab.nii.gz')
    nifti.write(pth, np.arange(24, dtype=np.float32).reshape(2, 3, 4), np.eye(4))
    sett = types.SimpleNamespace(device='cpu')
    x = struct._input(dat=torch.zeros(2, 3, 4))
    _util._read_label(x, pth, sett)
    assert x.label[0].dtype == torch.float32 and tuple(x.label[0].shape) == (2, 3, 4)
    assert torch.equal(x.label[0], torch.arange(24, dtype=torch.float32).reshape(2, 3, 4))
    x = struct._input(dat=torch.zeros(2, 3, 5))
    with pytest.raises(ValueError, match='Incorrect label dimensions.'):
        _util._read_label(x, pth, sett)


def test_warp_label_argument_errors_before_device_work():
    M, shape = torch.eye(4, dtype=torch.float64), (4, 4, 4)
    with pytest.raises(ValueError, match='Too many label values.'):
        _core._warp_label(torch.arange(256, dtype=torch.float32).reshape(4, 8, 8), M, shape)
    with pytest.raises(ValueError, match='finite'):
        _core._warp_label(torch.tensor([[[0.0, float('nan')]]]), M, shape)
    with pytest.raises(ValueError, match='finite'):
        _core._warp_label(torch.tensor([[[0.0, float('inf')]]]), M, shape)
    with pytest.raises(ValueError, match='float32'):
        _core._warp_label(torch.tensor([[[0, (1 << 24) + 1]]], dtype=torch.int64), M, shape)
    with pytest.raises(ValueError, match='float32'):
        _core._warp_label(torch.tensor([[[0.1, 0.0]]], dtype=torch.float64), M, shape)
    # 255 values of an integer type pass the checks and stop at the device check (no CPU path)
    with pytest.raises(RuntimeError, match='no CPU path'):
        _core._warp_label(torch.arange(255, dtype=torch.int32).reshape(5, 51, 1), M, shape)


def test_grid_pull_orders():
    src, M = torch.zeros(3, 3, 3), torch.eye(4)
    for order in (2, 3, 'cubic'):
        with pytest.raises(NotImplementedError):
            spatial.grid_pull(src, M, (3, 3, 3), interpolation=order)
    with pytest.raises(NotImplementedError):
        spatial.grid_pull(src, M, (3, 3, 3), interpolation=0, bound='dct2')
    for order in (0, 'nearest'):
        with pytest.raises(NotImplementedError):
            spatial.grid_push(src, M, (3, 3, 3), interpolation=order)
        with pytest.raises(NotImplementedError):
            spatial.grid_grad(src, M, (3, 3, 3), interpolation=order)
        # order 0 reaches the nearest-neighbour pull, which has no CPU path
        with pytest.raises(RuntimeError, match='no CPU path'):
            spatial.grid_pull(src, M, (3, 3, 3), interpolation=order)


# ---- pin of the restatement against the reference's own functions -------------------------------
def _raiser(name):
    def f(*a, **k):
        raise AssertionError('placeholder for nitorch.%s called' % name)
    return f


@pytest.fixture(scope='module')
def ref_core():
    """unires/_core.py of the reference, imported as it lies with nitorch bound to the oracle
    (tests/golden/make_golden_from_reference.py's shim) and the names it imports beyond the hot path
    stubbed; sys.modules / sys.path are restored afterwards."""
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
        yield RC
    finally:
        for k in [k for k in sys.modules if k not in mods]:
            del sys.modules[k]
        sys.modules.update(mods)
        sys.path[:] = path


def _case(seed, shape=(9, 8, 7), n_labels=6):
    gen = torch.Generator().manual_seed(seed)
    values = torch.randperm(40, generator=gen)[:n_labels].float() - 12.0
    return R.voronoi_labels(shape, values, gen)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_warp_label_restatement_pins_reference(ref_core, seed):
    lab = _case(seed)
    gen = torch.Generator().manual_seed(100 + seed)
    mats = [torch.eye(4, dtype=torch.float64), torch.diag(torch.tensor([0.5, 0.5, 2.0, 1.0], dtype=torch.float64))]
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = torch.linalg.matrix_exp(torch.tensor([[0, -.1, .05], [.1, 0, -.08], [-.05, .08, 0]], dtype=torch.float64))
    m[:3, 3] = torch.rand(3, generator=gen, dtype=torch.float64) * 2 - 1
    mats.append(m)
    for M in mats:
        grid = R.affine_grid(M, (11, 10, 9))
        want = ref_core._warp_label(lab.clone(), grid.clone())
        got = R.warp_label(lab, grid)[0]
        assert got.dtype == want.dtype and torch.equal(got, want)
    # ties: a half-voxel shift between two labels; the smaller value wins
    lab2 = torch.tensor([[[3.0, -2.0]]])
    grid = torch.tensor([[[[0.0, 0.0, 0.5]]]])
    assert float(ref_core._warp_label(lab2, grid)) == -2.0 == float(R.warp_label(lab2, grid)[0])
    with pytest.raises(ValueError, match='Too many label values.'):
        ref_core._warp_label(torch.arange(256.).reshape(4, 8, 8), grid)


def _inputs(seed, with_label=True, vx_x=(0.5, 1.0, 2.0)):
    lab = _case(seed)
    gen = torch.Generator().manual_seed(seed)
    mat = torch.diag(torch.tensor(list(vx_x) + [1.0], dtype=torch.float64))
    mat[:3, 3] = torch.tensor([-3.0, 2.0, 1.5], dtype=torch.float64)
    xn = types.SimpleNamespace(dat=torch.rand(lab.shape, generator=gen), mat=mat, dim=tuple(lab.shape),
                               label=[lab, None] if with_label else None)
    return xn


def _copy(xn):
    return types.SimpleNamespace(dat=xn.dat.clone(), mat=xn.mat.clone(), dim=tuple(xn.dim),
                                 label=None if xn.label is None else [xn.label[0].clone(), None])


def test_init_y_label_restatement_pins_reference(ref_core):
    x = [[_inputs(3), _inputs(4)], [_inputs(5, with_label=False)]]
    mat_y = torch.eye(4, dtype=torch.float64)
    mat_y[:3, :3] *= 0.75
    mat_y[:3, 3] = torch.tensor([-3.2, 1.9, 1.1])

    def outputs():
        return [types.SimpleNamespace(dim=(8, 7, 9), mat=mat_y.clone(), label=None) for _ in x]
    want = ref_core._init_y_label([[_copy(xn) for xn in xc] for xc in x], outputs(), None)
    got = R.init_y_label(x, outputs())
    assert torch.equal(got[0].label, want[0].label)
    assert got[1].label is None and want[1].label is None


@pytest.mark.parametrize('vx', [1.0, [1.5, 0.5, 1.0], (2.0, 2.0, 2.5)])
def test_resample_inplane_restatement_pins_reference(ref_core, vx):
    x = [[_inputs(6), _inputs(7, vx_x=(1.0, 1.0, 1.0))], [_inputs(8, with_label=False, vx_x=(0.4, 0.6, 1.0))]]
    for force, max_iter in ((True, 3), (False, 3), (True, 0)):
        sett = types.SimpleNamespace(force_inplane_res=force, max_iter=max_iter, vx=vx, device='cpu')
        want = ref_core._resample_inplane([[_copy(xn) for xn in xc] for xc in x], sett)
        got = R.resample_inplane([[_copy(xn) for xn in xc] for xc in x], force, max_iter, vx)
        for a, b in zip(sum(got, []), sum(want, [])):
            assert torch.equal(a.dat, b.dat) and torch.equal(a.mat, b.mat) and tuple(a.dim) == tuple(b.dim)
            assert (a.label is None) == (b.label is None)
            if a.label is not None:
                assert torch.equal(a.label[0], b.label[0])
