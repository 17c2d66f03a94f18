"""Initial guess of the reconstruction - counterparts of ``_init_y_dat``
(unires/_core.py:371-399), of the label path ``_init_y_label`` /
``_warp_label`` (:402-436) and of ``_resample_inplane`` (:457-492).  Everything else in the
reference's ``_core.py`` (I/O, hyper-parameter estimation, coregistration, mean-space
construction) is out of scope."""
import torch

from . import _ops
from .spatial import _mat_shape, _m12, voxel_size

MAX_LABELS = 255  # the reference's limit (unires/_core.py:425)


def _init_y_dat(x, y, sett=None):
    """y[c].dat = mean over repeats of each input trilinearly resliced into the output
    space (HIP pull with on-the-fly coordinates), clamped to the input's range."""
    dim_y = tuple(y[0].dim)
    mat_y = torch.as_tensor(y[0].mat).detach().to('cpu', torch.float64)
    for c in range(len(x)):
        dat_y, sm = None, None
        for xn in x[c]:
            mat_x = torch.as_tensor(xn.mat).detach().to('cpu', torch.float64)
            mat = torch.linalg.solve(mat_x, mat_y)                 # mat_x \ mat_y
            dat = xn.dat
            mn, mx = torch.min(dat), torch.max(dat)
            res = _ops.pull_affine(dat, _m12(mat), dim_y)
            res = torch.minimum(torch.maximum(res, mn), mx)
            dat_y = res if dat_y is None else dat_y + res
            cnt = (res > 0).to(res.dtype)
            sm = cnt if sm is None else sm + cnt
        sm = torch.where(sm == 0, torch.ones_like(sm), sm)
        y[c].dat = (dat_y / sm).contiguous()
        y[c].dim = dim_y
    return y


def _label_f32(label):
    """float32 copy of a label volume whose values float32 holds exactly; ValueError otherwise.
    Checked on the host side of any device work: non-finite values, more than MAX_LABELS values."""
    lab = torch.as_tensor(label)
    if lab.is_floating_point() and not bool(torch.isfinite(lab).all()):
        raise ValueError('Label values must be finite.')
    f32 = lab.to(torch.float32)
    if lab.dtype != torch.float32 and not bool((f32.to(lab.dtype) == lab).all()):
        raise ValueError('Label values must be exactly representable in float32.')
    if f32.unique().numel() > MAX_LABELS:
        raise ValueError('Too many label values.')
    return f32 + 0.0  # (-0 -> +0: one value, as the reference's label == u counts it)


def _warp_label(label, grid_or_mat, shape=None):
    """Warp a label image (unires/_core.py:419-436): the value u whose indicator (label == u) has
    the highest linear pull (bound 'zero', extrapolate=False) wins at each output voxel; ties go to
    the smallest value and a best of 0 gives 0.  One HIP gather instead of one pull and one select
    pass per value.  ``grid_or_mat``: the reference's dense affine grid, or the affine (output voxel
    -> label voxel) with ``shape``.  The result has the label's dtype."""
    lab = _label_f32(label)
    mat, shp = _mat_shape(grid_or_mat, shape)
    out = _ops.warp_label(lab, _m12(mat), shp)
    dtype = torch.as_tensor(label).dtype
    return out if dtype == torch.float32 else out.to(dtype)


def _init_y_label(x, y, sett=None):
    """y[c].label = the labels of the first repeat of channel c warped into the output space
    (unires/_core.py:402-416); channels without labels are left alone."""
    dim_y = tuple(y[0].dim)
    mat_y = torch.as_tensor(y[0].mat).detach().to('cpu', torch.float64)
    for c in range(len(x)):
        xn = x[c][0]
        if getattr(xn, 'label', None) is not None:
            mat_x = torch.as_tensor(xn.mat).detach().to('cpu', torch.float64)
            y[c].label = _warp_label(xn.label[0], torch.linalg.solve(mat_x, mat_y), dim_y)
    return y


def _resample_inplane(x, sett):
    """Force the voxel size of every observation up to at least the reconstruction's
    (``sett.vx``, a scalar or one per axis) by nearest-neighbour resampling, labels by
    ``_warp_label`` (unires/_core.py:457-492).  Runs only with ``sett.force_inplane_res`` and
    ``sett.max_iter > 0``; images already fine enough are skipped."""
    if not (sett.force_inplane_res and sett.max_iter > 0):
        return x
    I = torch.eye(4, dtype=torch.float64)
    for c in range(len(x)):
        for xn in x[c]:
            mat_x = torch.as_tensor(xn.mat).detach().to('cpu', torch.float64)
            vx_x = voxel_size(mat_x)
            D = I.clone()
            for i in range(3):
                vx = sett.vx[i] if isinstance(sett.vx, (list, tuple)) else sett.vx
                D[i, i] = max(float(vx) / float(vx_x[i]), 1.0)
            if float((I - D).abs().sum()) < 1e-4:
                continue
            dim_x = torch.as_tensor(xn.dim, dtype=torch.float64)
            dim_x = tuple(int(v) for v in (D[:3, :3].inverse() @ dim_x[:, None]).floor().squeeze().int().tolist())
            xn.dat = _ops.pull_nearest(xn.dat, _m12(D), dim_x)
            if getattr(xn, 'label', None) is not None:
                xn.label[0] = _warp_label(xn.label[0], D, dim_x)
            xn.mat = torch.as_tensor(xn.mat).matmul(D.to(torch.as_tensor(xn.mat)))
            xn.dim = dim_x
    return x
