"""Initial guess of the reconstruction - counterparts of ``_init_y_dat``
(unires/_core.py:371-399), of the label path ``_init_y_label`` /
``_warp_label`` (:402-436), of ``_resample_inplane`` (:457-492), and of the hyper-parameter step
``_estimate_hyperpar`` (:96-142) with the regularisation half of ``_format_y``, ``_init_lam``
(:273-281), and of the coregistration step ``_init_reg`` (:310-368).  Everything else in the
reference's ``_core.py`` (I/O, atlas alignment, mean-space construction) is out of scope."""
import math

import torch

from . import _ops, preproc, stats
from ._rigid import affine_basis
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


@_ops.on_device
def _estimate_hyperpar(x, sett):
    """Noise precision and mean foreground intensity of every observation (unires/_core.py:96-142):
    ``x[c][n].sd``, ``.tau = 1 / sd**2`` and ``.mu = |mean_fg - mean_bg|`` from a two-class mixture
    fit to the intensity histogram (``stats.estimate_noise``).  A non-CT observation
    keeps its voxels >= 0.  One histogram launch and one fit launch for all observations, one read
    back.  The values are float32 CPU scalars, with the reference's ``.float()`` arithmetic."""
    obs = [(c, n) for c in range(len(x)) for n in range(len(x[c]))]
    if not obs:
        return x
    counts, rng = stats.noise_hist([x[c][n].dat for c, n in obs], [bool(x[c][n].ct) for c, n in obs])
    rows = stats.noise_fit(counts, rng).cpu()
    for (c, n), row in zip(obs, rows):
        if row[stats.MODEL] < 0:
            raise ValueError('_estimate_hyperpar: channel %d, repeat %d has no usable voxels '
                             '(finite, non-zero%s) or all of them are equal'
                             % (c, n, '' if x[c][n].ct else ', >= 0'))
        prm_noise, prm_not_noise = stats._noise_params(row)
        sd_bg = prm_noise['sd'].float()
        x[c][n].sd = sd_bg
        x[c][n].tau = 1 / sd_bg ** 2
        x[c][n].mu = torch.abs(prm_not_noise['mean'].float() - prm_noise['mean'].float())
    return x


def _init_lam(x, y, sett):
    """Regularisation of every channel from the estimated intensities (the lambda half of
    ``_format_y``, unires/_core.py:273-281): ``y[c].lam0 = y[c].lam = sqrt(1/C) / mean_n(mu)``, a CT
    observation's ``mu`` divided by 4 in super-resolution.  Host arithmetic in float32."""
    C = len(x)
    for c in range(C):
        mu_c = torch.zeros(len(x[c]), dtype=torch.float32)
        for n in range(len(x[c])):
            mu_c[n] = float(x[c][n].mu)
            if x[c][n].ct and sett.method == 'super-resolution':
                mu_c[n] /= 4
        y[c].lam0 = math.sqrt(1 / C) / torch.mean(mu_c)
        y[c].lam = math.sqrt(1 / C) / torch.mean(mu_c)
    return y


def _init_reg(x, sett):
    """Initialise registration (unires/_core.py:310-368): ``sett.rigid_basis = affine_basis('SE')``;
    with ``sett.do_coreg`` and more than one observation, every observation is aligned rigidly to
    the observation of flat index ``sett.fix`` (``preproc.affine_align`` with
    ``sett.coreg_params``), ``sett.mat_coreg`` keeps the transforms and
    ``x[c][n].mat = mat_a[i] \\ x[c][n].mat``; every ``x[c][n].rigid_q`` is set to zeros(6).
    Labels are not touched (they share their image's orientation).  Atlas alignment is not built."""
    if sett.do_atlas_align:
        raise NotImplementedError('_init_reg: atlas alignment (do_atlas_align) is not built')
    N = sum(len(xc) for xc in x)
    sett.rigid_basis = affine_basis(group='SE', dtype=torch.float64)
    if sett.do_coreg and N > 1:
        imgs = [[x[c][n].dat, x[c][n].mat] for c in range(len(x)) for n in range(len(x[c]))]
        mat_a = preproc.affine_align(imgs, **sett.coreg_params, fix=sett.fix, device=sett.device)[1]
        sett.mat_coreg = mat_a
        i = 0
        for c in range(len(x)):
            for n in range(len(x[c])):
                mat = torch.as_tensor(x[c][n].mat, dtype=torch.float64)
                x[c][n].mat = torch.linalg.solve(mat_a[i].to(mat), mat)
                i += 1
    for c in range(len(x)):
        for n in range(len(x[c])):
            x[c][n].rigid_q = torch.zeros(sett.rigid_basis.shape[0], device=sett.device, dtype=torch.float64)
    return x, sett
