"""Initial guess of the reconstruction - counterparts of ``_init_y_dat``
(unires/_core.py:371-399), of the label path ``_init_y_label`` /
``_warp_label`` (:402-436), of ``_resample_inplane`` (:457-492), and of the hyper-parameter step
``_estimate_hyperpar`` (:96-142), of the coregistration step ``_init_reg`` (:310-368), and of the
steps between them that make ``run.init`` whole: ``_read_data`` (:495-584), the ``_fix_affine`` guard
(:145-168), ``_format_y`` (:171-285) with its regularisation half ``_init_lam`` (:273-281),
``_proj_info_add`` (:439-454) and ``_write_data`` (:587-670).  Atlas alignment and cropping
(``_crop_y``, ``reset_origin``) are out of scope."""
import math
import os

import torch

from . import _ops, nifti, preproc, stats
from . import _math
from ._project import _proj_info
from ._rigid import _expm, affine_basis
from ._util import _read_image, _read_label, _write_image
from .spatial import _mat_shape, _mean_space, _m12, affine_matrix_classic, voxel_size
from .struct import _input, _output

MAX_LABELS = 255  # the reference's limit (unires/_core.py:425)


def _init_weight(xn, sett):
    """The weight map ``init()`` honours for an observation: ``xn.weight`` with ``sett.voxel_init``, else None
    (``xn.weight`` is not touched)."""
    if sett is None or not getattr(sett, 'voxel_init', False):
        return None
    return getattr(xn, 'weight', None)


def _check_init_weights(x, sett):
    """With ``sett.voxel_init``: every ``x[c][n].weight`` becomes a contiguous float32 tensor on its observation's
    device; a map that is not finite and >= 0 everywhere is a ValueError naming channel and repeat."""
    for c in range(len(x)):
        for n, xn in enumerate(x[c]):
            g = _init_weight(xn, sett)
            if g is None:
                continue
            g = torch.as_tensor(g)
            if tuple(g.shape) != tuple(xn.dat.shape):
                raise ValueError('voxel_init: the weight map of channel %d, repeat %d has shape %s, its observation %s'
                                 % (c, n, tuple(g.shape), tuple(xn.dat.shape)))
            g = g.to(device=xn.dat.device, dtype=torch.float32).contiguous()
            if not bool((torch.isfinite(g) & (g >= 0)).all()):
                raise ValueError('voxel_init: the weight map of channel %d, repeat %d must be finite and >= 0' % (c, n))
            xn.weight = g
    return x


def _init_y_dat(x, y, sett=None):
    """y[c].dat = mean over repeats of each input trilinearly resliced into the output
    space (HIP pull with on-the-fly coordinates), clamped to the input's range.  With ``sett.voxel_init`` a repeat
    with a weight map takes its range over the voxels of weight > 0 and gives a value only where its pull read no
    other voxel (``_ops.pull_support``); an output voxel no repeat supports is 0."""
    dim_y = tuple(y[0].dim)
    mat_y = torch.as_tensor(y[0].mat).detach().to('cpu', torch.float64)
    for c in range(len(x)):
        dat_y, sm = None, None
        for xn in x[c]:
            mat_x = torch.as_tensor(xn.mat).detach().to('cpu', torch.float64)
            mat = torch.linalg.solve(mat_x, mat_y)                 # mat_x \ mat_y
            dat = xn.dat
            g = _init_weight(xn, sett)
            use = dat if g is None else dat[g > 0]
            res = _ops.pull_affine(dat, _m12(mat), dim_y)
            if use.numel() > 0:
                mn, mx = torch.min(use), torch.max(use)
                res = torch.minimum(torch.maximum(res, mn), mx)
            if g is not None:  # (after the clamp: an unsupported voxel is 0 whatever the range)
                res = torch.where(_ops.pull_support(g, _m12(mat), dim_y) != 0, res, torch.zeros_like(res))
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


NOISE_EST = ('mixture', 'mad')


def _noise_est(sett):
    """sett.noise_est ('mixture' where the settings object has none); any other name than NOISE_EST's is a ValueError."""
    name = getattr(sett, 'noise_est', 'mixture')
    if name not in NOISE_EST:
        raise ValueError("sett.noise_est must be 'mixture' or 'mad', not %r" % (name,))
    return name


def _thick_axis(mat):
    """The first of the largest voxel sizes of an observation's affine: the axis its slices are stacked along, as
    ``_proj_info`` picks ``dim_thick`` once the output space exists."""
    vx = [float(v) for v in voxel_size(torch.as_tensor(mat).detach().to('cpu', torch.float64)).tolist()]
    return vx.index(max(vx))


def _estimate_hyperpar_mad(x, obs, gs):
    """``_estimate_hyperpar`` with ``sett.noise_est = 'mad'``: ``sd`` from the exact median of the
    magnitude of the in-plane Haar diagonal detail (``stats.median_hh``, ``stats.mad_sd``), ``tau = 1 / sd**2`` in the
    same float32 arithmetic as the mixture's, and ``mu`` = |mean of the voxels read| - what |mean_fg - mean_bg| is
    without a background.  One scratch buffer for all observations, one read-back."""
    dev = x[obs[0][0]][obs[0][1]].dat.device
    work = stats.median_work(dev)
    res = torch.zeros((len(obs), 4), dtype=torch.float64, device=dev)  # median, cells, sum and count of the voxels read
    for r, ((c, n), g) in enumerate(zip(obs, gs)):
        xn = x[c][n]
        dat = xn.dat.contiguous()
        stats.median_hh(dat, _thick_axis(xn.mat), bool(xn.ct), g, work=work, out=res[r, :2])
        use = torch.isfinite(dat) & ((dat != 0) if xn.ct else (dat > 0))
        if g is not None:
            use = use & (g > 0)
        res[r, 2] = torch.where(use, dat, torch.zeros_like(dat)).sum(dtype=torch.float64)
        res[r, 3] = use.sum()
    res = res.cpu()
    for ((c, n), g), (med, cells, tot, cnt) in zip(zip(obs, gs), res.tolist()):
        if cells == 0 or med == 0:
            raise ValueError('_estimate_hyperpar: channel %d, repeat %d: noise_est=\'mad\' found %s'
                             % (c, n, 'no 2 x 2 in-plane cell of usable voxels (finite, non-zero%s%s)'
                                % ('' if x[c][n].ct else ', > 0', '' if g is None else ', weight > 0') if cells == 0
                                else 'a zero median detail: the image carries no noise to estimate'))
        sd = stats.mad_sd(torch.tensor(med, dtype=torch.float64))
        x[c][n].sd = sd
        x[c][n].tau = 1 / sd ** 2
        x[c][n].mu = torch.abs(torch.tensor(tot / cnt, dtype=torch.float64).float())
    return x


@_ops.on_device
def _estimate_hyperpar(x, sett):
    """Noise precision and mean foreground intensity of every observation (unires/_core.py:96-142):
    ``x[c][n].sd``, ``.tau = 1 / sd**2`` and ``.mu = |mean_fg - mean_bg|`` from a two-class mixture
    fit to the intensity histogram (``stats.estimate_noise``).  A non-CT observation
    keeps its voxels >= 0.  One histogram launch and one fit launch for all observations, one read
    back.  The values are float32 CPU scalars, with the reference's ``.float()`` arithmetic.  With
    ``sett.voxel_init`` an observation with a weight map is read only where the map is > 0.  ``sett.noise_est = 'mad'``
    replaces the mixture by ``_estimate_hyperpar_mad`` - for inputs without an air background."""
    obs = [(c, n) for c in range(len(x)) for n in range(len(x[c]))]
    if not obs:
        return x
    gs = [_init_weight(x[c][n], sett) for c, n in obs]  # (sett.voxel_init: only voxels of weight > 0)
    if _noise_est(sett) == 'mad':
        return _estimate_hyperpar_mad(x, obs, gs)
    counts, rng = stats.noise_hist([x[c][n].dat for c, n in obs], [bool(x[c][n].ct) for c, n in obs], gs)
    rows = stats.noise_fit(counts, rng).cpu()
    for (c, n), row, g in zip(obs, rows, gs):
        if row[stats.MODEL] < 0:
            raise ValueError('_estimate_hyperpar: channel %d, repeat %d has no usable voxels '
                             '(finite, non-zero%s%s) or all of them are equal'
                             % (c, n, '' if x[c][n].ct else ', >= 0', '' if g is None else ', weight > 0'))
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
    Labels are not touched (they share their image's orientation).  Atlas alignment is not built.
    With ``sett.voxel_init`` the weight maps go along as cost-function masks (``affine_align(weights=)``)."""
    if sett.do_atlas_align:
        raise NotImplementedError('_init_reg: atlas alignment (do_atlas_align) is not built')
    N = sum(len(xc) for xc in x)
    sett.rigid_basis = affine_basis(group='SE', dtype=torch.float64)
    if sett.do_coreg and N > 1:
        imgs = [[x[c][n].dat, x[c][n].mat] for c in range(len(x)) for n in range(len(x[c]))]
        gs = [_init_weight(x[c][n], sett) for c in range(len(x)) for n in range(len(x[c]))]
        if any(g is not None for g in gs):  # (sett.voxel_init: cost-function masking)
            mat_a = preproc.affine_align(imgs, **sett.coreg_params, fix=sett.fix, device=sett.device, weights=gs)[1]
        else:
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


_NOT_BUILT = {'crop': 'cropping to the atlas field of view', 'common_output': 'the atlas-aligned common output grid',
              'do_atlas_align': 'atlas alignment', 'write_jtv': 'writing the JTV image'}


def _not_built(sett, names):
    """NotImplementedError for those of the settings ``names`` that are set (they need nitorch's atlas,
    or an output fit() does not hand out); the message names the setting."""
    for name in names:
        if getattr(sett, name, False):
            raise NotImplementedError('sett.%s: %s is not built' % (name, _NOT_BUILT[name]))


def _read_data(data, sett):
    """Parse the input data into ``x[c][n]`` structs (unires/_core.py:495-584).  ``data``: a path, a
    list of paths (one per channel), a list of lists (repeats of a channel), ``[dat, mat]`` pairs in
    the same nestings, an (X, Y, Z, C) array with its affine in ``sett.mat``, or the path of a 4-D
    NIfTI.  Labels come from ``sett.label = (path, (channel, repeat))``."""
    mat_vol = sett.mat
    if isinstance(data, str):
        file = nifti.map_file(data)
        if len(file.shape) > 3:  # path to a 4-D NIfTI
            data = file.fdata()
            mat_vol = file.affine
    try:
        data.shape
        data = data[..., None]
        data = data[:, :, :, :, 0]
        if mat_vol is None:
            raise ValueError('Image data given as array, please also provide affine matrix in sett.mat!')
    except AttributeError:
        pass
    if isinstance(data, str):
        data = [data]
    C = data.shape[3] if mat_vol is not None else len(data)

    def one(src):
        xn = _input()
        xn.dat, xn.dim, xn.mat, xn.fname, xn.direc, xn.nam, xn.file, xn.ct = \
            _read_image(src, sett.device, is_ct=sett.ct)
        xn.dat = xn.dat.contiguous()  # (a channel of an (X, Y, Z, C) array is a strided view)
        return xn
    x = []
    for c in range(C):
        if mat_vol is None and isinstance(data[c], list) and isinstance(data[c][0], (str, list)):
            x.append([one(data[c][n]) for n in range(len(data[c]))])  # possibly several repeats
        elif mat_vol is not None:
            x.append([one([data[..., c], mat_vol])])
        else:
            x.append([one(data[c])])
    if sett.label is not None:
        pth_label, (c, n) = sett.label[0], sett.label[1]
        if 0 <= c < len(x) and 0 <= n < len(x[c]):
            x[c][n] = _read_label(x[c][n], pth_label, sett)
    if sett.do_print >= 1:
        for c in range(len(x)):
            for n in range(len(x[c])):
                print('c={:}, n={:} | fname={:}'.format(c, n, x[c][n].fname))
    return x


def _read_weights(x, sett):
    """``sett.weight`` -> ``x[c][n].weight``: per-voxel weight maps of the data term, a nested list shaped like the
    data (channels, then repeats; a channel of one repeat may give its entry without the inner list), each entry the
    path of a NIfTI (read through ``nifti.map_file``; non-finite values become 0, the way a mask written with NaN
    outside means it), a tensor / array, or None.  A map has its observation's shape - ValueError otherwise; whether
    its values are >= 0 is ``fit()``'s check.  ``sett.force_inplane_res`` resamples the observation and would leave
    the map behind: the combination is refused by name."""
    weight = getattr(sett, 'weight', None)
    if weight is None:
        return x
    if sett.force_inplane_res:
        raise NotImplementedError('sett.weight with sett.force_inplane_res: the observation is resampled in plane, '
                                  'resampling its weight map is not built')
    if isinstance(weight, str) or hasattr(weight, 'shape') or len(weight) != len(x):
        raise ValueError('sett.weight must be a list with one entry per channel (%d)' % len(x))
    for c, wc in enumerate(weight):
        if wc is None:
            continue
        if isinstance(wc, str) or hasattr(wc, 'shape'):
            wc = [wc]
        if len(wc) != len(x[c]):
            raise ValueError('sett.weight[%d] must have one entry per repeat (%d)' % (c, len(x[c])))
        for n, src in enumerate(wc):
            if src is None:
                continue
            g = nifti.map_file(src).fdata() if isinstance(src, str) else torch.as_tensor(src)
            if tuple(g.shape) != tuple(x[c][n].dat.shape):
                raise ValueError('sett.weight[%d][%d] has shape %s, its observation %s'
                                 % (c, n, tuple(g.shape), tuple(x[c][n].dat.shape)))
            if isinstance(src, str):
                g = torch.nan_to_num(g.float(), nan=0.0, posinf=0.0, neginf=0.0)
            x[c][n].weight = g.to(x[c][n].dat.device)
    return x


def _fix_affine(x, sett):
    """The reference resets the origin of CT observations here (unires/_core.py:145-168, nitorch's
    ``reset_origin``); that is not built, so the combination is refused."""
    if sett.do_res_origin and any(xn.ct for xc in x for xn in xc):
        raise NotImplementedError('sett.do_res_origin: resetting the origin of CT observations is not built')
    return x


def _all_mat_dim_vx(x):
    mats = torch.stack([torch.as_tensor(xn.mat).detach().to('cpu', torch.float64) for xc in x for xn in xc])
    dims = torch.tensor([[float(d) for d in xn.dim] for xc in x for xn in xc], dtype=torch.float64)
    return mats, dims, torch.stack([voxel_size(m) for m in mats])


def _format_y(x, sett):
    """Construct the output structs (unires/_core.py:171-285): decides between the three operator
    regimes - ``sett.do_proj = False`` (A = I: one voxel size, one grid), 'denoising' with projection
    (one voxel size, different fields of view: pull / push) and 'super-resolution' (thick slices) -,
    builds the mean space (``spatial._mean_space``) where one is needed, applies ``sett.pow`` and
    sets ``y[c].lam0`` (``_init_lam``).  ``y[c].mat`` is a float64 tensor on the host, like every
    4x4 of this package; ``y[c].dim`` a tuple of ints."""
    _not_built(sett, ('crop',))
    vx_y = sett.vx
    if vx_y == 0:
        vx_y = None
    if vx_y is not None:
        if isinstance(vx_y, int):
            vx_y = float(vx_y)
        if isinstance(vx_y, float):
            vx_y = (vx_y,) * 3
        vx_y = torch.tensor(vx_y, dtype=torch.float64)
    all_mat, all_dim, all_vx = _all_mat_dim_vx(x)
    N = all_mat.shape[0]
    if N == 1:
        sett.unified_rigid = False
        sett.clean_fov = True
    mat_same = dim_same = vx_same = True
    for n in range(1, N):
        mat_same = mat_same & torch.equal(_math.round(all_mat[n - 1], 3), _math.round(all_mat[n], 3))
        dim_same = dim_same & torch.equal(_math.round(all_dim[n - 1], 3), _math.round(all_dim[n], 3))
        vx_same = vx_same & torch.equal(_math.round(all_vx[n - 1], 3), _math.round(all_vx[n], 3))
    do_sr = True
    sett.do_proj = True
    if vx_y is None and ((N == 1) or vx_same):  # voxel size not given: the inputs'
        vx_y = all_vx[0]
    if vx_y is None:  # (the reference fails on the subtraction below)
        raise ValueError('sett.vx = 0 or None keeps the voxel size of the inputs, which must then share one')
    do_pow = (isinstance(sett.pow, (tuple, list)) and len(sett.pow) == 3) \
        or (isinstance(sett.pow, int) and sett.pow > 0)
    if vx_same and bool((torch.abs(all_vx[0] - vx_y) < 1e-3).all()):
        do_sr = False
        if mat_same and dim_same and not sett.unified_rigid and not do_pow:
            mat, dim = all_mat[0], all_dim[0]
            sett.do_proj = False
    if do_sr or sett.do_proj:
        mat, dim, vx_y = _mean_space(all_mat, all_dim, vx_y)
        if do_pow:  # fixed output dimensions, centred on the mean space's
            if isinstance(sett.pow, int):
                dim2 = _math.ceil_pow(dim, p=2.0, l=2.0, mx=sett.pow)
                dim3 = _math.ceil_pow(dim, p=2.0, l=3.0, mx=sett.pow)
                ndim = torch.minimum(dim2, dim3)
            else:
                ndim = torch.as_tensor(sett.pow)
            mat = mat.mm(affine_matrix_classic(-((ndim - dim) / 2).round()))
            dim = ndim
    sett.method = 'super-resolution' if do_sr else 'denoising'
    if sett.method == 'denoising' or (N == 1 and x[0][0].ct):
        sett.scaling = False
    dim = tuple(dim.int().tolist())
    if sett.do_print >= 1:
        print('Mean space | dim={}, vx={}'.format(dim, tuple(float('%4.2f' % v) for v in voxel_size(mat).tolist())))
    y = []
    for c in range(len(x)):
        y.append(_output())
        y[c].dim = dim
        y[c].mat = mat.double().clone()
    return _init_lam(x, y, sett), sett


RATIO_TOL = 1e-6  # relative: what _proj_info_add lets a voxel-size ratio exceed an integer by before rounding it up


def _proj_info_add(x, y, sett):
    """Adds the projection-operator descriptor ``po`` to every observation
    (unires/_core.py:439-454).  The voxel ratio is rounded up with ``ratio_tol = RATIO_TOL``: against a
    mean space, and after coregistration, the ratio of an axis that is not thick is 1 only up to the
    rounding of the 4x4 algebra, and the plain ceil of ``_proj_info`` would make it 2 by chance."""
    for c in range(len(x)):
        for xn in x[c]:
            rigid = _expm(xn.rigid_q, sett.rigid_basis)
            xn.po = _proj_info(y[c].dim, y[c].mat, xn.dim, xn.mat, prof_ip=sett.profile_ip,
                               prof_tp=sett.profile_tp, gap=sett.gap, device=sett.device, rigid=rigid,
                               ratio_tol=RATIO_TOL)
    return x


def _write_data(x, y, sett):
    """Format the output (unires/_core.py:587-670): every ``y[c].dat`` is clamped, in place, to the
    range of its channel's observations; with ``sett.write_out`` the channels are written as
    ``prefix + name`` (one file each, or one 4-D file when the data came as an array with
    ``sett.mat``) into ``sett.dir_out``, else the first input's directory, else 'UniRes-output', and
    the label image as ``prefix + 'label_' + name``.  Returns ``(dat_y (dim_y, C), pth_y, label,
    pth_label)``; as in the reference the paths are the ones before the ``bids`` tag is added."""
    _not_built(sett, ('write_jtv',))
    mat = y[0].mat
    dir_out = sett.dir_out
    if dir_out is None:
        dir_out = 'UniRes-output' if x[0][0].direc is None else x[0][0].direc
    if sett.write_out and not os.path.isdir(dir_out):
        os.makedirs(dir_out, exist_ok=True)

    def path(c):
        nam = str(c) + '.nii.gz' if x[c][0].nam is None else x[c][0].nam
        return nam, os.path.join(dir_out, sett.prefix + nam)
    pth_y, pth_label, label, chans = [], None, None, []
    for c in range(len(x)):
        dat = y[c].dat
        mn = torch.stack([torch.min(xn.dat) for xn in x[c]]).min()
        mx = torch.stack([torch.max(xn.dat) for xn in x[c]]).max()
        torch.clamp(dat, min=mn, max=mx, out=dat)
        if sett.write_out and sett.mat is None:
            nam, fname = path(c)
            pth_y.append(fname)
            _write_image(dat, fname, bids=sett.bids, mat=mat, file=x[c][0].file, do_print=sett.do_print > 0)
            if y[c].label is not None:
                pth_label = os.path.join(dir_out, sett.prefix + 'label_' + nam)
                label = y[c].label
                _write_image(label, pth_label, bids=sett.bids, mat=mat, file=x[c][0].label[1],
                             do_print=sett.do_print > 0)
        chans.append(dat)
    dat_y = torch.stack(chans, dim=3)
    if sett.write_out and sett.mat is not None:
        _, fname = path(0)
        pth_y.append(fname)
        _write_image(dat_y, fname, bids=sett.bids, mat=mat, file=x[0][0].file, do_print=sett.do_print > 0)
    return dat_y, pth_y, label, pth_label
