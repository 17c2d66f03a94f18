"""fit() - host-side mirror of the iteration loop of unires/run.py:24-207 on device-resident
structs (no file I/O, no plotting): coarse-to-fine regularisation schedule, ADMM iterations
until the model negative log-likelihood stops improving, optional even/odd slice-scaling
updates, clean_fov post-processing.  Everything heavy goes through libunires_hip.so.

init() and preproc() - the reference's entry points around it (unires/run.py:210-318): from
paths or arrays to the structs fit() takes, and from its result to clamped images on disk."""
import torch

from . import _lib
from ._core import (_check_init_weights, _estimate_hyperpar, _noise_est, _fix_affine, _format_y, _init_reg, _init_y_dat, _init_y_label,
                    _not_built, _proj_info_add, _read_data, _read_weights, _resample_inplane, _write_data)
from ._host import wait_blocking
from ._lib import check, i3
from ._ops import _ptr, _stream, on_device
from ._rigid import _update_rigid
from ._update import _admm_aux, _noise_model, _step_size, _update_admm, _update_scaling, _voxel_scale
from .stats import MAD_TO_SD, median_work
from .optim import get_gain
from .spatial import _m12
from .struct import settings


def _get_sched(N, sett):
    """Coarse-to-fine scaling of the regularisation (unires/_core.py:288-307):
    reg_scl = 4, sched_num = 3 -> [32, 16, 8, 4]; a single observation -> [4]."""
    if sett.sched_num < 0 or N == 1:
        sett.sched_num = 0
    if sett.rigid_mod < 1:
        sett.rigid_mod = 1
    scl = torch.as_tensor(sett.reg_scl, dtype=torch.float32).reshape(1)
    sched = (2.0 ** torch.arange(0, 32, dtype=torch.float32)).flip(0)
    ix = int(torch.min((sched - scl).abs(), dim=0)[1])
    sett.reg_scl = torch.cat((sched[ix - sett.sched_num:ix], scl))
    return sett


@on_device
def _clean_fov(x, y):
    """Zero the voxels of y[c] outside the field of view of any of its observations
    (unires/run.py:150-164)."""
    lib = _lib.load()
    for c in range(len(x)):
        for xn in x[c]:
            M = torch.linalg.solve(y[c].mat.double().cpu(), xn.po.rigid.double().cpu()
                                   .mm(torch.as_tensor(xn.mat).double().cpu())).inverse()
            check(lib.unires_clean_fov(_ptr(y[c].dat), i3(y[c].dim), _lib.c_f32x12(*_m12(M).tolist()),
                                       i3(xn.dim), _stream()))
    return y


def _init_slice_weights(x, sett, dev):
    """The observations' slice weights as the iterations take them: a user's ``_input.slice_w`` validated (one weight
    per slice along ``po.dim_thick``, finite, >= 0 - the one read-back) and moved to the device as float32; with
    ``sett.slice_robust`` all ones where there are none, so that the plans' kernels do not change mid-fit."""
    from ._project import _slice_axis
    robust = bool(getattr(sett, 'slice_robust', False))
    if robust and not float(getattr(sett, 'slice_k', 3.0)) > 0:
        raise ValueError('sett.slice_k must be positive')
    for c, xc in enumerate(x):
        for n, xn in enumerate(xc):
            w = getattr(xn, 'slice_w', None)
            if w is None and not robust:
                continue
            S = int(xn.dat.shape[_slice_axis(xn)])
            if w is None:
                xn.slice_w = torch.ones(S, dtype=torch.float32, device=dev)
                continue
            w = torch.as_tensor(w)
            if tuple(w.shape) != (S,):
                raise ValueError('x[%d][%d].slice_w has shape %s, expected (%d,): one weight per slice along axis %d'
                                 % (c, n, tuple(w.shape), S, _slice_axis(xn)))
            if w.is_complex() or w.dtype == torch.bool:
                raise ValueError('x[%d][%d].slice_w must be real numbers' % (c, n))
            w = w.detach().to(device=dev, dtype=torch.float32)
            if not bool((torch.isfinite(w) & (w >= 0)).all()):
                raise ValueError('x[%d][%d].slice_w must be finite and >= 0' % (c, n))
            xn.slice_w = w.clone() if w is xn.slice_w else w


def _init_slice_gains(x, sett, dev):
    """The observations' slice gains as the iterations take them: a user's ``_input.slice_gain`` validated (one gain
    per slice along ``po.dim_thick``, real, finite, > 0 - the one read-back) and moved to the device as float32; with
    ``sett.slice_gain`` every non-CT repeat starts from its own, or from ones where it has none, so that the plans'
    kernels do not change mid-fit, and the precision kappa of its gains' prior is fixed here (``gain_kappa``), so that
    the objective is one function for the whole fit.  The even / odd scaling is a special case of the gains:
    ``sett.scaling`` is refused by name (ValueError).  The rigid update carries the gains only with ``sett.gain_gn``:
    without it ``sett.unified_rigid`` is refused by name (NotImplementedError) rather than left to minimise another
    data term."""
    from ._project import _slice_axis
    from ._update import gain_kappa
    on = bool(getattr(sett, 'slice_gain', False))
    if not on and all(getattr(xn, 'slice_gain', None) is None for xc in x for xn in xc):
        for xc in x:
            for xn in xc:
                xn._gain_kappa = None
        return
    if getattr(sett, 'scaling', False):
        raise ValueError('sett.scaling with slice gains (_input.slice_gain, sett.slice_gain): the even / odd slice '
                         'scaling is a special case of the per-slice gains - use one of the two')
    if getattr(sett, 'unified_rigid', False) and not getattr(sett, 'gain_gn', False):
        raise NotImplementedError('sett.unified_rigid with slice gains (_input.slice_gain, sett.slice_gain): the '
                                  'rigid Gauss-Newton update carries per-slice gains only where asked to - set '
                                  'sett.gain_gn')
    if on and not float(getattr(sett, 'gain_reg', 0.1)) >= 0:
        raise ValueError('sett.gain_reg must be >= 0')
    if on and not float(getattr(sett, 'gain_max', 2.0)) > 1:
        raise ValueError('sett.gain_max must be > 1')
    for c, xc in enumerate(x):
        for n, xn in enumerate(xc):
            xn._gain_kappa = None
            est = on and not getattr(xn, 'ct', False)
            e = getattr(xn, 'slice_gain', None)
            S = int(xn.dat.shape[_slice_axis(xn)])
            if e is None:
                if est:
                    xn.slice_gain = torch.ones(S, dtype=torch.float32, device=dev)
            else:
                e = given = torch.as_tensor(e)
                if tuple(e.shape) != (S,):
                    raise ValueError('x[%d][%d].slice_gain has shape %s, expected (%d,): one gain per slice along axis %d'
                                     % (c, n, tuple(e.shape), S, _slice_axis(xn)))
                if e.is_complex() or e.dtype == torch.bool:
                    raise ValueError('x[%d][%d].slice_gain must be real numbers' % (c, n))
                e = e.detach().to(device=dev, dtype=torch.float32).contiguous()
                if not bool((torch.isfinite(e) & (e > 0)).all()):
                    raise ValueError('x[%d][%d].slice_gain must be finite and > 0' % (c, n))
                # (estimated gains are written in place: never into the user's memory)
                xn.slice_gain = e.clone() if est and e.data_ptr() == given.data_ptr() else e
            if est:
                xn._gain_kappa = gain_kappa(xn, getattr(sett, 'gain_reg', 0.1))


def _init_rician(x, sett):
    """sett.noise_model as the iterations take it.  'gaussian' (the default): nothing but forgetting an earlier fit()'s
    effective observations.  'rician': ``sett.scaling``, ``sett.unified_rigid`` and ``sett.slice_gain`` are refused by
    name (NotImplementedError) - those updates minimise the Gaussian term - unless ``sett.rician_gn`` carries the Rician
    term through the rigid update and the gain estimate (``sett.scaling`` stays refused; ``sett.unified_rigid`` with
    gains still needs ``sett.gain_gn``, ``_init_slice_gains``); every non-CT observation must be finite and >= 0 (ValueError naming channel and repeat; one reduction per
    repeat on the device, one read-back for all), and gets ``xn._rician_dat``, a float32 clone of ``xn.dat``: the
    effective observation of the FIRST y-update, which is therefore the Gaussian one (mu = 0 is a stationary point of
    the Rician likelihood: an effective observation x R(tau x A y0) of an all-zero first guess would stay 0).  Any
    other name: ValueError."""
    if _noise_model(sett) == 'gaussian':
        for xc in x:
            for xn in xc:
                if getattr(xn, '_rician_dat', None) is not None:
                    xn._rician_dat = None
        return x
    for name in ('scaling',) if getattr(sett, 'rician_gn', False) else ('scaling', 'unified_rigid', 'slice_gain'):
        if getattr(sett, name, False):
            raise NotImplementedError("sett.%s with sett.noise_model = 'rician': that update minimises the Gaussian data "
                                      "term; carrying the Rician majoriser through it is not built" % name)
    who = [(c, n) for c, xc in enumerate(x) for n, xn in enumerate(xc) if not xn.ct]
    if who:
        bad = torch.stack([~(torch.isfinite(x[c][n].dat).all() & (x[c][n].dat >= 0).all()) for c, n in who]).tolist()
        for (c, n), b in zip(who, bad):
            if b:
                raise ValueError("x[%d][%d].dat holds a negative or non-finite value: sett.noise_model = 'rician' takes "
                                 "magnitude data" % (c, n))
    for xc in x:
        for xn in xc:
            xn._rician_dat = None if xn.ct else xn.dat.float().contiguous().clone()
    return x


BIAS_STATE = ('_bias_coef', '_bias_est', '_bias_tab', '_bias_lam', '_bias_kappa', '_bias_b', '_bias_weight', '_bias_dat',
              '_bias_key', '_bias_E')


def _init_bias(x, sett, dev):
    """The observations' bias fields as the iterations take them.  A user's ``_input.bias_coef`` is
    validated - (kx, ky, kz) with 1 <= k_d <= min(8, n_d), real, finite; ValueError naming channel and repeat - and used
    as given, with ``sett.bias`` on or off: it is never re-estimated.  With ``sett.bias`` every other non-CT repeat
    starts from zeros of ``bias_orders``' shape (b = 1), and kappa = tau sum_{x != 0} x^2 (a float64 device sum, read
    back once, here) fixes its prior Lambda for the whole fit, so that the objective is one function.  Every repeat with
    a field gets three observation-sized float32 buffers - b, the plan's voxel map g b^2 and the effective observation
    x / b: 12 bytes per voxel of the observation - and its cosine tables on the device, composed here once.  The field
    is carried by the y-update and the objective alone: ``sett.noise_model = 'rician'``, ``sett.scaling``,
    ``sett.unified_rigid`` and ``sett.slice_gain`` (a per-slice constant would be left unidentified between the two)
    are refused with it, by name (NotImplementedError).  Without ``sett.bias`` and without coefficients: nothing but
    forgetting an earlier fit()'s fields."""
    import numpy as np
    from ._update import (BIAS_MAX_ORDER, _bias, _bias_compose, _bias_dev_tables, bias_kappa, bias_lambda, bias_orders)
    from .spatial import voxel_size
    on = _bias(sett)
    for xc in x:
        for xn in xc:
            for name in BIAS_STATE:
                setattr(xn, name, None)
            xn._bias_rev = 0
    if not on and all(getattr(xn, 'bias_coef', None) is None for xc in x for xn in xc):
        return x
    what = 'a bias field (sett.bias, _input.bias_coef)'
    if _noise_model(sett) == 'rician':
        raise NotImplementedError("%s with sett.noise_model = 'rician': the field under the Rician majoriser is not "
                                  "built" % what)
    for name, why in (('scaling', 'the even / odd scaling update does not carry the field'),
                      ('unified_rigid', 'the rigid Gauss-Newton update does not carry the field'),
                      ('slice_gain', 'estimating both would leave a per-slice constant unidentified')):
        if getattr(sett, name, False):
            raise NotImplementedError('%s with sett.%s: %s' % (what, name, why))
    if on and not float(getattr(sett, 'bias_cutoff', 60.0)) > 0:
        raise ValueError('sett.bias_cutoff must be positive')
    if on and not float(getattr(sett, 'bias_reg', 0.01)) >= 0:
        raise ValueError('sett.bias_reg must be >= 0')
    if not float(getattr(sett, 'bias_max', 4.0)) > 1:
        raise ValueError('sett.bias_max must be > 1')
    todo = []
    for c, xc in enumerate(x):
        for n, xn in enumerate(xc):
            given = getattr(xn, 'bias_coef', None)
            est = on and given is None and not getattr(xn, 'ct', False)
            if given is None and not est:
                continue
            shape = tuple(int(d) for d in xn.dat.shape)
            if given is None:
                coef = torch.zeros(bias_orders(xn, sett), dtype=torch.float64)
            else:
                coef = torch.as_tensor(given)
                if coef.dim() != 3 or any(not 1 <= int(k) <= min(BIAS_MAX_ORDER, d) for k, d in zip(coef.shape, shape)):
                    raise ValueError('x[%d][%d].bias_coef has shape %s, expected (kx, ky, kz) with 1 <= k_d <= min(8, n_d) '
                                     'on an observation of shape %s' % (c, n, tuple(coef.shape), shape))
                if coef.is_complex() or coef.dtype == torch.bool:
                    raise ValueError('x[%d][%d].bias_coef must be real numbers' % (c, n))
                coef = coef.detach().to(device='cpu', dtype=torch.float64).contiguous().clone()
                if not bool(torch.isfinite(coef).all()):
                    raise ValueError('x[%d][%d].bias_coef must be finite' % (c, n))
            todo.append((xn, coef, est, shape))
    for xn, coef, est, shape in todo:
        xn._bias_coef, xn._bias_est = coef, est
        xn._bias_tab = _bias_dev_tables(shape, tuple(coef.shape), dev)
        xn._bias_b = torch.empty(shape, dtype=torch.float32, device=dev)
        xn._bias_weight = torch.empty(shape, dtype=torch.float32, device=dev)
        xn._bias_dat = torch.empty(shape, dtype=torch.float32, device=dev)
        if est:
            xn._bias_kappa = float(bias_kappa(xn))
            xn._bias_lam = bias_lambda(shape, voxel_size(xn.mat).tolist(), tuple(coef.shape), xn._bias_kappa, sett)
        else:
            xn._bias_lam = np.zeros(tuple(coef.shape))
    _bias_compose(x, sett, force=True)
    return x


def _init_voxel_weights(x, sett, dev):
    """The observations' voxel weights as the iterations take them: a user's ``_input.weight`` validated (the
    observation's shape, real, finite, >= 0 - the one read-back) and moved to the device as contiguous float32.  With
    ``sett.voxel_robust`` a private clone of it is kept as the rule's prior (``xn._weight_prior``; None: ones) and
    every observation starts from its prior, or from ones where it has none, so that the plans' kernels do not change
    mid-fit.  The scaling and rigid Gauss-Newton updates carry voxel weights only with ``sett.voxel_gn``: without it
    they are refused by name rather than left to minimise another data term."""
    robust = bool(getattr(sett, 'voxel_robust', False))
    if robust and not float(getattr(sett, 'voxel_k', 3.0)) > 0:
        raise ValueError('sett.voxel_k must be positive')
    mad = _voxel_scale(sett) == 'mad' and robust
    work = median_work(dev) if mad else None  # (one scratch for the medians of every repeat: they share the stream)
    any_w = robust
    for c, xc in enumerate(x):
        for n, xn in enumerate(xc):
            xn._weight_prior = None
            # sett.voxel_scale = 'mad': (median |r|, N) of the repeat's last re-estimate, on the device, and the scratch
            xn._voxel_scale = torch.zeros(2, dtype=torch.float64, device=dev) if mad else None
            xn._median_work = work
            g = getattr(xn, 'weight', None)
            if g is None:
                if robust:
                    xn.weight = torch.ones(tuple(xn.dat.shape), dtype=torch.float32, device=dev)
                continue
            any_w = True
            g = given = torch.as_tensor(g)
            if tuple(g.shape) != tuple(xn.dat.shape):
                raise ValueError('x[%d][%d].weight has shape %s, expected %s: one weight per voxel of the observation'
                                 % (c, n, tuple(g.shape), tuple(xn.dat.shape)))
            if g.is_complex() or g.dtype == torch.bool:
                raise ValueError('x[%d][%d].weight must be real numbers' % (c, n))
            g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
            if not bool((torch.isfinite(g) & (g >= 0)).all()):
                raise ValueError('x[%d][%d].weight must be finite and >= 0' % (c, n))
            if robust:
                # (a conversion above made a copy already; a tensor that needed none still shares the user's memory)
                xn._weight_prior = g.clone() if g.data_ptr() == given.data_ptr() else g
                xn.weight = xn._weight_prior.clone()
            else:
                xn.weight = g
    if any_w and not getattr(sett, 'voxel_gn', False):
        for name in ('scaling', 'unified_rigid'):
            if getattr(sett, name, False):
                raise NotImplementedError('sett.%s with voxel weights (_input.weight, sett.voxel_robust): the '
                                          'Gauss-Newton updates carry per-voxel weights only where asked to - '
                                          'set sett.voxel_gn' % name)


@on_device
def fit(x, y, sett):
    """Fit model (unires/run.py:24-207).  ``x[c][n]`` / ``y[c]`` are the _input / _output
    structs with device tensors, as left by the initialisation (``_init_y_dat``,
    ``_proj_info``); ``y[c].lam0`` is the unscaled regularisation.

    Returns (dat_y, mat_y, R, info): reconstructions stacked to (dim_y, C) float32, the
    output affine, the rigid matrices (N, 4, 4) and a dict with the objective trace
    ``obj`` (n_iter, 3), the iteration count, the regularisation schedule and ``slice_w``: per channel a list with
    each repeat's final slice weights (a CPU float32 tensor, one per slice along ``po.dim_thick``) or None for a
    repeat without weights, and ``voxel_w``: likewise each repeat's final voxel weights (``_input.weight``,
    ``sett.voxel_robust``) as the DEVICE float32 tensor the iterations used, or None, and ``voxel_scale``: likewise each
    repeat's last robust residual scale 1.4826 median|x - A y| (a float32 CPU scalar) under ``sett.voxel_robust`` with
    ``sett.voxel_scale = 'mad'``, else None, and ``slice_gain``: likewise each repeat's final per-slice intensity gains
    (``_input.slice_gain``, ``sett.slice_gain``; a CPU float32 tensor, one per slice along ``po.dim_thick``) or None,
    and ``bias``: likewise each repeat's final bias coefficients (``_input.bias_coef``, ``sett.bias``; a CPU float64
    tensor (kx, ky, kz); ``unires_amd.bias_field`` synthesises the field from them) or None.

    A bias field models an observation as b . e . (A y), b = exp(beta) > 0 smooth (receive-coil shading): a separable
    cosine series on the observation's own grid, cut off at ``sett.bias_cutoff`` mm.  Under ``sett.bias`` the
    coefficients of every non-CT repeat without a user's ``_input.bias_coef`` take one Gauss-Newton step after every
    ADMM iteration's z / w update, before the slice and voxel rules write their weights (``_update_bias``), against a
    ridge whose precision is fixed here for the whole fit; the objective carries that ridge.  The plan reads g b^2 for
    the repeat's voxel map and x / b for its observation, recomposed once per iteration, so no solve kernel changes; that
    is three more observation-sized buffers per repeat with a field.  A user's coefficients are used as given and never
    re-estimated.  ``sett.noise_model = 'rician'``, ``sett.scaling``, ``sett.unified_rigid`` and ``sett.slice_gain`` are
    refused with a field, by name (NotImplementedError); a fixed ``_input.slice_gain``, slice and voxel weights with
    both rules and both scales, ``sett.mask_zeros``, ``sett.diff`` and channel streams work with it.

    Slice gains model an observation as e[s(v)] (A y)(v) (banding).  Under ``sett.slice_gain`` they are re-estimated
    after every ADMM iteration's z / w update, before the slice and voxel rules write their weights, against a ridge
    towards 1 whose precision is fixed here for the whole fit; the objective carries that ridge.  ``sett.scaling``
    is refused with gains, by name (ValueError).  With ``sett.gain_gn`` the rigid Gauss-Newton update of a gained
    repeat (``sett.unified_rigid``) takes its step on the same data term - objective, residual and Hessian weight
    carry the gains (``_update_rigid``), and it sees the gains ``_update_admm`` has just re-estimated; the ridge does
    not depend on the rigid parameters and is no part of that step.  Without ``sett.gain_gn`` (the default)
    ``sett.unified_rigid`` is refused with gains, by name (NotImplementedError).

    Slice weights define a repeat's data term, and every update minimises it: with ``sett.scaling`` or
    ``sett.unified_rigid`` the Gauss-Newton updates of a weighted repeat take the weights too (``_update_scaling``,
    ``_update_rigid``).  Under ``sett.slice_robust`` they see the weights ``_update_admm`` has just re-estimated.

    ``sett.noise_model = 'rician'`` gives every non-CT repeat the Rician data term W [1/2 tau (x - mu)^2 + c(tau x mu)],
    mu = e . A y, minimised by majorisation: every ADMM iteration's y-update is the Gaussian one on the effective
    observation ``xn._rician_dat`` = x I1/I0(tau x mu) of the previous iteration's y (a clone of ``xn.dat`` for the
    first: one more observation-sized buffer per repeat), and ``obj`` carries the term c.  Observations must be finite
    and >= 0 (ValueError); ``sett.scaling``, ``sett.unified_rigid`` and ``sett.slice_gain`` are refused with it, by name
    (NotImplementedError); a user's fixed ``_input.slice_gain``, both robust rules, ``sett.mask_zeros`` and channel
    streams work with it unchanged.  The default 'gaussian' runs what ran before the knob existed.  With
    ``sett.rician_gn`` the last two are allowed: the rigid update of a Rician repeat takes its step on the Rician term
    (exact objective, exact gradient, the majoriser's curvature: ``_update_rigid``), and the gain rule is taken on the
    effective observation the iteration has just written, so that it and the next y-update minimise one surrogate
    (``_update_slice_gains``); ``sett.scaling`` stays refused.

    Voxel weights define it likewise.  With ``sett.voxel_gn`` the two Gauss-Newton updates of a repeat that has voxel
    weights take them too - beside its slice weights, where it has both - and under ``sett.voxel_robust`` they see the
    weights ``_update_admm`` has just re-estimated.  Without ``sett.voxel_gn`` (the default) ``sett.scaling`` and
    ``sett.unified_rigid`` are refused with voxel weights, by name."""
    if len(x) != len(y):
        raise ValueError('one output per channel')
    with torch.no_grad():
        dev = y[0].dat.device
        _init_rician(x, sett)
        _init_slice_weights(x, sett, dev)
        _init_voxel_weights(x, sett, dev)
        _init_slice_gains(x, sett, dev)
        _init_bias(x, sett, dev)
        N = sum(len(xc) for xc in x)
        sett = _get_sched(N, sett)
        cnt_scl = 0
        for c in range(len(x)):
            y[c].lam = float(sett.reg_scl[cnt_scl]) * float(y[c].lam0)
        obj = torch.zeros(max(sett.max_iter, 1), 3, dtype=torch.float64, device=dev)
        tmp = torch.zeros_like(y[0].dat)
        n_done = 0
        if sett.max_iter > 0:
            rho = _step_size(x, y, sett)
            z, w = _admm_aux(y, sett)
        cnt_scl_iter = 0
        countdown0 = countdown1 = 6
        for n_iter in range(sett.max_iter):
            y, z, w, tmp, obj = _update_admm(x, y, z, w, rho, tmp, obj, n_iter, sett)
            n_done = n_iter + 1
            # one host read-back per ADMM iteration: the convergence logic below is the
            # reference's, on the same float64 objective values
            wait_blocking(dev)  # (sleep until the iteration is through: `.cpu()` alone polls)
            gain = get_gain(obj[:n_iter + 1, 0].cpu(), monotonicity='decreasing')
            if sett.do_print >= 1:
                print('{:3d} - Convergence ({} | {} | {} | gain={:0.7f})'.format(
                    n_iter, *['{:0.1f}'.format(v) for v in obj[n_iter].tolist()], float(gain)))
            if cnt_scl >= (sett.reg_scl.numel() - 1) and cnt_scl_iter > 20 \
                    and ((abs(gain) < sett.tolerance) or (n_iter >= (sett.max_iter - 1))):
                countdown0 -= 1
                if countdown0 == 0:
                    break
            else:
                countdown0 = 6
            if sett.scaling:
                x, _ = _update_scaling(x, y, sett, max_niter_gn=1, num_linesearch=6, verbose=0)
            if sett.unified_rigid and n_iter > 0 and (n_iter % sett.rigid_mod) == 0:
                x, _ = _update_rigid(x, y, sett, mean_correct=False, max_niter_gn=1,
                                     num_linesearch=6, verbose=0, samp=sett.rigid_samp)
            if cnt_scl + 1 < len(sett.reg_scl) and cnt_scl_iter > 16 and abs(gain) < 1e-3:
                countdown1 -= 1
                if countdown1 == 0:
                    cnt_scl_iter = 0
                    cnt_scl += 1
                    for c in range(len(x)):
                        y[c].lam = float(sett.reg_scl[cnt_scl]) * float(y[c].lam0)
                    rho = _step_size(x, y, sett)
            else:
                countdown1 = 6
            cnt_scl_iter += 1
        if sett.clean_fov:
            y = _clean_fov(x, y)
        R = torch.stack([xn.po.rigid.double().cpu() for xc in x for xn in xc])
        dat_y = torch.stack([yc.dat for yc in y], dim=-1)
        slice_w = [[None if getattr(xn, 'slice_w', None) is None else xn.slice_w.detach().cpu() for xn in xc] for xc in x]
        voxel_w = [[getattr(xn, 'weight', None) for xn in xc] for xc in x]
        # sett.voxel_scale = 'mad': the scale of every repeat's last re-estimate, read once, here
        meds = [xn._voxel_scale for xc in x for xn in xc if xn._voxel_scale is not None and n_done > 0]
        meds = iter(torch.stack(meds)[:, 0].cpu().float() if meds else ())
        voxel_scale = [[None if xn._voxel_scale is None or n_done == 0
                        else torch.tensor(MAD_TO_SD, dtype=torch.float32) * next(meds) for xn in xc] for xc in x]
        slice_gain = [[None if getattr(xn, 'slice_gain', None) is None else xn.slice_gain.detach().cpu() for xn in xc]
                      for xc in x]
        bias = [[None if getattr(xn, '_bias_coef', None) is None else xn._bias_coef.clone() for xn in xc] for xc in x]
        info = dict(obj=obj[:n_done].cpu(), n_iter=n_done, reg_scl=sett.reg_scl.clone(), slice_w=slice_w,
                    voxel_w=voxel_w, voxel_scale=voxel_scale, slice_gain=slice_gain, bias=bias)
        return dat_y, y[0].mat, R, info


def init(data, sett=None):
    """Model initialiser (unires/run.py:210-282): reads the data, estimates the noise and intensity
    hyper-parameters (with ``max_iter > 0``), resamples in plane where asked, coregisters, builds the
    output space and the projection operators, and makes the initial guess of images and labels.

    ``data``: paths (``['T1.nii', 'T2.nii']``; with repeats ``[['T1_1.nii', 'T1_2.nii'], ['T2.nii']]``),
    ``[dat, mat]`` pairs in the same nestings, an (X, Y, Z, C) array with ``sett.mat``, or the path
    of a 4-D NIfTI.  ``sett``: a ``settings()``; the defaults when None.  Returns ``(x, y, sett)``,
    what ``fit`` takes.  With ``sett.voxel_init`` the weight maps of ``sett.weight`` are validated here (finite, >= 0;
    ValueError naming channel and repeat) and a voxel of weight 0 is read by neither the hyper-parameter estimate, nor
    the coregistration, nor the first guess of ``y``; without it the three ignore the maps."""
    sett = settings() if sett is None else sett
    _not_built(sett, ('crop', 'common_output', 'do_atlas_align', 'write_jtv'))
    _noise_est(sett)  # (a name that is not built: ValueError before anything is read)
    for name in ('plot_conv', 'show_hyperpar', 'show_jtv'):
        if getattr(sett, name, False):
            raise NotImplementedError('sett.%s: plotting is not built' % name)
    with torch.no_grad():
        x = _read_data(data, sett)
        del data
        x = _read_weights(x, sett)
        if getattr(sett, 'voxel_init', False):
            x = _check_init_weights(x, sett)
        if sett.max_iter > 0:
            x = _estimate_hyperpar(x, sett)
        x = _fix_affine(x, sett)
        x = _resample_inplane(x, sett)
        x, sett = _init_reg(x, sett)
        y, sett = _format_y(x, sett)
        x = _proj_info_add(x, y, sett)
        y = _init_y_dat(x, y, sett)
        y = _init_y_label(x, y, sett)
        return x, y, sett


def preproc(data, sett=None):
    """Preprocess images (unires/run.py:285-318): ``init``, ``fit``, then ``_write_data``.  Returns
    ``(dat_y, mat_y, pth_y)``: the reconstructions (dim_y, C) float32, clamped to the range of their
    observations, the output affine, and the paths written (``prefix + name``; none with
    ``write_out = False``).  With ``max_iter = 0`` the result is the initial guess."""
    x, y, sett = init(data, sett)
    _, mat_y, _, _ = fit(x, y, sett)
    dat_y, pth_y, _, _ = _write_data(x, y, sett)
    return dat_y, mat_y, pth_y
