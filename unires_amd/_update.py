"""ADMM updates - host-side mirror of the y-update block of unires/_update.py
(:105-152), plus _step_size (:35-64) and _admm_aux (:17-32)."""
import ctypes as C

import torch

from . import _lib
from ._lib import check, f3, i3
from ._ops import _ptr, _stream, on_device
from ._host import Pacer
from ._plan import cg_many
from ._project import _channel_plan, _proj, _slice_axis
from .spatial import voxel_size
from .stats import MAD_TO_SD, median_absres, median_work


_PACERS = {}


def _admm_aux(y, sett):
    """ADMM variables z and w, (C, 3, dim_y) float32 zeros."""
    dim = (len(y), 3) + tuple(y[0].dim)
    z = torch.zeros(dim, dtype=torch.float32, device=sett.device)
    w = torch.zeros(dim, dtype=torch.float32, device=sett.device)
    return z, w


def _step_size(x, y, sett, verbose=False):
    """ADMM step size rho = rho_scl * sqrt(mean tau) / mean lam (float32 arithmetic,
    as the reference computes it on 0-d float32 tensors)."""
    rho = sett.rho
    if any(xn.ct for xc in x for xn in xc):
        rho = 1.0
    if rho is not None:
        return torch.tensor(rho, dtype=torch.float32)
    all_lam = torch.tensor([float(yc.lam) for yc in y], dtype=torch.float32)
    all_tau = torch.tensor([float(xn.tau) for xc in x for xn in xc], dtype=torch.float32)
    return sett.rho_scl * torch.sqrt(torch.mean(all_tau)) / torch.mean(all_lam)


def _diff(sett):
    """sett.diff ('forward' where the settings object has none), checked: the D of every term of the regulariser."""
    diff = getattr(sett, 'diff', 'forward')
    _lib.diff_code(diff, 'sett.diff')
    return diff


def _mask_zeros(sett):
    """sett.mask_zeros (False where the settings object has none): zero voxels of an observation are missing data in
    the y-update's system, as they are in every other consumer of an observation."""
    return bool(getattr(sett, 'mask_zeros', False))


def _slice_robust(sett):
    """sett.slice_robust (False where the settings object has none): per-slice weights of every observation are
    re-estimated from its residuals after each ADMM iteration (``_update_slice_weights``)."""
    return bool(getattr(sett, 'slice_robust', False))


NOISE_MODELS = ('gaussian', 'rician')


def _noise_model(sett):
    """sett.noise_model ('gaussian' where the settings object has none): the data term's noise model.  Any other name
    than NOISE_MODELS' is a ValueError."""
    name = getattr(sett, 'noise_model', 'gaussian')
    if name not in NOISE_MODELS:
        raise ValueError("sett.noise_model must be 'gaussian' or 'rician', not %r" % (name,))
    return name


def _is_rician(xn, sett):
    """Repeat ``xn`` has the Rician data term: sett.noise_model = 'rician' and not CT."""
    return _noise_model(sett) == 'rician' and not getattr(xn, 'ct', False)


def _obs(xn, sett):
    """What the y-update's right-hand side reads for repeat ``xn``: under the Rician model the effective observation
    ``xn._rician_dat`` (fit()'s clone of ``xn.dat`` before the first iteration, x R(tau x e . A y) after each), else
    ``xn.dat``.  For a repeat with a bias field it is ``xn._bias_dat`` = x / b (``_bias_compose``): with the plan's
    voxel map g b^2 the term reads A^T (W b x) (fit() refuses a field under the Rician model).  Masks, weights and every
    residual keep reading ``xn.dat``."""
    xb = getattr(xn, '_bias_dat', None)
    if xb is not None:
        return xb
    xt = getattr(xn, '_rician_dat', None)
    return xt if xt is not None and _is_rician(xn, sett) else xn.dat


class _Precond:
    """Callable x -> x / M like the lambda unires/_update.py:100 returns; carries the plan
    that holds the device copy of M so cg() can run the preconditioned iteration on device."""

    def __init__(self, plan, M, mode):
        self.plan, self.M, self.mode = plan, M, mode

    def __call__(self, v):
        return v if self.M is None else v / self.M


@on_device
def _precond(x, y, rho, sett):
    """Compute CG preconditioner (unires/_update.py:80-102): Jacobi,
    M = tau AtA(1) + 2 rho lam^2 sum(1/vx^2) for one channel (x = x[c], y = y[c])."""
    if len(x) != 1:
        raise ValueError('CG pre-conditioning only supports one repeat per contrast.')
    plan = _channel_plan(x, y, sett.method, sett.do_proj, voxel_size(y.mat).float(), diff=_diff(sett),
                         mask_zeros=_mask_zeros(sett), weights=True)
    M = torch.empty(tuple(y.dim), dtype=torch.float32, device=y.dat.device)
    plan.precond_build(float(rho), float(y.lam), mode='jacobi', out=M)
    return _Precond(plan, M, 'jacobi')


@on_device
def _update_y(x, y, z, w, rho, tmp, sett, info=None):
    """UPDATE: y  (unires/_update.py:118-152).  Per channel: assemble
    b = sum_n tau_n At x_n - lam Dt(w - rho z) and solve
    (sum tau AtA + rho lam^2 DtD) y = b by CG, in place on y[c].dat.

    The channels do not couple inside the y-update (no cross-channel term in
    :122-150), so each channel's RHS + CG is enqueued on its own HIP stream: the
    issue-bound push kernel of one channel overlaps the HBM-bound vector kernels of
    another.  Results are identical to the sequential loop; ``tmp`` (the reference's
    shared RHS buffer) holds channel 0's b, the other channels use per-plan buffers.

    With ``sett.cgs_tol > 0`` (the reference's default) the solves can stop early: the library feeds them to
    the device chunk by chunk and this call returns when the LAST chunk is enqueued - the calling thread stays
    in the feeder (napping between looks at a host-mapped progress word) for about as long as the solves run;
    host / device overlap beyond that needs ``cgs_tol = 0``.  Under stream capture the whole solve is enqueued
    instead (kernels after convergence return at entry).
    """
    vx_y = voxel_size(y[0].mat).float()
    rho = float(rho)
    sync = info is not None
    C = len(x)
    concurrent = C > 1 and not sync and channel_streams_on(sett, y[0].dat)
    pre = getattr(sett, 'cgs_precond', 'none')
    if not concurrent:
        for c in range(C):
            plan = _channel_plan(x[c], y[c], sett.method, sett.do_proj, vx_y, diff=_diff(sett),
                                 mask_zeros=_mask_zeros(sett), weights=True)
            plan.set_concurrency(1)
            lam = float(y[c].lam)
            if getattr(sett, 'cache_atx', True) and not sync:
                plan.rhs_cached([_obs(xn, sett) for xn in x[c]], w[c], z[c], rho, lam, out=tmp)
            else:
                plan.rhs([_obs(xn, sett) for xn in x[c]], w[c], z[c], rho, lam, out=tmp)
            if pre in ('jacobi', 'fft'):
                plan.precond_build(rho, lam, mode=pre)
            res = plan.cg(tmp, y[c].dat, rho, lam, max_iter=sett.cgs_max_iter,
                          tolerance=sett.cgs_tol, stop=sett.cgs_stop, sync=sync, precond=pre)
            if sync:
                info.append(res)
        return y
    main = torch.cuda.current_stream()
    # the plans first: fetching one may enqueue work on the main stream (the masks of sett.mask_zeros are built there,
    # the slice weights copied there), and the channel streams wait for `ready` only
    fetched = [_channel_plan(x[c], y[c], sett.method, sett.do_proj, vx_y, diff=_diff(sett),
                             mask_zeros=_mask_zeros(sett), weights=True) for c in range(C)]
    ready = torch.cuda.Event()
    ready.record(main)
    streams = _side_streams(y[0].dat.device, C)
    plans, bs = [], []
    for c in range(C):
        plan = fetched[c]
        plan.set_concurrency(C)  # (its persistent kernels leave the other channels' kernels room on the CUs)
        lam = float(y[c].lam)
        b = tmp if c == 0 else plan.rhs_buffer(tmp)
        with torch.cuda.stream(streams[c]):
            streams[c].wait_event(ready)
            if getattr(sett, 'cache_atx', True):
                plan.rhs_cached([_obs(xn, sett) for xn in x[c]], w[c], z[c], rho, lam, out=b)
            else:
                plan.rhs([_obs(xn, sett) for xn in x[c]], w[c], z[c], rho, lam, out=b)
            if pre in ('jacobi', 'fft'):
                plan.precond_build(rho, lam, mode=pre)
        plans.append(plan)
        bs.append(b)
    # the solves of all channels from one call: with a tolerance the library feeds them chunk by chunk
    # from one host loop (unires_cg_solve_many), each on its channel's stream
    cg_many(plans, bs, [yc.dat for yc in y], rho, [float(yc.lam) for yc in y], streams,
            max_iter=sett.cgs_max_iter, tolerance=sett.cgs_tol, stop=sett.cgs_stop, precond=pre)
    for c in range(C):
        main.wait_stream(streams[c])
    return y


# struct.settings.channel_streams = 'auto': the channels of a y-update go to separate HIP streams whenever there is
# more than one.  (Rounds 3 - 5 stopped at 10 M voxels: at 256^3 three streams bought nothing - every matvec kernel
# fills the chip - and cost 6 % before the runtime's signal pool was raised.  Since round 6 a plan that is told about
# its neighbours, `ChannelPlan.set_concurrency`, sizes its persistent kernels for them: profiles/r06_overlap_scan.txt,
# +6 % CG it/s at 256^3 x 3, +5 % at 384^3 x 4, +24 % at 181 x 217 x 181 x 3.)  None: no upper bound.
CHANNEL_STREAMS_MAX_VOXELS = None


def channel_streams_on(sett, dat):
    cs = getattr(sett, 'channel_streams', 'auto')
    if cs == 'auto':
        return CHANNEL_STREAMS_MAX_VOXELS is None or dat.numel() < CHANNEL_STREAMS_MAX_VOXELS
    return bool(cs)


_STREAMS = {}


def _side_streams(device, n):
    key = (device.type, device.index)
    pool = _STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def _chan_args(y):
    for yc in y:
        if not yc.dat.is_cuda or yc.dat.dtype != torch.float32 or not yc.dat.is_contiguous():
            raise RuntimeError('unires_amd: y[c].dat must be contiguous float32 CUDA/HIP tensors')
    ptrs = (C.c_void_p * len(y))(*[yc.dat.data_ptr() for yc in y])
    lams = (C.c_float * len(y))(*[float(yc.lam) for yc in y])
    return ptrs, lams


@on_device
def _update_zw(y, z, w, rho, tmp, sett):
    """UPDATE z and w  (unires/_update.py:160-193): joint-TV shrinkage and dual ascent,
    two fused kernels per channel instead of three im_gradient passes and a dozen
    temporaries.  ``tmp`` receives the shrinkage image, as in the reference."""
    for t in (z, w):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() \
                or tuple(t.shape) != (len(y), 3) + tuple(y[0].dim):
            raise ValueError('unires_amd: z/w must be contiguous (C,3,X,Y,Z) float32 device tensors')
    if not tmp.is_contiguous() or tuple(tmp.shape) != tuple(y[0].dim):
        raise ValueError('unires_amd: tmp must be a contiguous (X,Y,Z) tensor')
    vx = [float(v) for v in voxel_size(y[0].mat).tolist()]
    ptrs, lams = _chan_args(y)
    diff = _lib.diff_code(_diff(sett), 'sett.diff')
    check(_lib.load().unires_zw_update_which(ptrs, lams, len(y), i3(y[0].dim), f3(vx), diff, float(rho),
                                             float(sett.alpha), _ptr(z), _ptr(w), _ptr(tmp), _stream()))
    return z, w, tmp


def _voxel_robust(sett):
    """sett.voxel_robust (False where the settings object has none): per-voxel weights of every observation are
    re-estimated from its residuals after each ADMM iteration (``_update_voxel_weights``)."""
    return bool(getattr(sett, 'voxel_robust', False))


def _gn_weight(xn, sett):
    """The voxel weights the scaling and rigid Gauss-Newton updates carry for repeat ``xn``: ``xn.weight`` with
    ``sett.voxel_gn`` (checked: a contiguous float32 device tensor of the observation's shape, as ``fit()`` leaves
    it), else None - the switch is off by default, and the updates then ignore the map as they did before."""
    g = getattr(xn, 'weight', None)
    if g is None or not getattr(sett, 'voxel_gn', False):
        return None
    if not torch.is_tensor(g) or not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() \
            or tuple(g.shape) != tuple(xn.dat.shape):
        raise ValueError('unires_amd: xn.weight must be a contiguous float32 device tensor of the observation\'s '
                         'shape, as fit() leaves it')
    return g


VOXEL_SCALE = ('noise', 'mad')


def _voxel_scale(sett):
    """sett.voxel_scale ('noise' where the settings object has none): what the Huber rule's threshold is a multiple of.
    Any other name than VOXEL_SCALE's is a ValueError."""
    name = getattr(sett, 'voxel_scale', 'noise')
    if name not in VOXEL_SCALE:
        raise ValueError("sett.voxel_scale must be 'noise' or 'mad', not %r" % (name,))
    return name


def _slice_gain(sett):
    """sett.slice_gain (False where the settings object has none): per-slice intensity gains of every non-CT observation
    are re-estimated after each ADMM iteration (``_update_slice_gains``)."""
    return bool(getattr(sett, 'slice_gain', False))


def _check_gain(e, S):
    if not torch.is_tensor(e) or not e.is_cuda or e.dtype != torch.float32 or not e.is_contiguous() \
            or e.numel() != int(S):
        raise ValueError('unires_amd: xn.slice_gain must be a contiguous float32 device tensor with one gain per slice, '
                         'as fit() leaves it')
    return e


def _gn_gain(xn, sett):
    """The slice gains the rigid Gauss-Newton update carries for repeat ``xn``: ``xn.slice_gain`` with ``sett.gain_gn``
    (checked as ``_gained`` checks it), else None - the switch is off by default, and the update then ignores the gains
    as it did before."""
    e = getattr(xn, 'slice_gain', None)
    if e is None or not getattr(sett, 'gain_gn', False):
        return None
    return _check_gain(e, xn.dat.shape[_slice_axis(xn)])


def _gained(Ay, xn, out=None):
    """e . (A y): the prediction of a repeat with gains ``xn.slice_gain`` along ``po.dim_thick`` (``unires_slice_apply``,
    one float32 product per voxel; out of place unless ``out`` is ``Ay``).  ``Ay`` itself where the repeat has none."""
    e = getattr(xn, 'slice_gain', None)
    if e is None:
        return Ay
    _check_gain(e, Ay.shape[_slice_axis(xn)])
    out = torch.empty_like(Ay) if out is None else out
    check(_lib.load().unires_slice_apply(_ptr(Ay), _ptr(out), _ptr(e), i3(Ay.shape), _slice_axis(xn), _stream()))
    return out


def _bias(sett):
    """sett.bias (False where the settings object has none): every non-CT observation without a user's
    ``_input.bias_coef`` gets a smooth multiplicative bias field whose coefficients take one Gauss-Newton step after
    each ADMM iteration (``_update_bias``)."""
    return bool(getattr(sett, 'bias', False))


BIAS_MAX_ORDER = 8
BIAS_STEPS = tuple(2.0 ** -p for p in range(6))  # the line search's step lengths: 1, 1/2, ..., 2^-5


def _has_field(xn):
    """Repeat ``xn`` has a bias field: ``fit()`` (``_init_bias``) has made its buffers."""
    return getattr(xn, '_bias_b', None) is not None


def bias_orders_of(shape, vx, cutoff):
    """k_d = clamp(ceil(2 n_d vx_d / cutoff), 1, min(8, n_d)) per axis: the cosines whose half-period n_d vx_d / m is
    no shorter than ``cutoff`` / 2 ... mm, at least the constant, at most 8 and at most the complete basis."""
    import math
    return tuple(int(min(max(math.ceil(2.0 * int(n) * float(v) / float(cutoff)), 1), min(BIAS_MAX_ORDER, int(n))))
                 for n, v in zip(shape, vx))


def bias_orders(xn, sett):
    """The orders (kx, ky, kz) of the bias field of repeat ``xn`` on its own voxel grid, in the caller's layout
    (``bias_orders_of`` on ``xn.dat.shape``, the voxel sizes of ``xn.mat`` and ``sett.bias_cutoff``)."""
    return bias_orders_of(tuple(xn.dat.shape), voxel_size(xn.mat).tolist(), getattr(sett, 'bias_cutoff', 60.0))


def bias_tables(shape, orders):
    """The three cosine tables of a field of ``orders`` on a grid ``shape``, float64 numpy (2 k_d - 1, n_d): row m is
    the unnormalised DCT-II function phi_m(i) = cos(pi m (2 i + 1) / (2 n)), phi_0 = 1.  The first k_d rows synthesise
    the field; all 2 k_d - 1 are what the projection of W m^2 is taken on (``bias_hessian``).  Built on the host and
    handed to the kernels as they are: the float64 restatement under tests/ reads the same bits."""
    import numpy as np
    out = []
    for n, k in zip(shape, orders):
        m = np.arange(2 * int(k) - 1, dtype=np.float64)[:, None]
        i = np.arange(int(n), dtype=np.float64)[None, :]
        out.append(np.ascontiguousarray(np.cos(np.pi * m * (2.0 * i + 1.0) / (2.0 * int(n)))))
    return tuple(out)


def bias_lambda(shape, vx, orders, kappa, sett):
    """The diagonal of the coefficients' prior, float64 numpy (kx, ky, kz): Lambda = kappa bias_reg (1 + sum_d
    (bias_cutoff m_d / (2 n_d vx_d))^2) - a ridge that grows with the square of a term's spatial frequency in units of
    the cut-off, and is kappa bias_reg on the constant term."""
    import numpy as np
    cut, reg = float(getattr(sett, 'bias_cutoff', 60.0)), float(getattr(sett, 'bias_reg', 0.01))
    f = [(cut * np.arange(int(k), dtype=np.float64) / (2.0 * int(n) * float(v))) ** 2
         for n, v, k in zip(shape, vx, orders)]
    return float(kappa) * reg * (1.0 + f[0][:, None, None] + f[1][None, :, None] + f[2][None, None, :])


def bias_kappa(xn):
    """kappa = tau sum_{x != 0} x^2 of one observation: the curvature the constant term has at b = 1 on a prediction as
    large as the data.  A float64 sum on the device; a 0-d float64 device tensor, not read back here."""
    xd = xn.dat.double()
    return float(xn.tau) * (xd * xd).sum()


def bias_hessian(P, orders):
    """sum_v f(v) Phi_k(v) Phi_l(v) for all pairs of basis functions, (K, K) float64 numpy, K = kx ky kz, from ``P``, the
    projection of f onto the orders < 2 k_d - 1 ((2 kx - 1, 2 ky - 1, 2 kz - 1)): since phi_m phi_m' =
    (phi_|m - m'| + phi_(m + m')) / 2 along every axis, an entry is 1/8 of the sum of eight entries of ``P``."""
    import numpy as np
    P = np.asarray(P, dtype=np.float64)
    kx, ky, kz = (int(k) for k in orders)

    def pair(k):
        m = np.arange(k)
        return np.abs(m[:, None] - m[None, :]), m[:, None] + m[None, :]

    H = np.zeros((kx, ky, kz, kx, ky, kz), dtype=np.float64)
    for sa in pair(kx):
        for sb in pair(ky):
            for sc in pair(kz):
                H += P[sa[:, None, None, :, None, None], sb[None, :, None, None, :, None],
                       sc[None, None, :, None, None, :]]
    return H.reshape(kx * ky * kz, kx * ky * kz) / 8.0


def bias_energy(S, c, lam, tau):
    """E(c) = 1/2 tau S + 1/2 c^T Lambda c: ``S`` = sum W r^2 at the field of ``c``, ``lam`` the diagonal of Lambda."""
    import numpy as np
    c = np.asarray(c, dtype=np.float64)
    return 0.5 * float(tau) * float(S) + 0.5 * float((np.asarray(lam, dtype=np.float64) * c * c).sum())


def bias_step(c, G, P, lam, tau):
    """The float64 host rule of one Gauss-Newton step on the coefficients ``c`` ((kx, ky, kz) numpy): ``G`` the
    projection of W m r onto the orders < k, ``P`` that of W m^2 onto the orders < 2 k - 1 (``unires_bias_terms``),
    ``lam`` the diagonal of Lambda.  gradient = tau G + Lambda c; H = tau ``bias_hessian(P)`` + Lambda, the Gauss-Newton
    curvature (positive semi-definite: the exact one, which adds W m r to W m^2, can be negative); Delta = -H^-1 gradient.
    Returns (candidates, gradient, H): the candidates c + s Delta for s = 1, 1/2, ..., 2^-5 in the order the line search
    tries them - an empty list where H is singular or Delta is not finite (no data and no prior: c stays)."""
    import numpy as np
    c = np.asarray(c, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    grad = float(tau) * np.asarray(G, dtype=np.float64).reshape(c.shape) + lam * c
    H = float(tau) * bias_hessian(P, c.shape) + np.diag(lam.reshape(-1))
    try:
        delta = -np.linalg.solve(H, grad.reshape(-1)).reshape(c.shape)
    except np.linalg.LinAlgError:
        return [], grad, H
    if not np.isfinite(delta).all():
        return [], grad, H
    return [c + s * delta for s in BIAS_STEPS], grad, H


def _bias_dev_tables(shape, orders, dev):
    return tuple(torch.from_numpy(t).to(dev) for t in bias_tables(shape, orders))


@on_device
def _bias_field_call(coef, tabs, shape, beta_max, b, g=None, x=None, gb2=None, xb=None):
    """``unires_bias_field``: ``coef`` (kx, ky, kz) float64 (any device; moved to ``b``'s), ``tabs`` the device tables."""
    coef = torch.as_tensor(coef, dtype=torch.float64)
    cd = coef.to(b.device).contiguous()
    check(_lib.load().unires_bias_field(_ptr(cd), _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), i3(coef.shape), i3(shape),
                                        float(beta_max), None if g is None else _ptr(g), None if x is None else _ptr(x),
                                        _ptr(b), None if gb2 is None else _ptr(gb2), None if xb is None else _ptr(xb),
                                        _stream()))
    return b


def bias_field(coef, shape, device='cuda', bias_max=4.0):
    """The bias field b = exp(beta) of the coefficients ``coef`` ((kx, ky, kz), k_d <= min(8, shape[d]); what
    ``fit()`` returns in ``info['bias']``) on a voxel grid ``shape``, synthesised on the device: a float32 tensor of
    that shape.  log b is clamped to +- log(``bias_max``), as ``fit()`` clamps it (``sett.bias_max``)."""
    import math
    coef = torch.as_tensor(coef, dtype=torch.float64).detach().cpu()
    shape = tuple(int(n) for n in shape)
    if coef.dim() != 3 or len(shape) != 3 or any(not 1 <= int(k) <= min(BIAS_MAX_ORDER, n)
                                                   for k, n in zip(coef.shape, shape)):
        raise ValueError('bias_field: coef must be (kx, ky, kz) with 1 <= k_d <= min(8, shape[d]), got %s on %s'
                         % (tuple(coef.shape), shape))
    if not bool(torch.isfinite(coef).all()):
        raise ValueError('bias_field: coef must be finite')
    if not float(bias_max) > 1:
        raise ValueError('bias_field: bias_max must be > 1')
    dev = torch.device(device)
    b = torch.empty(shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(b.device):
        return _bias_field_call(coef, _bias_dev_tables(shape, tuple(coef.shape), b.device), shape,
                                math.log(float(bias_max)), b)


@on_device
def _bias_terms(xn, mu, b, full=True):
    """``unires_bias_terms`` of one repeat on the prediction ``mu`` = e . A y and the field ``b``: a float64 device
    tensor, (1 + K + Q,) with ``full`` (sum W r^2, the projection of W m r, the projection of W m^2), else (1,)."""
    xd = xn.dat.contiguous()
    k = tuple(xn._bias_coef.shape) if full else (0, 0, 0)
    q = tuple(2 * v - 1 for v in k) if full else (0, 0, 0)
    out = torch.empty(1 + k[0] * k[1] * k[2] + q[0] * q[1] * q[2], dtype=torch.float64, device=xd.device)
    g, u = getattr(xn, 'weight', None), getattr(xn, 'slice_w', None)
    t = xn._bias_tab
    check(_lib.load().unires_bias_terms(_ptr(xd), _ptr(mu.contiguous()), _ptr(b), None if g is None else _ptr(g.contiguous()),
                                        None if u is None else _ptr(u.contiguous()), _slice_axis(xn), _ptr(t[0]),
                                        _ptr(t[1]), _ptr(t[2]), i3(k), i3(xd.shape), _ptr(out), _stream()))
    return out


def _fielded(mu, xn, out=None):
    """b . mu: the prediction of a repeat with a bias field (``unires_voxel_apply``, one float32 product per voxel; out
    of place unless ``out`` is ``mu``).  ``mu`` itself where the repeat has none."""
    if not _has_field(xn):
        return mu
    out = torch.empty_like(mu) if out is None else out
    check(_lib.load().unires_voxel_apply(_ptr(mu), _ptr(out), _ptr(xn._bias_b), None, None, i3(mu.shape), 0, 0, None,
                                         _stream()))
    return out


def _predicted(Ay, xn, out=None):
    """b . e . (A y): the prediction of repeat ``xn`` - the gains first (``_gained``), then the field (``_fielded``);
    out of place unless ``out`` is ``Ay``.  ``Ay`` itself where the repeat has neither."""
    mu = _gained(Ay, xn, out)
    return _fielded(mu, xn, out=mu if (mu is not Ay or out is Ay) else None)


@on_device
def _bias_compose(x, sett, force=False):
    """The two volumes the plan reads for every repeat with a field, recomposed where its coefficients or its voxel
    weights changed since they were last written (``force``: regardless): ``xn._bias_weight`` = g b^2 (what
    ``_project._voxel_weights`` hands the plan for ``xn.weight``) and ``xn._bias_dat`` = x / b (what ``_obs`` hands the
    right-hand side), with ``xn._bias_b`` itself, in one ``unires_bias_field`` pass.  Their version counters are bumped:
    they tell the plan's copy of the map (``sync_voxel_weights``) and the cached sum tau At (W b . x)."""
    import math
    beta_max = math.log(float(getattr(sett, 'bias_max', 4.0)))
    for xc in x:
        for xn in xc:
            if not _has_field(xn):
                continue
            g = getattr(xn, 'weight', None)
            key = (xn._bias_rev, None if g is None else (id(g), g._version))
            if not force and key == getattr(xn, '_bias_key', None):
                continue
            _bias_field_call(xn._bias_coef, xn._bias_tab, xn.dat.shape, beta_max, xn._bias_b,
                             g=None if g is None else g.contiguous(), x=xn.dat.contiguous(), gb2=xn._bias_weight,
                             xb=xn._bias_dat)
            torch.autograd.graph.increment_version(xn._bias_weight)
            torch.autograd.graph.increment_version(xn._bias_dat)
            xn._bias_key = key
    return x


@on_device
def _update_bias(x, y, sett, raw=None):
    """One Gauss-Newton step on the bias coefficients of every repeat ``fit()`` estimates a field for
    (``xn._bias_est``), at the current y and the repeat's current weights (``raw``: what ``_slice_sums`` kept of the
    prediction e . A y WITHOUT the field for this y, computed here where missing).  One ``unires_bias_terms`` pass gives
    sum W r^2, the projection of W m r and the projection of W m^2; they are read back - one read-back per repeat and
    iteration - and the K x K algebra of the step (``bias_step``: Hessian assembly, solve, candidates) is numpy on the
    host in float64, as ``_update_rigid`` does its 6 x 6 algebra.  The line search then tries s = 1, 1/2, ..., 2^-5: the
    candidate's field is synthesised (``unires_bias_field``), its objective taken by the same kernel called for the
    objective alone (one 8-byte read-back each), and the first s with E(c + s Delta) <= E(c) is accepted; otherwise c
    stays.  ``xn._bias_coef`` and ``xn._bias_b`` are updated; the plan's volumes follow in ``_bias_compose``.
    ``xn._bias_E`` keeps (E before, E after, s) of the last step (s = 0: kept).  A user's fixed ``_input.bias_coef``
    is never touched."""
    import math
    import numpy as np
    beta_max = math.log(float(getattr(sett, 'bias_max', 4.0)))
    for c in range(len(x)):
        for n, xn in enumerate(x[c]):
            if not _has_field(xn) or not getattr(xn, '_bias_est', False):
                continue
            mu = None if raw is None else raw.get((c, n))
            if mu is None:
                Ay = _proj('A', y[c].dat, x[c], y[c], n=n, method=sett.method, do=sett.do_proj)
                mu = _gained(Ay, xn, out=Ay)
            tau, lam = float(xn.tau), xn._bias_lam
            c0 = xn._bias_coef.numpy().copy()
            k = c0.shape
            K = c0.size
            v = _bias_terms(xn, mu, xn._bias_b).cpu().numpy()  # the one read-back of the step
            E0 = bias_energy(v[0], c0, lam, tau)
            cands, _, _ = bias_step(c0, v[1:1 + K].reshape(k), v[1 + K:].reshape(tuple(2 * d - 1 for d in k)), lam, tau)
            xn._bias_E = (E0, E0, 0.0)
            if not np.isfinite(E0):
                continue
            bc = torch.empty_like(xn._bias_b)
            for s, cand in zip(BIAS_STEPS, cands):
                _bias_field_call(cand, xn._bias_tab, xn.dat.shape, beta_max, bc)
                E1 = bias_energy(float(_bias_terms(xn, mu, bc, full=False).cpu()[0]), cand, lam, tau)
                if E1 <= E0:
                    xn._bias_coef = torch.from_numpy(np.ascontiguousarray(cand))
                    xn._bias_b, bc = bc, xn._bias_b
                    xn._bias_rev += 1
                    xn._bias_E = (E0, E1, s)
                    break
    return x


@on_device
def _slice_sums(x, y, sett, ays=None, raw=None, proj=None, mus=None):
    """{(c, n): (2 S,) float64 device tensor} for every repeat that has slice or voxel weights or gains: SSE_s =
    sum_{v in s, x != 0} (x - A y)^2 and N_s = #{v in s : x != 0} per slice along ``po.dim_thick``
    (``unires_slice_sums``; float32 terms, float64 sums in a fixed order); for a repeat with voxel weights
    ``xn.weight`` both sums carry g(v) (``unires_voxel_sums``: sum g (x - A y)^2 and the effective count sum g).  A y
    is computed once per repeat; the result serves the objective (``_compute_nll``) and the rules
    (``_update_slice_weights``; ``_update_voxel_weights`` takes the A y itself from ``ays``, a dict filled here with
    (c, n): A y of the voxel-weighted repeats).  For a repeat with gains ``xn.slice_gain`` the prediction is
    e . (A y) throughout (``_gained``), and ``raw``, a dict, receives (c, n): its A y WITHOUT gains, which
    ``_update_slice_gains`` estimates from.  ``proj``: {(c, n): A y without gains} already computed for this y (the
    Rician repeats', ``_rician_terms``), only read.  For a repeat with a bias field the prediction is b . e . (A y)
    (``_fielded``), and ``mus``, a dict, receives (c, n): its e . A y WITHOUT the field, which ``_update_bias`` steps
    from.  Nothing is read back."""
    lib = _lib.load()
    out = {}
    for c in range(len(x)):
        for n, xn in enumerate(x[c]):
            g = getattr(xn, 'weight', None)
            if getattr(xn, 'slice_w', None) is None and g is None and getattr(xn, 'slice_gain', None) is None:
                continue
            Ay = None if proj is None else proj.get((c, n))
            if Ay is None:
                Ay = _proj('A', y[c].dat, x[c], y[c], n=n, method=sett.method, do=sett.do_proj)
            if getattr(xn, 'slice_gain', None) is not None:
                if raw is not None:
                    raw[(c, n)] = Ay
                Ay = _gained(Ay, xn)
            if _has_field(xn):  # (the field after the gains: the prediction is b . e . A y, out of place)
                if mus is not None:
                    mus[(c, n)] = Ay
                Ay = _fielded(Ay, xn)
            xd = xn.dat.contiguous()
            a = _slice_axis(xn)
            sums = torch.empty(2 * int(xd.shape[a]), dtype=torch.float64, device=xd.device)
            if g is None:
                check(lib.unires_slice_sums(_ptr(xd), _ptr(Ay), i3(xd.shape), a, _ptr(sums), _stream()))
            else:
                check(lib.unires_voxel_sums(_ptr(xd), _ptr(Ay), _ptr(g.contiguous()), i3(xd.shape), a, _ptr(sums),
                                            _stream()))
                if ays is not None:
                    ays[(c, n)] = Ay
            out[(c, n)] = sums
    return out


@on_device
def _update_voxel_weights(x, y, sett, ays=None):
    """Re-estimates the voxel weights of every observation that has some by the Huber rule: ``xn.weight`` <- prior . h,
    h = 1 where x == 0 or |x - A y| <= c, else c / |x - A y|, with c = sett.voxel_k / sqrt(tau) - voxel_k noise
    standard deviations (``unires_voxel_huber``; ``ays``: what ``_slice_sums`` kept of A y for this y, computed here
    where missing).  ``prior`` is the private clone ``fit()`` keeps of a user's ``_input.weight`` (None: ones), so a
    weight of 0 stays 0.  The weight tensors are written in place and their version counters bumped: they tell the
    plans (``sync_voxel_weights``, at the next y-update's plan fetch) and the cached sum tau At (g . x).  One
    streaming pass per repeat, no read-back.

    With ``sett.voxel_scale = 'mad'`` the threshold is voxel_k robust standard deviations of the residuals themselves:
    c = fl32(fl32(voxel_k) 1.4826) median|x - A y|, the exact median over the voxels the rule judges (x != 0, a finite
    residual, prior > 0) taken on the device (``unires_median_absres``) and read by the rule's kernel from there
    (``unires_voxel_huber_dev``): three more passes over x and A y, still no read-back.  No floor at the noise sd, and
    tau is not re-estimated.  ``xn._voxel_scale`` keeps (median, N) of the last estimate on the device."""
    lib = _lib.load()
    k = float(getattr(sett, 'voxel_k', 3.0))
    mad = _voxel_scale(sett) == 'mad'
    mult = float(torch.tensor(k, dtype=torch.float32) * torch.tensor(MAD_TO_SD, dtype=torch.float32))
    work = None
    if mad:  # one scratch for every repeat (they share the stream): fit()'s, or one made here for a direct call
        first = next((xn for xc in x for xn in xc if getattr(xn, 'weight', None) is not None), None)
        work = getattr(first, '_median_work', None)
        if work is None and first is not None:
            work = median_work(first.dat.device)
    for c in range(len(x)):
        for n, xn in enumerate(x[c]):
            g = getattr(xn, 'weight', None)
            if g is None:
                continue
            if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
                raise ValueError('unires_amd: x[%d][%d].weight must be a contiguous float32 device tensor, as fit() '
                                 'leaves it' % (c, n))
            Ay = None if ays is None else ays.get((c, n))
            if Ay is None:
                Ay = _proj('A', y[c].dat, x[c], y[c], n=n, method=sett.method, do=sett.do_proj)
                Ay = _predicted(Ay, xn, out=Ay)  # (a repeat with gains or a field: the residual is x - b . e . A y)
            xd = xn.dat.contiguous()
            prior = getattr(xn, '_weight_prior', None)
            if mad:
                if getattr(xn, '_voxel_scale', None) is None:
                    xn._voxel_scale = torch.zeros(2, dtype=torch.float64, device=xd.device)
                median_absres(xd, Ay, prior, work=work, out=xn._voxel_scale)
                check(lib.unires_voxel_huber_dev(_ptr(xd), _ptr(Ay), None if prior is None else _ptr(prior),
                                                 _ptr(xn._voxel_scale), mult, xd.numel(), _ptr(g), _stream()))
            else:
                check(lib.unires_voxel_huber(_ptr(xd), _ptr(Ay), None if prior is None else _ptr(prior),
                                             k / float(xn.tau) ** 0.5, xd.numel(), _ptr(g), _stream()))
            torch.autograd.graph.increment_version(g)
    return x


def slice_rule(sums, k):
    """The variance-ratio rule on one observation's slice sums ((2 S,) float64: SSE_s, then N_s): over the slices
    with N_s > 0, m_s = SSE_s / N_s and sigma^2 = their LOWER median (the ceil(K / 2)-th smallest of K, torch.median's
    convention); u_s = 1 where N_s = 0 or m_s <= k^2 sigma^2, else k^2 sigma^2 / m_s; all ones where no slice has
    data or sigma^2 = 0.  A slice keeps the observation's precision unless its own residual variance exceeds k^2
    times the typical slice's, and then gets the maximum-likelihood precision its residual supports.  float64 tensor
    ops on the device of ``sums``, no read-back.  Returns (S,) float64."""
    S = sums.numel() // 2
    sse, cnt = sums[:S], sums[S:]
    has = cnt > 0
    m = sse / cnt.clamp(min=1.0)
    K = has.sum()
    inf = torch.full_like(m, float('inf'))
    ranked = torch.where(has, m, inf).sort().values
    sig2 = ranked.gather(0, ((K + 1) // 2 - 1).clamp(min=0).reshape(1))[0]
    thr = (float(k) * float(k)) * sig2
    one = torch.ones_like(m)
    u = torch.where(has & (m > thr), thr / m, one)
    return torch.where((K > 0) & (sig2 > 0), u, one)


@on_device
def _update_slice_weights(x, y, sett, sums=None):
    """Re-estimates the slice weights of every observation that has some by ``slice_rule`` with k = sett.slice_k,
    from the residuals of the current y (``sums``: what ``_slice_sums`` returned for it, computed here when None).
    The weight tensors are updated in place: their version counters tell the plans (``sync_slice_weights``, at the
    next y-update's plan fetch) and the cached sum tau At (w . x)."""
    sums = _slice_sums(x, y, sett) if sums is None else sums
    k = float(getattr(sett, 'slice_k', 3.0))
    for (c, n), s in sums.items():
        if getattr(x[c][n], 'slice_w', None) is None:  # (voxel weights alone: nothing per slice to estimate)
            continue
        x[c][n].slice_w.copy_(slice_rule(s, k))
    return x


def gain_rule(sums, tau, kappa, gain_max):
    """The gains of one observation from its ``unires_gain_sums`` ((3 S,) float64: sum W x a, sum W a^2, sum W per
    slice, a = A y without gains): with P_s = tau sums[s] and Q_s = tau sums[S + s],
    e_s = clamp((P_s + kappa) / (Q_s + kappa), 1 / gain_max, gain_max) - the exact minimiser over that interval of
    1/2 tau sum_{v in s} W (x - e_s a)^2 + 1/2 kappa (e_s - 1)^2, a convex parabola in e_s.  A slice with
    Q_s + kappa = 0 (no data, no prior) keeps e_s = 1.  ``kappa``: a float or a 0-d float64 tensor on the device of
    ``sums``.  float64 tensor ops on that device, no read-back.  Returns (S,) float64."""
    S = sums.numel() // 3
    kappa = torch.as_tensor(kappa, dtype=torch.float64, device=sums.device)
    P, Q = float(tau) * sums[:S] + kappa, float(tau) * sums[S:2 * S] + kappa
    one = torch.ones_like(P)
    e = torch.where(Q > 0, P / torch.where(Q > 0, Q, one), one)
    return e.clamp(min=1.0 / float(gain_max), max=float(gain_max))


@on_device
def _gain_sums(xn, Ay, obs=None):
    """``unires_gain_sums`` of one repeat: (3 S,) float64 on the device, W = xn.weight . xn.slice_w (1 where None),
    ``Ay`` its A y WITHOUT gains.  ``obs``: what stands for the observation (None: ``xn.dat``) - the effective
    observation of a Rician repeat under ``sett.rician_gn`` (``_update_slice_gains``)."""
    xd = (xn.dat if obs is None else obs).contiguous()
    a = _slice_axis(xn)
    g, u = getattr(xn, 'weight', None), getattr(xn, 'slice_w', None)
    sums = torch.empty(3 * int(xd.shape[a]), dtype=torch.float64, device=xd.device)
    check(_lib.load().unires_gain_sums(_ptr(xd), _ptr(Ay.contiguous()), None if g is None else _ptr(g.contiguous()),
                                       None if u is None else _ptr(u.contiguous()), i3(xd.shape), a, _ptr(sums),
                                       _stream()))
    return sums


def gain_kappa(xn, gain_reg):
    """The precision of the gains' prior for one observation: kappa = gain_reg tau (sum_{x != 0} x^2) / K, K the number
    of slices along ``po.dim_thick`` that hold a non-zero voxel - gain_reg times the Q_s a typical slice has at
    e = 1.  A float64 sum on the device; returns a 0-d float64 device tensor (0 for an all-zero observation), not
    read back."""
    xd = xn.dat.double()
    a = _slice_axis(xn)
    K = (xn.dat != 0).sum(dim=[d for d in range(3) if d != a]).ne(0).sum()
    return float(gain_reg) * float(xn.tau) * (xd * xd).sum() / K.clamp(min=1).double()


@on_device
def _update_slice_gains(x, y, sett, raw=None):
    """Re-estimates the gains of every non-CT observation that has some by ``gain_rule``, from the current y and the
    repeat's current weights (``raw``: what ``_slice_sums`` kept of A y WITHOUT gains for this y, computed here where
    missing).  kappa is ``xn._gain_kappa``, which ``fit()`` fixes before the first iteration (computed here for a
    direct call).  The gain tensors are updated in place: their version counters tell the plans
    (``sync_slice_gains``, at the next y-update's plan fetch) and the cached sum tau At (w e . x).  No read-back.

    With ``sett.rician_gn`` a Rician repeat's sums are taken on its effective observation ``xn._rician_dat`` = x R(z),
    which ``_update_admm`` has just written at the current (y, e): ``gain_rule`` on it is
    the exact minimiser of the quadratic majoriser plus the ridge, so the gain step and the next y-update minimise one
    surrogate in turn, and neither increases the Rician objective.  The rule's x != 0 mask is then read on x R(z),
    which is 0 exactly where x is, apart from float32 underflow of the product.  kappa keeps reading ``xn.dat``.  A direct
    call reads the buffer as it finds it - a caller who has moved y or e since it was written calls ``_rician_terms``
    first, as ``_update_admm`` does; only where the repeat has none yet is it made here, at the current (y, e)."""
    reg, gmax = float(getattr(sett, 'gain_reg', 0.1)), float(getattr(sett, 'gain_max', 2.0))
    rician = bool(getattr(sett, 'rician_gn', False))
    for c in range(len(x)):
        for n, xn in enumerate(x[c]):
            e = getattr(xn, 'slice_gain', None)
            if e is None or getattr(xn, 'ct', False):
                continue
            Ay = None if raw is None else raw.get((c, n))
            if Ay is None:
                Ay = _proj('A', y[c].dat, x[c], y[c], n=n, method=sett.method, do=sett.do_proj)
            if getattr(xn, '_gain_kappa', None) is None:
                xn._gain_kappa = gain_kappa(xn, reg)
            obs = None
            if rician and _is_rician(xn, sett):
                if getattr(xn, '_rician_dat', None) is None:
                    _rician_terms([[xn]], [y[c]], sett, {(0, 0): Ay}, sums=False)
                obs = xn._rician_dat
            xn._gain_sums = _gain_sums(xn, Ay, obs)  # (kept: what the last estimate was taken from)
            e.copy_(gain_rule(xn._gain_sums, xn.tau, xn._gain_kappa, gmax))
    return x


def _slice_ll(tau, w, sums):
    """1/2 tau sum_s u_s SSE_s of one weighted repeat: ``w`` its (S,) weights, ``sums`` its ``unires_slice_sums``
    ((2 S,) float64: SSE_s, then N_s).  A float64 dot product on the device, no read-back.  The one statement of a
    weighted repeat's data term: the objective (``_compute_nll``) and the rigid update's line search take it from
    here.  ``w`` None: a repeat with voxel weights alone, u = 1 - ``sums`` are ``unires_voxel_sums``' then, which
    carry g."""
    if w is None:
        return 0.5 * float(tau) * sums[:sums.numel() // 2].sum()
    return 0.5 * float(tau) * (w.double() * sums[:w.numel()]).sum()


@on_device
def _rician_ll(w, L):
    """sum_s u_s L_s of one Rician repeat: ``L`` its (S,) float64 sums of g c(z) per slice (``unires_rician_terms``),
    ``w`` its (S,) slice weights or None (u = 1) - what the repeat's data term holds beside ``_slice_ll``'s (or the
    masked SSE's) Gaussian part, NOT multiplied by tau.  A float64 dot product on the device, no read-back."""
    return L.sum() if w is None else (w.double() * L).sum()


@on_device
def _rician_terms(x, y, sett, proj=None, sums=True, write=True):
    """One ``unires_rician_terms`` pass per Rician repeat (``_is_rician``) on the current y: with ``write`` the
    effective observation x R(tau x e . A y) goes in place into ``xn._rician_dat`` (made here where fit() has not),
    whose version counter is bumped - it tells the cached sum tau At (W e . x~) of the next y-update; with ``sums``
    returns {(c, n): (S,) float64 device tensor L_s = sum_{v in s} g c(z)}, else {} and nothing but x~ is written.
    ``proj``, a dict, holds (c, n): A y WITHOUT gains where already computed and receives it where computed here.  A
    user's fixed gains enter through mu = e . A y inside the kernel.  No read-back."""
    lib = _lib.load()
    out = {}
    for c in range(len(x)):
        for n, xn in enumerate(x[c]):
            if not _is_rician(xn, sett):
                continue
            Ay = None if proj is None else proj.get((c, n))
            if Ay is None:
                Ay = _proj('A', y[c].dat, x[c], y[c], n=n, method=sett.method, do=sett.do_proj)
                if proj is not None:
                    proj[(c, n)] = Ay
            xd = xn.dat.contiguous()
            a = _slice_axis(xn)
            g, e = getattr(xn, 'weight', None), getattr(xn, 'slice_gain', None)
            if e is not None:
                _check_gain(e, xd.shape[a])
            xt = None
            if write:
                if getattr(xn, '_rician_dat', None) is None:
                    xn._rician_dat = torch.empty_like(xd)
                xt = xn._rician_dat
            L = torch.empty(int(xd.shape[a]), dtype=torch.float64, device=xd.device) if sums else None
            check(lib.unires_rician_terms(_ptr(xd), _ptr(Ay.contiguous()),
                                          None if g is None or not sums else _ptr(g.contiguous()),
                                          None if e is None else _ptr(e), i3(xd.shape), a, float(xn.tau),
                                          None if xt is None else _ptr(xt), None if L is None else _ptr(L), _stream()))
            if write:
                torch.autograd.graph.increment_version(xt)
            if sums:
                out[(c, n)] = L
    return out


@on_device
def _compute_nll(x, y, sett, rho, sum_dtype=torch.float64, slice_sums=None, proj=None, rician=None):
    """Negative model log-likelihood (unires/_update.py:396-427); returns 0-d float64
    device tensors (nll_yx, nll_xy, nll_y) without synchronising.  A repeat with slice or voxel weights contributes
    1/2 tau sum_s u_s SSE_s (``slice_sums``: ``_slice_sums``' result for this y, computed here when None; SSE_s
    carries g for a voxel-weighted repeat, and is taken on e . A y for a repeat with gains).  Under ``sett.slice_gain``
    the gains' prior 1/2 kappa sum_s (e_s - 1)^2 of every estimated repeat is part of the data term's value.  Under
    ``sett.noise_model = 'rician'`` a non-CT repeat adds sum_s u_s L_s (``_rician_ll``; ``rician``: ``_rician_terms``'
    sums for this y, computed here - without touching the effective observations - when None; ``proj``: the A y
    without gains it computed); the term -log(tau x), which does not depend on y, is left out.  A repeat with a bias
    field is predicted by b . e . A y (``_predicted``), and under ``sett.bias`` the prior 1/2 c^T Lambda c of every
    estimated field is part of the data term's value."""
    dev = y[0].dat.device
    if rician is None and _noise_model(sett) == 'rician':
        proj = {} if proj is None else proj
        rician = _rician_terms(x, y, sett, proj, write=False)
    if slice_sums is None:
        slice_sums = _slice_sums(x, y, sett, proj=proj)
    lib = _lib.load()
    vx = [float(v) for v in voxel_size(y[0].mat).tolist()]
    nll_xy = torch.zeros((), dtype=torch.float64, device=dev)
    sse = torch.zeros((), dtype=torch.float64, device=dev)
    for c in range(len(x)):
        for n in range(len(x[c])):
            if _has_field(x[c][n]) and getattr(x[c][n], '_bias_est', False):  # (the estimated fields' prior)
                nll_xy = nll_xy + bias_energy(0.0, x[c][n]._bias_coef.numpy(), x[c][n]._bias_lam, 0.0)
            if rician and (c, n) in rician:
                nll_xy = nll_xy + _rician_ll(getattr(x[c][n], 'slice_w', None), rician[(c, n)])
            if (c, n) in slice_sums:
                nll_xy = nll_xy + _slice_ll(x[c][n].tau, getattr(x[c][n], 'slice_w', None), slice_sums[(c, n)])
                e = getattr(x[c][n], 'slice_gain', None)
                if e is not None and _slice_gain(sett) and not getattr(x[c][n], 'ct', False):
                    if getattr(x[c][n], '_gain_kappa', None) is None:
                        x[c][n]._gain_kappa = gain_kappa(x[c][n], getattr(sett, 'gain_reg', 0.1))
                    nll_xy = nll_xy + 0.5 * x[c][n]._gain_kappa * ((e.double() - 1.0) ** 2).sum()
                continue
            Ay = None if proj is None else proj.get((c, n))
            if Ay is None:
                Ay = _proj('A', y[c].dat, x[c], y[c], n=n, method=sett.method, do=sett.do_proj)
            Ay = _predicted(Ay, x[c][n])  # (a repeat with a field and no weights: b . A y, out of place)
            xd = x[c][n].dat.contiguous()
            check(lib.unires_masked_sse(_ptr(xd), _ptr(Ay), xd.numel(), _ptr(sse), _stream()))
            nll_xy = nll_xy + 0.5 * float(x[c][n].tau) * sse
    ptrs, lams = _chan_args(y)
    nll_y = torch.zeros((), dtype=torch.float64, device=dev)
    diff = _lib.diff_code(_diff(sett), 'sett.diff')
    check(lib.unires_nll_prior_which(ptrs, lams, len(y), i3(y[0].dim), f3(vx), diff, _ptr(nll_y), _stream()))
    return nll_xy + nll_y, nll_xy, nll_y


@on_device
def _update_scaling(x, y, sett, max_niter_gn=1, num_linesearch=4, verbose=0):
    """Updates the even/odd slice scaling parameter of every observation by Gauss-Newton
    (unires/_update.py:270-393).  ``A y`` comes from the fused pull+conv kernel, the five masked
    float64 sums of a step (ll, gradient and Hessian terms) from ONE reduction kernel instead
    of ten masked-index passes; the step logic - including the reference's line search, which
    rescales the already rescaled ``dat_y`` after a rejected step (:362-366) - runs on the host
    with one 40-byte read-back per evaluation.  ``po.rigid`` is used where the reference
    recomputes the same matrix from ``rigid_q`` (:301).  Returns (x, sll).

    A repeat with slice weights (``xn.slice_w``, a float32 device tensor as ``fit()`` leaves it) minimises its own data
    term 1/2 tau sum_v u[s(v)] [x != 0] (x - A y)^2: every one of the five sums carries the weight of the voxel's slice
    (``unires_scaling_sums_w``).  A repeat whose weights are all zero has no data term: its ``po.scl`` is left as it
    is and it adds 0 to ``sll``.  A repeat without weights runs exactly what it ran before.

    With ``sett.voxel_gn`` a repeat with voxel weights (``xn.weight``, a contiguous float32 device tensor as ``fit()``
    leaves it) minimises 1/2 tau sum_v g(v) u[s(v)] [x != 0] (x - A y)^2: the five sums carry g, and the slice weights
    where the repeat has both (``unires_scaling_sums_g``); all weights zero: left alone, as above.  Without
    ``sett.voxel_gn`` ``xn.weight`` is ignored, as it was before the update could carry it."""
    from ._project import _apply_scaling
    if sett.method != 'super-resolution':
        raise ValueError('_update_scaling needs the super-resolution projection '
                         '(slice profile + slice scaling)')
    lib = _lib.load()
    dev = y[0].dat.device
    sll = torch.zeros((), dtype=torch.float64, device=dev)
    sums = torch.empty(5, dtype=torch.float64, device=dev)
    for c in range(len(x)):
        for n_x in range(len(x[c])):
            xn = x[c][n_x]
            if xn.ct:  # do not optimise scaling for CT data (:288-290)
                continue
            po = xn.po
            dim_thick, tau, scl = int(po.dim_thick), float(xn.tau), float(po.scl)
            plan = _channel_plan(x[c], y[c], sett.method, sett.do_proj)
            dat_x = xn.dat.contiguous()
            dat_y = plan.proj_apply(n_x, 'A', y[c].dat)  # pull + conv + S(scl)  (:316-322)
            u = getattr(xn, 'slice_w', None)
            u = None if u is None else u.contiguous()
            g = _gn_weight(xn, sett)

            def evaluate(ay):
                if g is not None:
                    check(lib.unires_scaling_sums_g(_ptr(dat_x), _ptr(ay), i3(dat_x.shape), dim_thick, _ptr(g),
                                                    None if u is None else _ptr(u), _ptr(sums), _stream()))
                elif u is None:
                    check(lib.unires_scaling_sums(_ptr(dat_x), _ptr(ay), i3(dat_x.shape), dim_thick,
                                                  _ptr(sums), _stream()))
                else:
                    check(lib.unires_scaling_sums_w(_ptr(dat_x), _ptr(ay), i3(dat_x.shape), dim_thick, _ptr(u),
                                                    _ptr(sums), _stream()))
                return sums.tolist()  # one small device-to-host copy

            ll = 0.0
            empty = False
            for _ in range(max_niter_gn):
                s = evaluate(dat_y)
                ll = 0.5 * tau * s[0]
                gr = tau * (s[1] - s[2])
                hes = tau * (s[3] + s[4])
                if (u is not None or g is not None) and hes == 0.0:  # (all weights zero: no data term, no step - not the 0 / 0 below)
                    empty = True
                    break
                update = float(torch.tensor(gr, dtype=torch.float64) / torch.tensor(hes, dtype=torch.float64))  # IEEE: 0/0 -> nan, like the reference's tensors
                old_scl, old_ll, armijo = scl, ll, 1.0
                if num_linesearch == 0:
                    scl = old_scl - armijo * update
                else:
                    for _ls in range(num_linesearch):
                        scl = old_scl - armijo * update
                        dat_y = _apply_scaling(dat_y, scl - old_scl, dim_thick)
                        ll = 0.5 * tau * evaluate(dat_y)[0]
                        if ll < old_ll:
                            break
                        scl, ll = old_scl, old_ll
                        armijo *= 0.5
                if verbose >= 1:
                    print('c={}, n={} | exp(s)={:.5f} ll={:.2f}'.format(c, n_x, torch.tensor(scl).exp(), ll))
            if empty:
                continue
            po.scl = scl  # the next _channel_plan() call rebuilds the operator with it
            sll = sll + ll
    return x, sll


@on_device
def _update_admm(x, y, z, w, rho, tmp, obj, n_iter, sett, info=None):
    """One ADMM iteration (unires/_update.py:105-195): y-update (CG), objective,
    z-update, w-update - same order, same in-place semantics, `tmp` returned as the
    joint-TV shrinkage image."""
    y = _update_y(x, y, z, w, rho, tmp, sett, info)
    want_obj = obj is not None and sett.tolerance > 0
    # (the per-slice residual sums of the weighted repeats: once, for the objective and for the rules; A y of the
    # voxel-weighted repeats is kept for the Huber rule)
    ays = {} if _voxel_robust(sett) else None
    raw = {} if _slice_gain(sett) else None  # (A y without gains of the gained repeats, for the gain rule)
    # (the Rician repeats: A y once - it serves the sums below, the objective's correction and the effective
    # observation of the next y-update, written here; without an objective nothing but that is written)
    proj = {} if _noise_model(sett) == 'rician' else None
    rician = _rician_terms(x, y, sett, proj, sums=want_obj) if proj is not None else None
    mus = {} if _bias(sett) else None  # (e . A y without the field of the repeats with one, for the bias step)
    sums = _slice_sums(x, y, sett, ays, raw, proj, mus) if want_obj or _slice_robust(sett) or _slice_gain(sett) else None
    if want_obj:
        obj[n_iter, 0], obj[n_iter, 1], obj[n_iter, 2] = _compute_nll(x, y, sett, rho, slice_sums=sums, proj=proj,
                                                                     rician=rician)
    z, w, tmp = _update_zw(y, z, w, rho, tmp, sett)
    if _slice_gain(sett):  # (before the rules below write their weights: it reads the W this iteration's y-update used;
        _update_slice_gains(x, y, sett, raw)  # sums and ays keep the prediction e . A y of that y-update's gains)
    if _bias(sett):  # (in the same place, for the same reason; fit() refuses the two together)
        _update_bias(x, y, sett, mus)
    if _slice_robust(sett):  # (after the objective: each iteration's is taken with the weights its y-update used)
        _update_slice_weights(x, y, sett, sums)
    if _voxel_robust(sett):  # (likewise; A y is computed there where the sums above were not wanted)
        _update_voxel_weights(x, y, sett, ays)
    if any(_has_field(xn) for xc in x for xn in xc):  # (after the rules: g b^2 and x / b follow the new c and g)
        _bias_compose(x, sett)
    # An iteration is enqueue-only (no read-back): a host loop would run ahead until the hardware queue is
    # full and then spin inside every launch call.  The pacer parks the thread - sleeping between looks at a
    # stream mark (_host.StreamMark) - until the device is at most `host_pace` iterations behind (settings.host_pace; 0: off).
    depth = int(getattr(sett, 'host_pace', 2) or 0)
    if depth > 0 and y[0].dat.is_cuda:
        key = (y[0].dat.device.index, depth)
        pacer = _PACERS.get(key)
        if pacer is None:
            pacer = _PACERS[key] = Pacer(depth)
        pacer.step()
    return y, z, w, tmp, obj
