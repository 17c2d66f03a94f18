"""Projection operators of the y-update - host-side mirror of
unires/_project.py (same names, argument meaning and errors), backed by HIP.

    _apply_scaling   unires/_project.py:9-24
    _check_adjoint   unires/_project.py:27-51
    _proj            unires/_project.py:54-96
    _proj_apply      unires/_project.py:99-190
    _proj_info       unires/_project.py:193-297
    _DtD             unires/_project.py:300-317
"""
import math

import numpy as np
import torch

from . import _kernels, _lib, _ops
from ._plan import ChannelPlan, proj_matrix
from .spatial import _m12, voxel_size
from .struct import _proj_op

_F64 = torch.float64


def _apply_scaling(dat, scl, dim):
    """Even/odd slice scaling along ``dim`` (a conv with a 1-tap identity kernel and
    the scaling epilogue of the conv kernel)."""
    one = [np.ones(1, np.float32)] * 3
    return _ops.conv_down(dat, one, (1, 1, 1), scl=float(scl), scl_dim=int(dim))


def _proj_info(dim_y, mat_y, dim_x, mat_x, rigid=None, prof_ip=0, prof_tp=0, gap=0.0,
               device='cuda', scl=0.0, samp=0, gauss_lim=None, ratio_tol=0.0):
    """Define a projection operator object for _proj_apply.  All 4x4 arithmetic is
    float64 on the host (it is set-up work: once per input, again per rigid update)."""
    po = _proj_op()
    mat_y = torch.as_tensor(mat_y).detach().to('cpu', _F64)
    mat_x = torch.as_tensor(mat_x).detach().to('cpu', _F64)
    dim_y = tuple(int(d) for d in dim_y)
    dim_x = tuple(int(d) for d in dim_x)
    if len(dim_y) != 3 or len(dim_x) != 3:
        raise ValueError('only 3-D volumes are built')
    po.dim_y, po.mat_y, po.vx_y = dim_y, mat_y, voxel_size(mat_y)
    po.dim_x, po.mat_x, po.vx_x = dim_x, mat_x, voxel_size(mat_x)
    po.rigid = torch.eye(4, dtype=_F64) if rigid is None \
        else torch.as_tensor(rigid).detach().to('cpu', _F64)
    po.D_x = po.D_y = None
    # thick-slice axis and per-axis profile / gap: from the ORIGINAL voxel size, before any
    # sub-sampling (unires/_project.py:239-243 sit above the samp block :245-264; decimation can move
    # the argmax: vx_x = (0.4, 0.4, 1), samp = 1 decimates to (0.8, 0.8, 1) - still z - but
    # vx_x = (0.5, 0.5, 0.8) becomes (1, 1, 0.8))
    po.dim_thick = int(torch.max(po.vx_x, dim=0)[1])
    profile = [int(prof_ip)] * 3
    gaps = [0.0] * 3
    profile[po.dim_thick] = int(prof_tp)
    gaps[po.dim_thick] = float(gap)
    if samp > 0:
        # sub-sampling for the rigid Gauss-Newton (unires/_project.py:245-264): the low-res image is
        # decimated by sk = max(1, floor(samp / vx_x + 0.5)) voxels per axis: mat_x <- mat_x D_x,
        # dim_x <- floor(dim_x / sk).  (The high-res branch is dead code in the reference - :255
        # compares vx_x with itself - so D_y stays None.)  po.sk is the decimation the caller
        # applies to the data: nearest-neighbour pull at the integer coordinates D_x u = a strided
        # slice (unires/_update.py:589-593).
        sk = torch.clamp(torch.floor(float(samp) / po.vx_x + 0.5), min=1.0)
        po.sk = tuple(int(v) for v in sk.tolist())
        po.D_x = torch.diag(torch.cat((sk, torch.ones(1, dtype=_F64))))
        mat_x = mat_x.mm(po.D_x)
        dim_x = tuple(int(math.floor(d / k)) for d, k in zip(dim_x, po.sk))
        if min(dim_x) < 1:
            raise ValueError('sub-sampling leaves an empty image')
        po.dim_x, po.mat_x, po.vx_x = dim_x, mat_x, voxel_size(mat_x)
    # low-res / high-res voxel ratio, rounded up, at least one.  ratio_tol (relative; 0: the reference's plain
    # ceil) is the fraction by which a ratio may exceed an integer and still count as that integer: the ratio of
    # equal voxel sizes comes out of the solve as 1 + 2e-16 as soon as mat_x carries a rotation (after
    # coregistration, against a mean space), and a rotated affine read from a float32 sform as r (1 + 1e-7); the
    # plain ceil turns either into the next integer
    lin = torch.linalg.solve(mat_y, mat_x)[:3, :3]
    ratio = ((lin ** 2).sum(0).sqrt() * (1.0 - float(ratio_tol))).ceil().clamp(1)
    po.ratio = tuple(int(r) for r in ratio.tolist())
    # intermediate (high-res sampling of the low-res FOV) space
    po.mat_yx = mat_x.matmul(torch.diag(torch.cat((1.0 / ratio, torch.ones(1, dtype=_F64)))))
    dim_yx = [(dx - 1) * r + 1 for dx, r in zip(dim_x, po.ratio)]
    # slice profile (dirac where the ratio is one), separable factors + dense form
    k1 = []
    for d in range(3):
        kind = -1 if po.ratio[d] == 1 else profile[d]
        k1.append(_kernels.smooth1d(kind, (1.0 - gaps[d]) * po.ratio[d], gauss_lim))
    po.smo_ker_1d = [torch.from_numpy(k.astype(np.float32)) for k in k1]
    dense = k1[0][:, None, None] * k1[1][None, :, None] * k1[2][None, None, :]
    po.smo_ker = torch.from_numpy(dense.astype(np.float32))[None, None].to(device)
    # centre the kernel: shift the intermediate space by floor(-(k-1)/2) and grow it
    off = [int(math.floor(-(len(k) - 1) / 2.0)) for k in k1]
    mat_off = torch.eye(4, dtype=_F64)
    mat_off[:3, 3] = torch.tensor(off, dtype=_F64)
    po.mat_yx = po.mat_yx.matmul(mat_off)
    po.dim_yx = tuple(int(n + 2 * abs(o)) for n, o in zip(dim_yx, off))
    po.scl = scl if isinstance(scl, torch.Tensor) else torch.tensor(scl, dtype=torch.float32)
    return po


def _taps(po):
    if getattr(po, 'smo_ker_1d', None) is None:  # user supplied only the dense kernel
        po.smo_ker_1d = [torch.from_numpy(k) for k in
                         _kernels.factorise(po.smo_ker.detach().cpu().numpy())]
    return [k.detach().cpu().numpy() for k in po.smo_ker_1d]


def _proj_apply(operator, dat, po, method='super-resolution', bound='zero',
                interpolation='linear'):
    """Applies A, At or AtA (denoising or super-resolution) to (1,1,X,Y,Z) data.
    Composed from op-level HIP kernels with on-the-fly coordinates."""
    if operator not in ['A', 'At', 'AtA', 'none']:
        raise ValueError('Undefined operator')
    if method not in ['denoising', 'super-resolution']:
        raise ValueError('Undefined method')
    if bound != 'zero' or interpolation not in ('linear', 1):
        raise NotImplementedError("only bound='zero', interpolation='linear' are built")
    if operator == 'none':
        return dat
    mat, dim_g = proj_matrix(po, method)
    M = _m12(mat)
    scl = float(po.scl)
    if method == 'super-resolution':
        taps = _taps(po)
        if operator == 'A':
            return _ops.conv_down(_ops.pull_affine(dat, M, dim_g), taps, po.ratio, scl,
                                  po.dim_thick)
        if operator == 'At':
            return _ops.push_affine(_ops.conv_up(dat, taps, po.ratio, scl, po.dim_thick), M,
                                    po.dim_y)
        low = _ops.conv_down(_ops.pull_affine(dat, M, dim_g), taps, po.ratio, 2.0 * scl,
                             po.dim_thick)
        return _ops.push_affine(_ops.conv_up(low, taps, po.ratio), M, po.dim_y)
    if operator == 'A':
        return _ops.pull_affine(dat, M, dim_g)
    if operator == 'At':
        return _ops.push_affine(dat, M, po.dim_y)
    return _ops.push_affine(_ops.pull_affine(dat, M, dim_g), M, po.dim_y)


def _plan_regime(method, do, mask_zeros=False):
    """(method, do) a channel's plan is built with.  The user's, but for regime A = I (``do`` false) under
    ``sett.mask_zeros``: that regime's matvec is the flat stencil alone and has no x-space intermediate to mask, so
    the plan is built in the denoising regime with the identity affine and runs pull -> mask -> push.  A channel
    with a weighted repeat (``_input.slice_w``) takes the same detour: ``_channel_plan`` passes ``mask_zeros`` true
    for it."""
    if method not in ('denoising', 'super-resolution'):
        raise ValueError('Undefined method')
    if mask_zeros and not do:
        return 'denoising', True
    return method, bool(do)


_IDENTITY_PO = {}


def _identity_po(y):
    """The descriptor of an observation on the output's own grid: A = I as a denoising-regime operator (one per
    output shape, kept)."""
    dim = tuple(int(d) for d in y.dim)
    po = _IDENTITY_PO.get(dim)
    if po is None:
        po = _IDENTITY_PO[dim] = _proj_op()
        po.mat_y = po.mat_x = po.rigid = torch.eye(4, dtype=_F64)
        po.dim_x = po.dim_y = dim
    return po


def _plan_repeats(x, y, do, mask_zeros):
    """(po, tau) per repeat, as the plan takes them (``_plan_regime``)."""
    if mask_zeros and not do:
        po = _identity_po(y)
        return [(po, xn.tau) for xn in x]
    return [(xn.po, xn.tau) for xn in x]


def _plan_signature(x, y, method, do, mask_zeros=False):
    """What identifies a cached plan.  The setting is part of it where it decides the plan's regime (A = I); a plan
    with projection serves both values, its masks set or cleared in place."""
    sig = [method, (bool(do), bool(mask_zeros) and not do), tuple(y.dim)]
    for xn in x:
        po = xn.po
        if do:
            mat, dim_g = proj_matrix(po, method)
            taps = tuple(tuple(float(v) for v in k) for k in _taps(po)) \
                if method == 'super-resolution' else ()
            sig.append((tuple(_m12(mat).tolist()), dim_g, tuple(po.dim_x), float(po.scl),
                        float(xn.tau), tuple(po.ratio), taps))
        else:
            sig.append((float(xn.tau),))
    return tuple(sig)


def _slice_axis(xn):
    """The caller's voxel axis the slices of an observation are counted along: ``po.dim_thick`` (the last axis where
    the descriptor names none)."""
    return _thick_axis(xn.po)


def _thick_axis(po):
    """``po.dim_thick``, the last axis where the descriptor names none."""
    a = getattr(po, 'dim_thick', None)
    return 2 if a is None else int(a)


def _slice_weights(x):
    """Per repeat ``(axis, weights)`` or None, as ``ChannelPlan.sync_slice_weights`` takes them; None when no repeat
    of the channel has weights."""
    ws = [None if getattr(xn, 'slice_w', None) is None else (_slice_axis(xn), xn.slice_w) for xn in x]
    return ws if any(w is not None for w in ws) else None


def _voxel_weights(x):
    """Per repeat the voxel weights ``xn.weight`` or None, as ``ChannelPlan.sync_voxel_weights`` takes them; None when
    no repeat of the channel has some.  For a repeat with a bias field the plan's map is ``xn._bias_weight`` = g b^2
    (``_update._bias_compose``; g = 1 without weights): W b^2 in the matrix and, with the effective observation x / b,
    W b x on the right.  Everything else that reads ``xn.weight`` - the sums, the Huber rule, its prior - keeps the
    true g."""
    gs = [getattr(xn, 'weight', None) if getattr(xn, '_bias_weight', None) is None else xn._bias_weight for xn in x]
    return gs if any(g is not None for g in gs) else None


def _slice_gains(x):
    """Per repeat ``(axis, gains)`` or None, as ``ChannelPlan.sync_slice_gains`` takes them; None when no repeat of the
    channel has gains."""
    es = [None if getattr(xn, 'slice_gain', None) is None else (_slice_axis(xn), xn.slice_gain) for xn in x]
    return es if any(e is not None for e in es) else None


def _channel_plan(x, y, method, do, vx_y=None, diff=None, mask_zeros=None, weights=None):
    """Fused per-channel plan, cached on the output struct and rebuilt when any
    operator parameter (rigid, scl, tau, dims) changed.  ``diff``: the difference of the plan's D
    ('forward' | 'backward' | 'central'); None leaves the plan's as it is (callers that do not involve D).
    ``mask_zeros``: ``sett.mask_zeros`` - the plan's A^T A treats the zero voxels of each observation as missing
    (``ChannelPlan.set_missing``; the masks follow the observation tensors and their versions); None leaves the plan
    as it is (callers that apply A or A^T only, which no mask changes).
    ``weights``: True - the plan's A^T A and right-hand side carry the per-slice weights ``xn.slice_w`` of the repeats
    that have some (``ChannelPlan.set_slice_weights``; they follow the weight tensors and their versions); False -
    the unweighted operator; None leaves the plan as it is.  The per-voxel weights ``xn.weight``
    (``ChannelPlan.set_voxel_weights``) and the per-slice gains ``xn.slice_gain`` (``ChannelPlan.set_slice_gains``) go
    with them."""
    cached = getattr(y, '_plan', None)
    if mask_zeros is None:
        mask_zeros = cached[1].mask_zeros if cached is not None else False
    if weights is None:
        weights = cached[1].weights if cached is not None else False
    ws = _slice_weights(x) if weights else None
    gs = _voxel_weights(x) if weights else None
    es = _slice_gains(x) if weights else None
    # (regime A = I has no x-space intermediate for any of the passes: the denoising regime with the identity affine)
    plan = _channel_plan_any(x, y, method, do, vx_y,
                             bool(mask_zeros) or ws is not None or gs is not None or es is not None)
    if diff is not None:
        plan.set_diff(diff)
    plan.sync_missing([xn.dat for xn in x] if mask_zeros else None)
    plan.sync_slice_weights(ws)
    plan.sync_voxel_weights(gs)
    plan.sync_slice_gains(es)
    plan.mask_zeros, plan.weights = bool(mask_zeros), bool(weights)
    return plan


def _channel_plan_any(x, y, method, do, vx_y=None, mask_zeros=False):
    sig = _plan_signature(x, y, method, do, mask_zeros)
    repeats = _plan_repeats(x, y, do, mask_zeros)
    method, do = _plan_regime(method, do, mask_zeros)
    cached = getattr(y, '_plan', None)
    if cached is not None and cached[0] == sig:
        return cached[1]
    if cached is not None and len(cached[0]) == len(sig) and cached[0][:3] == sig[:3]:
        # same volume and method, some repeat's operator changed (rigid / scaling update):
        # swap the descriptors in place, keeping the plan's device workspace
        plan = cached[1]
        try:
            for n, (old, new) in enumerate(zip(cached[0][3:], sig[3:])):
                if old != new:
                    plan.set_repeat(n, *repeats[n])
            plan.dims_x = [tuple(po.dim_x) for po, _ in repeats] if do else plan.dims_x
            plan._atx = None  # cached sum tau At x belongs to the old operator
            y._plan = (sig, plan)
            return plan
        except ValueError:
            pass  # the new repeat does not fit the workspace: build a new plan
    old_diff = 'forward'
    if cached is not None:
        old_diff = cached[1].diff
        cached[1].close()
    if vx_y is None:
        vx_y = voxel_size(y.mat)
    vx = [float(v) for v in torch.as_tensor(vx_y).detach().cpu().tolist()]
    plan = ChannelPlan(y.dim, vx, repeats, method, do, device=y.dat.device, diff=old_diff)
    y._plan = (sig, plan)
    return plan


def _proj(operator, dat, x, y, method='super-resolution', do=True, rho=1, n=0, vx_y=None,
          interpolation='linear', bound='zero', diff='forward'):
    """Projects image data by A, At or AtA; ``x`` is the list of repeats of one
    channel, ``y`` its output struct.  'AtA' is the fused
    sum_n tau_n AtA_n dat + rho lam^2 DtD dat."""
    _lib.diff_code(diff, 'diff')
    if bound != 'zero' or interpolation not in ('linear', 1):
        raise NotImplementedError("only bound='zero', linear are built")
    # (the facade's AtA is the reference's, which has no mask and no weights; A and At take the plan as it is)
    plan = _channel_plan(x, y, method, do, vx_y, diff=diff if operator == 'AtA' else None,
                         mask_zeros=False if operator == 'AtA' else None, weights=False if operator == 'AtA' else None)
    if operator == 'AtA':
        return plan.matvec(dat, float(rho), float(y.lam))
    if operator not in ('A', 'At'):
        raise ValueError('Undefined operator')
    return plan.proj_apply(n, operator, dat)


def _DtD(dat, vx_y, bound='zero', diff='forward'):
    """Divergence of the gradient, one stencil pass (7 points; central differences: the 6 at distance 2)."""
    _lib.diff_code(diff, 'diff')
    if bound != 'zero':
        raise NotImplementedError("only bound='zero' is built")
    return _ops.dtd(dat, vx_y, a=0.0, c=1.0, which=diff)


def _check_adjoint(po, method, bound='zero', interpolation='linear', dtype=torch.float32):
    """<Ay, x> - <Atx, y> with seed-0 uniform inputs.  Returns the value (the
    reference prints it).  The kernels are float32; float64 is not built."""
    if dtype != torch.float32:
        raise NotImplementedError('the HIP kernels are float32')
    torch.manual_seed(0)
    dev = po.smo_ker.device
    x = torch.rand((1, 1) + tuple(po.dim_x), dtype=dtype).to(dev)
    y = torch.rand((1, 1) + tuple(po.dim_y), dtype=dtype).to(dev)
    Ay = _proj_apply('A', y, po, method=method, bound=bound, interpolation=interpolation)
    Atx = _proj_apply('At', x, po, method=method, bound=bound, interpolation=interpolation)
    val = torch.sum(Ay * x, dtype=torch.float64) - torch.sum(Atx * y, dtype=torch.float64)
    return val.item()
