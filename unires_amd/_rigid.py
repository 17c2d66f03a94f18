"""Unified rigid registration - host-side mirror of unires/_update.py:198-266 (_update_rigid),
:448-538 (_rigid_match) and :541-710 (_update_rigid_channel).

One Gauss-Newton step per observation on q in se(3):  rigid = expm(sum_i q_i B_i).
The reference builds ~40 volume-sized temporaries per step (Hes (dim,6), 18 dAff volumes, 27
masked products); here a step is: pull, conv, residual, conv_transpose, grid_grad with the HIP
ops, then ONE reduction kernel (unires_rigid_sums) that returns the 6-gradient and the 21
Hessian entries.  The 4x4 algebra (expm and its derivative) is float64 host work.

Basis: the reference takes nitorch's affine_basis('SE') (unires/_core.py:317).  A Gauss-Newton
step, the Armijo line search and the mean correction are invariant under any linear change of
basis of se(3) (g' = S^T g, H' = S^T H S, q' = S^-1 q give the same algebra element), so the
rigid matrices and log-likelihoods this module produces do not depend on nitorch's ordering or
sign conventions; only the numeric values of rigid_q do.  Ours: three translations, then the
rotation generators about x, y, z.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, _ops
from ._host import light_host
from ._lib import check, i3
from ._ops import _ptr, _stream, on_device
from ._project import _apply_scaling, _proj_info, _slice_axis, _taps, _thick_axis
from ._update import _check_gain, _gn_gain, _gn_weight, _is_rician, _rician_ll, _slice_ll
from .spatial import _m12

_F64 = torch.float64


def affine_basis(group='SE', device='cpu', dtype=_F64):
    """(6, 4, 4) generators of se(3): T_x, T_y, T_z, R_x, R_y, R_z."""
    if group != 'SE':
        raise NotImplementedError("only the rigid group 'SE' is built")
    B = torch.zeros(6, 4, 4, dtype=dtype)
    for d in range(3):
        B[d, d, 3] = 1.0
    B[3, 1, 2], B[3, 2, 1] = -1.0, 1.0
    B[4, 0, 2], B[4, 2, 0] = 1.0, -1.0
    B[5, 0, 1], B[5, 1, 0] = -1.0, 1.0
    return B


def _expm_small(M):
    """Matrix exponential of a small float64 matrix: scaling and squaring with a degree-16 Taylor
    polynomial (norm scaled below 1/4: truncation error < 1e-20)."""
    import numpy as np
    nrm = np.abs(M).sum(1).max()
    sq = max(0, int(np.ceil(np.log2(max(nrm, 1e-300) * 4.0))))
    A = M / (2.0 ** sq)
    E = np.eye(M.shape[0])
    T = np.eye(M.shape[0])
    for k in range(1, 17):
        T = T @ A / k
        E = E + T
    for _ in range(sq):
        E = E @ E
    return E


def _expm(q, basis, grad_X=False):
    """rigid = expm(sum_i q_i basis_i) [, d rigid / d q_i as (num_q, 4, 4)]  (float64, host)."""
    import numpy as np
    expm = _expm_small  # tiny matrices: plain numpy beats torch's threaded CPU ops (and scipy) here
    qn = np.asarray(torch.as_tensor(q, dtype=_F64).cpu())
    Bn = np.asarray(basis.to('cpu', _F64))
    X = np.einsum('i,ijk->jk', qn, Bn)
    if not grad_X:
        return torch.from_numpy(expm(X))
    # Frechet derivative by the block trick: expm([[X, B_i], [0, X]]) = [[e^X, dexp_X(B_i)], [0, e^X]]
    dR = np.empty((Bn.shape[0], 4, 4))
    R = None
    for i in range(Bn.shape[0]):
        M = np.zeros((8, 8))
        M[:4, :4] = X
        M[4:, 4:] = X
        M[:4, 4:] = Bn[i]
        E = expm(M)
        R, dR[i] = E[:4, :4], E[:4, 4:]
    return torch.from_numpy(R.copy()), torch.from_numpy(dR)


def _logq(rigid, basis):
    """q with expm(sum q_i B_i) = rigid (principal logarithm), for structs that carry only
    po.rigid."""
    import numpy as np
    from scipy.linalg import logm
    L = np.real(logm(torch.as_tensor(rigid, dtype=_F64).cpu().numpy()))
    A = basis.to('cpu', _F64).reshape(basis.shape[0], -1).T.contiguous().numpy()  # (16, num_q)
    # numpy's least squares, not torch's: torch.linalg.lstsq on this 16 x 6 system returns different last bits from one
    # call to the next (13 distinct results in 300 calls on the same matrix; the logarithm above does not vary), and
    # two rigid updates of the same data then differ in every bit that follows.  numpy's gave one result in 500 calls,
    # within 6e-17 of torch's.
    q = np.linalg.lstsq(A, np.ascontiguousarray(L).reshape(-1), rcond=None)[0]
    return torch.from_numpy(np.array(q, dtype=np.float64))


def _grid_matrix(po, rigid, method):
    mat = po.mat_yx if method == 'super-resolution' else po.mat_x
    dim = tuple(po.dim_yx) if method == 'super-resolution' else tuple(po.dim_x)
    return torch.linalg.solve(po.mat_y, torch.as_tensor(rigid, dtype=_F64).cpu().mm(mat)), dim


@on_device
def _rigid_terms(dat_x, dat_y, po, tau, rigid, sett, diff=False, slice_w=None, axis=None, weight=None, gain=None,
                 rician=False):
    """ll and, if ``diff``, the raw ingredients of the derivatives: gr3 (dim,3) = grid_grad,
    dg (dim) = residual in grid space.

    ``slice_w``: the repeat's slice weights along ``axis`` of ``dat_x`` (float32, on the device, one per slice of
    ``dat_x`` - already decimated where ``dat_x`` is), or None.  With weights the terms are those of the weighted data
    term 1/2 tau sum_v u[s(v)] [x != 0] (x - A y)^2: ll = 1/2 tau sum_s u_s SSE_s from ``unires_slice_sums``
    (``_update._slice_ll``, the objective's own expression) and the x-space residual u[s(v)] (A y - x), masked, in one
    pass (``unires_rigid_resid``).  Without, the code path is what it was.

    ``weight``: the repeat's voxel weights (float32, on the device, the shape of ``dat_x`` - already decimated where
    ``dat_x`` is), or None; ``axis`` is then the repeat's slice axis whether or not it has slice weights.  The terms are
    those of 1/2 tau sum_v g(v) u[s(v)] [x != 0] (x - A y)^2: ll = 1/2 tau sum_s u_s SSE_s with SSE_s from
    ``unires_voxel_sums``, which carries g - the statement ``_compute_nll`` takes a voxel-weighted repeat's term from -
    and the residual g u[s(v)] (A y - x), masked, in one pass (``unires_rigid_resid_g``).

    ``gain``: the repeat's slice gains along ``axis`` (float32, on the device, one per slice of ``dat_x`` - already
    decimated where ``dat_x`` is), or None.  The terms are those of 1/2 tau sum_v g(v) u[s(v)] [x != 0] (x - e[s(v)] A y)^2
    (g, u = 1 where None) on the gained prediction p = fl32(e A y), which is formed in registers and never stored: one
    pass (``unires_rigid_terms_e``) gives the slice sums of x - p - ll = 1/2 tau sum_s u_s SSE_s by ``_slice_ll``, to the
    bit ``_compute_nll``'s term of the repeat - and, with ``diff``, the residual g u e (p - x), masked where x or p is 0:
    the factor e is the chain rule through diag(e).  The ridge 1/2 kappa sum (e - 1)^2 of ``sett.slice_gain`` does not
    depend on the rigid parameters and is left out of ll.

    ``rician``: the repeat has the Rician data term (``sett.noise_model = 'rician'`` with ``sett.rician_gn``; ``axis`` is
    then its slice axis whatever else it has, ``dat_x`` the TRUE observation, never the effective one).  The terms are
    those of sum_v W [1/2 tau (x - p)^2 + c(tau x p)], W = g u [x != 0 for the square], p = fl32(e A y), from one pass
    (``unires_rigid_terms_r``; g, u, e each optional): ll = ``_slice_ll`` of its first 2 S sums plus ``_rician_ll`` of
    its last S - ``_compute_nll``'s statement for the repeat, to the bit where the repeat has weights or gains - and,
    with ``diff``, the residual W e (p - x R(tau x p)), masked where x or p is 0: tau times it is the exact derivative
    of the Rician term in A y, the Gaussian residual on the effective observation taken at the current prediction."""
    method = sett.method
    lib = _lib.load()
    mat, dim = _grid_matrix(po, rigid, method)
    M = _m12(mat)
    dat_yx = _ops.pull_affine(dat_y, M, dim)
    if method == 'super-resolution':
        scl = float(po.scl)
        dat_yx = _ops.conv_down(dat_yx, _taps(po), po.ratio, scl, po.dim_thick)
    dat_yx = dat_yx.reshape(tuple(dat_x.shape))
    if rician:
        dat_x, dat_yx = dat_x.contiguous(), dat_yx.contiguous()
        S = int(dat_x.shape[axis])
        if gain is not None:
            _check_gain(gain, S)
        if weight is not None:
            weight = weight.contiguous()
            if weight.dtype != torch.float32 or tuple(weight.shape) != tuple(dat_x.shape):
                raise ValueError('weight: one float32 weight per voxel of dat_x')
        if slice_w is not None:
            slice_w = slice_w.contiguous()
            if slice_w.dtype != torch.float32 or slice_w.numel() != S:
                raise ValueError('slice_w: one float32 weight per slice of dat_x along axis %d' % axis)
        sums = torch.empty(3 * S, dtype=_F64, device=dat_x.device)
        # (with diff the residual goes over A y in place: A y is not needed again)
        check(lib.unires_rigid_terms_r(_ptr(dat_x), _ptr(dat_yx), None if weight is None else _ptr(weight),
                                       None if slice_w is None else _ptr(slice_w), None if gain is None else _ptr(gain),
                                       i3(dat_x.shape), axis, float(tau), _ptr(sums), _ptr(dat_yx) if diff else None,
                                       _stream()))
        # (L_s in a tensor of its own, as _compute_nll holds it: the same reduction, whatever the offset of a view)
        ll = _slice_ll(tau, slice_w, sums[:2 * S]) + _rician_ll(slice_w, sums[2 * S:].clone())
    elif gain is not None:
        dat_x, dat_yx = dat_x.contiguous(), dat_yx.contiguous()
        _check_gain(gain, dat_x.shape[axis])
        if weight is not None:
            weight = weight.contiguous()
            if weight.dtype != torch.float32 or tuple(weight.shape) != tuple(dat_x.shape):
                raise ValueError('weight: one float32 weight per voxel of dat_x')
        if slice_w is not None:
            slice_w = slice_w.contiguous()
            if slice_w.dtype != torch.float32 or slice_w.numel() != dat_x.shape[axis]:
                raise ValueError('slice_w: one float32 weight per slice of dat_x along axis %d' % axis)
        sums = torch.empty(2 * int(dat_x.shape[axis]), dtype=_F64, device=dat_x.device)
        # (with diff the residual goes over A y in place: A y is not needed again)
        check(lib.unires_rigid_terms_e(_ptr(dat_x), _ptr(dat_yx), None if weight is None else _ptr(weight),
                                       None if slice_w is None else _ptr(slice_w), _ptr(gain), i3(dat_x.shape), axis,
                                       _ptr(sums), _ptr(dat_yx) if diff else None, _stream()))
        ll = _slice_ll(tau, slice_w, sums)
    elif weight is not None:
        dat_x, dat_yx, weight = dat_x.contiguous(), dat_yx.contiguous(), weight.contiguous()
        if weight.dtype != torch.float32 or tuple(weight.shape) != tuple(dat_x.shape):
            raise ValueError('weight: one float32 weight per voxel of dat_x')
        if slice_w is not None:
            slice_w = slice_w.contiguous()
            if slice_w.dtype != torch.float32 or slice_w.numel() != dat_x.shape[axis]:
                raise ValueError('slice_w: one float32 weight per slice of dat_x along axis %d' % axis)
        sums = torch.empty(2 * int(dat_x.shape[axis]), dtype=_F64, device=dat_x.device)
        check(lib.unires_voxel_sums(_ptr(dat_x), _ptr(dat_yx), _ptr(weight), i3(dat_x.shape), axis, _ptr(sums),
                                    _stream()))
        ll = _slice_ll(tau, slice_w, sums)
    elif slice_w is None:
        sse = torch.zeros((), dtype=_F64, device=dat_x.device)
        check(lib.unires_masked_sse(_ptr(dat_x), _ptr(dat_yx), dat_x.numel(), _ptr(sse), _stream()))
        ll = 0.5 * float(tau) * sse
    else:
        dat_x, dat_yx, slice_w = dat_x.contiguous(), dat_yx.contiguous(), slice_w.contiguous()
        if slice_w.dtype != torch.float32 or slice_w.numel() != dat_x.shape[axis]:
            raise ValueError('slice_w: one float32 weight per slice of dat_x along axis %d' % axis)
        sums = torch.empty(2 * slice_w.numel(), dtype=_F64, device=dat_x.device)
        check(lib.unires_slice_sums(_ptr(dat_x), _ptr(dat_yx), i3(dat_x.shape), axis, _ptr(sums), _stream()))
        ll = _slice_ll(tau, slice_w, sums)
    if not diff:
        return ll, None, None
    gr3 = _ops.pull_grad_affine(dat_y, M, dim).reshape(dim + (3,))
    if rician or gain is not None:
        d = dat_yx  # (written above, with the sums)
    elif weight is not None:
        d = dat_yx  # (in place: A y is not needed again)
        check(lib.unires_rigid_resid_g(_ptr(dat_x), _ptr(dat_yx), _ptr(weight), i3(dat_x.shape), axis,
                                       None if slice_w is None else _ptr(slice_w), _ptr(d), _stream()))
    elif slice_w is None:
        d = dat_yx - dat_x
        d[(dat_x == 0) | (dat_yx == 0)] = 0  # :517-519
    else:
        d = dat_yx  # (in place: A y is not needed again)
        check(lib.unires_rigid_resid(_ptr(dat_x), _ptr(dat_yx), i3(dat_x.shape), axis, _ptr(slice_w), _ptr(d),
                                     _stream()))
    if method == 'super-resolution':
        d = _ops.conv_up(d, _taps(po), po.ratio)  # no slice scaling here (:524)
    return ll, gr3, d.reshape(dim).contiguous()


@on_device
def _rigid_match(dat_x, dat_y, po, tau, rigid, sett, CtC=None, diff=False, verbose=0, slice_w=None, weight=None,
                 gain=None, rician=False):
    """Rigid matching term with the reference's return shapes (unires/_update.py:448-538):
    ll, gr (dim, 3) = grid_grad * residual, Hes (dim, 6) = outer(grid_grad) [* CtC].
    ``slice_w``: the observation's slice weights along ``po.dim_thick`` (``_rigid_terms``); ``weight``: its voxel
    weights, the shape of ``dat_x``; ``gain``: its slice gains along ``po.dim_thick``; the Hessian's weight is the
    caller's ``CtC`` (``_ctc`` with the same weights and gains).  ``rician``: ll and the residual are the Rician term's
    (``_rigid_terms``); the Hessian is what it is without - the majoriser's curvature."""
    weighted = slice_w is not None or weight is not None or gain is not None
    ll, gr3, d = _rigid_terms(dat_x, dat_y, po, tau, rigid, sett, diff=diff, slice_w=slice_w,
                              axis=_thick_axis(po) if weighted or rician else None, weight=weight, gain=gain,
                              rician=rician)
    if not diff:
        return ll, None, None
    Hes = torch.stack([gr3[..., 0] * gr3[..., 0], gr3[..., 1] * gr3[..., 1], gr3[..., 2] * gr3[..., 2],
                       gr3[..., 0] * gr3[..., 1], gr3[..., 0] * gr3[..., 2], gr3[..., 1] * gr3[..., 2]], -1)
    if sett.method == 'super-resolution' or (weighted and CtC is not None):
        Hes = Hes * CtC[..., None]
    return ll, gr3 * d[..., None], Hes


def _spread(slice_w, shape, axis):
    """The (S,) weights as a view of ``shape``: u[s(v)] at every voxel, s counted along ``axis``."""
    view = [1, 1, 1]
    view[axis] = int(shape[axis])
    return slice_w.reshape(view).expand(tuple(int(v) for v in shape))


def _voxel_times(src, weight, slice_w, axis):
    """g [u[s(v)]] src in place on ``src`` (contiguous float32, ``weight``'s shape): ``unires_voxel_apply`` without a
    mask - g u is exact in float64, g u src one rounding to float32."""
    check(_lib.load().unires_voxel_apply(_ptr(src), _ptr(src), _ptr(weight), None,
                                         None if slice_w is None else _ptr(slice_w), i3(weight.shape), axis, 0, None,
                                         _stream()))
    return src


def _gain_w_mat(slice_w, gain):
    """The Hessian's slice factor of a gained repeat: w_mat[s] = fl32(fl64(fl64(u e) e)), the table the plan's A^T A
    applies between its halves (``k_gain_compose``'s roundings: u e is exact in float64, u e e rounded there once, then
    once more to float32); u = 1 where ``slice_w`` is None."""
    ev = gain.double()
    ue = ev if slice_w is None else slice_w.double() * ev
    return (ue * ev).float().contiguous()


def _ctc(po, dim, device, slice_w=None, axis=None, weight=None, gain=None):
    """conv_transpose(conv(1)) (unires/_update.py:603-607); with slice weights conv_transpose(u . conv(1)): the
    weights applied in x space between the two halves (times 1 is exact: u = 1 gives the unweighted bits).  With voxel
    weights ``weight`` (contiguous float32, the decimated observation's shape) conv_transpose(W . conv(1)), W = g or
    g u[s(v)]: one pass and one rounding (``_voxel_times``; g = 1 gives the bits of the form above).  With slice
    gains ``gain`` the slice factor is w_mat = u e^2 in the place of u (``_gain_w_mat``): W e^2 per voxel."""
    if gain is not None:
        slice_w = _gain_w_mat(slice_w, gain)
    ones = torch.ones(dim, dtype=torch.float32, device=device)
    low = _ops.conv_down(ones, _taps(po), po.ratio)
    if weight is not None:
        low = _voxel_times(low.contiguous().reshape(tuple(weight.shape)), weight, slice_w, axis)
    elif slice_w is not None:
        low = low * _spread(slice_w, low.shape, axis)
    return _ops.conv_up(low, _taps(po), po.ratio).contiguous()


@on_device
@light_host
def _update_rigid_channel(xc, yc, sett, max_niter_gn=1, num_linesearch=4, verbose=0, samp=3, c=1):
    """Updates the rigid parameters of all images of one channel (unires/_update.py:541-710).

    A repeat with slice weights (``xn.slice_w``, a float32 device tensor as ``fit()`` leaves it) takes its step on
    the weighted data term: the objective of the step and of every line-search evaluation, the residual and the
    Hessian's weight - conv_transpose(u . conv(1)), or the volume u[s(v)] in the denoising regime - all carry the
    weights, decimated with the observation (``u[::sk[a]][:dim_x[a]]``) and built once per repeat.  A repeat whose
    weights are all zero has a zero Hessian: its ``rigid_q`` and ``po.rigid`` are left as they are and it adds 0 to
    ``sll``.  A repeat without weights runs exactly what it ran before.

    With ``sett.voxel_gn`` a repeat with voxel weights (``xn.weight``) takes its step on 1/2 tau sum_v g(v) u[s(v)]
    [x != 0] (x - A y)^2 in the same way: the map is decimated as the data are (``g[::sk[0], ::sk[1], ::sk[2]]``, cut
    to ``dim_x``), the Hessian's weight is conv_transpose(W . conv(1)) with W = g or g u[s(v)] - the volume W in the
    denoising regime - and a map that is all zero leaves the repeat alone.  Without ``sett.voxel_gn`` the map is
    ignored, as it was before the update could carry it.

    With ``sett.gain_gn`` a repeat with slice gains (``xn.slice_gain``) takes its step on 1/2 tau sum_v W [x != 0]
    (x - e[s(v)] A y)^2, W = g u (1 where the repeat has none, g only with ``sett.voxel_gn``): the gains are decimated
    with the observation as u is (``e[::sk[a]][:dim_x[a]]``); objective and residual W e (e A y - x) come from one
    pass on the gained prediction (``unires_rigid_terms_e``), and the Hessian's weight is W e^2 - the forms above with
    w_mat = fl32(fl64(fl64(u e) e)) in the place of u, built once per repeat and call.  ll and sll are the data term
    alone: the ridge of ``sett.slice_gain`` does not depend on the rigid parameters.  The all-weights-zero rule
    applies unchanged.  Without ``sett.gain_gn`` the gains are ignored, as they were before the update could carry
    them.

    With ``sett.rician_gn`` a repeat with the Rician data term (``sett.noise_model = 'rician'``, not CT) takes its step
    on sum_v W [1/2 tau (x - e A y)^2 + c(tau x e A y)], with W and e as above: the objective of the step and of every
    line-search evaluation is that term, exactly - ``_compute_nll``'s statement for the repeat - and the residual is
    W e (e A y - x R(z)), tau times which is its exact derivative; both come from one pass over the TRUE observation
    ``xn.dat`` (``unires_rigid_terms_r``; ``xn._rician_dat`` is the y-update's and is never read here).  The Hessian's
    weight ``CtC`` is exactly what the repeat would get without the Rician model, W e^2: the curvature of the quadratic
    majoriser, which bounds the term's own second derivative tau [1 - tau x^2 R'(z)] from above, so the step is a
    Gauss-Newton step on the majoriser at the current parameters, guarded by the line search on the exact term.  The
    all-weights-zero rule is unchanged.  CT repeats, the Gaussian model and the switch off run what they ran."""
    lib = _lib.load()
    dev = yc.dat.device
    method = sett.method
    basis = sett.rigid_basis
    num_q = basis.shape[0]
    sll = torch.zeros((), dtype=_F64, device=dev)
    sums = torch.empty(27, dtype=_F64, device=dev)
    iu = np.triu_indices(num_q)
    for n_x in range(len(xc)):
        xn = xc[n_x]
        if xn.rigid_q is None:
            xn.rigid_q = _logq(xn.po.rigid, basis)
        q = torch.as_tensor(xn.rigid_q, dtype=_F64).cpu().clone()
        tau = float(xn.tau)
        armijo = 1.0
        po = _proj_info(xn.po.dim_y, xn.po.mat_y, xn.po.dim_x, xn.po.mat_x, rigid=xn.po.rigid,
                        prof_ip=sett.profile_ip, prof_tp=sett.profile_tp, gap=sett.gap,
                        device=dev, scl=xn.po.scl, samp=samp)
        mat = po.mat_yx if method == 'super-resolution' else po.mat_x
        dim = tuple(po.dim_yx) if method == 'super-resolution' else tuple(po.dim_x)
        # nearest-neighbour resample of the data onto the decimated lattice (unires/_update.py:589-593:
        # grid_pull at the integer coordinates D_x u, interpolation 0) = a strided slice
        sk = getattr(po, 'sk', (1, 1, 1))
        dat_x = xn.dat[::sk[0], ::sk[1], ::sk[2]][:po.dim_x[0], :po.dim_x[1], :po.dim_x[2]].contiguous()
        dat_y = yc.dat
        u = getattr(xn, 'slice_w', None)
        g = _gn_weight(xn, sett)
        a = _slice_axis(xn)
        e = _gn_gain(xn, sett)
        rc = bool(getattr(sett, 'rician_gn', False)) and _is_rician(xn, sett)  # (the Rician term: objective and residual)
        if u is not None:
            u = u[::sk[a]][:po.dim_x[a]].contiguous()
        uh = u  # (the Hessian's slice factor: u, or w_mat = u e^2 for a gained repeat, once per repeat and call)
        if e is not None:
            e = e[::sk[a]][:po.dim_x[a]].contiguous()
            uh = _gain_w_mat(u, e)
        if g is not None:
            # (the map decimated as the data are; the Hessian's weight W = g [u] once per repeat and call)
            g = g[::sk[0], ::sk[1], ::sk[2]][:po.dim_x[0], :po.dim_x[1], :po.dim_x[2]].contiguous()
            if method == 'super-resolution':
                CtC = _ctc(po, dim, dev, uh, a, weight=g)
            else:
                CtC = g if uh is None else _voxel_times(torch.ones_like(g), g, uh, a)
        elif uh is None:
            CtC = _ctc(po, dim, dev) if method == 'super-resolution' else None
        else:
            CtC = _ctc(po, dim, dev, uh, a) if method == 'super-resolution' else _spread(uh, dat_x.shape, a).contiguous()
        empty = False
        ll = torch.zeros((), dtype=_F64, device=dev)
        rigid = _expm(q, basis)
        for _gn in range(max_niter_gn):
            rigid, d_rigid = _expm(q, basis, grad_X=True)
            D = torch.stack([torch.linalg.solve(po.mat_y, d_rigid[i].mm(mat)) for i in range(num_q)])
            ll, gr3, dg = _rigid_terms(dat_x, dat_y, po, tau, rigid, sett, diff=True, slice_w=u, axis=a, weight=g,
                                       gain=e, rician=rc)
            d72 = (C.c_float * 72)(*D[:, :3, :].reshape(-1).float().tolist())
            check(lib.unires_rigid_sums(_ptr(gr3), _ptr(dg), _ptr(CtC) if CtC is not None else None,
                                        i3(dim), d72, _ptr(sums), _stream()))
            s = sums.cpu().numpy()  # (6x6 host algebra in numpy: torch's CPU ops cost ~10 ms each here)
            Hes = np.zeros((num_q, num_q))
            Hes[iu] = s[num_q:]
            Hes = Hes + np.triu(Hes, 1).T
            if (u is not None or g is not None or e is not None) and not Hes.any():  # (all weights zero: no data term, no step - nothing to solve)
                empty = True
                break
            Update = torch.from_numpy(np.linalg.solve(Hes, s[:num_q]))
            old_ll, old_q, old_rigid = ll.clone(), q.clone(), rigid.clone()
            if num_linesearch == 0:
                q = old_q - armijo * Update
                rigid = _expm(q, basis)
            else:
                for n_ls in range(num_linesearch):
                    q = old_q - armijo * Update
                    rigid = _expm(q, basis)
                    ll = _rigid_terms(dat_x, dat_y, po, tau, rigid, sett, slice_w=u, axis=a, weight=g, gain=e,
                                      rician=rc)[0]
                    if bool(ll < old_ll):
                        armijo = min(1.25 * armijo, 1.0)
                        if verbose >= 1:
                            print('c={}, n={}, ls={} | :) ll={:0.2f} | q={}'.format(
                                c, n_x, n_ls, float(ll), [round(v, 7) for v in q.tolist()]))
                        break
                    ll, q, rigid = old_ll, old_q, old_rigid
                    armijo *= 0.5
        if empty:
            continue
        xn.rigid_q = q
        xn.po.rigid = rigid
        sll = sll + ll
    return xc, sll


@on_device
@light_host
def _update_rigid(x, y, sett, mean_correct=True, max_niter_gn=1, num_linesearch=4, verbose=0, samp=3):
    """Updates each input image's registration parameters x[c][n].rigid_q by Gauss-Newton and
    refreshes x[c][n].po.rigid (unires/_update.py:198-266).  Returns (x, sll)."""
    if getattr(sett, 'rigid_basis', None) is None:
        sett.rigid_basis = affine_basis('SE')
    dev = y[0].dat.device
    sll = torch.zeros((), dtype=_F64, device=dev)
    for c in range(len(x)):
        x[c], sllc = _update_rigid_channel(x[c], y[c], sett, max_niter_gn=max_niter_gn,
                                           num_linesearch=num_linesearch, verbose=verbose,
                                           samp=samp, c=c)
        sll = sll + sllc
    if mean_correct:
        qs = [xn.rigid_q for xc in x for xn in xc]
        mean_q = torch.stack(qs).sum(0) / float(len(qs))
        for xc in x:
            for xn in xc:
                xn.rigid_q = xn.rigid_q - mean_q
                xn.po.rigid = _expm(xn.rigid_q, sett.rigid_basis)
    return x, sll
