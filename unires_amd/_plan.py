"""ChannelPlan - Python handle of ``unires_plan_t``: the per-channel operator
``sum_n tau_n A_n^T A_n + rho lam^2 D^T D`` with all its device workspace."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import (REGIME_DENOISE, REGIME_IDENTITY, REGIME_SUPERRES, Repeat, check, f3, i3)
from ._ops import FOV_TOL, _ptr, _stream, _vol, on_device
from .spatial import _m12, voxel_size


def proj_matrix(po, method):
    """float64 mat_y \\ (rigid @ mat_yx | mat_x) and the grid dims
    (unires/_project.py:145-150)."""
    if method == 'super-resolution':
        return torch.linalg.solve(po.mat_y, po.rigid.mm(po.mat_yx)), tuple(po.dim_yx)
    if method == 'denoising':
        return torch.linalg.solve(po.mat_y, po.rigid.mm(po.mat_x)), tuple(po.dim_x)
    raise ValueError('Undefined method')


def regime_of(method, do_proj):
    if method not in ('denoising', 'super-resolution'):
        raise ValueError('Undefined method')
    if not do_proj:
        return REGIME_IDENTITY
    return REGIME_SUPERRES if method == 'super-resolution' else REGIME_DENOISE


def _repeat_desc(po, tau, method, regime, keep):
    r = Repeat()
    r.tau = float(tau)
    if regime == REGIME_IDENTITY:
        return r
    mat, dim_g = proj_matrix(po, method)
    r.dim_x = i3(po.dim_x)
    r.dim_g = i3(dim_g)
    r.M = _lib.c_f32x12(*_m12(mat).tolist())
    if regime == REGIME_SUPERRES:
        taps = [np.ascontiguousarray(np.asarray(k, dtype=np.float32)) for k in po.smo_ker_1d]
        keep.extend(taps)
        r.ratio = i3(po.ratio)
        r.ntaps = i3([len(k) for k in taps])
        r.taps = _lib.c_fptrx3(*[k.ctypes.data_as(C.POINTER(C.c_float)) for k in taps])
        r.scl = float(po.scl)
        r.dim_thick = int(po.dim_thick)
    else:
        r.ratio = i3((1, 1, 1))
        r.ntaps = i3((1, 1, 1))
    return r


class ChannelPlan:
    """One channel's fused operator. ``xs``: list of (po, tau) per repeat."""

    def __init__(self, dim_y, vx_y, repeats, method, do_proj, fov_tol=FOV_TOL, device=None, diff='forward'):
        _lib.diff_code(diff, 'diff')
        self.lib = _lib.load()
        # the plan's workspace lives on ONE device: the one current when it is created
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self._create(dim_y, vx_y, repeats, method, do_proj, fov_tol)
        self.set_diff(diff)

    def _create(self, dim_y, vx_y, repeats, method, do_proj, fov_tol):
        self.dim_y = tuple(int(d) for d in dim_y)
        self.regime = regime_of(method, do_proj)
        self.method = method
        self.n_repeats = len(repeats)
        keep = []
        arr = (Repeat * len(repeats))(*[_repeat_desc(po, tau, method, self.regime, keep)
                                       for po, tau in repeats])
        self._h = C.c_void_p()
        self._concurrency = 1
        self.diff = 'forward'
        self._missing = [None] * len(repeats)  # per repeat: (weak reference, version) of the tensor its mask was built from, or None
        self.mask_zeros = False  # the setting the plan was last fetched with (_project._channel_plan)
        self._slice_w = [None] * len(repeats)  # per repeat: (weak reference, version, axis) of the weight tensor the plan holds, or None
        self.weights = False  # whether the plan was last fetched with the observations' slice weights (_channel_plan)
        self._voxel_w = [None] * len(repeats)  # per repeat: (weak reference, version) of the voxel-weight tensor the plan holds, or None
        self._slice_e = [None] * len(repeats)  # per repeat: (weak reference, version, axis) of the gain tensor the plan holds, or None
        check(self.lib.unires_plan_create(C.byref(self._h), i3(self.dim_y), f3(vx_y), self.regime,
                                          len(repeats), arr, fov_tol))
        self.dims_x = [self.dim_y if self.regime == REGIME_IDENTITY else tuple(po.dim_x)
                       for po, _ in repeats]

    def rhs_buffer(self, like):
        """A per-plan (X,Y,Z) buffer for the RHS when channels run on separate streams."""
        buf = getattr(self, '_rhs_buf', None)
        if buf is None or buf.shape != like.shape or buf.device != like.device:
            buf = torch.empty_like(like)
            self._rhs_buf = buf
        return buf

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            try:
                with torch.cuda.device(self.device):
                    self.lib.unires_plan_destroy(self._h)
            except Exception:  # interpreter shutdown
                self.lib.unires_plan_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def workspace_bytes(self):
        return int(self.lib.unires_plan_workspace_bytes(self._h))

    def repeat_info(self, n):
        """Which kernels repeat n runs on and how its voxel axes were relabelled
        (``unires_plan_repeat_info``): dict(perm, flip, pull2, splat2_axis, shift, separable, fused, masked, weighted,
        voxel_weighted);
        ``fused``: the single-pass AtA kernel (denoising regime, ata1.hip) serves the CG matvec; ``masked``: the
        repeat has a validity mask (:meth:`set_missing`), ``weighted``: per-slice weights
        (:meth:`set_slice_weights`), ``voxel_weighted``: per-voxel weights (:meth:`set_voxel_weights`), ``gained``:
        per-slice gains (:meth:`set_slice_gains`) - ``shift`` and ``fused`` are then False."""
        info = (C.c_int32 * 8)()
        check(self.lib.unires_plan_repeat_info(self._h, int(n), info))
        v = list(info)
        return dict(perm=tuple(v[:3]), flip=tuple((v[3] >> j) & 1 for j in range(3)), pull2=bool(v[4]),
                    splat2_axis=None if v[5] == 0 else v[5] - 2, shift=bool(v[6] & 1), separable=bool(v[7]),
                    fused=bool(v[6] & 2), masked=bool(v[6] & 4), weighted=bool(v[6] & 8),
                    voxel_weighted=bool(v[6] & 16), gained=bool(v[6] & 32))

    @on_device
    def time_matvecs(self, on=True):
        """Measurement aid: bracket every operator application of the following solves with HIP events
        (the solves then run as plain launches, not as a hipGraph).  ``on=2``: no events - every A(p) is enqueued
        twice instead, inside the solve's hipGraph (same result; the time difference to a plain solve is the cost of
        the operator applications as production runs them)."""
        check(self.lib.unires_plan_time_matvecs(self._h, 2 if on == 2 else (1 if on else 0)))

    def cg_ring(self, k=0):
        """Deferred iterate update of tol = 0 solves (``unires_plan_cg_ring``): ``k > 0`` asks for a ring of k
        directions (1: x updated every iteration); returns the ring size the plan's last solve ran with."""
        last = C.c_int32(0)
        check(self.lib.unires_plan_cg_ring(self._h, int(k), C.byref(last)))
        return int(last.value)

    @property
    def cg_lockstep(self):
        """Whether the plan's last solve ran inside the channels' two-lane schedule (``unires_plan_cg_lockstep``)."""
        return bool(self.lib.unires_plan_cg_lockstep(self._h))

    @on_device
    def matvec_time(self):
        """(launches, total microseconds) recorded since the last call; waits for them."""
        n, us = C.c_int32(0), C.c_double(0.0)
        check(self.lib.unires_plan_matvec_time(self._h, C.byref(n), C.byref(us)))
        return int(n.value), float(us.value)

    @on_device
    def set_repeat(self, n, po, tau):
        keep = []
        r = _repeat_desc(po, tau, self.method, self.regime, keep)
        check(self.lib.unires_plan_set_repeat(self._h, n, C.byref(r)))

    @on_device
    def set_missing(self, n, dat):
        """Voxels of repeat n's observation ``dat`` that are exactly 0 are missing data (``unires_plan_set_missing``):
        the plan's AtA_n becomes A_n^T diag(dat != 0) A_n in the matvec, the CG solves and the preconditioners; A, At
        and the right-hand side are unchanged.  ``dat=None`` clears the mask.  Call again when the values of the
        observation change; a change drops the captured solve and the built preconditioner."""
        import weakref
        self._missing[n] = None
        if dat is None:
            check(self.lib.unires_plan_set_missing(self._h, int(n), None, _stream()))
            return
        d = _vol(dat, 'x')[0]
        if tuple(d.shape) != tuple(self.dims_x[n]):
            raise ValueError('unires_amd: observation shape mismatch')
        check(self.lib.unires_plan_set_missing(self._h, int(n), _ptr(d), _stream()))
        self._missing[n] = (weakref.ref(dat), dat._version)

    def sync_missing(self, x_dats):
        """:meth:`set_missing` for every repeat whose observation is not the tensor, at the version, its mask was
        built from (the key of :meth:`rhs_cached`: the tensor OBJECT and its version counter); ``x_dats=None``
        clears every mask.  Free when nothing changed.  The masks are built on the current stream: a caller that
        uses the plan on another stream orders that stream after this call (``_update_y`` fetches its plans before it
        records the event its channel streams wait for)."""
        for n in range(self.n_repeats):
            if x_dats is None:
                if self._missing[n] is not None:
                    self.set_missing(n, None)
                continue
            t, key = x_dats[n], self._missing[n]
            if key is not None and key[0]() is t and key[1] == t._version:
                continue
            self.set_missing(n, t)

    @on_device
    def set_slice_weights(self, n, axis, w):
        """Per-slice weights of repeat n's data term (``unires_plan_set_slice_weights``): ``w`` a float32 device tensor
        with one weight >= 0 per slice along the caller's voxel axis ``axis`` (not checked here: ``fit`` validates the
        user's once).  The plan's AtA_n becomes A_n^T diag(w) A_n - on top of a mask, where the repeat has one - in
        the matvec, the CG solves and the preconditioners, and its right-hand side term A_n^T (w . x_n); A and At of
        :meth:`proj_apply` stay unweighted.  ``w=None`` clears.  The plan keeps a copy: call again when the values
        change (that rebuilds nothing, a captured solve reads the new values; a first set or a clear changes the
        repeat's kernels)."""
        import weakref
        n, axis = int(n), int(axis)
        if not 0 <= n < self.n_repeats:
            raise ValueError('unires_amd: repeat index out of range')
        if axis not in (0, 1, 2):
            raise ValueError('unires_amd: slice axis must be 0, 1 or 2')
        if w is not None and (not w.is_cuda or w.dtype != torch.float32
                              or tuple(w.shape) != (int(self.dims_x[n][axis]),)):
            raise ValueError('unires_amd: slice weights must be a float32 device tensor of shape (%d,)'
                             % int(self.dims_x[n][axis]))
        self._slice_w[n] = None
        self._atx = None  # (sum tau At (w . x) follows the weights)
        if w is None:
            check(self.lib.unires_plan_set_slice_weights(self._h, n, axis, None, _stream()))
            return
        wc = w.contiguous()
        check(self.lib.unires_plan_set_slice_weights(self._h, int(n), axis, _ptr(wc), _stream()))
        self._slice_w[n] = (weakref.ref(w), w._version, axis)

    def sync_slice_weights(self, ws):
        """:meth:`set_slice_weights` for every repeat whose weights are not the tensor, at the version and axis, the
        plan holds (``ws``: per repeat ``(axis, tensor)`` or None for an unweighted repeat; ``ws=None``: clear all).
        Free when nothing changed.  Runs on the current stream, like :meth:`sync_missing`: ``_update_y`` fetches its
        plans before it records the event its channel streams wait for."""
        for n in range(self.n_repeats):
            want = None if ws is None else ws[n]
            key = self._slice_w[n]
            if want is None:
                if key is not None:
                    self.set_slice_weights(n, key[2], None)
                continue
            axis, t = want
            if key is not None and key[0]() is t and key[1] == t._version and key[2] == int(axis):
                continue
            self.set_slice_weights(n, axis, t)

    def _slice_key(self):
        """The weights' part of :meth:`rhs_cached`'s key: (object, version) per repeat, slice weights, then voxel
        weights, then slice gains."""
        return (tuple(None if k is None else (id(k[0]()), k[1]) for k in self._slice_w),
                tuple(None if k is None else (id(k[0]()), k[1]) for k in self._voxel_w),
                tuple(None if k is None else (id(k[0]()), k[1]) for k in self._slice_e))

    @on_device
    def set_slice_gains(self, n, axis, e):
        """Per-slice intensity gains of repeat n's data term (``unires_plan_set_slice_gains``): ``e`` a float32 device
        tensor with one gain > 0 per slice along the caller's voxel axis ``axis`` (not checked here: ``fit`` validates
        the user's once).  The observation is modelled as e . (A_n y): the plan's AtA_n becomes A_n^T diag(W e^2) A_n
        and its right-hand side term A_n^T (W e . x_n), W the repeat's weights and mask; A and At of
        :meth:`proj_apply` stay without gains.  ``e=None`` clears.  The plan keeps a copy: call again when the values
        change (that rebuilds nothing, a captured solve reads the new values; a first set or a clear changes the
        repeat's kernels).  The axis is the one the repeat's slice weights run along, where it has some."""
        import weakref
        n, axis = int(n), int(axis)
        if not 0 <= n < self.n_repeats:
            raise ValueError('unires_amd: repeat index out of range')
        if axis not in (0, 1, 2):
            raise ValueError('unires_amd: slice axis must be 0, 1 or 2')
        if e is not None and (not e.is_cuda or e.dtype != torch.float32
                              or tuple(e.shape) != (int(self.dims_x[n][axis]),)):
            raise ValueError('unires_amd: slice gains must be a float32 device tensor of shape (%d,)'
                             % int(self.dims_x[n][axis]))
        self._slice_e[n] = None
        self._atx = None  # (sum tau At (w e . x) follows the gains)
        if e is None:
            check(self.lib.unires_plan_set_slice_gains(self._h, n, axis, None, _stream()))
            return
        ec = e.contiguous()
        check(self.lib.unires_plan_set_slice_gains(self._h, n, axis, _ptr(ec), _stream()))
        self._slice_e[n] = (weakref.ref(e), e._version, axis)

    def sync_slice_gains(self, es):
        """:meth:`set_slice_gains` for every repeat whose gains are not the tensor, at the version and axis, the plan
        holds (``es``: per repeat ``(axis, tensor)`` or None for a repeat without gains; ``es=None``: clear all).  Free
        when nothing changed.  Runs on the current stream, like :meth:`sync_slice_weights`."""
        for n in range(self.n_repeats):
            want = None if es is None else es[n]
            key = self._slice_e[n]
            if want is None:
                if key is not None:
                    self.set_slice_gains(n, key[2], None)
                continue
            axis, t = want
            if key is not None and key[0]() is t and key[1] == t._version and key[2] == int(axis):
                continue
            self.set_slice_gains(n, axis, t)

    @on_device
    def set_voxel_weights(self, n, g):
        """Per-voxel weights of repeat n's data term (``unires_plan_set_voxel_weights``): ``g`` a float32 device tensor
        of the observation's shape with weights >= 0 (not checked here: ``fit`` validates the user's once).  The
        plan's AtA_n becomes A_n^T diag(g) A_n - on top of a mask and slice weights, where the repeat has them, in
        one pass - in the matvec, the CG solves and the preconditioners, and its right-hand side term A_n^T (g . x_n);
        A and At of :meth:`proj_apply` stay unweighted.  ``g=None`` clears.  The plan keeps a copy: call again when
        the values change (that rebuilds nothing, a captured solve reads the new values; a first set or a clear
        changes the repeat's kernels)."""
        import weakref
        n = int(n)
        if not 0 <= n < self.n_repeats:
            raise ValueError('unires_amd: repeat index out of range')
        if g is not None and (not g.is_cuda or g.dtype != torch.float32
                              or tuple(g.shape) != tuple(int(d) for d in self.dims_x[n])):
            raise ValueError('unires_amd: voxel weights must be a float32 device tensor of shape %s'
                             % (tuple(int(d) for d in self.dims_x[n]),))
        self._voxel_w[n] = None
        self._atx = None  # (sum tau At (g . x) follows the weights)
        if g is None:
            check(self.lib.unires_plan_set_voxel_weights(self._h, n, None, _stream()))
            return
        gc = g.contiguous()
        check(self.lib.unires_plan_set_voxel_weights(self._h, n, _ptr(gc), _stream()))
        self._voxel_w[n] = (weakref.ref(g), g._version)

    def sync_voxel_weights(self, gs):
        """:meth:`set_voxel_weights` for every repeat whose weights are not the tensor, at the version, the plan holds
        (``gs``: per repeat a tensor or None for a repeat without voxel weights; ``gs=None``: clear all).  Free when
        nothing changed.  Runs on the current stream, like :meth:`sync_slice_weights`."""
        for n in range(self.n_repeats):
            t = None if gs is None else gs[n]
            key = self._voxel_w[n]
            if t is None:
                if key is not None:
                    self.set_voxel_weights(n, None)
                continue
            if key is not None and key[0]() is t and key[1] == t._version:
                continue
            self.set_voxel_weights(n, t)

    def set_concurrency(self, n):
        """Tell the plan that ``n`` solves run on the device at once (the channels of a y-update on streams of their
        own): its persistent kernels then leave room for the others' (``unires_plan_set_concurrency``).  Free when
        ``n`` is what the plan already has."""
        n = max(1, int(n))
        if n != self._concurrency:
            check(self.lib.unires_plan_set_concurrency(self._h, n))
            self._concurrency = n

    def set_diff(self, diff):
        """The difference of the plan's D: 'forward' (a new plan's) | 'backward' | 'central' (``unires_plan_set_diff``):
        the matvec, the right-hand side and the FFT preconditioner follow it.  Free when it is what the plan has;
        a change drops the captured solve and the built preconditioner."""
        code = _lib.diff_code(diff, 'diff')
        if diff != self.diff:
            with torch.cuda.device(self.device):
                check(self.lib.unires_plan_set_diff(self._h, code))
            self.diff = diff

    def _y(self, t, name):
        v, _ = _vol(t, name)
        if tuple(v.shape) != self.dim_y:
            raise ValueError('unires_amd: %s has shape %s, expected %s'
                             % (name, tuple(v.shape), self.dim_y))
        return v

    @on_device
    def proj_apply(self, n, operator, dat):
        """_proj_apply(operator, dat, po_n) without tau."""
        if operator not in _lib.OP:
            raise ValueError('Undefined operator')
        d, lead = _vol(dat)
        out_dim = self.dims_x[n] if operator == 'A' else self.dim_y
        in_dim = self.dims_x[n] if operator == 'At' else self.dim_y
        if tuple(d.shape) != tuple(in_dim):
            raise ValueError('unires_amd: input has shape %s, expected %s'
                             % (tuple(d.shape), tuple(in_dim)))
        out = torch.empty(out_dim, dtype=torch.float32, device=d.device)
        check(self.lib.unires_proj_apply(self._h, n, _lib.OP[operator], _ptr(d), _ptr(out),
                                         _stream()))
        return out.reshape(lead + tuple(out_dim))

    @on_device
    def matvec(self, p, rho, lam, out=None, dot=None):
        """q = sum tau AtA p + rho lam^2 DtD p; ``dot``: 0-d float64 device tensor or None."""
        p = self._y(p, 'p')
        if out is None:
            out = torch.empty_like(p)
        check(self.lib.unires_ata_matvec(self._h, float(rho), float(lam), _ptr(p), _ptr(out),
                                         _ptr(dot) if dot is not None else None, _stream()))
        return out

    @on_device
    def rhs(self, x_dats, w_c, z_c, rho, lam, out=None):
        """b = sum tau At x - lam Dt(w - rho z)   (unires/_update.py:124-133)."""
        xs = [_vol(t, 'x')[0] for t in x_dats]
        for t, dx in zip(xs, self.dims_x):
            if tuple(t.shape) != tuple(dx):
                raise ValueError('unires_amd: observation shape mismatch')
        if len(xs) != self.n_repeats:
            raise ValueError('unires_amd: need one observation per repeat')
        for t in (w_c, z_c):
            if tuple(t.shape) != (3,) + self.dim_y or not t.is_cuda or t.dtype != torch.float32:
                raise ValueError('unires_amd: w/z must be (3,X,Y,Z) float32 device tensors')
        w_c, z_c = w_c.contiguous(), z_c.contiguous()
        if out is None:
            out = torch.empty(self.dim_y, dtype=torch.float32, device=w_c.device)
        ptrs = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
        check(self.lib.unires_rhs_assemble(self._h, ptrs, _ptr(w_c), _ptr(z_c), float(rho),
                                           float(lam), _ptr(out), _stream()))
        return out

    @on_device
    def rhs_cached(self, x_dats, w_c, z_c, rho, lam, out):
        """Same b as :meth:`rhs`, but sum_n tau_n At x_n is kept on the plan and only
        recomputed when an observation tensor or a repeat's slice weights changed (the plan itself
        is rebuilt when a rigid / scaling / tau changes).  The reference recomputes it every ADMM iteration
        (unires/_update.py:125-128)."""
        xs = [_vol(t, 'x')[0] for t in x_dats]
        # The cache is keyed on the caller's tensor OBJECTS (weak references) and their version
        # counters - not on addresses: a new tensor can land on a freed tensor's address with version
        # 0.  An observation that had to be copied to become contiguous is never cached.
        import weakref
        copied = any(v is not t and v.data_ptr() != t.data_ptr() for v, t in zip(xs, x_dats))
        key = None if copied else (tuple((id(t), t._version) for t in x_dats), self._slice_key())
        cache = getattr(self, '_atx', None)
        alive = cache is not None and all(r() is t for r, t in zip(cache[2], x_dats)) \
            and len(cache[2]) == len(x_dats)
        if cache is None or key is None or not alive or cache[0] != key:
            atx = cache[1] if cache is not None else torch.empty(self.dim_y, dtype=torch.float32,
                                                                 device=xs[0].device)
            ptrs = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
            check(self.lib.unires_atx_assemble(self._h, ptrs, _ptr(atx), _stream()))
            refs = [] if key is None else [weakref.ref(t) for t in x_dats]
            self._atx = cache = (key, atx, refs)
        w_c, z_c = w_c.contiguous(), z_c.contiguous()
        check(self.lib.unires_rhs_from_atx(self._h, _ptr(cache[1]), _ptr(w_c), _ptr(z_c),
                                           float(rho), float(lam), _ptr(out), _stream()))
        return out

    @on_device
    def precond_build(self, rho, lam, mode='jacobi', out=None):
        """Diagonal of unires/_update.py:80-102 for this channel, kept in the plan for
        ``cg(precond='jacobi')``; ``out`` (dim_y tensor) optionally receives a copy."""
        if mode not in _lib.PRECOND:
            raise ValueError('Undefined preconditioner')
        if out is not None:
            out = self._y(out, 'out')
        check(self.lib.unires_precond_build(self._h, _lib.PRECOND[mode], float(rho), float(lam),
                                            _ptr(out) if out is not None else None, _stream()))
        return out

    @on_device
    def precond_apply(self, v, out=None):
        """out = precond(v) for the preconditioner last built on this plan (identity: copy)."""
        v = self._y(v, 'v')
        if out is None:
            out = torch.empty_like(v)
        check(self.lib.unires_precond_apply(self._h, _ptr(v), _ptr(out), _stream()))
        return out

    @on_device
    def cg(self, b, x, rho, lam, max_iter=20, tolerance=1e-3, stop='max_gain', sync=True,
           precond='none'):
        """In-place CG on x (must be contiguous (X,Y,Z)).  Returns (iters, obj) when
        ``sync`` (one stream sync), else None with everything left enqueued.
        ``precond='jacobi' | 'fft'`` needs :meth:`precond_build` with the same mode, rho, lam first.
        With a tolerance the call keeps the calling thread until the last chunk of iterations is enqueued
        (``sync=False`` does not return early then); on a capturing stream the whole solve joins the capture."""
        if precond not in _lib.PRECOND:
            raise ValueError('Undefined preconditioner')
        pm = _lib.PRECOND[precond]
        b = self._y(b, 'b')
        if not x.is_contiguous():
            raise ValueError('unires_amd: cg updates x in place and needs it contiguous')
        self._y(x, 'x')
        s = stop if stop in _lib.STOP else stop[0].lower()
        mode = _lib.STOP[s] if s in _lib.STOP else (0 if s == 'e' else 3)
        max_iter = int(max_iter)
        if sync:
            it = C.c_int32(0)
            obj = (C.c_double * (min(max_iter, 4096) + 1))()
            check(self.lib.unires_cg_solve(self._h, float(rho), float(lam), _ptr(b), _ptr(x),
                                           int(max_iter), float(tolerance), mode, pm, C.byref(it),
                                           obj, _stream()))
            trace = _trace(list(obj), it.value) if tolerance else None
            return it.value, trace
        check(self.lib.unires_cg_solve(self._h, float(rho), float(lam), _ptr(b), _ptr(x),
                                       int(max_iter), float(tolerance), mode, pm, None, None,
                                       _stream()))
        return None


def _trace(ring, it):
    """Objective trace of a solve that realised ``it`` iterations from the library's ring of ``len(ring)``
    slots (iteration k lives in slot k mod len): all it + 1 values while they fit, else the LAST len(ring) of
    them, oldest first (budgets beyond 4 096 iterations, `optim.cg(max_iter=None)`)."""
    n = len(ring)
    if it < n:
        return ring[:it + 1]
    start = (it + 1) % n
    return ring[start:] + ring[:start]


def cg_many(plans, bs, xs, rho, lams, streams, max_iter=20, tolerance=1e-3, stop='max_gain', precond='none',
            sync=False):
    """The solves of several channels at once, channel c on ``streams[c]`` (``unires_cg_solve_many``): with
    a tolerance the library feeds every solve chunk by chunk from one host loop, so the channels keep
    overlapping on the device.  Returns [(iters, obj), ...] when ``sync``."""
    if precond not in _lib.PRECOND:
        raise ValueError('Undefined preconditioner')
    n = len(plans)
    lib = plans[0].lib
    s = stop if stop in _lib.STOP else stop[0].lower()
    mode = _lib.STOP[s] if s in _lib.STOP else (0 if s == 'e' else 3)
    for pl, b, x in zip(plans, bs, xs):
        pl._y(b, 'b')
        if not x.is_contiguous():
            raise ValueError('unires_amd: cg updates x in place and needs it contiguous')
        pl._y(x, 'x')
    max_iter = int(max_iter)
    nobj = min(max_iter, 4096) + 1
    it = (C.c_int32 * n)() if sync else None
    obj = (C.c_double * (n * nobj))() if sync else None
    with torch.cuda.device(plans[0].device):
        check(lib.unires_cg_solve_many(
            n, (C.c_void_p * n)(*[pl._h.value for pl in plans]), (C.c_float * n)(*[float(rho)] * n),
            (C.c_float * n)(*[float(v) for v in lams]), (C.c_void_p * n)(*[b.data_ptr() for b in bs]),
            (C.c_void_p * n)(*[x.data_ptr() for x in xs]), max_iter, float(tolerance), mode,
            _lib.PRECOND[precond], it, obj, (C.c_void_p * n)(*[st.cuda_stream for st in streams])))
    if not sync:
        return None
    return [(it[c], _trace(list(obj[c * nobj:(c + 1) * nobj]), it[c]) if tolerance else None) for c in range(n)]
