"""Rigid coregistration of observations - the counterpart of nitorch's ``affine_align`` as the
reference's ``_init_reg`` calls it (unires/_core.py:310-368), on the estimator DESIGN 8.2 states:
SPM's ``spm_coreg`` scheme restated.  Every observation is quantised to uint8, each one is aligned
pairwise to the fixed observation by a Powell search over se(3) that minimises a histogram cost
(normalised mutual information by default).

The voxel work is HIP (``coreg.hip``): one launch quantises every observation, and each step of
the search evaluates one cost per pair that is still searching with one histogram launch, one cost
launch and one read-back.  The optimiser is float64 host code: one generator per pair, driven in
lockstep."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, _ops
from ._lib import check
from ._ops import _stream, on_device
from ._rigid import _expm, affine_basis
from .spatial import _m12, voxel_size

BINS = 256
QBINS = 1024
QOUT = 8
MN, MAX, MX, SCALE, STATUS = 0, 1, 2, 3, 4  # columns of unires_coreg_quantise's params rows
COST_FUNS = {'nmi': 0, 'mi': 1, 'ecc': 2}
JITTER = 97
PHI = 0.6180339887498949
# Powell: initial directions (3 translations in mm, 3 rotations in rad) and line tolerances
STEP = np.array([0.4, 0.4, 0.4, 0.02, 0.02, 0.02])
TOL = np.array([0.02, 0.02, 0.02, 0.001, 0.001, 0.001])
MAX_SWEEPS = 32
FTOL = 1e-7


def jitter_table():
    """The sampling jitter: T[k] = frac((k + 1) * 0.6180339887498949) in float64, as float32."""
    x = np.arange(1, JITTER + 1, dtype=np.float64) * PHI
    return (x % 1.0).astype(np.float32)


class Job(C.Structure):
    """``unires_coreg_job_t``."""
    _fields_ = [('G', C.c_void_p), ('F', C.c_void_p), ('dim_g', _lib.c_i32x3), ('dim_f', _lib.c_i32x3),
                ('M', _lib.c_f32x12), ('step', _lib.c_f32x3)]


def _vol(dat, name='dat'):
    if not isinstance(dat, torch.Tensor) or not dat.is_cuda:
        raise RuntimeError('unires_amd: %s must be a CUDA/HIP tensor (no CPU path)' % name)
    if dat.dim() != 3:
        raise ValueError('unires_amd: %s must be (X, Y, Z)' % name)
    return dat.contiguous()


@on_device
def coreg_quantise(dats):
    """uint8 copies of float32 volumes, one launch for all (DESIGN 8.2 rule 1).  Returns
    ``(vols, counts, params)``: the uint8 volumes, the (N, 1024) int32 histograms of the finite
    voxels over [min, max] and the (N, 8) float32 rows (min, max, robust max, scale, status, ...),
    all on the device.  Raises ValueError for a volume with no finite voxel or a constant one."""
    vols = [_vol(d) for d in dats]
    if any(v.dtype != torch.float32 for v in vols):
        raise TypeError('unires_amd: coreg_quantise takes float32 volumes')
    n = len(vols)
    dev = vols[0].device
    outs = [torch.empty(v.shape, dtype=torch.uint8, device=dev) for v in vols]
    counts = torch.empty((n, QBINS), dtype=torch.int32, device=dev)
    params = torch.empty((n, QOUT), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * n)(*[v.data_ptr() for v in vols])
    sizes = (C.c_int64 * n)(*[v.numel() for v in vols])
    optrs = (C.c_void_p * n)(*[u.data_ptr() for u in outs])
    check(_lib.load().unires_coreg_quantise(n, ptrs, sizes, optrs, C.c_void_p(counts.data_ptr()),
                                            C.c_void_p(params.data_ptr()), _stream()))
    status = params[:, STATUS].cpu()
    for i, s in enumerate(status.tolist()):
        if s == 1:
            raise ValueError('coreg: observation %d has no finite voxel' % i)
        if s == 2:
            raise ValueError('coreg: observation %d is constant' % i)
    return outs, counts, params


def _job(G, F, M, step):
    j = Job()
    j.G, j.F = G.data_ptr(), F.data_ptr()
    j.dim_g = _lib.c_i32x3(*G.shape)
    j.dim_f = _lib.c_i32x3(*F.shape)
    j.M = _lib.c_f32x12(*[float(v) for v in np.asarray(M, dtype=np.float32).reshape(-1)])
    j.step = _lib.c_f32x3(*[float(v) for v in np.asarray(step, dtype=np.float32)])
    return j


@on_device
def coreg_hist(jobs):
    """Joint histograms of ``jobs``, a list of ``(G, F, M, step)``: uint8 device volumes, the
    float32 3x4 (12,) map from G voxels to F voxels and the sampling step in G voxels.  One launch
    -> (N, 256, 256) int64 device counts in Q16 units (DESIGN 8.2 rule 2)."""
    n = len(jobs)
    for G, F, _, _ in jobs:
        for v in (G, F):
            if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.uint8 and v.dim() == 3
                    and v.is_contiguous()):
                raise ValueError('unires_amd: coreg_hist takes contiguous (X, Y, Z) uint8 device volumes')
    dev = jobs[0][0].device
    arr = (Job * n)(*[_job(*j) for j in jobs])
    hist = torch.empty((n, BINS, BINS), dtype=torch.int64, device=dev)
    check(_lib.load().unires_coreg_hist(n, arr, C.c_void_p(hist.data_ptr()), _stream()))
    return hist


@on_device
def coreg_cost(hist, cost_fun='nmi', fwhm=7.0):
    """Costs of (N, 256, 256) Q16 histograms in one launch -> (N,) float64 device (DESIGN 8.2
    rule 3)."""
    if cost_fun not in COST_FUNS:
        raise NotImplementedError("coreg: cost_fun %r is not built (only 'nmi', 'mi', 'ecc')" % (cost_fun,))
    n = hist.shape[0]
    if hist.shape != (n, BINS, BINS) or hist.dtype != torch.int64:
        raise ValueError('unires_amd: coreg_cost takes (N, 256, 256) int64 histograms')
    hist = hist.contiguous()
    work = torch.empty((n, 2, BINS, BINS), dtype=torch.float64, device=hist.device)
    cost = torch.empty((n,), dtype=torch.float64, device=hist.device)
    check(_lib.load().unires_coreg_cost(n, C.c_void_p(hist.data_ptr()), COST_FUNS[cost_fun], float(fwhm),
                                        C.c_void_p(work.data_ptr()), C.c_void_p(cost.data_ptr()), _stream()))
    return cost


# ---- optimiser -------------------------------------------------------------------------------------
GOLD, GLIMIT, CGOLD, TINY = 1.618034, 100.0, 0.3819660, 1e-20


def _line(p, d, f0, tol):
    """Minimise along p + t d from t = 0 (cost f0): bracket, then Brent with absolute tolerance
    ``tol`` on t.  A generator: yields points, receives their costs; returns (t, f)."""
    ax, bx, fa = 0.0, 1.0, f0
    fb = yield p + bx * d
    if fb > fa:
        ax, bx, fa, fb = bx, ax, fb, fa
    cx = bx + GOLD * (bx - ax)
    fc = yield p + cx * d
    for _ in range(64):
        if not fb > fc:
            break
        r = (bx - ax) * (fb - fc)
        q = (bx - cx) * (fb - fa)
        u = bx - ((bx - cx) * q - (bx - ax) * r) / (2.0 * math.copysign(max(abs(q - r), TINY), q - r))
        ulim = bx + GLIMIT * (cx - bx)
        if (bx - u) * (u - cx) > 0.0:
            fu = yield p + u * d
            if fu < fc:
                ax, bx, fa, fb = bx, u, fb, fu
                break
            if fu > fb:
                cx, fc = u, fu
                break
            u = cx + GOLD * (cx - bx)
            fu = yield p + u * d
        elif (cx - u) * (u - ulim) > 0.0:
            fu = yield p + u * d
            if fu < fc:
                bx, cx, u = cx, u, u + GOLD * (u - cx)
                fb, fc = fc, fu
                fu = yield p + u * d
        elif (u - ulim) * (ulim - cx) >= 0.0:
            u = ulim
            fu = yield p + u * d
        else:
            u = cx + GOLD * (cx - bx)
            fu = yield p + u * d
        ax, bx, cx = bx, cx, u
        fa, fb, fc = fb, fc, fu
    # Brent on [a, b] around bx
    a, b = min(ax, cx), max(ax, cx)
    x = w = v = bx
    fx = fw = fv = fb
    e = dd = 0.0
    for _ in range(100):
        xm = 0.5 * (a + b)
        tol1 = tol + 1e-10
        tol2 = 2.0 * tol1
        if abs(x - xm) <= tol2 - 0.5 * (b - a):
            break
        if abs(e) > tol1:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            pp = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                pp = -pp
            q = abs(q)
            etemp, e = e, dd
            if abs(pp) >= abs(0.5 * q * etemp) or pp <= q * (a - x) or pp >= q * (b - x):
                e = (a - x) if x >= xm else (b - x)
                dd = CGOLD * e
            else:
                dd = pp / q
                u = x + dd
                if u - a < tol2 or b - u < tol2:
                    dd = math.copysign(tol1, xm - x)
        else:
            e = (a - x) if x >= xm else (b - x)
            dd = CGOLD * e
        u = x + dd if abs(dd) >= tol1 else x + math.copysign(tol1, dd)
        fu = yield p + u * d
        if fu <= fx:
            if u >= x:
                a = x
            else:
                b = x
            v, w, x = w, x, u
            fv, fw, fx = fw, fx, fu
        else:
            if u < x:
                a = u
            else:
                b = u
            if fu <= fw or w == x:
                v, w, fv, fw = w, u, fw, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x, fx


def _line_tol(d, tol):
    """Tolerance on t along d: the step whose displacement, in units of the per-parameter
    tolerances, has unit length."""
    return 1.0 / math.sqrt(float(np.sum((d / tol) ** 2)))


def powell(x0, step=STEP, tol=TOL, max_sweeps=MAX_SWEEPS, ftol=FTOL):
    """Powell's method with Brent line minimisation, as a generator: yields float64 points, receives
    their costs (``gen.send(cost)``), returns ``(x, f, evaluations)``.  Initial directions: the unit
    axes scaled by ``step``.  Stops after a sweep that moves no parameter by more than its ``tol``,
    or that gains less than ``ftol`` relative, or after ``max_sweeps`` sweeps."""
    p = np.array(x0, dtype=np.float64)
    n = p.size
    xi = [np.eye(n)[i] * step[i] for i in range(n)]
    nev = 1
    fret = yield p.copy()
    for _ in range(max_sweeps):
        fp, pt = fret, p.copy()
        ibig, dlt = 0, 0.0
        for i in range(n):
            fptt = fret
            t, fret, k = yield from _counted(_line(p.copy(), xi[i], fret, _line_tol(xi[i], tol)))
            nev += k
            p = p + t * xi[i]
            if fptt - fret > dlt:
                dlt, ibig = fptt - fret, i
        if np.all(np.abs(p - pt) <= tol) or 2.0 * (fp - fret) <= ftol * (abs(fp) + abs(fret)) + 1e-20:
            break
        xit = p - pt
        fptt = yield 2.0 * p - pt
        nev += 1
        if fptt < fp:
            t = 2.0 * (fp - 2.0 * fret + fptt) * (fp - fret - dlt) ** 2 - dlt * (fp - fptt) ** 2
            if t < 0.0:
                s, fret, k = yield from _counted(_line(p.copy(), xit, fret, _line_tol(xit, tol)))
                nev += k
                p = p + s * xit
                xi[ibig] = xi[n - 1]
                xi[n - 1] = xit
    return p, fret, nev


def _counted(gen):
    """Forward a sub-generator's requests and count them; returns its value + (count,)."""
    k = 0
    try:
        req = next(gen)
        while True:
            k += 1
            cost = yield req
            req = gen.send(cost)
    except StopIteration as stop:
        return tuple(stop.value) + (k,)


def lockstep(gens, evaluate):
    """Advance every generator of ``gens`` together: each step gathers one request per generator
    that is still running, evaluates them with one ``evaluate([(index, point), ...])`` call (one
    list of costs back) and sends each its cost.  Returns the generators' return values and the
    number of steps."""
    out = [None] * len(gens)
    reqs = {}
    for i, g in enumerate(gens):
        try:
            reqs[i] = next(g)
        except StopIteration as stop:
            out[i] = stop.value
    steps = 0
    while reqs:
        idx = sorted(reqs)
        costs = evaluate([(i, reqs[i]) for i in idx])
        steps += 1
        for i, c in zip(idx, costs):
            try:
                reqs[i] = gens[i].send(float(c))
            except StopIteration as stop:
                out[i] = stop.value
                del reqs[i]
    return out, steps


# ---- affine_align ------------------------------------------------------------------------------------
def _smooth_taps(fwhm):
    """A Gaussian of FWHM ``fwhm`` voxels convolved with the unit box (SPM's kernel), over
    -ceil(2 fwhm) .. ceil(2 fwhm) (at most 15), normalised to sum 1."""
    if fwhm <= 0:
        return np.ones(1, dtype=np.float32)
    R = min(int(math.ceil(2.0 * fwhm)), 15)
    s = (fwhm / math.sqrt(8.0 * math.log(2.0))) ** 2 + np.finfo(np.float64).eps
    w1 = 1.0 / math.sqrt(2.0 * s)
    k = np.array([0.5 * (math.erf(w1 * (i + 0.5)) - math.erf(w1 * (i - 0.5))) for i in range(-R, R + 1)])
    k = np.maximum(k, 0.0)
    return (k / k.sum()).astype(np.float32)


def _level_volume(dat, vx, samp):
    """The float volume sampled at ``samp`` mm: smoothed along every axis whose voxel is smaller
    than ``samp`` by a Gaussian of FWHM sqrt(samp^2 - vx^2) mm (zero padding, same size)."""
    taps = [_smooth_taps(math.sqrt(max(samp ** 2 - float(v) ** 2, 0.0)) / float(v)) for v in vx]
    if all(t.size == 1 for t in taps):
        return dat
    full = _ops.conv_up(dat, taps, (1, 1, 1))
    R = [(t.size - 1) // 2 for t in taps]
    X, Y, Z = dat.shape
    return full[R[0]:R[0] + X, R[1]:R[1] + Y, R[2]:R[2] + Z].contiguous()


def _mat64(mat):
    return np.asarray(torch.as_tensor(mat).detach().to('cpu', torch.float64).numpy())


def voxel_map(q, basis, mat_moving, mat_fix):
    """M = mat_moving^-1 R(q) mat_fix (float64 4x4): fixed voxel -> moving voxel."""
    R = _expm(q, basis).numpy()
    return np.linalg.solve(mat_moving, R @ mat_fix)


def affine_align(imgs, cost_fun='nmi', group='SE', samp=1, fwhm=7, mean_space=False, fix=0, device=None):
    """Align every observation of ``imgs`` (``[[dat, mat], ...]``) rigidly to ``imgs[fix]``.
    Returns ``(q, mat_a)``: the (N, 6) float64 parameters (``_rigid.affine_basis('SE')``) and
    the (N, 4, 4) float64 transforms ``mat_a[i] = expm(q_i)``, ``mat_a[fix] = I``; observation
    i's aligned orientation is ``mat_a[i]^-1 mat_i``.  ``samp``: sampling distance in mm, or a
    tuple of them run coarse to fine.  DESIGN 8.2 states the estimator."""
    if group != 'SE':
        raise NotImplementedError("affine_align: only group='SE' (rigid) is built")
    if mean_space:
        raise NotImplementedError('affine_align: groupwise alignment (mean_space=True) is not built')
    if cost_fun not in COST_FUNS:
        raise NotImplementedError("affine_align: cost_fun %r is not built (only 'nmi', 'mi', 'ecc')" % (cost_fun,))
    N = len(imgs)
    if not 0 <= fix < N:
        raise ValueError('affine_align: fix must index imgs')
    levels = [float(s) for s in (samp if isinstance(samp, (list, tuple)) else [samp])]
    basis = affine_basis('SE')
    q = np.zeros((N, 6))
    mats = [_mat64(m) for _, m in imgs]
    pairs = [i for i in range(N) if i != fix]
    if pairs:
        dev = torch.device(device) if device is not None else None
        dats = []
        for d, _ in imgs:
            d = torch.as_tensor(d)
            if dev is not None and dev.type == 'cuda':
                d = d.to(dev)
            dats.append(d.to(torch.float32).contiguous())
        vxs = [voxel_size(m).numpy() for m in mats]
        for s in levels:
            vols = [_level_volume(d, vx, s) for d, vx in zip(dats, vxs)]
            u8, _, _ = coreg_quantise(vols)
            step = (s / vxs[fix]).astype(np.float32)

            def evaluate(reqs, u8=u8, step=step):
                jobs = [(u8[fix], u8[pairs[k]], _m12(voxel_map(x, basis, mats[pairs[k]], mats[fix])), step)
                        for k, x in reqs]
                return coreg_cost(coreg_hist(jobs), cost_fun, fwhm).cpu().tolist()

            res, _ = lockstep([powell(q[i]) for i in pairs], evaluate)
            for k, i in enumerate(pairs):
                q[i] = res[k][0]
    mat_a = torch.stack([_expm(q[i], basis) if i != fix else torch.eye(4, dtype=torch.float64) for i in range(N)])
    return torch.from_numpy(q), mat_a
