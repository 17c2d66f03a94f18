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


class JobM(C.Structure):
    """``unires_coreg_job_m_t``."""
    _fields_ = Job._fields_ + [('mG', C.c_void_p), ('mF', C.c_void_p)]


def _u8vol(v):
    return (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.uint8 and v.dim() == 3
            and v.is_contiguous())


@on_device
def coreg_quantise(dats, masks=None):
    """uint8 copies of float32 volumes, one launch for all (DESIGN 8.2 rule 1).  Returns
    ``(vols, counts, params)``: the uint8 volumes, the (N, 1024) int32 histograms of the finite
    voxels over [min, max] and the (N, 8) float32 rows (min, max, robust max, scale, status, ...),
    all on the device.  Raises ValueError for a volume with no finite voxel or a constant one.
    ``masks``: one uint8 device support (non-zero usable) or None per volume; range, histogram and
    robust maximum are then those of the finite usable voxels, and every finite voxel is converted
    with them."""
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
    masked = masks is not None and any(m is not None for m in masks)
    if masked:
        if len(masks) != n or any(m is not None and not (_u8vol(m) and m.shape == v.shape) for m, v in zip(masks, vols)):
            raise ValueError('unires_amd: coreg_quantise takes one contiguous uint8 device support of its '
                             "volume's shape (or None) per volume")
        mptrs = (C.c_void_p * n)(*[None if m is None else m.data_ptr() for m in masks])
        check(_lib.load().unires_coreg_quantise_m(n, ptrs, sizes, mptrs, optrs, C.c_void_p(counts.data_ptr()),
                                                  C.c_void_p(params.data_ptr()), _stream()))
    else:
        check(_lib.load().unires_coreg_quantise(n, ptrs, sizes, optrs, C.c_void_p(counts.data_ptr()),
                                                C.c_void_p(params.data_ptr()), _stream()))
    status = params[:, STATUS].cpu()
    for i, s in enumerate(status.tolist()):
        usable = ' usable' if masked and masks[i] is not None else ''
        if s == 1:
            raise ValueError('coreg: observation %d has no finite%s voxel' % (i, usable))
        if s == 2:
            raise ValueError('coreg: observation %d is constant%s' % (i, ' over its usable voxels' if usable else ''))
    return outs, counts, params


@on_device
def coreg_cellmask(mask):
    """Cell support of a uint8 device support (X, Y, Z): 1 where the eight voxels of the interpolation
    cell that starts at the voxel are all usable, 0 elsewhere and in the last plane of every axis
    (DESIGN 8.10)."""
    if not _u8vol(mask):
        raise ValueError('unires_amd: coreg_cellmask takes a contiguous (X, Y, Z) uint8 device volume')
    cell = torch.empty_like(mask)
    check(_lib.load().unires_coreg_cellmask(C.c_void_p(mask.data_ptr()), _lib.i3(mask.shape),
                                            C.c_void_p(cell.data_ptr()), _stream()))
    return cell


def _job(G, F, M, step, mG=None, mF=None, cls=Job):
    j = cls()
    j.G, j.F = G.data_ptr(), F.data_ptr()
    j.dim_g = _lib.c_i32x3(*G.shape)
    j.dim_f = _lib.c_i32x3(*F.shape)
    j.M = _lib.c_f32x12(*[float(v) for v in np.asarray(M, dtype=np.float32).reshape(-1)])
    j.step = _lib.c_f32x3(*[float(v) for v in np.asarray(step, dtype=np.float32)])
    if cls is JobM:
        j.mG = None if mG is None else mG.data_ptr()
        j.mF = None if mF is None else mF.data_ptr()
    return j


@on_device
def coreg_hist(jobs):
    """Joint histograms of ``jobs``, a list of ``(G, F, M, step)``: uint8 device volumes, the
    float32 3x4 (12,) map from G voxels to F voxels and the sampling step in G voxels.  One launch
    -> (N, 256, 256) int64 device counts in Q16 units (DESIGN 8.2 rule 2).  A job may be
    ``(G, F, M, step, mG, mF)``: the cell supports (``coreg_cellmask``) of G and F, each or both None;
    a sample point in an unsupported cell of G, or imaged into an unsupported cell of F, is dropped
    (DESIGN 8.10)."""
    n = len(jobs)
    for job in jobs:
        if len(job) not in (4, 6):
            raise ValueError('unires_amd: a coreg_hist job is (G, F, M, step) or (G, F, M, step, mG, mF)')
        for v in job[:2]:
            if not _u8vol(v):
                raise ValueError('unires_amd: coreg_hist takes contiguous (X, Y, Z) uint8 device volumes')
        for m, v in zip(job[4:], job[:2]):
            if m is not None and not (_u8vol(m) and m.shape == v.shape):
                raise ValueError("unires_amd: a cell support is a contiguous uint8 device volume of its image's shape")
    dev = jobs[0][0].device
    hist = torch.empty((n, BINS, BINS), dtype=torch.int64, device=dev)
    if any(len(job) == 6 and (job[4] is not None or job[5] is not None) for job in jobs):
        arr = (JobM * n)(*[_job(*j, cls=JobM) for j in jobs])
        check(_lib.load().unires_coreg_hist_m(n, arr, C.c_void_p(hist.data_ptr()), _stream()))
        return hist
    arr = (Job * n)(*[_job(*j[:4]) for j in jobs])
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


def _level_taps(vx, samp):
    return [_smooth_taps(math.sqrt(max(samp ** 2 - float(v) ** 2, 0.0)) / float(v)) for v in vx]


def erode_support(sup, radius):
    """Erode a boolean support (X, Y, Z) along each axis d by ``radius[d]`` voxels: a voxel stays
    usable only if no voxel within +-radius[d] along that axis is unusable.  Voxels beyond the
    volume's end count as usable (the smoothing pads with zeros there with or without a support).
    Exact integer arithmetic (a running count of unusable voxels per line), one axis after the other."""
    bad = ~sup
    for ax, r in enumerate(radius):
        if r <= 0:
            continue
        n = bad.shape[ax]
        c = torch.cumsum(bad.to(torch.int32), dim=ax)
        c = torch.cat([torch.zeros_like(c.narrow(ax, 0, 1)), c], dim=ax)  # c[k] = unusable among [0, k)
        idx = torch.arange(n, device=bad.device)
        hi, lo = torch.clamp(idx + r + 1, max=n), torch.clamp(idx - r, min=0)
        bad = (c.index_select(ax, hi) - c.index_select(ax, lo)) > 0
    return ~bad


def _level_support(weight, vx, samp):
    """uint8 support of a level volume: the support of the map (> 0), eroded by the tap radius along
    every axis ``_level_volume`` smooths."""
    R = [(t.size - 1) // 2 for t in _level_taps(vx, samp)]
    return erode_support(weight > 0, R).to(torch.uint8).contiguous()


def _level_volume(dat, vx, samp):
    """The float volume sampled at ``samp`` mm: smoothed along every axis whose voxel is smaller
    than ``samp`` by a Gaussian of FWHM sqrt(samp^2 - vx^2) mm (zero padding, same size)."""
    taps = _level_taps(vx, samp)
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


def affine_align(imgs, cost_fun='nmi', group='SE', samp=1, fwhm=7, mean_space=False, fix=0, device=None,
                 weights=None):
    """Align every observation of ``imgs`` (``[[dat, mat], ...]``) rigidly to ``imgs[fix]``.
    Returns ``(q, mat_a)``: the (N, 6) float64 parameters (``_rigid.affine_basis('SE')``) and
    the (N, 4, 4) float64 transforms ``mat_a[i] = expm(q_i)``, ``mat_a[fix] = I``; observation
    i's aligned orientation is ``mat_a[i]^-1 mat_i``.  ``samp``: sampling distance in mm, or a
    tuple of them run coarse to fine.  DESIGN 8.2 states the estimator.  ``weights``: one map of its
    image's shape (or None) per image - cost-function masking: voxels where a map is not > 0 enter
    neither the quantisation parameters nor any counted sample of the histograms."""
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
        maps = None
        if weights is not None and any(w is not None for w in weights):
            if len(weights) != N:
                raise ValueError('affine_align: weights must have one entry (a map or None) per image')
            maps = [None if w is None else torch.as_tensor(w).to(d.device) for w, d in zip(weights, dats)]
            if any(g is not None and g.shape != d.shape for g, d in zip(maps, dats)):
                raise ValueError("affine_align: a weight map must have its image's shape")
        for s in levels:
            vols = [_level_volume(d, vx, s) for d, vx in zip(dats, vxs)]
            step = (s / vxs[fix]).astype(np.float32)
            if maps is None:
                u8, _, _ = coreg_quantise(vols)
                cell = [None] * N
            else:  # supports of the level volumes, then their cell supports: once per level
                sup = [None if g is None else _level_support(g, vx, s) for g, vx in zip(maps, vxs)]
                u8, _, _ = coreg_quantise(vols, sup)
                cell = [None if m is None else coreg_cellmask(m) for m in sup]

            def evaluate(reqs, u8=u8, step=step, cell=cell):
                jobs = [(u8[fix], u8[pairs[k]], _m12(voxel_map(x, basis, mats[pairs[k]], mats[fix])), step)
                        for k, x in reqs]
                if maps is not None:
                    jobs = [j + (cell[fix], cell[pairs[k]]) for j, (k, _) in zip(jobs, reqs)]
                return coreg_cost(coreg_hist(jobs), cost_fun, fwhm).cpu().tolist()

            res, _ = lockstep([powell(q[i]) for i in pairs], evaluate)
            for k, i in enumerate(pairs):
                q[i] = res[k][0]
    mat_a = torch.stack([_expm(q[i], basis) if i != fix else torch.eye(4, dtype=torch.float64) for i in range(N)])
    return torch.from_numpy(q), mat_a
