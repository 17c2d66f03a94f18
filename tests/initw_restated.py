"""NumPy restatement of voxel weight maps in the initialisation: the support of a map decides which
voxels the noise estimator, the coregistration and the first guess read.  Exact integers, float64, and the float32
operation order of tests/coreg_restated.py where the GPU's bits are to be met; nothing is copied from
noise_restated / coreg_restated / voxel64, they are imported."""
import numpy as np

from tests import coreg_restated as CR
from tests import noise_restated as NR

F32, F64 = np.float32, np.float64


# ---- noise ------------------------------------------------------------------------------------------------------
def usable(weight):
    """Support of a map: weight > 0 (NaN is not), flat bool."""
    return np.asarray(weight, dtype=F32).ravel() > 0


def select(dat, ct, weight=None):
    """The voxels the masked histogram takes: those of noise_restated.select whose weight is > 0."""
    v = np.asarray(dat, dtype=F32).ravel()
    if weight is None:
        return NR.select(v, ct)
    return NR.select(v[usable(weight)], ct)


def histogram(dat, ct, weight=None):
    """(counts (1024,) int64 or None, (mn, mx)) of the usable selected voxels, by noise_restated's rule."""
    v = np.asarray(dat, dtype=F32).ravel()
    if weight is None:
        return NR.histogram(v, ct)
    u = usable(weight)
    keep = np.isfinite(v) & (v != 0) & u
    if not ct:
        keep &= v >= 0
    w = v[keep]
    if w.size == 0:
        return None, (F32(np.inf), F32(-np.inf))
    mn, mx = w.min(), w.max()
    if not mx > mn:
        return None, (mn, mx)
    q = ((w.astype(F64) - F64(mn)) * float(NR.BINS)) / (F64(mx) - F64(mn))
    return np.bincount(np.minimum(np.floor(q).astype(np.int64), NR.BINS - 1), minlength=NR.BINS), (mn, mx)


# ---- coregistration ---------------------------------------------------------------------------------------------
def quantise(vol, mask=None):
    """coreg_restated.quantise with range, histogram and robust maximum over the finite USABLE voxels; every finite
    voxel is converted.  -> (uint8 volume, counts (1024,), (mn, max, mx, scale))."""
    v = np.ascontiguousarray(vol, dtype=F32)
    if mask is None:
        return CR.quantise(v)
    flat = v.reshape(-1)
    fin = np.isfinite(flat)
    use = fin & (np.asarray(mask).reshape(-1) != 0)
    if not use.any():
        raise ValueError('no finite usable voxel')
    vu = flat[use]
    lo, hi = vu.min(), vu.max()
    if not hi > lo:
        raise ValueError('constant')
    width = F64(hi) - F64(lo)
    bins = np.minimum(np.floor(((vu.astype(F64) - F64(lo)) * 1024.0) / width).astype(np.int64), 1023)
    counts = np.bincount(bins, minlength=1024).astype(np.int64)
    cum = np.cumsum(counts)
    k = int(np.argmax(cum * 10000 >= cum[-1] * 9999))
    mx = F32(F64(lo) + (F64(hi) - F64(lo)) * (k + 1) / 1024.0)
    if not mx > lo:
        raise ValueError('constant')
    scale = F32(255.0) / (mx - lo)
    q = np.zeros(flat.shape, dtype=F32)
    q[fin] = np.minimum(np.maximum(np.rint((flat[fin] - lo) * scale), F32(0)), F32(255))
    return q.astype(np.uint8).reshape(v.shape), counts, (lo, hi, mx, scale)


def cellmask(mask):
    """cell[i0, i1, i2] = 1 iff the eight voxels (i0..i0+1, i1..i1+1, i2..i2+1) are usable, for i_d <= dim_d - 2;
    0 in the last plane of every axis (no cell starts there)."""
    m = np.asarray(mask) != 0
    cell = np.zeros(m.shape, np.uint8)
    if min(m.shape) < 2:
        return cell
    c = np.ones(tuple(n - 1 for n in m.shape), bool)
    for o0 in (0, 1):
        for o1 in (0, 1):
            for o2 in (0, 1):
                c &= m[o0:m.shape[0] - 1 + o0, o1:m.shape[1] - 1 + o1, o2:m.shape[2] - 1 + o2]
    cell[:-1, :-1, :-1] = c
    return cell


def defined(shape):
    """Where a cell support is defined: i_d <= dim_d - 2."""
    d = np.zeros(shape, bool)
    d[:-1, :-1, :-1] = True
    return d


def _cell_of(cell, x):
    i = [np.minimum(np.floor(xx).astype(np.int64), cell.shape[k] - 2) for k, xx in enumerate(x)]
    return cell[i[0], i[1], i[2]] != 0


def hist(G, F, M, step, mG=None, mF=None, return_kept=False):
    """coreg_restated.hist with the drop rule: a sample point kept by its rule (inside G) is dropped when its G cell
    has mG == 0, or when its image lies inside F and its F cell has mF == 0; a point imaged outside F counts with
    f = 0 whatever mF says.  mG / mF: cell supports (``cellmask``) or None.  Q16 (256, 256) uint64."""
    M = np.asarray(M, dtype=F32).reshape(-1)
    s = np.asarray(step, dtype=F32)
    ng = CR.grid(G.shape, s)
    p = np.arange(ng[0] * ng[1] * ng[2], dtype=np.int64)
    i2 = p % ng[2]
    t = p // ng[2]
    i1, i0 = t % ng[1], t // ng[1]
    T = CR.jitter_table()
    k0 = (3 * (p % CR.JITTER)) % CR.JITTER
    k1 = (k0 + 1) % CR.JITTER
    k2 = (k1 + 1) % CR.JITTER
    x = [(i0.astype(F32) + T[k0]) * s[0], (i1.astype(F32) + T[k1]) * s[1], (i2.astype(F32) + T[k2]) * s[2]]
    ok = np.ones(p.shape, bool)
    for xx, n in zip(x, G.shape):
        ok &= (xx >= 0) & (xx <= F32(n - 1))
    x = [xx[ok] for xx in x]
    if mG is not None:
        keep = _cell_of(mG, x)
        x = [xx[keep] for xx in x]
    y = [((M[4 * e] * x[0] + M[4 * e + 1] * x[1]) + M[4 * e + 2] * x[2]) + M[4 * e + 3] for e in range(3)]
    inf = np.ones(x[0].shape, bool)
    for yy, n in zip(y, F.shape):
        inf &= (yy >= 0) & (yy <= F32(n - 1))
    if mF is not None:
        keep = np.ones(x[0].shape, bool)
        keep[inf] = _cell_of(mF, [yy[inf] for yy in y])
        x, y, inf = [xx[keep] for xx in x], [yy[keep] for yy in y], inf[keep]
    g = np.minimum(np.rint(CR._tri(G, *x)).astype(np.int64), 255)
    f = np.zeros(x[0].shape, F32)
    f[inf] = np.minimum(CR._tri(F, *[yy[inf] for yy in y]), F32(255))
    fl = np.floor(f).astype(np.int64)
    whi = np.rint((f - fl.astype(F32)) * F32(65536)).astype(np.int64)
    wlo = 65536 - whi
    H = np.bincount(g * 256 + fl, weights=wlo.astype(F64), minlength=65536)
    hi = fl < 255
    H += np.bincount(g[hi] * 256 + fl[hi] + 1, weights=whi[hi].astype(F64), minlength=65536)
    H = H.astype(np.uint64).reshape(256, 256)
    return (H, int(x[0].size)) if return_kept else H


def erode(sup, radius):
    """Erode a boolean support along each axis d by radius[d]: a voxel stays usable only if no voxel within
    +-radius[d] along that axis (inside the volume) is unusable; one axis after the other."""
    out = np.asarray(sup, dtype=bool)
    for ax, r in enumerate(radius):
        if r <= 0:
            continue
        n = out.shape[ax]
        src = out
        out = src.copy()
        for k in range(max(-r, 1 - n), min(r, n - 1) + 1):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[ax] = slice(max(0, -k), min(n, n - k))   # voxels i with i + k inside the volume
            b[ax] = slice(max(0, k), min(n, n + k))    # their neighbours i + k
            out[tuple(a)] &= src[tuple(b)]
    return out


# ---- first guess ------------------------------------------------------------------------------------------------
TIE = 1e-4


def support(g, M, gdim, fov_tol=5e-2):
    """Support of the trilinear pull (zero bound, in-FOV mask with ``fov_tol``) of a volume with the weight map g
    under the affine M (12,) float32, in float64: 1 iff the coordinate c = M (i, j, k) is inside the FOV and every
    corner (floor(c_d) | floor(c_d) + 1) that lies inside the volume has g > 0.  Returns (support uint8, flag bool):
    a voxel is flagged a near tie when a coordinate component lies within 1e-4 of an integer or of a FOV threshold
    (-fov_tol, dim_d - 1 + fov_tol) - there a float32 coordinate may fall on the other side."""
    g = np.asarray(g)
    use = g > 0
    sd = g.shape
    M = np.asarray(M, dtype=F32).astype(F64).reshape(3, 4)
    ijk = np.stack(np.meshgrid(*[np.arange(n, dtype=F64) for n in gdim], indexing='ij'), -1)
    c = ijk @ M[:, :3].T + M[:, 3]
    flag = np.zeros(tuple(gdim), bool)
    fov = np.ones(tuple(gdim), bool)
    for d in range(3):
        cd = c[..., d]
        flag |= np.abs(cd - np.rint(cd)) < TIE
        flag |= (np.abs(cd + fov_tol) < TIE) | (np.abs(cd - (sd[d] - 1 + fov_tol)) < TIE)
        fov &= (cd > -fov_tol) & (cd < sd[d] - 1 + fov_tol)
    fl = np.floor(c).astype(np.int64)
    ok = fov.copy()
    for o0 in (0, 1):
        for o1 in (0, 1):
            for o2 in (0, 1):
                i = [fl[..., 0] + o0, fl[..., 1] + o1, fl[..., 2] + o2]
                inside = np.ones(tuple(gdim), bool)
                for d in range(3):
                    inside &= (i[d] >= 0) & (i[d] < sd[d])
                ic = [np.clip(i[d], 0, sd[d] - 1) for d in range(3)]
                ok &= ~inside | use[ic[0], ic[1], ic[2]]
    return ok.astype(np.uint8), flag
