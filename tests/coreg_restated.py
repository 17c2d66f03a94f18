"""NumPy restatement of the coregistration estimator (rules 1-3): quantisation, the
Q16 partial-volume joint histogram and the histogram costs.  float32 for everything up to the
integer counts, in the kernels' operation order (coreg.hip compiles without FP contraction), so that
quantised volumes and histograms agree bit for bit; float64 after."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
JITTER = 97


def jitter_table():
    x = np.arange(1, JITTER + 1, dtype=F64) * 0.6180339887498949
    return (x % 1.0).astype(F32)


def quantise(vol):
    """-> (uint8 volume, counts (1024,), (mn, max, mx, scale)); ValueError as the GPU path."""
    v = np.ascontiguousarray(vol, dtype=F32)
    flat = v.reshape(-1)
    fin = np.isfinite(flat)
    if not fin.any():
        raise ValueError('no finite voxel')
    vf = flat[fin]
    lo, hi = vf.min(), vf.max()
    if not hi > lo:
        raise ValueError('constant')
    width = F64(hi) - F64(lo)
    bins = np.minimum(np.floor(((vf.astype(F64) - F64(lo)) * 1024.0) / width).astype(np.int64), 1023)
    counts = np.bincount(bins, minlength=1024).astype(np.int64)
    cum = np.cumsum(counts)
    k = int(np.argmax(cum * 10000 >= cum[-1] * 9999))
    mx = F32(F64(lo) + (F64(hi) - F64(lo)) * (k + 1) / 1024.0)
    if not mx > lo:
        raise ValueError('constant')
    scale = F32(255.0) / (mx - lo)
    q = np.zeros(flat.shape, dtype=F32)
    q[fin] = np.minimum(np.maximum(np.rint((vf - lo) * scale), F32(0)), F32(255))
    return q.astype(np.uint8).reshape(v.shape), counts, (lo, hi, mx, scale)


def grid(dim_g, step):
    return [int(math.floor(F64(dim_g[d] - 1) / F64(F32(step[d])))) + 1 for d in range(3)]


def _tri(vol, x0, x1, x2):
    d = vol.shape
    i = [np.minimum(np.floor(x).astype(np.int64), d[k] - 2) for k, x in enumerate((x0, x1, x2))]
    f = [x - i[k].astype(F32) for k, x in enumerate((x0, x1, x2))]
    a = [F32(1) - t for t in f]
    v = vol.astype(F32)

    def at(o0, o1, o2):
        return v[i[0] + o0, i[1] + o1, i[2] + o2]
    c00 = at(0, 0, 0) * a[0] + at(1, 0, 0) * f[0]
    c01 = at(0, 0, 1) * a[0] + at(1, 0, 1) * f[0]
    c10 = at(0, 1, 0) * a[0] + at(1, 1, 0) * f[0]
    c11 = at(0, 1, 1) * a[0] + at(1, 1, 1) * f[0]
    e0 = c00 * a[1] + c10 * f[1]
    e1 = c01 * a[1] + c11 * f[1]
    return e0 * a[2] + e1 * f[2]


def hist(G, F, M, step):
    """Q16 joint histogram (256, 256) uint64 of fixed G / moving F (uint8), M: (12,) float32 G
    voxel -> F voxel, step: sampling step in G voxels."""
    M = np.asarray(M, dtype=F32).reshape(-1)
    s = np.asarray(step, dtype=F32)
    ng = grid(G.shape, s)
    p = np.arange(ng[0] * ng[1] * ng[2], dtype=np.int64)
    i2 = p % ng[2]
    t = p // ng[2]
    i1, i0 = t % ng[1], t // ng[1]
    T = jitter_table()
    k0 = (3 * (p % JITTER)) % JITTER
    k1 = (k0 + 1) % JITTER
    k2 = (k1 + 1) % JITTER
    x0 = (i0.astype(F32) + T[k0]) * s[0]
    x1 = (i1.astype(F32) + T[k1]) * s[1]
    x2 = (i2.astype(F32) + T[k2]) * s[2]
    ok = np.ones(p.shape, bool)
    for x, n in zip((x0, x1, x2), G.shape):
        ok &= (x >= 0) & (x <= F32(n - 1))
    x0, x1, x2 = x0[ok], x1[ok], x2[ok]
    y = [((M[4 * e] * x0 + M[4 * e + 1] * x1) + M[4 * e + 2] * x2) + M[4 * e + 3] for e in range(3)]
    inf = np.ones(x0.shape, bool)
    for yy, n in zip(y, F.shape):
        inf &= (yy >= 0) & (yy <= F32(n - 1))
    g = np.minimum(np.rint(_tri(G, x0, x1, x2)).astype(np.int64), 255)
    f = np.zeros(x0.shape, F32)   # outside F: f = 0
    f[inf] = np.minimum(_tri(F, *[yy[inf] for yy in y]), F32(255))
    fl = np.floor(f).astype(np.int64)
    whi = np.rint((f - fl.astype(F32)) * F32(65536)).astype(np.int64)
    wlo = 65536 - whi
    H = np.bincount(g * 256 + fl, weights=wlo.astype(F64), minlength=65536)
    hi = fl < 255
    H += np.bincount(g[hi] * 256 + fl[hi] + 1, weights=whi[hi].astype(F64), minlength=65536)
    return H.astype(np.uint64).reshape(256, 256)


def taps(fwhm):
    R = int(math.floor(2.0 * fwhm + 0.5))  # lround
    s = (fwhm / math.sqrt(8.0 * math.log(2.0))) ** 2 + np.finfo(F64).eps
    w1 = 1.0 / math.sqrt(2.0 * s)
    k = np.array([0.5 * (math.erf(w1 * (i + 0.5)) - math.erf(w1 * (i - 0.5))) for i in range(-R, R + 1)])
    k = np.maximum(k, 0.0)
    return k / k.sum()


def _smooth(H, w, axis):
    R = (len(w) - 1) // 2
    out = np.zeros_like(H)
    n = H.shape[axis]
    for k in range(-R, R + 1):
        src = slice(max(0, k), min(n, n + k))
        dst = slice(max(0, -k), min(n, n - k))
        if axis == 1:
            out[:, dst] += w[k + R] * H[:, src]
        else:
            out[dst, :] += w[k + R] * H[src, :]
    return out


def cost(H, cost_fun='nmi', fwhm=7.0):
    """float64 cost of one Q16 histogram H[g][f]."""
    h = np.asarray(H, dtype=np.uint64).astype(F64) / 65536.0
    w = taps(fwhm)
    h = _smooth(_smooth(h, w, 1), w, 0) + np.finfo(F64).eps
    sh = h.sum()
    p = h / sh
    s1 = h.sum(0) / sh  # over g: per f
    s2 = h.sum(1) / sh  # over f: per g
    e1 = float(np.sum(s1 * np.log2(s1)))
    e2 = float(np.sum(s2 * np.log2(s2)))
    hj = float(np.sum(p * np.log2(p)))
    mi = float(np.sum(p * np.log2(p / (s2[:, None] * s1[None, :]))))
    if cost_fun == 'nmi':
        return -(e1 + e2) / hj
    if cost_fun == 'mi':
        return -mi
    if cost_fun == 'ecc':
        return 2.0 * mi / (e1 + e2)
    raise NotImplementedError(cost_fun)
