"""numpy restatement of the voxel weights in the two Gauss-Newton updates: the five sums of the scaling
step with per-voxel weights (unires_scaling_sums_g), the x-space residual of the rigid step with them
(unires_rigid_resid_g) and the rule a weight map is decimated by.  Built on tests/gn64.py (the slice-weighted forms),
tests/voxel64.py (the apply pass's rounding), tests/admm64.py (the float32 terms and the summation depth of
k_scaling_sums) and tests/slice64.py; the reference has no counterpart, so nothing here is pinned against it.

The data term of a repeat is 1/2 tau sum_v W(v) [x(v) != 0] (x(v) - (A y)(v))^2 with W(v) = g(v) u[s(v)], g a float32
volume, u float32 weights per slice along ``axis`` or None (= 1).
"""
import math

import numpy as np

from tests import admm64, gn64, slice64, voxel64  # noqa: F401  (slice64: the weight patterns the tests draw u from)


def weight64(g, axis, u):
    """W = g u[s(v)] as a float64 volume: two float32 factors, at most 48 significant bits - exact.  u None: g."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    return g if u is None else g * gn64._u_at(g.shape, axis, u)


def _split(w):
    """w = hi + lo, both with at most 24 significant bits (hi the float32 nearest w; w has at most 48): the product of
    either with a float32 value is exact in float64."""
    hi = w.astype(np.float32).astype(np.float64)
    return hi, w - hi


def scaling_sums_g(x, ay, axis, g, u):
    """(ref[5], tol[5]) of unires_scaling_sums_g.  ref: the exact sums (math.fsum) of the exact weighted terms W t, t
    the float32 terms of admm64.scaling_terms - W t has up to 72 bits where both weights are present, so it is summed as
    hi t + lo t, two exact float64 products (``_split``).  tol: admm64.scaling_sums' own - the depth of
    k_scaling_sums' summation, which the kernel shares, times 2^-53 of the sum of |W t| - and, where both weights are
    present, 2^-53 sum |W t| more for the one rounding of every summand fl64(W t)."""
    x = np.asarray(x, dtype=np.float32)
    s0, gg, hh, ev = admm64.scaling_terms(x, ay, axis)
    w = weight64(g, axis, u)[x != 0]
    hi, lo = _split(w)

    def exact(t, m):
        return math.fsum((hi[m] * t[m]).tolist() + (lo[m] * t[m]).tolist())

    every = np.ones_like(ev)
    ref = [exact(s0, every), exact(gg, ev), exact(gg, ~ev), exact(hh, ev), exact(hh, ~ev)]
    n = int(x.size)
    nb = max(1, min(1024, -(-n // 256)))
    dep = admm64.depth(-(-n // (nb * 256)), nb) + 1
    if u is not None:
        dep += 1
    ga = np.abs(gg)
    mags = (w * s0, (w * ga)[ev], (w * ga)[~ev], (w * hh)[ev], (w * hh)[~ev])
    return ref, [dep * admm64.U64 * float(v.sum()) for v in mags]


def rigid_resid_g32(x, ay, axis, g, u):
    """The residual of the rigid step with voxel weights in float32, as the kernel forms it: r = fl32(ay - x), then
    voxel64.apply32's product - fl32(g r) without u, fl32(fl64(fl64(g u) r)) with - where x != 0 and ay != 0, else +0."""
    x, ay = np.asarray(x, dtype=np.float32), np.asarray(ay, dtype=np.float32)
    r = (ay - x).astype(np.float32)
    out = voxel64.apply32(r, g, u, axis)
    return np.where((x != 0) & (ay != 0), out, np.float32(0.0)).astype(np.float32)


def decimate(weight, sk, dim_x):
    """The weight map on the decimated lattice of the rigid update: every sk[a]-th voxel along axis a from the first,
    cut to dim_x - the nearest-neighbour rule the observation itself is decimated by."""
    w = np.asarray(weight)[::sk[0], ::sk[1], ::sk[2]]
    return np.ascontiguousarray(w[:dim_x[0], :dim_x[1], :dim_x[2]])


def box_weights(shape, box):
    """Ones with weight 0 in ``box`` = ((i0, i1), (j0, j1), (k0, k1)), float32."""
    w = np.ones(tuple(int(s) for s in shape), dtype=np.float32)
    (i0, i1), (j0, j1), (k0, k1) = box
    w[i0:i1, j0:j1, k0:k1] = 0.0
    return w
