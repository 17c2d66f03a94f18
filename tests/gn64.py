"""numpy restatement of the slice weights in the two Gauss-Newton updates: the five weighted scaling
sums (unires_scaling_sums_w), the weighted x-space residual of the rigid step (unires_rigid_resid) and the weighted
objective 1/2 tau sum_s u_s SSE_s the rigid step and its line search minimise.  Built on tests/admm64.py (the float32
terms and the summation depth of k_scaling_sums) and tests/slice64.py (the per-slice sums); the reference has no
counterpart, so nothing here is pinned against it.

The weighted data term of a repeat is 1/2 tau sum_v u[s(v)] [x(v) != 0] (x(v) - (A y)(v))^2, s(v) the index of voxel v
along ``axis`` and u float32.
"""
import math
from fractions import Fraction

import numpy as np

from tests import admm64, slice64


def _u_at(shape, axis, u):
    """u[s(v)] as a float64 volume of ``shape``."""
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    assert u.shape == (shape[axis],)
    view = [1, 1, 1]
    view[axis] = shape[axis]
    return np.broadcast_to(u.reshape(view), shape)


def scaling_terms_w(x, ay, axis, u):
    """admm64.scaling_terms times the weight of each masked voxel's slice.  A term is a float32 value and the weight a
    float32 value: their float64 product has at most 48 significant bits and is exact."""
    x = np.asarray(x, dtype=np.float32)
    s0, g, h, ev = admm64.scaling_terms(x, ay, axis)
    uu = _u_at(x.shape, axis, u)[x != 0]
    return uu * s0, uu * g, uu * h, ev


def scaling_sums_w(x, ay, axis, u):
    """(ref[5], tol[5]) of unires_scaling_sums_w: exact sums (math.fsum) of the exact weighted terms; the tolerance is
    admm64.scaling_sums' own - the depth of k_scaling_sums' summation, which the weighted kernel shares, times 2^-53
    of the sum of |u t|."""
    terms = scaling_terms_w(x, ay, axis, u)
    s0, g, h, ev = terms
    n = int(np.asarray(x).size)
    nb = max(1, min(1024, -(-n // 256)))
    dep = admm64.depth(-(-n // (nb * 256)), nb) + 1
    ga = np.abs(g)
    tol = [dep * admm64.U64 * float(v) for v in (s0.sum(), ga[ev].sum(), ga[~ev].sum(), h[ev].sum(), h[~ev].sum())]
    return admm64.scaling_sums_of(terms), tol


def rigid_resid32(x, ay, axis, u):
    """The residual of the rigid step in float32, as the kernel forms it: fl(u[s(v)] fl(ay - x)) where x != 0 and
    ay != 0, else +0; u None: fl(ay - x).  numpy's float32 subtraction and product are IEEE round-to-nearest, as
    __fsub_rn / __fmul_rn are: bit-exact."""
    x, ay = np.asarray(x, dtype=np.float32), np.asarray(ay, dtype=np.float32)
    r = (ay - x).astype(np.float32)
    if u is not None:
        r = (_u_at(x.shape, axis, u).astype(np.float32) * r).astype(np.float32)
    return np.where((x != 0) & (ay != 0), r, np.float32(0.0)).astype(np.float32)


def weighted_sse(x, ay, axis, u):
    """(ref, tol) of sum_s u_s SSE_s: the exact value (rational arithmetic on slice64.slice_sums64's exact per-slice
    sums) and the bound on the device's float64 form - every SSE_s within N_s 2^-53 SSE_s, carried
    through its weight, plus S 2^-53 sum_s u_s SSE_s for the dot product's S products and S - 1 additions (times
    1 + 2^-50: the higher orders, and the rounding of the exact value to float64)."""
    sse, cnt, bound = slice64.slice_sums64(x, ay, axis)
    uu = np.asarray(u, dtype=np.float32).astype(np.float64)
    exact = sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(uu, sse)), Fraction(0))
    mag = math.fsum((uu * sse).tolist())
    tol = math.fsum((uu * bound).tolist()) + len(uu) * 2.0 ** -53 * mag * (1.0 + 2.0 ** -50)
    return float(exact), tol
