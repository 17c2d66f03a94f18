"""Restatement of the Rician noise model in the rigid Gauss-Newton update (sett.rician_gn): the data
term of a Rician repeat with its first and second derivative in float64, the float64 statement of
unires_rigid_terms_r's outputs, and the float32 residual by the kernel's operation sequence.  Built on
tests/rician64.py (R, c, the kernel's p, z and effective observation), tests/gne64.py (the weights and tables),
tests/gn64.py / tests/gnv64.py / tests/voxel64.py (the residual's roundings) and tests/slice64.py / tests/voxel64.py
(the slice sums); the reference has no counterpart, so nothing here is pinned against it.

With a = A y, p = e[s(v)] a, z = tau x p and W = g u[s(v)] (g a float32 volume or None = 1, u and e float32 per slice
along ``axis`` or None = 1), the data term of a Rician repeat is

    E(a) = sum_v W(v) { [x != 0] 1/2 tau (x - p)^2 + c(z) },        c(z) = (z - |z|) - log i0e(|z|)

(c(0) = 0: a voxel with x = 0 adds nothing).  For z > 0, c'(z) = 1 - R(z), R = I1 / I0, so

    dE/da   = tau W e (p - x R(z))                      the Gaussian residual on the effective observation x R(z)
    d2E/da2 = tau W e^2 (1 - tau x^2 R'(z))             R'(z) = 1 - R / z - R^2 in (0, 1/2], R'(0) = 1/2

and d2E/da2 <= tau W e^2, the curvature of the quadratic majoriser - the Gaussian term's.
"""
import numpy as np

from tests import gne64, rician64, slice64, voxel64


def _e_at(e, shape, axis, dtype=np.float64):
    return np.ones((1, 1, 1), dtype) if e is None else gne64._at(np.asarray(e, np.float32).astype(dtype), shape, axis)


# ---- float64: the term and its derivatives ----------------------------------------------------------------------------------
def energy64(a, x, axis, g, u, e, tau):
    """E(a) in float64."""
    a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
    W = gne64.weight64(x.shape, axis, g, u)
    p = _e_at(e, x.shape, axis) * a
    return float(np.sum(np.where(x != 0, W * (0.5 * tau * (x - p) ** 2 + rician64.c64(tau * x * p)), 0.0)))


def resid64(a, x, axis, g, u, e, tau=1.0):
    """dE/da in float64: tau W e (p - x R(z)) where x != 0, else 0."""
    a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
    ev = _e_at(e, x.shape, axis)
    p = ev * a
    return np.where(x != 0, tau * gne64.weight64(x.shape, axis, g, u) * ev * (p - x * rician64.ratio64(tau * x * p)), 0.0)


def dratio64(z):
    """R'(z) = 1 - R / z - R^2 in float64; 1/2 - z^2 3/16 below |z| = 1e-4, where the closed form cancels (the next
    term of the series is 5 z^4 / 96: below 1e-17 there)."""
    z = np.asarray(z, np.float64)
    r = rician64.ratio64(z)
    safe = np.where(np.abs(z) < 1e-4, 1.0, z)
    return np.where(np.abs(z) < 1e-4, 0.5 - 0.1875 * z * z, 1.0 - r / safe - r * r)


def hess64(a, x, axis, g, u, e, tau):
    """d2E/da2 (diagonal) in float64: tau W e^2 (1 - tau x^2 R'(z)) where x != 0, else 0."""
    a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
    ev = _e_at(e, x.shape, axis)
    z = tau * x * ev * a
    return np.where(x != 0, tau * gne64.weight64(x.shape, axis, g, u) * ev * ev * (1.0 - tau * x * x * dratio64(z)), 0.0)


def majoriser_curvature64(x, axis, g, u, e, tau):
    """tau W e^2 where x != 0, else 0: the Hessian weight the rigid step builds (gne64.hess64; e None: 1)."""
    x = np.asarray(x, np.float64)
    ev = _e_at(e, x.shape, axis)
    return np.where(x != 0, tau * gne64.weight64(x.shape, axis, g, u) * ev * ev, 0.0)


# ---- the entry point ----------------------------------------------------------------------------------------------------------
def factor32(u, e):
    """t = fl32(fl64(u) fl64(e)) per slice, float32 - exact in float64, rounded once; the table that is there where the
    other is None; None where both are."""
    if u is None and e is None:
        return None
    if u is None or e is None:
        return np.asarray(e if u is None else u, np.float32).copy()
    return (np.asarray(u, np.float32).astype(np.float64) * np.asarray(e, np.float32).astype(np.float64)).astype(np.float32)


def resid32(x, ay, axis, g, u, e, tau):
    """``out`` of unires_rigid_terms_r by the kernel's operation sequence, float32: p, z and x~ = fl32(x R(z)) are
    rician64's; d = fl32(p - x~); then gn64.rigid_resid32's product fl32(t d) (no table: d itself) or, with g,
    voxel64.apply32's - fl32(g d) without a table, fl32(fl64(fl64(g t) d)) with one; +0 where x == 0 or p == 0, the
    mask read on the TRUE x (rigid_resid32 would read it on x~, which can underflow to 0 where x is not)."""
    x = np.asarray(x, np.float32)
    p, _ = rician64.z32(x, ay, e, tau, axis)
    xt, _ = rician64.terms32(x, ay, e, tau, axis)
    t = factor32(u, e)
    with np.errstate(all='ignore'):
        d = (p - xt).astype(np.float32)
        if g is not None:
            out = voxel64.apply32(d, g, t, axis)
        elif t is not None:
            out = (gne64._at(t, x.shape, axis) * d).astype(np.float32)
        else:
            out = d
    return np.where((x != 0) & (p != 0), out, np.float32(0.0)).astype(np.float32)


def terms_r64(x, ay, axis, g, u, e, tau):
    """The float64 statement of unires_rigid_terms_r on float32 inputs -> (out, out_bound, sums, sums_bound).

    out: t64 g (p64 - x R(z64)) with nothing rounded (tau as the float32 the kernel takes), 0 where x == 0 or the
    float32 p == 0 (the kernel's mask: e ay != 0 in float64 can round to a float32 0 only by underflow).

    out_bound: the bound on |out32 - out| that follows from rician64's cap on the float32 R (2e-6 relative) and the
    residual's roundings, eps = 2^-24, to first order with a factor 1.01 for the higher orders:
        p32 = p (1 + d1),                         |d1| <= eps           (one product; exact without e)
        z32 = z (1 + d1)(1 + d2)(1 + d3),         two products after p: R is evaluated at a z off by 3 eps relative, and
                                                  |R(z') - R(z)| <= |z' - z| R' <= 3 eps z R'(z) <= 3 eps R(z): R is
                                                  concave on z > 0 with R(0) = 0, so z R'(z) <= R(z)
        x~32 = x R32 (1 + d4),                    |x~32 - x R(z)| <= (2e-6 + 4 eps) |x R(z)|   (tests/test_rician.py's bound)
        d32 = fl32(p32 - x~32),                   |d32 - (p - x R)| <= eps |p| + (2e-6 + 4 eps) |x R| + eps |d|
        out32 = fl32(fl64(g t32) d32),            t32 = t (1 + d5): 2 eps |out| more (one rounding of t, one of the product)
    so  |out32 - out| <= 1.01 { |t g| [eps |p| + (2e-6 + 4 eps) |x R(z)|] + 3 eps |out| } + (1 + |t g|) 2^-149
    (the last term: x~ or the product may be subnormal, and then rounds to a multiple of 2^-149).  A z32 that underflows
    to 0 is outside the bound: R32 is then 0 where R(z) is not.

    sums: (3 S,) - the exact SSE and count of slice64 / voxel64 on (x, p32), then rician64.sums64's exact sums of
    fl64(g c32); sums_bound: their bounds on a float64 accumulation in any order."""
    x, ay = np.asarray(x, np.float32), np.asarray(ay, np.float32)
    p32, z32 = rician64.z32(x, ay, e, tau, axis)
    x64 = x.astype(np.float64)
    p64 = ay.astype(np.float64) * _e_at(e, x.shape, axis)
    tau32 = float(np.float32(tau))
    xr = x64 * rician64.ratio64(tau32 * x64 * p64)
    W = gne64.weight64(x.shape, axis, None if g is None else np.asarray(g, np.float32),
                       None if u is None else np.asarray(u, np.float32)) * _e_at(e, x.shape, axis)
    keep = (x != 0) & (p32 != 0)
    out = np.where(keep, W * (p64 - xr), 0.0)
    eps = 2.0 ** -24
    bound = np.where(keep, 1.01 * (np.abs(W) * (eps * np.abs(p64) + (2e-6 + 4 * eps) * np.abs(xr)) + 3 * eps * np.abs(out))
                     + (1.0 + np.abs(W)) * 2.0 ** -149, 0.0)
    if g is None:
        sse, cnt, b = slice64.slice_sums64(x, p32, axis)
        b_cnt = np.zeros_like(b)
    else:
        sse, cnt, _, b, b_cnt = voxel64.voxel_sums64(x, p32, g, axis)
    lik, b_lik, _ = rician64.sums64(rician64.c32(z32).astype(np.float64), g, axis)
    return out, bound, np.concatenate([sse, cnt, lik]), np.concatenate([b, b_cnt, b_lik])
