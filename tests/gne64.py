"""numpy restatement of the slice gains in the rigid Gauss-Newton update (sett.gain_gn): the per-slice
tables, the gained prediction, the float32 residual and the exact slice sums of unires_rigid_terms_e, the rule the
gains are decimated by, and the data term with its first and second derivative in float64.  Built on tests/gain64.py
(the tables), tests/gn64.py and tests/gnv64.py (the residual's roundings), tests/slice64.py and tests/voxel64.py (the
sums and their bound); the reference has no counterpart, so nothing here is pinned against it.

The data term of a gained repeat is E(a) = 1/2 tau sum_v W(v) [x(v) != 0] (x(v) - e[s(v)] a(v))^2 with a = A y,
W = g u[s(v)] (g a float32 volume or None = 1, u float32 per slice along ``axis`` or None = 1), e float32 per slice.
"""
import numpy as np

from tests import gain64, gn64, gnv64, slice64, voxel64


def tables(u, e):
    """(w_mat, w_rhs, t) float32: gain64.compose32's two tables - w_mat = fl32(fl64(fl64(u e) e)) is the Hessian's slice
    factor, w_rhs = fl32(fl64(u e)) - and the residual's slice factor t, which is w_rhs: u e is exact in float64 and
    rounded to float32 once (u None: t = e)."""
    w_mat, w_rhs = gain64.compose32(u, e)
    return w_mat, w_rhs, w_rhs.copy()


def _at(v, shape, axis):
    view = [1, 1, 1]
    view[axis] = int(shape[axis])
    v = np.asarray(v)
    assert v.shape == (shape[axis],)
    return v.reshape(view)


def gained32(ay, e, axis):
    """p = fl32(e[s(v)] ay(v)): one float32 product per voxel, unires_slice_apply's."""
    ay = np.asarray(ay, np.float32)
    return (_at(np.asarray(e, np.float32), ay.shape, axis) * ay).astype(np.float32)


def terms_e32(x, ay, axis, g, u, e):
    """(out, sums, bound) of unires_rigid_terms_e.  out: the float32 residual with the kernel's roundings, bit for bit -
    gn64.rigid_resid32 (g None) or gnv64.rigid_resid_g32 on the gained prediction p with t in the place of u.  sums:
    (2 S,) float64, the exact per-slice sums of the float32 terms on p (slice64.slice_sums64, or voxel64.voxel_sums64
    with g) and the count / effective count; bound: (2 S,) the bound on their float64 accumulation in any order,
    N_s 2^-53 sum |term| (1 + N_s 2^-53) - 0 for a count of integers, which float64 holds exactly."""
    x = np.asarray(x, np.float32)
    p = gained32(ay, e, axis)
    t = tables(u, e)[2]
    if g is None:
        out = gn64.rigid_resid32(x, p, axis, t)
        sse, cnt, b = slice64.slice_sums64(x, p, axis)
        return out, np.concatenate([sse, cnt]), np.concatenate([b, np.zeros_like(b)])
    out = gnv64.rigid_resid_g32(x, p, axis, g, t)
    sse, gs, _, b_sse, b_gs = voxel64.voxel_sums64(x, p, g, axis)
    return out, np.concatenate([sse, gs]), np.concatenate([b_sse, b_gs])


def decimate_gain(e, sk, n):
    """The gains on the decimated lattice of the rigid update: every sk-th slice from the first, cut to n - the rule
    the observation's slices (and its slice weights) are decimated by."""
    return np.ascontiguousarray(np.asarray(e)[::int(sk)][:int(n)])


def weight64(shape, axis, g, u):
    """W = g u[s(v)] as a float64 volume (either factor 1 where None)."""
    W = np.ones(tuple(shape), np.float64)
    if g is not None:
        W = W * np.asarray(g, np.float64)
    if u is not None:
        W = W * _at(np.asarray(u, np.float64), shape, axis)
    return W


def energy64(a, x, axis, g, u, e, tau=1.0):
    """E(a) in float64: 1/2 tau sum_v W [x != 0] (x - e[s(v)] a)^2."""
    a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
    W = weight64(x.shape, axis, g, u)
    r = x - _at(np.asarray(e, np.float64), x.shape, axis) * a
    return 0.5 * float(tau) * float(np.sum(np.where(x != 0, W * r * r, 0.0)))


def resid64(a, x, axis, g, u, e, tau=1.0):
    """dE/da in float64: tau W e (e a - x) where x != 0, else 0 - the factor e is the chain rule through diag(e)."""
    a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
    ev = _at(np.asarray(e, np.float64), x.shape, axis)
    return np.where(x != 0, float(tau) * weight64(x.shape, axis, g, u) * ev * (ev * a - x), 0.0)


def hess64(x, axis, g, u, e, tau=1.0):
    """d2E/da2 (diagonal) in float64: tau W e^2 where x != 0, else 0."""
    x = np.asarray(x, np.float64)
    ev = _at(np.asarray(e, np.float64), x.shape, axis)
    return np.where(x != 0, float(tau) * weight64(x.shape, axis, g, u) * ev * ev, 0.0)
