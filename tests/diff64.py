"""float64 restatement of the regulariser's difference operators for the three values of ``sett.diff`` / nitorch's
``which`` - D (``gradient``), D^T (``divergence``, the positive transpose) and D^T D (``dtd``) - with their
absolute-value companions and the per-voxel bounds a float32 kernel of them must meet.

Definitions (zero bound: samples outside the volume read as 0; per axis d, n = dim_d).  They are restated from
nitorch's published ``diff1d`` / ``div1d``  [recalled]: nitorch is not available to this project, so parity at this
boundary is unpinned, like the rest of the nitorch boundary.

    which       (D y)[i]                        (D^T g)[i]
    forward     (y[i+1] - y[i]) / vx            (g[i-1] - g[i]) / vx
    backward    (y[i] - y[i-1]) / vx            (g[i] - g[i+1]) / vx
    central     (y[i+1] - y[i-1]) / (2 vx)      (g[i-1] - g[i+1]) / (2 vx)

One table states all of it: row i of D has the coefficients ``COEF[which]`` = {offset: c} at columns i + offset
(where in range), over vx; row i of D^T then has c at column i - offset.  The absolute-value companions |D|, |D|^T
and |D|^T |D| take |c|: they are what a chain of float32 roundings is counted against.

Everything is computed in float64 from the float32 inputs the kernel reads, with the float32 constants the kernel
forms once taken as they are.  u = 2^-24; every bound carries (u + 2^-53): the reference rounds the same chains in
float64.

Bounds (lengths of the longest float32 chain, counted per output voxel; none is fitted to an observation):

- ``grad64`` / ``gradient``: one difference and one product on s_d = fl(lam fl(1 / vx_d)) (central's 1/2 is a power
  of two: folded into s_d exactly) - 2 u in the kernel, 5 u against the float32 oracle's difference, / vx, x lam and
  its own scale: tests/admm64.py's C_G = 5 on |Dy|_A = (|y[upper]| + |y[lower]|) s_d, with (upper, lower) =
  (i+1, i), (i, i-1), (i+1, i-1).  ``grad64`` has admm64.grad64's signature with ``which`` added, so admm64's
  ``zw_update`` / ``nll_prior`` run unchanged - bounds included - on a generalised gradient.
- ``divergence``: per axis a difference and a product on fl(1 / vx_d) (2 u on that axis' absolute term), the
  three-term sum (2 more on terms that pass through both additions): a chain of 4, and (1 + u)^4 - 1 < 5 u:
  C_DIV = 5 on sum_d (|g_d[a]| + |g_d[b]|) fl(1 / vx_d) h, h = 1/2 for central.
- ``dtd``: the constant tests/test_gpu_voxelwise.py uses for q = a p + c DtD p, ref64.C_DTD + 2 (the stencil's 20:
  c in 2, 1 / vx^2 in 2, their product 1, the six differences and their seven-term sum 13, a x p and the final add
  2; + 2 for forming c = rho lam^2 and tau from float32 inputs), on |a| |p| + c |D|^T |D| |p| - ``dtd_abs``,
  ref64.dtd_abs generalised over ``which``.  Central's weight c / (4 vx^2) differs from c / vx^2 by a power of two
  and its stencil has as many terms (two per axis), so the count carries over.
"""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
UU = U + U64
C_G = 5
C_DIV = 5
C_DTD = 20 + 2

WHICH = ('forward', 'backward', 'central')
# row i of D: coefficient c at column i + offset, over vx
COEF = {'forward': {1: 1.0, 0: -1.0}, 'backward': {0: 1.0, -1: -1.0}, 'central': {1: 0.5, -1: -0.5}}


def coef(which):
    try:
        return COEF[which]
    except (KeyError, TypeError):
        raise ValueError("which must be 'forward', 'backward' or 'central', not %r" % (which,)) from None


def shifted(y, d, k):
    """out[i] = y[i + k] along axis d, 0 where i + k is outside the volume."""
    y = np.asarray(y, dtype=np.float64)
    out = np.zeros_like(y)
    n = y.shape[d]
    if abs(k) >= n:
        return out
    to, frm = [slice(None)] * y.ndim, [slice(None)] * y.ndim
    to[d] = slice(max(0, -k), n - max(0, k))
    frm[d] = slice(max(0, k), n - max(0, -k))
    out[tuple(to)] = y[tuple(frm)]
    return out


def _apply(y, d, which, transpose, absolute):
    """(D y) or (D^T y) along axis d, without the 1 / vx; absolute: with |coefficients| (y is then |y|)."""
    out = 0.0
    for off, c in coef(which).items():
        out = out + (abs(c) if absolute else c) * shifted(y, d, -off if transpose else off)
    return out


def f32(v):
    return float(np.float32(v))


def inv_vx(vx):
    """fl(1 / vx_d): what the kernels form once per axis."""
    return [float(np.float32(1.0) / np.float32(v)) for v in vx]


def grad64(y, s, which):
    """(Dy, |Dy|_A), (3, *dim) float64 each, for the float32-formed scales s_d (lam / vx_d, tests/admm64.py
    ``grad_scales``): admm64.grad64 for any ``which``."""
    y64 = np.asarray(y, dtype=np.float64)
    g = [_apply(y64, d, which, False, False) * s[d] for d in range(3)]
    ga = [_apply(np.abs(y64), d, which, False, True) * s[d] for d in range(3)]
    return np.stack(g), np.stack(ga)


def gradient(y, vx, which):
    """(ref, tol) of im_gradient(y, vx, which): (3, *dim)."""
    g, ga = grad64(y, inv_vx(vx), which)
    return g, UU * C_G * ga


def divergence(g3, vx, which):
    """(ref, tol) of im_divergence(g3, vx, which), g3 (3, *dim)."""
    s = inv_vx(vx)
    g3 = np.asarray(g3, dtype=np.float64)
    ref = sum(_apply(g3[d], d, which, True, False) * s[d] for d in range(3))
    mag = sum(_apply(np.abs(g3[d]), d, which, True, True) * s[d] for d in range(3))
    return ref, UU * C_DIV * mag


def _vx64(vx):
    return [float(np.float32(v)) for v in vx]


def dtd(p, vx, which):
    """D^T D p summed over the axes, float64 (vx: the float32 values, upcast)."""
    p = np.asarray(p, dtype=np.float64)
    vx = _vx64(vx)
    return sum(_apply(_apply(p, d, which, False, False), d, which, True, False) / (vx[d] * vx[d]) for d in range(3))


def dtd_abs(pa, vx, which):
    """|D|^T |D| |p|: ref64.dtd_abs for any ``which``."""
    pa = np.abs(np.asarray(pa, dtype=np.float64))
    vx = _vx64(vx)
    return sum(_apply(_apply(pa, d, which, False, True), d, which, True, True) / (vx[d] * vx[d]) for d in range(3))


def a_plus_c_dtd(p, vx, which, a, c):
    """(ref, tol) of a p + c DtD p for float32 a, c."""
    p64 = np.asarray(p, dtype=np.float64)
    a, c = f32(a), f32(c)
    ref = a * p64 + c * dtd(p64, vx, which)
    return ref, UU * C_DTD * (abs(a) * np.abs(p64) + abs(c) * dtd_abs(p64, vx, which))


def dense_1d(n, vx, which, transpose=False):
    """The n x n matrix of D (or D^T) along one axis, from the same table (tests/test_diff.py checks it against
    matrices written out from the definitions)."""
    M = np.zeros((n, n))
    for i in range(n):
        for off, c in coef(which).items():
            if 0 <= i + off < n:
                M[i, i + off] = c / vx
    return M.T.copy() if transpose else M


def dense_dtd(dim, vx, which):
    """The dense float64 matrix of D^T D on a (small) volume, C order: sum_d I x .. x D_d^T D_d x .. x I."""
    vx = _vx64(vx)
    A = np.zeros((int(np.prod(dim)),) * 2)
    for d in range(3):
        D = dense_1d(dim[d], vx[d], which)
        f = [np.eye(dim[0]), np.eye(dim[1]), np.eye(dim[2])]
        f[d] = D.T @ D
        A += np.kron(np.kron(f[0], f[1]), f[2])
    return A
