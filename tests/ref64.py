"""float64 reference of the y-update operator and a per-voxel error bound for float32 kernels of it.

The reference is the oracle's own composition (oracle/unires_restated.py ``proj_apply`` / ``DtD``, nitorch_restated
``grid_pull`` / ``grid_push``) evaluated in float64 on the reference's float32 grid ``affine_grid(mat.float(), dim)``
and the reference's float32 taps, both upcast: the FOV-mask and floor decisions are the reference's own, and the
reference's rounding is out of the picture.

For every output voxel v a float32 implementation must satisfy

    |out_v - ref_v| <= u c_M M_v + G_v + D_v,        u = 2^-24

- ``M_v`` = (|A| |p|)_v: the same operator with absolute taps on |p| (|A|^T |A| |p| for A^T A; the matvec adds
  rho lam^2 |D|^T |D| |p|).  A float32 chain of n roundings over terms whose absolute sum is M is off by <= n u M.
- ``G_v``: the coordinate-rounding term: sum over the axes d of the same operator with the in-bounds trilinear
  corner weights along d replaced by 1 and each grid point's value scaled by delta_d, that point's bound on its
  coordinate error along d (``coord_error``; for A^T A: |A|^T G_A(|p|) + G_At(|A| |p|)).  A coordinate off by delta
  along d moves a trilinear sample by <= delta * sum_pairs w_other (|p_lo| + |p_hi|), which is that operator.  This
  is the issue's u c_G R G made local: delta_d from the magnitudes of the partial results at the point instead of
  u c_G R everywhere, and unit weights along one axis at a time instead of all three at once times 3 axes.  Both
  are sound; the global form allows 1.6e-3 of the value in mid-size AtA and passes a 1e-3 error in a whole
  8 x 4 x 30 tile.  Where a
  coordinate lies within eta = max delta of an integer, the floor itself may differ, so the unit-weight corners
  along d are every integer in [floor(g - eta), floor(g + eta) + 1].
- ``R`` = max_i (sum_j |M_ij| (n_j - 1) + |t_i|): the magnitude of the coordinate arithmetic (reported).
- ``D_v`` = |A_dropped| |p|: the end taps ``trim_taps`` (api_plan.hip) drops, below 2^-22 sum |t|.  Zero for the rect and
  triangular profiles (their dropped taps are exact zeros); zero by construction with ``trimmed=True``, where the
  reference is built with the taps the plan uses.

The reference itself rounds in float64: its chains are the same, so every c_M u M term carries (u + 2^-53).
Without that, a voxel where the kernel returns 0 and the reference only the dropped taps' share (err = D) would
pass or fail on the last bit of two float64 sums.

Wherever M = G = D = 0 the bound is 0: the kernel must return exactly 0.0 outside the operator's footprint.

Constants (each the length of the longest float32 chain, counted per output voxel; not fitted to observations):

delta_d                                   coordinate rounding, per grid point and axis: see ``coord_error``.
C_LERP = 1                                the lerp form fmaf(w, b - a, a): (b - a) rounds by <= u (|a| + |b|) at
    each of the 3 levels, weighted by the other levels' weights: u per axis of G, carried in delta_d.
C_TAP = 6                                 the reference's dense float32 kernel (float64 product rounded once: u)
    against the kernels' product of three float32 1-D taps (3 u) formed in float32 (2 u).
C_SCALE = 2                               the slice scaling: expf (1 u) and the product (1 u).
C_PULL = 11                               trilinear sample, product form (the longest: weights w x w y w z, 2 u;
    1 - w, 1 u; weight x value, 1 u; 8 corner terms summed, 7 u); the lerp form is 3 u on M (+ C_LERP on G).
C_STORE = 3                               roundings of stored intermediates (grid-space scratch, x-space
    way station, the hybrid / separable 1-D passes' scratch).
N_TAPS                                    the conv chain: a sum of prod n_d tap products (n - 1 additions + the
    products: n u); taken as the full product even where a form runs separable passes (sum n_d + 2 <= prod n_d).
C_PUSH = 4 + K                            push: corner weight product (2 u), 1 - w (1 u), weight x value (1 u),
    and K terms accumulated into one voxel (K - 1 u, any order, + 1): K is the largest number of grid points that
    reach one voxel, counted on this geometry by the unit-weight push of ones.
C_DTD = 20                                the stencil: rho lam^2 (2 u), 1 / vx^2 (2 u), the product (1 u), the 6
    differences and their 7-term sum (13 u), tau x (AtA p) and the final add (2 u).

c_M(A)      = C_TAP + C_SCALE + C_PULL + C_STORE + N_TAPS
c_M(At)     = C_TAP + C_SCALE + C_STORE + N_TAPS + C_PUSH
c_M(AtA)    = c_M(A) + c_M(At)           (the forward error, carried by |A|^T, plus the push's own)
c_M(matvec) = c_M(AtA) + C_DTD

sett.diff = 'backward' / 'central': ``bound_matvec(..., which)`` takes D^T D and |D|^T |D| from tests/diff64.py with the
same constants (the count is in its docstring); ``bound_matvec_reps`` is the same bound over several repeats (+ 1
per accumulating store) and ``bound_rhs`` the bound of b = sum tau A^T x - lam D^T (w - rho z).
"""
import math

import torch
from torch.nn import functional as F

from oracle import nitorch_restated as N
from oracle import unires_restated as O

U = 2.0 ** -24
U64 = 2.0 ** -53  # the float64 reference's own rounding: the same chains, counted in float64 ulps
FOV_TOL = N.FOV_TOL
C_TAP = 6
C_SCALE = 2
C_PULL = 11
C_STORE = 3
C_DTD = 20
TRIM_REL = 2.384185791015625e-7  # trim_taps: |t| < 2^-22 sum |t|


def trimmed_taps(taps_1d):
    """trim_taps (api_plan.hip) restated: per axis, the leading / trailing taps below 2^-22 sum |t| (sum in double, at
    least one tap kept).  Returns per axis a 0/1 float64 mask of the taps the plan keeps."""
    keep = []
    for t in taps_1d:
        t = [float(v) for v in torch.as_tensor(t, dtype=torch.float32).tolist()]
        n = len(t)
        eps = sum(abs(v) for v in t) * TRIM_REL
        lead = trail = 0
        while lead < n - 1 and abs(t[lead]) < eps:
            lead += 1
        while trail < n - 1 - lead and abs(t[n - 1 - trail]) < eps:
            trail += 1
        m = torch.zeros(n, dtype=torch.float64)
        m[lead:n - trail] = 1.0
        keep.append(m)
    return keep


def _unit_corners(g, n, eta):
    """Per axis, the candidate corners of a coordinate whose float32 value may be off by eta: every integer in
    [floor(g - eta), floor(g + eta) + 1] (2 of them, 3 within eta of an integer), and their 0/1 validity."""
    lo = torch.floor(g - eta).long()
    hi = torch.floor(g + eta).long() + 1
    out = []
    for o in range(3):
        i = lo + o
        ok = (i <= hi) & (i >= 0) & (i < n)
        out.append((i.clamp(0, n - 1), ok))
    return out


def _weights(g, n):
    """The reference's two corners along one axis: (index, weight, 0/1 validity) each."""
    i0, i1, w1, ok0, ok1 = N._corners(g, n)
    return [(i0, 1 - w1, ok0), (i1, w1, ok1)]


def _sens_terms(grid, shape, eta, delta):
    """The corner terms of sum_d delta_d G_d: for each axis d, the widened unit-weight corners along d times the
    true weights along the other two axes, times the grid point's coordinate error bound along d.  Yields (flat
    index, weight) pairs."""
    nx, ny, nz = shape
    true = [_weights(grid[..., a], n) for a, n in enumerate(shape)]
    unit = [[(i, ok.double(), ok) for i, ok in _unit_corners(grid[..., a], n, eta)] for a, n in enumerate(shape)]
    for d in range(3):
        ax = [unit[a] if a == d else true[a] for a in range(3)]
        for ix, wx, okx in ax[0]:
            for iy, wy, oky in ax[1]:
                for iz, wz, okz in ax[2]:
                    w = wx * wy * wz * (okx & oky & okz) * delta[d]
                    yield (ix * ny + iy) * nz + iz, w


def unit_pull(inp, grid, shape, eta, delta, fov=True):
    """G of the pull: sum over the axes d of the pull with unit corner weights along d (the corner set widened by
    eta) and the true weights along the other two - the bound on |d sample / d g_d|."""
    src = inp.reshape(-1)
    acc = torch.zeros(grid.shape[:3], dtype=torch.float64)
    for idx, w in _sens_terms(grid, shape, eta, delta):
        acc += src[idx] * w
    if fov:
        acc = acc * N._fov_mask(grid, shape, FOV_TOL)
    return acc


def unit_push(val, grid, shape, eta, delta, fov=True):
    """Adjoint of unit_pull."""
    nx, ny, nz = shape
    if fov:
        val = val * N._fov_mask(grid, shape, FOV_TOL)
    val = val.reshape(-1)
    out = torch.zeros(nx * ny * nz, dtype=torch.float64)
    for idx, w in _sens_terms(grid, shape, eta, delta):
        out.index_add_(0, idx.reshape(-1), val * w.reshape(-1))
    return out.reshape(shape)


def reach_count(val, grid, shape, eta):
    """Per voxel, the sum of ``val`` over the grid points whose widened corner set touches it."""
    nx, ny, nz = shape
    val = val.reshape(-1)
    cs = [_unit_corners(grid[..., a], n, eta) for a, n in enumerate(shape)]
    out = torch.zeros(nx * ny * nz, dtype=torch.float64)
    for ix, okx in cs[0]:
        for iy, oky in cs[1]:
            for iz, okz in cs[2]:
                ok = (okx & oky & okz).reshape(-1)
                out.index_add_(0, ((ix * ny + iy) * nz + iz).reshape(-1), val * ok)
    return out.reshape(shape)


def reach_push(val, grid, shape, eta):
    """0/1 reach of a grid-space mask: every voxel any widened corner of a marked grid point touches."""
    return reach_count(val, grid, shape, eta) > 0


def orientation_of(m):
    """The canonical voxel order the plan relabels x space into (orient.hip orient_of, restated): canonical axis j
    is the x axis perm[j] of the permutation that maximises sum_j |m[j, perm[j]]| / |column perm[j]| (the identity
    keeps ties), reversed where m[j, perm[j]] < 0.  Returns (perm, flip, oriented)."""
    import itertools
    m = m.float()
    norm = [float(torch.linalg.norm(m[:3, c].double())) or 1.0 for c in range(3)]
    best, best_score = None, -1.0
    for perm in itertools.permutations(range(3)):
        score = sum(abs(float(m[j, perm[j]])) / norm[perm[j]] for j in range(3))
        if score > best_score * (1.0 + 1e-12) + 1e-12:
            best, best_score = perm, score
    flip = tuple(int(float(m[j, best[j]]) < 0) for j in range(3))
    return tuple(best), flip, tuple(best) != (0, 1, 2) or any(flip)


def coord_error(m, dim_g, grid, oriented):
    """Per grid point and axis, the bound on |float32 coordinate - reference's float32 coordinate| (in voxels),
    first order in u, from the magnitudes of the partial results (S_d = sum_j |m_dj ijk_j|, g_d, t_d):
    - the reference's grid, torch.matmul + offset in float32: 3 products / sums over S_d, the add: u (3 S_d + |g_d|);
    - the kernels' chain fmaf(c2, k, fmaf(c1, j, c0 i)) + t: the same, u (3 S_d + |g_d|) - in a reversed (canonical)
      voxel order the chain runs from the far corner: S_d up to Smax_d = sum_j |m_dj| (n_j - 1), t up to
      |t_d| + Smax_d;
    - the host's roundings of the translation: trim_taps (t + lead m, lead <= 2 here) and, reversed, canonicalise:
      u |t'| each;
    - + u for the lerp form's (b - a) (see C_LERP).
    Returns (3, *dim_g) float64."""
    ijk = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in dim_g], indexing='ij'), -1)
    out = []
    for d in range(3):
        md = m[d, :3].abs()
        S = (ijk * md).sum(-1)
        g = grid[..., d].abs()
        t = abs(float(m[d, 3]))
        smax = float(sum(float(md[j]) * (dim_g[j] - 1) for j in range(3)))
        ref = 3 * S + g
        if oriented:
            gpu = 3 * smax + g + (t + smax + 2 * float(md.sum())) * 2
        else:
            gpu = 3 * S + g + (t + 2 * float(md.sum()))
        out.append(U * (ref + gpu + 1.0))
    return torch.stack(out)


class Operator64:
    """One repeat's A (y -> x) in float64 on the reference's float32 grid, with its |A|, unit-weight and
    dropped-tap companions.  ``trimmed``: the reference's taps restricted to those the plan keeps (D = 0)."""

    def __init__(self, po, method, trimmed=False, oriented=None):
        self.method = method
        self.dim_y = tuple(po.dim_y)
        self.dim_x = tuple(po.dim_x)
        mat, dim_g = O.proj_matrix(po, method)
        self.dim_g = tuple(dim_g)
        self.grid = N.affine_grid(mat.float(), self.dim_g).double()
        m = mat.float().double()
        self.R = float(max(sum(abs(float(m[i, j])) * (self.dim_g[j] - 1) for j in range(3)) + abs(float(m[i, 3]))
                           for i in range(3)))
        self.oriented = orientation_of(m)[2] if oriented is None else bool(oriented)
        self.delta = coord_error(m, self.dim_g, self.grid, self.oriented)
        self.eta = float(self.delta.max())
        if method == 'super-resolution':
            K = po.smo_ker.double()
            keep = trimmed_taps(po.smo_ker_1d)
            kmask = keep[0][:, None, None] * keep[1][None, :, None] * keep[2][None, None, :]
            self.K_drop = (K * (1 - kmask)).abs()
            self.K = K * kmask if trimmed else K
            if trimmed:
                self.K_drop = torch.zeros_like(K)
            self.ratio = tuple(po.ratio)
            self.scl = float(po.scl)
            self.dim_thick = po.dim_thick
            self.n_taps = int(kmask.sum())
        else:
            self.K = torch.ones((1, 1, 1, 1, 1), dtype=torch.float64)
            self.K_drop = torch.zeros_like(self.K)
            self.ratio = (1, 1, 1)
            self.scl = 0.0
            self.dim_thick = 0
            self.n_taps = 1
        self.Ka = self.K.abs()
        self.has_drop = bool((self.K_drop != 0).any())
        # K: the most grid points one voxel receives (the push's accumulation length)
        g1 = torch.ones(self.dim_g, dtype=torch.float64) * N._fov_mask(self.grid, self.dim_y, FOV_TOL)
        self.K_push = int(reach_count(g1, self.grid, self.dim_y, self.eta).max().item())
        self.c_A = C_TAP + C_SCALE + C_PULL + C_STORE + self.n_taps
        self.c_At = C_TAP + C_SCALE + C_STORE + self.n_taps + 4 + self.K_push
        self.c_AtA = self.c_A + self.c_At

    # -- pieces ---------------------------------------------------------------------------------------------------
    def _scale(self, x, s):
        if s == 0:
            return x
        return O.apply_scaling(x, torch.tensor(s, dtype=torch.float32).double(), self.dim_thick)

    def _conv(self, g, K):
        return F.conv3d(g[None, None], K, stride=self.ratio)[0, 0]

    def _conv_t(self, x, K):
        return F.conv_transpose3d(x[None, None], K, stride=self.ratio)[0, 0]

    def _pull(self, p):
        return N.grid_pull(p[None, None], self.grid[None], bound='zero', extrapolate=False)[0, 0]

    def _push(self, g):
        return N.grid_push(g[None, None], self.grid[None], shape=self.dim_y, bound='zero', extrapolate=False)[0, 0]

    # -- operators (float64) --------------------------------------------------------------------------------------
    def A(self, p, K=None, unit=False):
        K = self.K if K is None else K
        g = unit_pull(p, self.grid, self.dim_y, self.eta, self.delta) if unit else self._pull(p)
        return self._scale(self._conv(g, K), self.scl)

    def At(self, v, K=None, unit=False):
        K = self.K if K is None else K
        g = self._conv_t(self._scale(v, self.scl), K)
        return unit_push(g, self.grid, self.dim_y, self.eta, self.delta) if unit else self._push(g)

    # -- reference + bound ----------------------------------------------------------------------------------------
    def bound_A(self, p):
        """(ref, tol) of A p, over x space."""
        p = p.double()
        pa = p.abs()
        ref = self.A(p)
        M = self.A(pa, self.Ka)
        G = self.A(pa, self.Ka, unit=True)
        D = self.A(pa, self.K_drop) if self.has_drop else 0.0
        return ref, (U + U64) * self.c_A * M + G + D

    def bound_At(self, v):
        v = v.double()
        va = v.abs()
        ref = self.At(v)
        M = self.At(va, self.Ka)
        G = self.At(va, self.Ka, unit=True)
        D = self.At(va, self.K_drop) if self.has_drop else 0.0
        return ref, (U + U64) * self.c_At * M + G + D

    def parts_AtA(self, p):
        """(ref, M, G, D) of A^T A p."""
        p = p.double()
        pa = p.abs()
        ref = self.At(self.A(p))
        MA = self.A(pa, self.Ka)
        M = self.At(MA, self.Ka)
        G = self.At(self.A(pa, self.Ka, unit=True), self.Ka) + self.At(MA, self.Ka, unit=True)
        if self.has_drop:
            DA = self.A(pa, self.K_drop)
            D = self.At(DA, self.Ka) + self.At(MA, self.K_drop)
        else:
            D = torch.zeros_like(ref)
        return ref, M, G, D

    def bound_AtA(self, p):
        ref, M, G, D = self.parts_AtA(p)
        return ref, (U + U64) * self.c_AtA * M + G + D

    def bound_matvec(self, p, tau, rho, lam, vx, which='forward'):
        """q = tau A^T A p + rho lam^2 D^T D p with the float32 tau, rho, lam, vx the kernels see, upcast.

        ``which`` = 'backward' / 'central' (sett.diff): D^T D from tests/diff64.py, Md = c |D|^T |D| |p| with the same
        difference, and the same form of bound, (u + 2^-53) (c_AtA + C_DTD) (tau M + Md) + tau (G + D).  The count
        carries over: a non-forward plan runs A^T A on its usual kernel without a stencil epilogue - that chain,
        c_AtA, already ends in the float32 store of tau A^T A p - and a second pass loads the stored value where a
        forward epilogue forms a0 p, and adds c D^T D p to it once: the load is exact, and the add is the "final add"
        of C_DTD, which also counts a product (a x p) that this pass does not form.  The stencil's own chain (c, 1 /
        vx^2, their product, the six differences and the seven-term sum) is forward's term for term: central's 1/4 is
        a power of two.  See ``bound_matvec_reps`` (this is its one-repeat case)."""
        if which != 'forward':
            return bound_matvec_reps([self], [tau], p, rho, lam, vx, which)
        tau, rho, lam = (float(torch.tensor(float(v), dtype=torch.float32)) for v in (tau, rho, lam))
        vx = torch.as_tensor(vx, dtype=torch.float32).double()
        ref, M, G, D = self.parts_AtA(p)
        c = rho * lam * lam
        p64 = p.double()
        ref = tau * ref + c * O.DtD(p64, vx)
        Md = c * dtd_abs(p64.abs(), vx)
        tol = (U + U64) * (self.c_AtA + C_DTD) * (tau * M + Md) + tau * G + tau * D
        return ref, tol

    # -- FOV ties -------------------------------------------------------------------------------------------------
    def tie_masks(self, po):
        """Voxels a grid point within 2 eta of an in-FOV threshold can reach (eta = the largest coordinate error
        bound: the reference's and the kernel's float32 coordinates may fall on either side): (x-space mask for A,
        y-space mask for A^T, y-space mask for A^T A, number of near grid points)."""
        from tests.helpers import fov_near_points
        _, near = fov_near_points(po, self.method, self.dim_y, 2 * self.eta)
        nf = near.double()
        ones = torch.ones_like(self.Ka)
        mx = F.conv3d(nf[None, None], ones, stride=self.ratio)[0, 0] > 0
        my = reach_push(nf, self.grid, self.dim_y, self.eta)
        # A^T A: every grid point that reads a tied x voxel pushes a changed value
        gx = F.conv_transpose3d(mx.double()[None, None], ones, stride=self.ratio)[0, 0]
        myy = my | reach_push(gx, self.grid, self.dim_y, self.eta)
        return mx, my, myy, int(near.sum())


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def bound_matvec_reps(ops, taus, p, rho, lam, vx, which='forward', parts=None):
    """(ref, tol) of q = sum_n tau_n A_n^T A_n p + rho lam^2 D^T D p over the repeats ``ops`` of one channel, D taking
    the difference ``which`` (tests/diff64.py).

        tol = (u + 2^-53) (c_AtA + C_DTD + nrep - 1) (sum_n tau_n M_n + Md) + sum_n tau_n (G_n + D_n)

    ``Operator64.bound_matvec``'s form with M, G and D summed over the repeats with their tau, and c_AtA the longest of
    the repeats' chains.  The stencil goes in once (a forward plan adds it in the first repeat's epilogue, a
    non-forward one in the closing pass), so Md = c |D|^T |D| |p| appears once.  Every repeat after the first adds its
    term to the stored q: one more rounding of the running sum per accumulating store, nrep - 1 in all.  With one
    repeat this is ``Operator64.bound_matvec``'s bound.  Voxels to leave out: the union of the repeats' ``myy``
    (``tie_masks``).
    ``parts``: the repeats' ``parts_AtA(p)`` where the caller has them already (they do not depend on ``which``)."""
    from tests import diff64
    rho, lam = _f32(rho), _f32(lam)
    taus = [_f32(t) for t in taus]
    vx = [float(v) for v in torch.as_tensor(vx, dtype=torch.float32).double()]
    if parts is None:
        parts = [op.parts_AtA(p) for op in ops]
    c_m = max(op.c_AtA for op in ops) + C_DTD + len(ops) - 1
    c = rho * lam * lam
    p64 = p.double().numpy()
    ref = c * torch.from_numpy(diff64.dtd(p64, vx, which))
    mag = c * torch.from_numpy(diff64.dtd_abs(p64, vx, which))  # Md, then + sum tau M
    rest = torch.zeros_like(mag)
    for tau, (r, M, G, D) in zip(taus, parts):
        ref = ref + tau * r
        mag = mag + tau * M
        rest = rest + tau * G + tau * D
    return ref, (U + U64) * c_m * mag + rest


C_RHS = 3  # on top of diff64.C_DIV: the product rho z, the subtraction w - rho z, the product with lam


def bound_rhs(ops, taus, x_list, w, z, rho, lam, vx, which='forward', at=None):
    """(ref, tol) of b = sum_n tau_n A_n^T x_n - lam D^T (w - rho z) (unires_rhs_assemble), D^T the transpose of the
    difference ``which``; w, z: (3, *dim_y).  An entry None of ``ops`` is A = I.

    The chain, counted: g = w - rho z costs a product and a subtraction (2 u on |w| + rho |z|); the divergence of g
    is diff64's chain (C_DIV = 5 on |D|^T (|w| + rho |z|)); the product with lam 1 more; then every repeat adds
    tau_n A_n^T x_n to the stored b, nrep roundings of the running sum:

        tol = (u + 2^-53) (C_DIV + 3 + nrep) lam |D|^T (|w| + rho |z|)
              + sum_n tau_n tol_n + (u + 2^-53) (1 + nrep) tau_n (|ref_n| + tol_n)

    with (ref_n, tol_n) = ``Operator64.bound_At(x_n)``: the push's own chain, then the product with tau_n (1) and at
    most nrep accumulating adds, on the magnitude of the value those act on, at most |ref_n| + tol_n.  Voxels to
    leave out: the union of the repeats' ``my`` (``tie_masks``).
    ``at``: the repeats' (ref_n, tol_n) where the caller has them already (they do not depend on ``which``)."""
    from tests import diff64
    rho, lam = _f32(rho), _f32(lam)
    taus = [_f32(t) for t in taus]
    vx = [float(v) for v in torch.as_tensor(vx, dtype=torch.float32).double()]
    nrep = len(ops)
    if at is None:
        at = [(x.double(), torch.zeros(tuple(x.shape), dtype=torch.float64)) if op is None else op.bound_At(x)
              for op, x in zip(ops, x_list)]
    w64, z64 = w.double().numpy(), z.double().numpy()
    s = diff64.inv_vx(vx)
    g = w64 - rho * z64
    ga = abs(w64) + rho * abs(z64)
    div = sum(diff64._apply(g[d], d, which, True, False) * s[d] for d in range(3))
    mag = sum(diff64._apply(ga[d], d, which, True, True) * s[d] for d in range(3))
    ref = -lam * torch.from_numpy(div)
    tol = (U + U64) * (diff64.C_DIV + C_RHS + nrep) * lam * torch.from_numpy(mag)
    for tau, (r, t) in zip(taus, at):
        ref = ref + tau * r
        tol = tol + tau * t + (U + U64) * (1 + nrep) * tau * (r.abs() + t)
    return ref, tol


def dtd_abs(pa, vx):
    """|D|^T |D| |p| for the forward-difference gradient with zero bound (oracle im_gradient / im_divergence with
    absolute coefficients)."""
    out = torch.zeros_like(pa)
    for d in range(3):
        n = pa.shape[d]
        nxt = torch.zeros_like(pa)
        sl = [slice(None)] * 3
        src = [slice(None)] * 3
        sl[d], src[d] = slice(0, n - 1), slice(1, n)
        nxt[tuple(sl)] = pa[tuple(src)]
        # |g_d|[i] <= (|p[i+1]| + |p[i]|) / vx (|p[i]| alone at the last index: p[n] = 0); the divergence takes
        # g_d[i - 1] and g_d[i]
        g = (nxt + pa) / float(vx[d])
        gp = torch.zeros_like(g)
        gp[tuple(src)] = g[tuple(sl)]
        out += (g + gp) / float(vx[d])
    return out


def compare(out, ref, tol, exclude=None):
    """Per-voxel check.  Returns dict(ok, worst err / tol ratio, count of violations, excluded count, first
    violation index).  tol == 0 demands out == 0.0 exactly (outside the footprint)."""
    out = out.double()
    err = (out - ref.double()).abs()
    keep = torch.ones_like(err, dtype=torch.bool) if exclude is None else ~exclude
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    bad = (err > tol) & keep
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                         torch.zeros_like(err)))
    ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
    first = None
    if bad.any():
        first = tuple(int(v) for v in torch.nonzero(bad)[0].tolist())
    return dict(ok=not bool(bad.any()), max_ratio=float(ratio.max()), n_bad=int(bad.sum()),
                excluded=0 if exclude is None else int(exclude.sum()), first=first,
                first_err=None if first is None else float(err[first]),
                first_tol=None if first is None else float(tol[first]))
