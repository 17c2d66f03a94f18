"""float64 references and per-voxel / per-sum error bounds for the kernels that follow the y-update in every ADMM
and Gauss-Newton iteration (admm.hip): the z / w update with its joint-TV shrinkage image (k_jtv_scale,
k_zw_update), the prior term of the objective (unires_nll_prior), the masked likelihood sum (k_masked_sse), the
slice-scaling sums (k_scaling_sums), the rigid Gauss-Newton sums (k_rigid_sums), the field-of-view cleaner
(k_clean_fov) and the gradient of the trilinear pull the rigid sums are fed with (k_pull_grad, ``pull_grad``: its
bound is derived in its own docstring).

Every reference is computed in float64 from the same float32 inputs the kernel reads, with the float32 constants
the kernel forms once taken as they are: the gradient scale s_d = fl(lam fl(1 / vx_d)), alpha, and the 1e-7 of the
shrinkage.  u = 2^-24; every count below is the length of the longest float32 chain of the kernel or of the
float32 oracle (oracle/unires_restated.py ``update_zw`` / ``compute_nll``), whichever is longer; every bound
carries (u + 2^-53) so that the reference's own float64 rounding of the same chain is covered.

z / w update, per voxel v, channel c, axis d (``zw_update``):

- Dy = (y[v + e_d] - y[v]) s_d (zero bound).  Kernel: difference and product, 2 u; oracle: difference, / vx,
  x lam, 3 u, plus its lam / vx against s_d, 2 u: C_G = 5 on |Dy|_A = (|y[v + e_d]| + |y[v]|) s_d.
- alpha != 1: g = alpha Dy + (1 - alpha) z_old: (1 - alpha), two products and the sum, 3 more on
  |g|_A = |alpha| |Dy|_A + |1 - alpha| |z_old|.
- u = w / rho + g: the kernel's fl(1 / rho) (2 u: the division is counted as twice a correctly rounded one), the
  product and the sum: 4 more on |u|_A = |w| / rho + |g|_A, so C_U = C_G + 4 with alpha = 1 and C_U = C_G + 3 + 4
  with alpha != 1.
- n = sqrt(sum_c,d u^2): | ||u^|| - ||u|| | <= ||u^ - u|| <= C_U u n_A, n_A = sqrt(sum |u|_A^2); the 3 C squares
  and their 3 C additions (one per term, the chained launches of more than 8 channels store and reload the float32
  running sum exactly) perturb n^2 by (3 C + 1) u relative, n by half of it; the square root 2 u:
  dn = (C_U + (3 C + 1) / 2 + 2) u n_A.
- s = max(n - 1 / rho, 0) / (n + 1e-7) is continuous at the kink, with |ds / dn| <= 1 / (n + 1e-7) (for
  n > 1 / rho: (1 / rho + 1e-7) / (n + 1e-7)^2 <= 1 / (n + 1e-7)), so no tie mask: the kernel's s is within
  (dn + u (n + 2 / rho)) / ((n - dn)^+ + 1e-7) + 4 u s of the reference (the fl(1 / rho) in the numerator, the
  subtraction, the sum and the division).
- z = s u: ds |u|_A + s (C_U + 1) u |u|_A.
- w' = w + rho (g - z): rho (dg + dz) + 3 u (|w| + rho (|g|_A + s |u|_A)), dg = C_U - 4 on |g|_A.

The prior term (``nll_prior``): the kernel runs the same shrinkage pass with w = 0 and alpha = 1 and adds the
per-voxel n (float32) into float64 sums: |out - sum n| <= sum dn (C_U -> C_G) + the float64 summation slack.

float64 summation slack (``depth``): a term that passes through k float64 additions is off by <= k 2^-53 of the
sum of |term| (first order).  The reductions here are a per-lane loop over the lane's share (ceil(n / stride)
additions), block_sum (a 6-level wave tree and 4 waves in sequence: 10), k_sum_cols (ceil(blocks / 256) per lane,
then block_sum again: + 10): depth = ceil(n / stride) + ceil(blocks / 256) + 21.  The references are exact sums
(math.fsum), so that depth is the whole tolerance.

``masked_sse`` and ``scaling_sums`` pin their float32 terms (__fsub_rn / __fmul_rn; a plain float32 subtraction
rounds the same way): NumPy's float32 operations round each term identically, so the per-term values are exact and
the only slack is the summation's.  'even' is index 1::2 along dim_thick, 'odd' 0::2, as in the reference.

``rigid_sums`` forms everything in float64 from float32 inputs: the affine terms a_qd = D_q[d, :3] . (i, j, k) +
D_q[d, 3] (3 additions), s_q = sum_d g_d a_qd (3 products, 2 additions), the gradient df s_q (1 more) and the
Hessian c s_a s_b (2 products on two s): at most 14 float64 roundings per term on the absolute-value form of the
term, as many again for the reference's own float64 chain, plus the depth of the sum: tol = (28 + depth) 2^-53
sum |term|_A (about 1e-14 of the sum at the shapes
tested: far below the 1e-12 the float32 inputs would allow, and still exact enough to see one wrong voxel).

``clean_fov``: y[v] = 0 where the float32 chain fmaf(m2, k, fmaf(m1, j, m0 i)) + m3 falls outside [0, n) on any
axis.  Its error is <= u (|a0| + |a1| + |a2| + |g|) with a0 = m0 i, a1 = a0 + m1 j, a2 = a1 + m2 k, g = a2 + m3;
voxels whose float64 coordinate lies within that of 0 or n on some axis are ties, the rest must be exact: 0.0
where outside, the input's bits where inside.  A row whose entries are multiples of 2^-8 with every partial below
2^16 is computed exactly in float32 (no tie band): the integer-shift geometries test the thresholds themselves.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
UU = U + U64
EPS_S = float(np.float32(1e-7))  # the 1e-7 of the shrinkage, as a float32 constant
C_G = 5
C_ALPHA = 3
C_W = 4


# -- helpers ------------------------------------------------------------------------------------------------------
def f32(v):
    return float(np.float32(v))


def grad_scales(lam, vx):
    """s_d = fl(lam fl(1 / vx_d)): the scale the kernels form once per channel and axis."""
    ivx = [np.float32(1.0) / np.float32(v) for v in vx]
    return [float(np.float32(np.float32(lam) * i)) for i in ivx]


def _fwd(y, d):
    """y[v + e_d], zero at the last index, as float64."""
    y = np.asarray(y, dtype=np.float64)
    out = np.zeros_like(y)
    sl_to = [slice(None)] * 3
    sl_from = [slice(None)] * 3
    sl_to[d], sl_from[d] = slice(0, -1), slice(1, None)
    out[tuple(sl_to)] = y[tuple(sl_from)]
    return out


def grad64(y, s):
    """(Dy, |Dy|_A): (3, *dim) each, float64."""
    y64 = np.asarray(y, dtype=np.float64)
    g, ga = [], []
    for d in range(3):
        nxt = _fwd(y64, d)
        g.append((nxt - y64) * s[d])
        ga.append((np.abs(nxt) + np.abs(y64)) * s[d])
    return np.stack(g), np.stack(ga)


def jtv_grid(dim):
    """k_jtv_scale's launch (admm.hip jtv_grid): (z patches, y patches, x slots)."""
    tz, ty = -(-dim[2] // 64), -(-dim[1] // 4)
    gx = min(dim[0], max(1, 4096 // (tz * ty)))
    if tz * ty * gx > 65535 * 16:
        gx = 1
    return tz, ty, gx


def depth(n_lane, blocks):
    """Additions a term passes through in a per-lane loop of n_lane terms, block_sum and k_sum_cols."""
    return n_lane + -(-blocks // 256) + 21


# -- z / w update and the prior term -----------------------------------------------------------------------------
def zw_inputs(dim, C, rho, alpha=1.0, seed=5, vx=(1.0, 1.0, 1.0)):
    """y (C, *dim), lam (C,), z, w (C, 3, *dim) float32 with the joint norm n on either side of 1 / rho: u is
    linear in (lam, z, w), so one rescale of the three puts the median of n at 1 / rho."""
    g = torch.Generator().manual_seed(seed)
    ys = (torch.rand((C,) + tuple(dim), generator=g) * 100.0).float()
    lam = [0.3 / (rho * 100.0 * math.sqrt(3 * C)) * (1 + 0.3 * (c % 3)) for c in range(C)]
    z = torch.randn((C, 3) + tuple(dim), generator=g, dtype=torch.float64) * 0.4 / (rho * math.sqrt(3 * C))
    w = torch.randn((C, 3) + tuple(dim), generator=g, dtype=torch.float64) * 0.8 / math.sqrt(3 * C)
    n = zw_update(ys.numpy(), lam, vx, rho, alpha, z.float().numpy(), w.float().numpy())['n']
    f = 1.0 / (f32(rho) * float(np.median(n)))
    return ys, [f32(v * f) for v in lam], (z * f).float(), (w * f).float()


def zw_update(ys, lams, vx, rho, alpha, z, w):
    """float64 z / w update from float32 inputs: ys (C, *dim), lams (C,), vx (3,), z, w (C, 3, *dim).  Returns
    dict: 's' = (ref, tol) of the shrinkage image, 'n' the joint norm, and 'chan', a function of the channel c that
    returns dict(z=(ref, tol), w=(ref, tol)) of that channel's (3, *dim) z and w (one channel at a time: the
    volumes of all channels at once in float64 take several GB at the largest shapes tested)."""
    C = len(ys)
    rho32 = f32(rho)
    a = f32(alpha)
    c_g = C_G + (C_ALPHA if a != 1.0 else 0)
    c_u = c_g + C_W

    def parts(c):
        g, ga = grad64(ys[c], grad_scales(lams[c], vx))
        w64 = np.asarray(w[c], dtype=np.float64)
        if a != 1.0:
            z64 = np.asarray(z[c], dtype=np.float64)
            g = a * g + (1.0 - a) * z64
            ga = abs(a) * ga + abs(1.0 - a) * np.abs(z64)
        return g, ga, w64, w64 / rho32 + g, np.abs(w64) / rho32 + ga

    n2 = na2 = 0.0
    for c in range(C):
        _, _, _, u, ua = parts(c)
        n2 = n2 + (u * u).sum(0)
        na2 = na2 + (ua * ua).sum(0)
    n, na = np.sqrt(n2), np.sqrt(na2)
    del n2, na2
    dn = UU * (c_u + (3 * C + 1) / 2 + 2) * na
    irho = 1.0 / rho32
    s = np.maximum(n - irho, 0.0) / (n + EPS_S)
    ds = (dn + UU * (n + 2 * irho)) / (np.maximum(n - dn, 0.0) + EPS_S) + 4 * UU * s
    sp = s + ds

    def chan(c):
        g, ga, w64, u, ua = parts(c)
        zr = s * u
        dz = ds * ua + sp * (c_u + 1) * UU * ua
        wr = w64 + rho32 * (g - zr)
        dw = rho32 * (c_g * UU * ga + dz) + 3 * UU * (np.abs(w64) + rho32 * (ga + sp * ua))
        return dict(z=(zr, dz), w=(wr, dw))

    return dict(s=(s, ds), n=n, chan=chan)


def nll_prior(ys, lams, vx):
    """(ref, tol) of sum_v sqrt(sum_c |lam_c D y_c|^2) (float64 out of a float32 per-voxel norm)."""
    C = len(ys)
    n2 = 0.0
    na2 = 0.0
    for c in range(C):
        g, ga = grad64(ys[c], grad_scales(lams[c], vx))
        n2 = n2 + (g * g).sum(0)
        na2 = na2 + (ga * ga).sum(0)
    n, na = np.sqrt(n2), np.sqrt(na2)
    dim = np.shape(ys[0])
    tz, ty, gx = jtv_grid(dim)
    dep = depth(-(-dim[0] // gx), tz * ty * gx)
    tol = UU * (C_G + (3 * C + 1) / 2 + 2) * math.fsum(na.ravel().tolist()) + (dep + 1) * U64 * float(na.sum())
    return math.fsum(n.ravel().tolist()), tol


# -- float64 sums of exact float32 terms -------------------------------------------------------------------------
def masked_sse_blocks(n):
    return max(1, min(512, -(-n // 256)))


def masked_sse(x, ay):
    """(ref, tol): sum over x != 0 of the float32 (x - ay)^2, summed exactly; tol the kernel's summation slack."""
    x = np.asarray(x, dtype=np.float32).ravel()
    ay = np.asarray(ay, dtype=np.float32).ravel()
    m = x != 0
    r = x[m] - ay[m]
    t = (r * r).astype(np.float64)
    n = x.size
    b = masked_sse_blocks(n)
    dep = depth(-(-n // (b * 256)), b)
    return math.fsum(t.tolist()), (dep + 1) * U64 * float(t.sum())


def scaling_terms(x, ay, dim_thick):
    """The float32 terms of k_scaling_sums as float64 arrays over the masked voxels: (s0, g, h, even)."""
    x = np.asarray(x, dtype=np.float32)
    ay = np.asarray(ay, dtype=np.float32)
    idx = np.indices(x.shape)[dim_thick]
    m = x != 0
    xv, yv = x[m], ay[m]
    r = xv - yv
    return ((r * r).astype(np.float64), (yv * r).astype(np.float64), (yv * yv).astype(np.float64),
            (idx[m] & 1).astype(bool))


def scaling_sums_of(terms):
    s0, g, h, ev = terms
    return [math.fsum(s0.tolist()), math.fsum(g[ev].tolist()), math.fsum(g[~ev].tolist()),
            math.fsum(h[ev].tolist()), math.fsum(h[~ev].tolist())]


def scaling_sums(x, ay, dim_thick):
    """(ref[5], tol[5]) of unires_scaling_sums."""
    terms = scaling_terms(x, ay, dim_thick)
    s0, g, h, ev = terms
    n = int(np.asarray(x).size)
    nb = max(1, min(1024, -(-n // 256)))
    dep = depth(-(-n // (nb * 256)), nb) + 1
    ga, ha = np.abs(g), h
    tol = [dep * U64 * float(v) for v in (s0.sum(), ga[ev].sum(), ga[~ev].sum(), ha[ev].sum(), ha[~ev].sum())]
    return scaling_sums_of(terms), tol


def scaling_totals(x, ay):
    """(sums, tols) of the g and h terms of k_scaling_sums over all masked voxels, formed without any parity split:
    the kernel's even + odd sums must add up to them."""
    s0, g, h, _ = scaling_terms(x, ay, 0)
    n = int(np.asarray(x).size)
    nb = max(1, min(1024, -(-n // 256)))
    dep = depth(-(-n // (nb * 256)), nb) + 1
    return [math.fsum(g.tolist()), math.fsum(h.tolist())], [dep * U64 * float(np.abs(g).sum()),
                                                            dep * U64 * float(h.sum())]


def rigid_terms(gr3, diff, ctc, D):
    """Per voxel, the 27 terms of k_rigid_sums and their absolute-value forms: (27, n) float64 each.  gr3 (*dim, 3),
    diff (*dim), ctc (*dim) or None, D (6, 3, 4) float32."""
    dim = np.shape(diff)
    ijk = [v.ravel().astype(np.float64) for v in np.indices(dim)]
    g = np.asarray(gr3, dtype=np.float64).reshape(-1, 3)
    df = np.asarray(diff, dtype=np.float64).ravel()
    c = np.ones_like(df) if ctc is None else np.asarray(ctc, dtype=np.float64).ravel()
    D = np.asarray(D, dtype=np.float32).astype(np.float64).reshape(6, 3, 4)
    s, sa = [], []
    for q in range(6):
        acc = 0.0
        acca = 0.0
        for d in range(3):
            m = D[q, d]
            aff = m[0] * ijk[0] + m[1] * ijk[1] + m[2] * ijk[2] + m[3]
            affa = abs(m[0]) * ijk[0] + abs(m[1]) * ijk[1] + abs(m[2]) * ijk[2] + abs(m[3])
            acc = acc + g[:, d] * aff
            acca = acca + np.abs(g[:, d]) * affa
        s.append(acc)
        sa.append(acca)
    t = [df * s[q] for q in range(6)]
    ta = [np.abs(df) * sa[q] for q in range(6)]
    for a in range(6):
        for b in range(a, 6):
            t.append(c * s[a] * s[b])
            ta.append(np.abs(c) * sa[a] * sa[b])
    return np.stack(t), np.stack(ta)


def rigid_sums(gr3, diff, ctc, D):
    """(ref[27], tol[27]) of unires_rigid_sums: [0..5] gradient, [6..26] the Hessian's upper triangle row by row."""
    t, ta = rigid_terms(gr3, diff, ctc, D)
    n = t.shape[1]
    b = max(1, min(512, -(-n // 256)))
    dep = depth(-(-n // (b * 256)), b)
    ref = [math.fsum(row.tolist()) for row in t]
    tol = [(28 + dep + 1) * U64 * float(v) for v in ta.sum(1)]
    return ref, tol


def check_sums(out, ref, tol):
    """Per-sum check: dict(ok, worst err / tol, first failing index)."""
    err = [abs(float(o) - r) for o, r in zip(out, ref)]
    ratio = [e / t if t > 0 else (math.inf if e > 0 else 0.0) for e, t in zip(err, tol)]
    bad = [k for k, (e, t) in enumerate(zip(err, tol)) if e > t]
    return dict(ok=not bad, max_ratio=max(ratio), first=bad[0] if bad else None, err=err, tol=list(tol))


# -- clean_fov -----------------------------------------------------------------------------------------------------
def _row_exact(m, dim):
    q = np.asarray(m, dtype=np.float64) * 256.0
    big = sum(abs(float(m[j])) * (dim[j] - 1) for j in range(3)) + abs(float(m[3]))
    return bool(np.all(q == np.round(q))) and big < 2.0 ** 16


def clean_fov(y, M, dim_x):
    """(expected, tie mask): y with the voxels outside the FOV zeroed, in float32; tie voxels may go either way."""
    y = np.asarray(y, dtype=np.float32)
    dim = y.shape
    M = np.asarray(M, dtype=np.float32).astype(np.float64).reshape(3, 4)
    ijk = np.indices(dim).astype(np.float64)
    keep = np.ones(dim, dtype=bool)
    tie = np.zeros(dim, dtype=bool)
    for d in range(3):
        m = M[d]
        a0 = m[0] * ijk[0]
        a1 = a0 + m[1] * ijk[1]
        a2 = a1 + m[2] * ijk[2]
        g = a2 + m[3]
        keep &= (g >= 0) & (g < dim_x[d])
        if not _row_exact(m, dim):
            eta = UU * (np.abs(a0) + np.abs(a1) + np.abs(a2) + np.abs(g)) + 2.0 ** -149
            tie |= (np.abs(g) <= eta) | (np.abs(g - dim_x[d]) <= eta)
    out = np.where(keep, y, np.float32(0.0)).astype(np.float32)
    return out, tie


# -- grid_grad (k_pull_grad) ---------------------------------------------------------------------------------------
C_PG = 12


def pull_grad(src, M, gdim, fov_tol=0.05):
    """float64 spatial gradient of the trilinear sample of ``src`` (zero bound, FOV mask) at the float64 grid
    M (i, j, k) of the float32 M: (ref (*gdim, 3), tol (*gdim, 3), tie (*gdim)).

    Within a cell, d/dg_a of the sample does not depend on g_a and is linear in the other two coordinates, so a
    coordinate off by eta_b along b != a moves it by <= eta_b L_ab, L_ab = the sum over the 8 corners of |v| with
    unit weights along a and b and the true weight along the third axis.  Rounding: the kernel's chain (1 - w, the
    z lerp, the y and x sums: 9 u) and the oracle's (three weights and their product, 8 terms summed: 12 u) on
    M_a = sum |v| (unit weight along a): C_PG = 12.  eta_b is clean_fov's coordinate bound (0 on rows computed
    exactly).  Ties: a coordinate within eta of an integer (the cell, and with it the corners' zero-bound validity,
    changes) or of an FOV threshold (-tol and fl(fl(n - 1) + tol), widened by the rounding of the threshold the
    oracle forms in one step)."""
    src = np.asarray(src, dtype=np.float32).astype(np.float64)
    n = src.shape
    M = np.asarray(M, dtype=np.float32).astype(np.float64).reshape(3, 4)
    ijk = np.indices(gdim).astype(np.float64)
    t = f32(fov_tol)
    g, eta = [], []
    for d in range(3):
        m = M[d]
        a0 = m[0] * ijk[0]
        a1 = a0 + m[1] * ijk[1]
        a2 = a1 + m[2] * ijk[2]
        gd = a2 + m[3]
        g.append(gd)
        eta.append(np.zeros_like(gd) if _row_exact(m, gdim) else
                   UU * (np.abs(a0) + np.abs(a1) + np.abs(a2) + np.abs(gd)) + 2.0 ** -149)
    inside = np.ones(gdim, dtype=bool)
    tie = np.zeros(gdim, dtype=bool)
    for d in range(3):
        hi = f32(f32(n[d] - 1) + t)
        inside &= (g[d] > -t) & (g[d] < hi)
        e = eta[d]
        tie |= (e > 0) & ((np.abs(g[d] - np.round(g[d])) <= e) | (np.abs(g[d] + t) <= e + U * t)
                          | (np.abs(g[d] - hi) <= e + 2 * U * hi))
    corners = []
    for d in range(3):
        f = np.floor(g[d])
        w1 = g[d] - f
        lo, up = f.astype(np.int64), f.astype(np.int64) + 1
        corners.append([(lo, 1.0 - w1, -1.0, (lo >= 0) & (lo < n[d])), (up, w1, 1.0, (up >= 0) & (up < n[d]))])
    ref = np.zeros((3,) + tuple(gdim))
    Ma = np.zeros_like(ref)
    L = np.zeros_like(ref)
    flat = src.ravel()
    for cx in corners[0]:
        for cy in corners[1]:
            for cz in corners[2]:
                ok = cx[3] & cy[3] & cz[3]
                idx = (np.clip(cx[0], 0, n[0] - 1) * n[1] + np.clip(cy[0], 0, n[1] - 1)) * n[2] + \
                    np.clip(cz[0], 0, n[2] - 1)
                v = np.where(ok, flat[idx], 0.0)
                av = np.abs(v)
                c3 = (cx, cy, cz)
                for a in range(3):
                    b, c = [k for k in range(3) if k != a]
                    ref[a] += v * c3[a][2] * c3[b][1] * c3[c][1]
                    Ma[a] += av * c3[b][1] * c3[c][1]
                    L[a] += av * (eta[b] * c3[c][1] + eta[c] * c3[b][1])
    tol = UU * C_PG * Ma + L
    ref, tol = ref * inside, tol * inside
    return np.moveaxis(ref, 0, -1), np.moveaxis(tol, 0, -1), tie
