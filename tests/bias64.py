"""float64 restatement of the bias field (sett.bias, _input.bias_coef) in numpy: the cosine tables, the
field, the terms of its Gauss-Newton step (dense, without the product identity), the objective, the rule and the two
volumes the plan reads.  Nothing here imports unires_amd.

A repeat's data term is E(c) = 1/2 tau sum_v W (x - b mu)^2 + 1/2 c^T Lambda c with W = g . u . [x != 0], b = exp(beta),
beta(i, j, k) = sum_abc c_abc phi_a(i) phi_b(j) phi_c(k), phi_m(i) = cos(pi m (2 i + 1) / (2 n)).

The bound on the device's sums.  The device forms, per voxel, m = fl32(b mu) and from it in float64 - each operation
rounded on its own - the summand f(v) (W r^2, W m r or W m^2); ``summands64`` reproduces these bits.  An output is
sum_v f(v) phi_a(i) phi_b(j) phi_c(k): on top of f the device makes three products (one with each table, at some
stage of its folds) and N - 1 additions in an order of its own, N the voxels of the observation.  To first order every
term therefore carries at most (N - 1) + 3 relative errors of 2^-53, whatever the order of summation and of the folds:
|device - exact| <= (N + 2) 2^-53 sum_v |f phi_a phi_b phi_c|.  The restatement sums in long double where the platform
has one (64 significant bits: its own error is 2^-11 of that) and in float64 otherwise, where it has the same bound;
``terms64`` therefore returns 2 (N + 3) 2^-53 sum |term|, which covers both sides, the rounding of the tables' product
in the bound itself and leaves nothing to the measured values.
"""
import numpy as np

U53 = 2.0 ** -53
STEPS = tuple(2.0 ** -p for p in range(6))


def tables64(shape, orders, proj=True):
    """Per axis (2 k - 1, n) with ``proj`` (what the projections are taken on), else (k, n): row m is phi_m."""
    out = []
    for n, k in zip(shape, orders):
        rows = 2 * int(k) - 1 if proj else int(k)
        m = np.arange(rows, dtype=np.float64)[:, None]
        i = np.arange(int(n), dtype=np.float64)[None, :]
        out.append(np.ascontiguousarray(np.cos(np.pi * m * (2.0 * i + 1.0) / (2.0 * int(n)))))
    return tuple(out)


def orders64(shape, vx, cutoff):
    return tuple(int(min(max(np.ceil(2.0 * n * v / cutoff), 1), min(8, n))) for n, v in zip(shape, vx))


def lambda64(shape, vx, orders, kappa, reg, cutoff):
    lam = np.zeros(tuple(orders))
    for a in range(orders[0]):
        for b in range(orders[1]):
            for c in range(orders[2]):
                f = sum((cutoff * m / (2.0 * n * v)) ** 2 for m, n, v in zip((a, b, c), shape, vx))
                lam[a, b, c] = kappa * reg * (1.0 + f)
    return lam


def beta64(coef, shape):
    coef = np.asarray(coef, dtype=np.float64)
    tx, ty, tz = tables64(shape, coef.shape, proj=False)
    return np.einsum('abc,ai,bj,ck->ijk', coef, tx, ty, tz)


def field64(coef, shape, bias_max=4.0):
    """b = fl32(exp(clamp(beta, +- log bias_max))), beta in float64."""
    lim = np.log(float(bias_max))
    return np.exp(np.clip(beta64(coef, shape), -lim, lim)).astype(np.float32)


def compose32(g, b, x):
    """(g b^2, x / b) as the plan takes them, float32: fl32(fl64(fl64(g b) b)), g = 1 where None - g b is exact in
    float64 - and the float32 quotient, +0 where x == 0."""
    b64 = b.astype(np.float64)
    g64 = np.ones_like(b64) if g is None else g.astype(np.float64)
    gb2 = ((g64 * b64) * b64).astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        xb = np.where(x == 0, np.float32(0), x.astype(np.float32) / b.astype(np.float32)).astype(np.float32)
    return gb2, xb


def weights64(shape, g, u, axis):
    W = np.ones(shape, dtype=np.float64) if g is None else g.astype(np.float64)
    if u is not None:
        view = [1, 1, 1]
        view[axis] = shape[axis]
        W = W * u.astype(np.float64).reshape(view)  # (24 + 24 significant bits: exact)
    return W


def summands64(x, mu, b, g, u, axis):
    """The device's summands, bit for bit: (W r^2, W m r, W m^2) float64 volumes, zero where x == 0."""
    m = (b.astype(np.float32) * mu.astype(np.float32)).astype(np.float32).astype(np.float64)
    r = m - x.astype(np.float64)
    W = weights64(x.shape, g, u, axis) * (x != 0)
    wm = W * m
    return (W * r) * r, wm * r, wm * m


def _project(f, tabs, rows):
    ld = np.longdouble
    t = np.tensordot(tabs[0][:rows[0]].astype(ld), f.astype(ld), axes=(1, 0))          # (a, j, k)
    t = np.tensordot(tabs[1][:rows[1]].astype(ld), t, axes=(1, 1))                      # (b, a, k)
    t = np.tensordot(tabs[2][:rows[2]].astype(ld), t, axes=(1, 2))                      # (c, b, a)
    return np.transpose(t, (2, 1, 0))


def terms64(x, mu, b, g, u, axis, orders):
    """(want, bound) of ``unires_bias_terms``: (1 + K + Q,) each - sum W r^2, the projection of W m r onto the orders
    < k, the projection of W m^2 onto the orders < 2 k - 1; the bound is the docstring's 2 (N + 3) 2^-53 sum |term|."""
    fo, fg, fh = summands64(x, mu, b, g, u, axis)
    N = x.size
    want, mass = [np.array([fo.astype(np.longdouble).sum()])], [np.array([np.abs(fo).sum()])]
    if any(orders):
        tabs = tables64(x.shape, orders)
        absT = tuple(np.abs(t) for t in tabs)
        q = tuple(2 * k - 1 for k in orders)
        for f, rows in ((fg, orders), (fh, q)):
            want.append(_project(f, tabs, rows).reshape(-1))
            mass.append(_project(np.abs(f), absT, rows).reshape(-1))
    want = np.concatenate(want).astype(np.float64)
    bound = 2.0 * (N + 3) * U53 * np.concatenate(mass).astype(np.float64)
    return want, bound


def basis64(shape, orders):
    """The dense basis (K, N): row (a, b, c) is phi_a(i) phi_b(j) phi_c(k) over the voxels."""
    tx, ty, tz = tables64(shape, orders, proj=False)
    return np.einsum('ai,bj,ck->abcijk', tx, ty, tz).reshape(int(np.prod(orders)), -1)


def dense_terms64(f_g, f_h, shape, orders):
    """(sum f_g Phi_k, sum f_h Phi_k Phi_l) by the dense basis: no product identity."""
    Phi = basis64(shape, orders)
    return Phi @ f_g.reshape(-1), (Phi * f_h.reshape(1, -1)) @ Phi.T


def hessian_from_projection64(P, orders):
    """The same (K, K) matrix from the projection of f_h onto the orders < 2 k - 1, entry by entry: phi_m phi_m' =
    (phi_|m - m'| + phi_(m + m')) / 2 along every axis - eight entries of P, over 8."""
    k = tuple(int(v) for v in orders)
    K = k[0] * k[1] * k[2]
    H = np.zeros((K, K))
    idx = [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]
    for p, (a, b, c) in enumerate(idx):
        for q, (a2, b2, c2) in enumerate(idx):
            s = 0.0
            for ia in (abs(a - a2), a + a2):
                for ib in (abs(b - b2), b + b2):
                    for ic in (abs(c - c2), c + c2):
                        s += P[ia, ib, ic]
            H[p, q] = s / 8.0
    return H


def objective64(coef, x, mu, g, u, axis, lam, tau, bias_max=4.0):
    """E(c) in float64 throughout (b is NOT rounded to float32: the function central differences are taken of)."""
    lim = np.log(float(bias_max))
    b = np.exp(np.clip(beta64(coef, x.shape), -lim, lim))
    r = b * mu.astype(np.float64) - x.astype(np.float64)
    W = weights64(x.shape, g, u, axis) * (x != 0)
    c = np.asarray(coef, dtype=np.float64)
    return 0.5 * tau * float((W * r * r).sum()) + 0.5 * float((lam * c * c).sum())


def gradient64(coef, x, mu, g, u, axis, lam, tau, bias_max=4.0):
    """dE/dc = tau sum_v W m r Phi_k + Lambda c, m = b mu, r = m - x (inside the clamp)."""
    lim = np.log(float(bias_max))
    b = np.exp(np.clip(beta64(coef, x.shape), -lim, lim))
    m = b * mu.astype(np.float64)
    W = weights64(x.shape, g, u, axis) * (x != 0)
    c = np.asarray(coef, dtype=np.float64)
    Gd, _ = dense_terms64(W * m * (m - x), W * m * m, x.shape, c.shape)
    return tau * Gd.reshape(c.shape) + lam * c


def energy64(S, c, lam, tau):
    return 0.5 * tau * float(S) + 0.5 * float((lam * c * c).sum())


def step64(c, G, P, lam, tau):
    """(Delta, gradient, H): gradient = tau G + Lambda c, H = tau (assembled from P) + Lambda, Delta = -H^-1 gradient."""
    c = np.asarray(c, dtype=np.float64)
    grad = tau * np.asarray(G).reshape(c.shape) + lam * c
    H = tau * hessian_from_projection64(np.asarray(P), c.shape) + np.diag(lam.reshape(-1))
    return -np.linalg.solve(H, grad.reshape(-1)).reshape(c.shape), grad, H


def line_search64(c, delta, E0, energy):
    """The first s of 1, 1/2, ..., 2^-5 with energy(c + s delta) <= E0: (c + s delta, E, s); (c, E0, 0) where none."""
    for s in STEPS:
        cand = c + s * delta
        E1 = energy(cand)
        if E1 <= E0:
            return cand, E1, s
    return c, E0, 0.0
