"""float64 restatement of the per-slice intensity gains (sett.slice_gain, _input.slice_gain): the
float32 terms of the gain sums as the kernel forms them, their exact per-slice sums with the bound of a float64
accumulation, the gain rule, and the two per-slice tables a gained repeat's passes read.  The reference has no
counterpart (its even / odd scaling is one special case): nothing here is pinned against it.

The data term of repeat n is 1/2 tau sum_v W(v) (x(v) - e[s(v)] a(v))^2 + 1/2 kappa sum_s (e_s - 1)^2 with a = A_n y,
W = g . u . [x != 0] and s(v) the index of voxel v along ``po.dim_thick`` in the caller's layout.
"""
import math

import numpy as np
import torch

U53 = 2.0 ** -53


def gains(S, pattern, seed=43):
    """(S,) float32 gains: 'pow2' - seeded draws from {1/4, 1/2, 1} (products with them are exact, and e^2 <= 1);
    'generic' - seeded values in [0.5, 2]; 'ones'."""
    gen = torch.Generator().manual_seed(seed)
    if pattern == 'pow2':
        return torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (S,), generator=gen)]
    if pattern == 'generic':
        return (0.5 + 1.5 * torch.rand(S, generator=gen)).float()
    assert pattern == 'ones', pattern
    return torch.ones(S)


def terms32(x, ay):
    """The float32 terms of the gain sums as the kernel forms them, as float64: (fl(x ay), fl(ay ay), [x != 0]); the
    products 0 where x == 0.  numpy's float32 product is the IEEE operation __fmul_rn is."""
    x, ay = np.asarray(x, np.float32), np.asarray(ay, np.float32)
    nz = x != 0
    tp = (x * ay).astype(np.float32).astype(np.float64)
    tq = (ay * ay).astype(np.float32).astype(np.float64)
    return np.where(nz, tp, 0.0), np.where(nz, tq, 0.0), nz


def _spread(u, shape, axis):
    view = [1, 1, 1]
    view[axis] = int(shape[axis])
    return np.asarray(u, np.float32).astype(np.float64).reshape(view)


def gain_sums64(x, ay, g, u, axis):
    """(sums, bound), each (3 S,) float64: the exact (math.fsum) per-slice sums of the summands the kernel adds -
    fl64(W fl32(x ay)), fl64(W fl32(ay ay)) and W, W = g u formed in float64 where it is exact (24 + 24 significant
    bits; either factor 1 where None) - and the bound on their float64 accumulation in any order:

        N_s 2^-53 sum |summand| (1 + N_s 2^-53)      (slice64.slice_sums64's, with magnitudes: x ay may be negative)

    plus, where g AND u are given, 2^-53 sum |summand|: W t then has up to 72 significant bits and is rounded to float64
    once.  numpy's float64 product is that rounding, so the summands here are the kernel's own and the term only
    widens the bound; with one factor W t is exact (48 bits)."""
    tp, tq, nz = terms32(x, ay)
    shape = tp.shape
    W = np.ones(shape, np.float64)
    if g is not None:
        W = W * np.asarray(g, np.float32).astype(np.float64)
    if u is not None:
        W = W * _spread(u, shape, axis)
    W = np.where(nz, W, 0.0)
    cols = (W * tp, W * tq, W)
    other = tuple(a for a in range(3) if a != axis)
    S = shape[axis]
    cnt = nz.sum(axis=other).astype(np.float64)
    sums, bound = np.zeros(3 * S), np.zeros(3 * S)
    for k, col in enumerate(cols):
        for s in range(S):
            v = np.take(col, s, axis=axis).ravel()
            mag = math.fsum(np.abs(v).tolist())
            sums[k * S + s] = math.fsum(v.tolist())
            bound[k * S + s] = cnt[s] * U53 * mag * (1.0 + cnt[s] * U53)
            if g is not None and u is not None and k < 2:
                bound[k * S + s] += U53 * mag
    return sums, bound


def rule64(sums, tau, kappa, gain_max):
    """The gain rule in numpy float64, stated on its own: P_s = tau sums[s], Q_s = tau sums[S + s];
    e_s = (P_s + kappa) / (Q_s + kappa) clamped to [1 / gain_max, gain_max]; 1 where Q_s + kappa = 0."""
    sums = np.asarray(sums, np.float64)
    S = sums.size // 3
    P = float(tau) * sums[:S] + float(kappa)
    Q = float(tau) * sums[S:2 * S] + float(kappa)
    e = np.ones(S, np.float64)
    ok = Q > 0
    e[ok] = P[ok] / Q[ok]
    return np.clip(e, 1.0 / float(gain_max), float(gain_max))


def energy64(e, P, Q, X, kappa):
    """E(e) = 1/2 sum_s (X_s - 2 e_s P_s + e_s^2 Q_s) + 1/2 kappa sum_s (e_s - 1)^2 with X_s = tau sum W x^2,
    P_s = tau sum W x a, Q_s = tau sum W a^2: the repeat's data term as a function of its gains at a fixed y and W."""
    e = np.asarray(e, np.float64)
    return 0.5 * float(np.sum(X - 2.0 * e * P + e * e * Q)) + 0.5 * float(kappa) * float(np.sum((e - 1.0) ** 2))


def compose32(u, e):
    """(w_mat, w_rhs) float32, bit for bit what the plan's compose kernel writes: w_rhs = fl32(fl64(u e)),
    w_mat = fl32(fl64(fl64(u e) e)); u None: ones.  u e is exact in float64; its product with e rounds there once
    (numpy's float64 product) and once more to float32."""
    e64 = np.asarray(e, np.float32).astype(np.float64)
    u64 = np.ones_like(e64) if u is None else np.asarray(u, np.float32).astype(np.float64)
    ue = u64 * e64
    return (ue * e64).astype(np.float32), ue.astype(np.float32)
