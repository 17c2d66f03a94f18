"""Restatement of the per-voxel weights (_input.weight, sett.voxel_robust): weight volumes, the Huber
rule in numpy float32 - bit for bit what k_voxel_huber computes - the apply pass in numpy, and the exact sums of the
float32 terms of unires_voxel_sums with their rounding bound.  The reference has no counterpart: nothing here is pinned
against it.  The float64 operator with a general x-space W between A and At is tests/slice64.weighted_matvec64.

The data term of repeat n is 1/2 tau_n sum_v g_n(v) u_n[s(v)] m_n(v) (x_n(v) - (A_n y)(v))^2.
"""
import math

import numpy as np
import torch


def weights(shape, pattern, seed=19):
    """float32 weight volume of ``shape``: 'pow2' - seeded draws from {0, 1/4, 1/2, 1}: a float32 product with one is
    exact; 'ramp' - generic values in [0, 1] (the first voxel 0, the last 1); 'ones'; 'zeros'."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    if pattern == 'pow2':
        gen = torch.Generator().manual_seed(seed)
        return torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (n,), generator=gen)].reshape(shape)
    if pattern == 'ramp':
        gen = torch.Generator().manual_seed(seed + 1)
        w = torch.rand(n, generator=gen)
        w[0], w[-1] = 0.0, 1.0
        return w.float().reshape(shape)
    if pattern == 'ones':
        return torch.ones(shape)
    assert pattern == 'zeros', pattern
    return torch.zeros(shape)


def apply32(src, g, u=None, axis=2, mask=None):
    """The apply pass in numpy, bit for bit: fl32(g src) without slice weights (numpy's float32 product is the IEEE
    operation __fmul_rn is); with u (one per slice along ``axis``) fl32(fl64(g u) src) - g u is exact in float64 (48
    significant bits), its product with src rounds to float64 and then to float32, as the kernel's casts do; +0 where
    the mask byte is 0."""
    src, g = np.asarray(src, np.float32), np.asarray(g, np.float32)
    if u is None:
        out = (g * src).astype(np.float32)
    else:
        view = [1, 1, 1]
        view[axis] = src.shape[axis]
        w = g.astype(np.float64) * np.asarray(u, np.float32).astype(np.float64).reshape(view)
        out = (w * src.astype(np.float64)).astype(np.float32)
    if mask is not None:
        out = np.where(np.asarray(mask) != 0, out, np.float32(0.0)).astype(np.float32)
    return out


def huber64(x, ay, prior, c):
    """g = prior . h in numpy float32 (prior None: h): r = fl(x - ay); h = 1 where x == 0 or |r| <= c, else fl(c / |r|);
    g = fl(prior h).  numpy's float32 -, * and / are the IEEE operations __fsub_rn, __fmul_rn and __fdiv_rn are."""
    x, ay, c = np.asarray(x, np.float32), np.asarray(ay, np.float32), np.float32(c)
    a = np.abs((x - ay).astype(np.float32))
    with np.errstate(divide='ignore', invalid='ignore'):
        h = np.where((x == 0) | (a <= c), np.float32(1.0), (c / a).astype(np.float32)).astype(np.float32)
    if prior is None:
        return h
    return (np.asarray(prior, np.float32) * h).astype(np.float32)


def terms32(x, ay, g):
    """The float32 terms of the weighted slice sums as the kernel forms them, as float64: r = fl(x - ay), t = fl(r r),
    fl(g t); 0 where x == 0."""
    x, ay, g = np.asarray(x, np.float32), np.asarray(ay, np.float32), np.asarray(g, np.float32)
    r = (x - ay).astype(np.float32)
    t = (r * r).astype(np.float32)
    return np.where(x != 0, (g * t).astype(np.float32).astype(np.float64), 0.0)


def voxel_sums64(x, ay, g, axis):
    """(SSE_s, G_s, N_s, bound_sse, bound_g): the exact (math.fsum) per-slice sums of ``terms32`` and of g over the
    voxels with x != 0, the count of terms, and tests/slice64.slice_sums64's bound on a float64 accumulation of N_s
    non-negative terms in any order: N_s 2^-53 SSE_s (1 + N_s 2^-53) - and the same with G_s for the sums of g."""
    t = terms32(x, ay, g)
    nz = np.asarray(x) != 0
    gz = np.where(nz, np.asarray(g, np.float32).astype(np.float64), 0.0)
    other = tuple(a for a in range(3) if a != axis)
    S = t.shape[axis]
    sse = np.array([math.fsum(np.take(t, s, axis=axis).ravel().tolist()) for s in range(S)])
    gs = np.array([math.fsum(np.take(gz, s, axis=axis).ravel().tolist()) for s in range(S)])
    cnt = nz.sum(axis=other).astype(np.float64)
    bound = lambda tot: cnt * 2.0 ** -53 * tot * (1.0 + cnt * 2.0 ** -53)
    return sse, gs, cnt, bound(sse), bound(gs)
