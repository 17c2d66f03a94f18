"""float64 restatement of the per-slice weights (sett.slice_robust, _input.slice_w): the weights put
between tests/ref64.py's Operator64 ``A`` and ``At``, the variance-ratio rule, the float32 terms of the slice sums, and
the rounding bounds of the weighted operator.  The reference has no counterpart: nothing here is pinned against it.

The weighted data term of repeat n is 1/2 tau_n sum_v u_n[s(v)] m_n(v) (x_n(v) - (A_n y)(v))^2, s(v) the index of voxel v
along ``po.dim_thick`` in the caller's layout, and its system sum_n tau_n A_n^T diag(u_n . m_n) A_n + rho lam^2 D^T D.
"""
import numpy as np
import torch

from tests import ref64


def weights(S, pattern, seed=17):
    """(S,) float32 weights: 'pow2' - seeded draws from {0, 1/4, 1/2, 1}: a float32 product with one is exact;
    'ramp' - generic values in [0, 1] (the first 0, the last 1); 'ones'; 'zeros'."""
    if pattern == 'pow2':
        gen = torch.Generator().manual_seed(seed)
        return torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (S,), generator=gen)]
    if pattern == 'ramp':
        gen = torch.Generator().manual_seed(seed + 1)
        w = torch.rand(S, generator=gen)
        w[0], w[-1] = 0.0, 1.0
        return w.float()
    if pattern == 'ones':
        return torch.ones(S)
    assert pattern == 'zeros', pattern
    return torch.zeros(S)


def spread(w, shape, axis):
    """The (S,) weights as a float64 volume of ``shape``: w[s(v)] at every voxel, s counted along ``axis``."""
    view = [1, 1, 1]
    view[axis] = int(shape[axis])
    assert w.numel() == int(shape[axis])
    return w.double().reshape(view).expand(tuple(shape)).clone()


def rule64(sse, cnt, k):
    """The variance-ratio rule in numpy float64, stated on its own: over the slices with N_s > 0, m_s = SSE_s / N_s;
    sigma^2 = the LOWER median of those m_s - the ceil(K / 2)-th smallest of K values (torch.median's convention, not
    numpy's mean of the middle two); u_s = 1 where N_s = 0 or m_s <= k^2 sigma^2, else (k^2 sigma^2) / m_s; all ones
    where no slice has data or sigma^2 = 0."""
    sse, cnt = np.asarray(sse, np.float64), np.asarray(cnt, np.float64)
    u = np.ones(sse.shape, np.float64)
    has = cnt > 0
    K = int(has.sum())
    if K == 0:
        return u
    m = sse[has] / cnt[has]
    sig2 = np.sort(m)[(K + 1) // 2 - 1]
    if not sig2 > 0:
        return u
    thr = (float(k) * float(k)) * sig2
    um = np.ones(K, np.float64)
    big = m > thr
    um[big] = thr / m[big]
    u[has] = um
    return u


def terms32(x, ay):
    """The float32 terms of the slice sums as the kernel forms them, as float64: (x - ay) rounded, its square rounded;
    0 where x == 0.  numpy's float32 subtraction and product are the IEEE operations __fsub_rn / __fmul_rn are."""
    x, ay = np.asarray(x, np.float32), np.asarray(ay, np.float32)
    r = (x - ay).astype(np.float32)
    t = (r * r).astype(np.float32).astype(np.float64)
    return np.where(x != 0, t, 0.0)


def slice_sums64(x, ay, axis):
    """(SSE_s, N_s, bound_s): the exact (math.fsum) per-slice sums of ``terms32``, the counts, and the bound on a
    float64 accumulation of N_s non-negative terms in any order: each of the N_s - 1 additions rounds a partial sum that
    is at most SSE_s by 2^-53 relative, so |computed - exact| <= N_s 2^-53 SSE_s to first order; the factor
    (1 + N_s 2^-53) on top covers the higher orders."""
    import math
    t = terms32(x, ay)
    nz = np.asarray(x) != 0
    other = tuple(a for a in range(3) if a != axis)
    S = t.shape[axis]
    sse = np.array([math.fsum(np.take(t, s, axis=axis).ravel().tolist()) for s in range(S)])
    cnt = nz.sum(axis=other).astype(np.float64)
    bound = cnt * 2.0 ** -53 * sse * (1.0 + cnt * 2.0 ** -53)
    return sse, cnt, bound


def weighted_matvec64(ops, taus, Ws, p, rho, lam, vx, which='forward', parts=None, Ap=None, exact=True):
    """(ref, tol) of q = sum_n tau_n A_n^T (W_n . A_n p) + rho lam^2 D^T D p; W_n = u_n[s(v)] m_n(v) as a float64
    x-space volume in the caller's layout (``spread``), or None for a repeat without weights.

    The tolerance starts from ``ref64.bound_matvec_reps`` of the UNWEIGHTED operator.  It stays a bound for weights in
    [0, 1]: the weighted repeat runs the same forward and the same push around a pass that multiplies the intermediate
    by W <= 1, and every error the forward made reaches the push scaled by W <= 1, while every magnitude sum of the
    bound (M = |A|^T |A| |p|, G, D) is taken with W = 1.  With ``exact`` (weights whose float32 product with any
    intermediate is exact: 0, 1 and powers of two short of underflow) that is all.  Otherwise the pass rounds the
    intermediate once more, W a -> fl(W a): at most u W |a| with |a| <= (1 + c_A u) |A| |p|, carried through tau |A|^T
    like any stored intermediate:

        extra_n = (u + 2^-53) (1 + c_A u) tau_n |A_n|^T (W_n . |A_n| |p|)."""
    taus64 = [ref64._f32(t) for t in taus]
    if parts is None:
        parts = [op.parts_AtA(p) for op in ops]
    ref, tol = ref64.bound_matvec_reps(ops, taus, p, rho, lam, vx, which, parts=parts)
    p64 = p.double()
    for n, (op, tau, W) in enumerate(zip(ops, taus64, Ws)):
        if W is None:
            continue
        a = op.A(p64) if Ap is None else Ap[n]
        ref = ref + tau * (op.At(W * a) - parts[n][0])  # (the unweighted term out, the weighted one in)
        if not exact:
            tol = tol + (ref64.U + ref64.U64) * (1.0 + op.c_A * ref64.U) * tau * op.At(W * op.A(p64.abs(), op.Ka), op.Ka)
    return ref, tol
