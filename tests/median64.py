"""NumPy restatement of the exact medians of ``unires_amd/csrc/median.hip`` and of what is built on them (DESIGN.md
8.11): the key of a magnitude, the eligibility rules, the float32 term t in the kernel's order, the lower median, the
three-pass digit select, and the float32 chains sd / mu / mult of ``sett.noise_est = 'mad'`` and ``sett.voxel_scale =
'mad'``.  numpy's float32 -, + and * are the IEEE operations __fsub_rn, __fadd_rn and __fmul_rn are.  The reference has
no counterpart: nothing here is pinned against it."""
import numpy as np

MAD_TO_SD = np.float32(1.4826)  # 1 / Phi^-1(3/4)
BITS = (11, 11, 10)  # the digits of the three passes, from the most significant bits down


def key(t):
    """uint32 bit pattern of fabsf(t): monotone in |t| for every non-NaN float32, -0 -> +0."""
    return np.abs(np.asarray(t, np.float32)).view(np.uint32)


def lower_median(m):
    """(median, N) of the magnitudes ``m``: the ceil(N / 2)-th smallest, torch.median's convention; (0, 0) of none."""
    m = np.asarray(m, np.float32).ravel()
    N = m.size
    if N == 0:
        return np.float32(0.0), 0
    return np.sort(m)[(N + 1) // 2 - 1], N


def digit_select(m):
    """The same (median, N) as the kernels find it: histogram the top digit of the keys, pick the bin that holds the
    rank, keep the rank inside it, filter on the prefix, repeat."""
    k = key(np.asarray(m, np.float32).ravel())
    N = k.size
    if N == 0:
        return np.float32(0.0), 0
    rank, prefix, shift = (N + 1) // 2, 0, 32
    for bits in BITS:
        shift -= bits
        sel = k[(k >> np.uint32(shift + bits)) == prefix] if shift + bits < 32 else k
        counts = np.bincount(((sel >> np.uint32(shift)) & np.uint32((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
        cum = np.cumsum(counts)
        b = int(np.searchsorted(cum, rank, side='left'))
        rank -= int(cum[b] - counts[b])
        prefix = (prefix << bits) | b
    return np.array([prefix], np.uint32).view(np.float32)[0], N


def absres(x, ay, prior=None):
    """|fl32(x - ay)| of the eligible voxels: x != 0, a finite difference, prior > 0 where there is one."""
    x, ay = np.asarray(x, np.float32).ravel(), np.asarray(ay, np.float32).ravel()
    with np.errstate(invalid='ignore', over='ignore'):
        a = np.abs((x - ay).astype(np.float32))
    ok = (x != 0) & np.isfinite(a)
    if prior is not None:
        ok &= np.asarray(prior, np.float32).ravel() > 0
    return a[ok]


def median_absres(x, ay, prior=None):
    return lower_median(absres(x, ay, prior))


def hh(dat, axis, ct=False, w=None):
    """|((a - b) - c) + d| in float32, in this order, of every 2 x 2 cell of the planes orthogonal to ``axis`` whose
    four voxels are finite, != 0 (not ct: > 0) and, with ``w``, of weight > 0; a = x[p, q], b = x[p + 1, q],
    c = x[p, q + 1], d = x[p + 1, q + 1], p and q the two other axes in ascending order."""
    x = np.asarray(dat, np.float32)
    p, q = [a for a in range(3) if a != axis]
    ok = np.isfinite(x) & ((x != 0) if ct else (x > 0))
    if w is not None:
        ok &= np.asarray(w, np.float32) > 0

    def corner(v, dp, dq):
        sl = [slice(None)] * 3
        sl[p] = slice(dp, v.shape[p] - 1 + dp)
        sl[q] = slice(dq, v.shape[q] - 1 + dq)
        return v[tuple(sl)]
    a, b, c, d = corner(x, 0, 0), corner(x, 1, 0), corner(x, 0, 1), corner(x, 1, 1)
    use = corner(ok, 0, 0) & corner(ok, 1, 0) & corner(ok, 0, 1) & corner(ok, 1, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        t = (((a - b).astype(np.float32) - c).astype(np.float32) + d).astype(np.float32)
    return np.abs(t[use])


def median_hh(dat, axis, ct=False, w=None):
    return lower_median(hh(dat, axis, ct, w))


def sd_of(med):
    """fl32(fl32(1.4826 med) 0.5): the detail of i.i.d. noise of variance s^2 has variance 4 s^2."""
    return np.float32(np.float32(MAD_TO_SD * np.float32(med)) * np.float32(0.5))


def tau_of(sd):
    """1 / sd**2 in float32, as torch's float32 CPU scalars compute it: the square, then the reciprocal."""
    sd = np.float32(sd)
    return np.float32(np.float32(1.0) / np.float32(sd * sd))


def mu_of(dat, ct=False, w=None):
    """|mean| of the voxels that are finite, != 0 (not ct: > 0) and of weight > 0, in float64."""
    x = np.asarray(dat, np.float32)
    ok = np.isfinite(x) & ((x != 0) if ct else (x > 0))
    if w is not None:
        ok &= np.asarray(w, np.float32) > 0
    return abs(float(x[ok].astype(np.float64).mean()))


def mult_of(k):
    """fl32(fl32(voxel_k) 1.4826): what the device median is multiplied by to give the Huber threshold."""
    return np.float32(np.float32(k) * MAD_TO_SD)


def threshold(med, k):
    """c = fl32(mult (float) med)."""
    return np.float32(mult_of(k) * np.float32(med))


PHANTOM_DIM = (48, 48, 40)


def phantom(sd, seed=11):
    """A background-free volume: nested off-centre balls of constant intensity (piecewise constant, curved edges) under
    a smooth multiplicative shading, Gaussian noise of standard deviation ``sd``, exactly 0 outside a ball of radius
    21 voxels.  Every voxel inside is far above 0.  float32 (48, 48, 40)."""
    X, Y, Z = PHANTOM_DIM
    i, j, k = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij')
    r = lambda c, s=(1.0, 1.0, 1.0): np.sqrt(((i - c[0]) * s[0]) ** 2 + ((j - c[1]) * s[1]) ** 2 + ((k - c[2]) * s[2]) ** 2)
    v = np.full(PHANTOM_DIM, 400.0)
    v[r((22, 25, 19)) < 15] = 520.0
    v[r((27, 20, 22)) < 8] = 300.0
    v[r((18, 29, 15), (1.0, 1.4, 1.0)) < 6] = 650.0
    shade = 1.0 + 0.15 * np.sin(i / 17.0) * np.cos(j / 23.0) + 0.1 * (k - Z / 2) / Z
    rng = np.random.RandomState(seed)
    v = v * shade + sd * rng.standard_normal(PHANTOM_DIM)
    v[r((23.5, 23.5, 19.5), (1.0, 1.0, 1.1)) >= 21] = 0.0
    return v.astype(np.float32)
