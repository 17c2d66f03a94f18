"""float64 restatement of the Rician data term (sett.noise_model = 'rician').  The reference has no
counterpart (its data term is Gaussian): nothing here is pinned against it.

With mu = e . (A y), z = tau x mu and sigma^2 = 1 / tau, the negative log-likelihood of a magnitude voxel is

    -log p(x | mu) = 1/2 tau (x - mu)^2 + c(z) - log(tau x),      c(z) = (z - |z|) - log i0e(|z|),

i0e(z) = exp(-|z|) I0(z).  (For z >= 0, c >= 0; for z < 0 it is 2 z - log i0e(|z|): the formula is the likelihood's on
both sides.)  log I0 is convex, so its tangent at z0 = tau x mu0 lies below it, and

    1/2 tau (x - mu)^2 + c(tau x mu)  <=  1/2 tau (mu - x R(z0))^2 + const(mu0),      R = I1 / I0,

with equality and equal gradients at mu = mu0: the surrogate.  ``ratio64`` / ``c64`` are float64 statements from
torch.special; ``ratio32`` / ``c32`` emulate the kernel's float32 operation sequence in numpy (every operation an IEEE
float32 one, as the kernel is compiled without contraction; only log is a library call, good to about an ulp on either
side).
"""
import math

import numpy as np
import torch

U53 = 2.0 ** -53
BRANCH = np.float32(3.75)
# Abramowitz & Stegun 9.8.1 - 9.8.4, highest degree first
P0 = (0.0045813, 0.0360768, 0.2659732, 1.2067492, 3.0899424, 3.5156229, 1.0)
P1 = (0.00032411, 0.00301532, 0.02658733, 0.15084934, 0.51498869, 0.87890594, 0.5)
Q0 = (0.00392377, -0.01647633, 0.02635537, -0.02057706, 0.00916281, -0.00157565, 0.00225319, 0.01328592, 0.39894228)
Q1 = (-0.00420059, 0.01787654, -0.02895312, 0.02282967, -0.01031555, 0.00163801, -0.00362018, -0.03988024, 0.39894228)


def ratio64(z):
    """R(z) = I1(z) / I0(z) in float64 (the scaled functions: no overflow); odd, R(+-inf) = +-1."""
    z = torch.as_tensor(np.asarray(z, np.float64))
    a = z.abs()
    r = torch.special.i1e(a) / torch.special.i0e(a)
    r = torch.where(torch.isinf(a), torch.ones_like(r), r)
    return (torch.sign(z) * r).numpy()


def c64(z):
    """c(z) = (z - |z|) - log i0e(|z|) in float64."""
    z = torch.as_tensor(np.asarray(z, np.float64))
    a = z.abs()
    return ((z - a) - torch.log(torch.special.i0e(a))).numpy()


def _horner32(coef, s):
    p = np.full(s.shape, np.float32(coef[0]), np.float32)
    for k in coef[1:]:
        p = (p * s).astype(np.float32)
        p = (p + np.float32(k)).astype(np.float32)
    return p


def _forms32(z):
    """The kernel's sequence on float32 z: (R(|z|) clamped to 1, c(z)), both float32."""
    z = np.asarray(z, np.float32)
    with np.errstate(all='ignore'):
        a = np.abs(z)
        small = a <= BRANCH
        t = (a / BRANCH).astype(np.float32)
        s = (t * t).astype(np.float32)
        u = (BRANCH / a).astype(np.float32)
        p0, q0 = _horner32(P0, s), _horner32(Q0, u)
        rs = ((a * _horner32(P1, s)).astype(np.float32) / p0).astype(np.float32)
        rl = (_horner32(Q1, u) / q0).astype(np.float32)
        r = np.minimum(np.where(small, rs, rl), np.float32(1.0)).astype(np.float32)
        l = np.log(np.where(small, p0, (q0 / np.sqrt(a).astype(np.float32)).astype(np.float32)).astype(np.float32))
        c0 = (np.where(small, a, np.float32(0.0)).astype(np.float32) - l.astype(np.float32)).astype(np.float32)
        c = (c0 + (z - a).astype(np.float32)).astype(np.float32)
        c = np.where(np.isinf(a), z, c).astype(np.float32)
    return r, c


def ratio32(z):
    """The kernel's R(z), float32: odd, |R| <= 1."""
    z = np.asarray(z, np.float32)
    return np.copysign(_forms32(z)[0], z).astype(np.float32)


def c32(z):
    """The kernel's c(z), float32."""
    return _forms32(z)[1]


def _spread(e, shape, axis):
    view = [1, 1, 1]
    view[axis] = int(shape[axis])
    return np.asarray(e, np.float32).reshape(view)


def z32(x, ay, e, tau, axis=None):
    """(p, z) as the kernel forms them: p = fl32(e[s] ay) (ay itself without e), z = fl32(fl32(tau x) p)."""
    x, ay = np.asarray(x, np.float32), np.asarray(ay, np.float32)
    p = ay if e is None else (ay * _spread(e, ay.shape, axis)).astype(np.float32)
    with np.errstate(all='ignore'):
        return p, ((np.float32(tau) * x).astype(np.float32) * p).astype(np.float32)


def terms32(x, ay, e, tau, axis=None):
    """(xt, c) float32 by the kernel's operation sequence: xt = fl32(x R(z)), +0 where x == 0; c = c(z)."""
    x = np.asarray(x, np.float32)
    _, z = z32(x, ay, e, tau, axis)
    with np.errstate(all='ignore'):
        xt = np.where(x == 0, np.float32(0.0), (x * ratio32(z)).astype(np.float32)).astype(np.float32)
    return xt, c32(z)


def terms64(x, ay, e, tau, axis=None):
    """(xt, c) in float64 from the float32 inputs: no rounding of p or z."""
    x64, ay64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(ay, np.float32).astype(np.float64)
    p = ay64 if e is None else ay64 * _spread(e, ay64.shape, axis).astype(np.float64)
    z = float(np.float32(tau)) * x64 * p
    return np.where(x64 == 0, 0.0, x64 * ratio64(z)), c64(z)


def sums64(c, g, axis):
    """(sums, bound, mag), each (S,) float64, of the per-slice sums of g c: the exact (math.fsum) sums of the summands
    fl64(g c) - numpy's float64 product is the kernel's rounding - the bound on their float64 accumulation in any order

        N_s 2^-53 sum |summand| (1 + N_s 2^-53)        (gain64.gain_sums64's, N_s the voxels of the slice)

    and sum |summand|.  ``c``: the terms as float64 values (float32 terms widened, or float64 terms); ``g``: float32 or
    None."""
    c = np.asarray(c, np.float64)
    col = c if g is None else np.asarray(g, np.float32).astype(np.float64) * c
    S = c.shape[axis]
    sums, bound, mags = np.zeros(S), np.zeros(S), np.zeros(S)
    for s in range(S):
        v = np.take(col, s, axis=axis).ravel()
        mag = math.fsum(np.abs(v).tolist())
        sums[s], mags[s] = math.fsum(v.tolist()), mag
        bound[s] = v.size * U53 * mag * (1.0 + v.size * U53)
    return sums, bound, mags


def nll64(x, mu, tau):
    """1/2 tau (x - mu)^2 + c(tau x mu) per voxel, float64: the negative log-likelihood without -log(tau x)."""
    x, mu = np.asarray(x, np.float64), np.asarray(mu, np.float64)
    return 0.5 * tau * (x - mu) ** 2 + c64(tau * x * mu)


def surrogate64(x, mu0, mu, tau):
    """The majoriser of ``nll64`` at mu0 as a function of mu: 1/2 tau (mu - x R(z0))^2 + const, the constant set so
    that it touches nll64 at mu = mu0."""
    x, mu0, mu = (np.asarray(v, np.float64) for v in (x, mu0, mu))
    xt = x * ratio64(tau * x * mu0)
    return 0.5 * tau * (mu - xt) ** 2 + (nll64(x, mu0, tau) - 0.5 * tau * (mu0 - xt) ** 2)


def rice(nu, sigma, shape, gen):
    """Seeded Rician samples |nu + sigma (n1 + i n2)| as float64 torch tensor."""
    n1 = torch.randn(shape, generator=gen, dtype=torch.float64)
    n2 = torch.randn(shape, generator=gen, dtype=torch.float64)
    return torch.sqrt((torch.as_tensor(nu, dtype=torch.float64) + sigma * n1) ** 2 + (sigma * n2) ** 2)


def fixed_point64(x, tau, n_steps=8):
    """mu <- mean(x R(tau x mu)) from the plain mean: the MM iteration on a flat region; returns (mu, mean)."""
    x = np.asarray(x, np.float64)
    mu = mean = float(x.mean())
    for _ in range(n_steps):
        mu = float((x * ratio64(tau * x * mu)).mean())
    return mu, mean
