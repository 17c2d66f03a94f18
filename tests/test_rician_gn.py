"""The Rician noise model in the rigid Gauss-Newton update and the gain estimate, without a GPU (sett.rician_gn;
DESIGN.md 8.15): the derivative tests/rgn64.py states against central differences of the Rician term in float64, the
majoriser's curvature claim, one Gauss-Newton step with the halving line search on a planted rigid problem, the gain rule
on the effective observation, the switch and what fit() refuses with and without it, the new symbol and its argument
checks (they come before anything touches the device; the pointers are never followed), and rgn64's float32 residual
against its float64 one."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gain64, gne64, rgn64, rician64, slice64, voxel64
from tests.test_rician import _cpu_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
ARMS = ('none', 'g', 'u', 'e', 'all')


def _problem(arm, axis=1, shape=(6, 5, 4)):
    """x >= 0 with zeros, a > 0 dyadic (multiples of 2^-6 in [0.5, 10): a +- h is exact); with the tests' tau = 0.1, z = tau x e a
    runs from 0 to about 10 (20 with gains), across the branch of the float32 forms at 3.75."""
    gen = torch.Generator().manual_seed(23 + ARMS.index(arm))
    x = (torch.rand(shape, generator=gen) * 10).double().numpy()
    x[x < 2.0] = 0.0
    a = (torch.randint(32, 640, shape, generator=gen).double() / 64.0).numpy()
    g = voxel64.weights(shape, 'ramp').double().numpy() if arm in ('g', 'all') else None
    u = slice64.weights(shape[axis], 'ramp', seed=3).double().numpy() if arm in ('u', 'all') else None
    e = gain64.gains(shape[axis], 'generic').double().numpy() if arm in ('e', 'all') else None
    return x, a, g, u, e, axis


def test_the_third_derivative_of_c_is_bounded_by_a_quarter():
    """c''' = -R'' and R'' = -R'/z + R/z^2 - 2 R R': |R''| <= 1/4 on a grid of 600 001 points of (0, 60] (its maximum,
    0.2245, is at z = 1.03; it decays like 1 / z^3 beyond) - the constant of the truncation term below.  And
    0 < R' <= 1/2: the term's curvature lies below the majoriser's."""
    z = np.linspace(1e-3, 60.0, 600001)
    r, rp = rician64.ratio64(z), rgn64.dratio64(z)
    r2 = -rp / z + r / z ** 2 - 2 * r * rp
    print('sup |R\'\'| = %.4f at z = %.3f; R\' in [%.3g, %.6f]' % (np.abs(r2).max(), z[np.abs(r2).argmax()], rp.min(), rp.max()))
    assert np.abs(r2).max() <= 0.25
    assert rp.min() > 0 and rp.max() <= 0.5 and float(rgn64.dratio64(0.0)) == 0.5


@pytest.mark.parametrize('arm', ARMS)
def test_the_residual_is_the_derivative_of_the_rician_term(arm):
    """Central differences of E in every component of a against tau W e (p - x R(z)), and the second difference
    against the majoriser's curvature tau W e^2.

    Rounding, as tests/test_gain_gn.py states it: one evaluation of E adds N terms; a term is W [1/2 tau (x - e a)^2 +
    c(z)] - 5 roundings for the square as there, a few more for c, which torch.special's i0e and log evaluate to a few
    ulp of 1 in absolute terms where i0e is near 1 - so |fl(E) - E| <= gamma M + 8 2^-53 sum W, gamma = (N + 16) 2^-53
    (1 + 1e-2), M = sum W [1/2 tau (|x| + e (|a| + h))^2 + c(tau x e (|a| + h))] (z >= 0 here, where c >= 0 grows with z).
    Truncation - the term is not a quadratic: the central difference is off by h^2 / 6 |d3E/da3| at most, and
    d3E/da3 = W (tau x e)^3 c'''(z) with |c'''| = |R''| <= 1/4 (the test above).  Hence, with r = gamma M + 8 2^-53 sum W,
        |FD1 - dE/da| <= r / h + h^2 / 24 W (tau x e)^3 + 16 2^-53 tau W e (|p| + |x|)   (the last: the derivative's own)
        FD2 <= tau W e^2 + 4 r / h^2        (the second difference is an average of d2E/da2 over [a - h, a + h])."""
    x, a, g, u, e, axis = _problem(arm)
    tau, h = 0.1, 2.0 ** -10
    N = a.size
    W = gne64.weight64(a.shape, axis, g, u)
    ev = np.broadcast_to(rgn64._e_at(e, a.shape, axis), a.shape)
    top = ev * (np.abs(a) + h)
    M = float(np.sum(np.where(x != 0, W * (0.5 * tau * (np.abs(x) + top) ** 2 + rician64.c64(tau * x * top)), 0.0)))
    r = (N + 16) * U53 * 1.01 * M + 8 * U53 * float(W.sum())
    d1 = rgn64.resid64(a, x, axis, g, u, e, tau)
    d2, cap = rgn64.hess64(a, x, axis, g, u, e, tau), rgn64.majoriser_curvature64(x, axis, g, u, e, tau)
    E0 = rgn64.energy64(a, x, axis, g, u, e, tau)
    worst1 = worst2 = 0.0
    for idx in np.ndindex(a.shape):
        ap, am = a.copy(), a.copy()
        ap[idx] += h
        am[idx] -= h
        assert ap[idx] - a[idx] == h and a[idx] - am[idx] == h  # (the steps are exact)
        Ep, Em = rgn64.energy64(ap, x, axis, g, u, e, tau), rgn64.energy64(am, x, axis, g, u, e, tau)
        fd1, fd2 = (Ep - Em) / (2 * h), (Ep - 2 * E0 + Em) / (h * h)
        b1 = r / h + h * h / 24 * W[idx] * (tau * x[idx] * ev[idx]) ** 3 \
            + 16 * U53 * tau * W[idx] * ev[idx] * (ev[idx] * abs(a[idx]) + abs(x[idx]))
        assert abs(fd1 - d1[idx]) <= b1, (idx, fd1, d1[idx], b1)
        assert fd2 <= cap[idx] + 4 * r / (h * h), (idx, fd2, cap[idx])
        worst1 = max(worst1, abs(fd1 - d1[idx]) / b1)
        worst2 = max(worst2, (fd2 - cap[idx]) / (4 * r / (h * h)))
    # the closed-form curvature lies below the majoriser's everywhere, strictly where there is data
    assert bool((d2 <= cap).all()) and bool((d2[(x != 0) & (W > 0)] < cap[(x != 0) & (W > 0)]).all())
    assert bool((d1[x == 0] == 0).all()) and bool((x == 0).any())
    z = tau * x * ev * a
    assert (z[x != 0] < 3.75).any() and (z > 3.75).any()
    print('%s: worst |FD1 - d1| / bound %.3g, worst (FD2 - tau W e^2) / rounding %.3g' % (arm, worst1, worst2))


@pytest.mark.parametrize('arm', ARMS)
def test_float32_residual_follows_the_float64_one(arm):
    """rgn64.resid32 (the kernel's operation sequence) lies within rgn64.terms_r64's stated bound of the float64
    residual, is +0 where x == 0, and its sums restate slice64's / voxel64's and rician64's."""
    x, a, g, u, e, axis = _problem(arm)
    f32 = lambda v: None if v is None else np.asarray(v, np.float32)
    x, a, g, u, e = f32(x), f32(a), f32(g), f32(u), f32(e)
    tau = 0.1
    out = rgn64.resid32(x, a, axis, g, u, e, tau)
    ref, bound, sums, sums_bound = rgn64.terms_r64(x, a, axis, g, u, e, tau)
    assert out.dtype == np.float32 and bool((np.abs(out - ref) <= bound).all())
    assert (out[x == 0].view(np.uint32) == 0).all()
    S = a.shape[axis]
    assert sums.shape == (3 * S,) and sums_bound.shape == (3 * S,)
    # tau times it is the derivative of the term
    d1 = rgn64.resid64(a, x, axis, g, u, e, float(np.float32(tau)))
    assert np.allclose(float(np.float32(tau)) * ref, d1, rtol=1e-12, atol=0)


def test_factor_table():
    u = slice64.weights(16, 'ramp', seed=3).numpy()
    e = gain64.gains(16, 'generic').numpy()
    assert rgn64.factor32(None, None) is None
    assert np.array_equal(rgn64.factor32(u, None), u) and np.array_equal(rgn64.factor32(None, e), e)
    assert np.array_equal(rgn64.factor32(u, e).view(np.uint32), gne64.tables(u, e)[2].view(np.uint32))


# ---- one Gauss-Newton step ---------------------------------------------------------------------------------------------------
def _image(r, q):
    """A smooth image - three Gaussian blobs on a floor - at the points r (N, 3) moved by q = (translation, small
    rotation about z through the middle of the volume), and its Jacobian in q (N, 4), float64, closed form."""
    r = r - np.array([5.5, 4.5, 2.5])
    c, s = np.cos(q[3]), np.sin(q[3])
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    dR = np.array([[-s, -c, 0.0], [c, -s, 0.0], [0.0, 0.0, 0.0]])
    m = r @ R.T + q[:3] + np.array([5.5, 4.5, 2.5])
    val, grad = np.full(len(r), 0.5), np.zeros((len(r), 3))
    for amp, mu, wd in ((4.0, (4.0, 5.0, 3.0), 2.5), (2.5, (8.0, 3.0, 4.0), 2.0), (1.5, (6.0, 8.0, 2.0), 3.0)):
        d = m - np.asarray(mu)
        b = amp * np.exp(-0.5 * (d * d).sum(1) / wd ** 2)
        val += b
        grad += -(b / wd ** 2)[:, None] * d
    J = np.concatenate([grad, (grad * (r @ dR.T)).sum(1, keepdims=True)], 1)
    return val, J


@pytest.mark.parametrize('sigma', [1.0, 0.5])
def test_one_gauss_newton_step_does_not_increase_the_rician_objective(sigma):
    """Rician samples (1 - 3 sigma in most of the volume) of the image under a planted q; from q = 0 one step with the
    exact gradient J^T tau W e (p - x R(z)), the majoriser's Hessian J^T (tau W e^2) J and the update's line search
    (halving, up to 6 evaluations, the start kept where none is lower): the exact objective does not increase, the step
    is a descent direction, and q moves towards the planted one."""
    shape, axis = (12, 10, 6), 2
    gen = torch.Generator().manual_seed(31)
    ii = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij'), -1).reshape(-1, 3)
    planted = np.array([0.6, -0.4, 0.3, 0.05])
    e = gain64.gains(shape[axis], 'generic').double().numpy()
    u = slice64.weights(shape[axis], 'ramp', seed=3).double().numpy()
    g = voxel64.weights(shape, 'ramp').double().numpy()
    ev = np.broadcast_to(gne64._at(e, shape, axis), shape).reshape(-1)
    W = gne64.weight64(shape, axis, g, u).reshape(-1)
    nu = ev * _image(ii, planted)[0]
    x = rician64.rice(torch.from_numpy(nu), sigma, nu.shape, gen).numpy()
    tau = sigma ** -2

    def objective(q):
        p = ev * _image(ii, q)[0]
        return float(np.sum(W * (0.5 * tau * (x - p) ** 2 + rician64.c64(tau * x * p))))

    q0 = np.zeros(4)
    a, J = _image(ii, q0)
    p = ev * a
    resid = tau * W * ev * (p - x * rician64.ratio64(tau * x * p))
    grad = J.T @ resid
    H = J.T @ ((tau * W * ev * ev)[:, None] * J)
    step = np.linalg.solve(H, grad)
    assert float(grad @ step) > 0  # (H is positive definite: -step is a descent direction)
    old, armijo, q, new, taken = objective(q0), 1.0, q0, None, None
    for n_ls in range(6):
        cand = q0 - armijo * step
        val = objective(cand)
        if val < old:
            q, new, taken = cand, val, n_ls
            break
        armijo *= 0.5
    new = old if new is None else new
    print('sigma %.1f: objective %.6f -> %.6f at halving %s; |q - planted| %.4f -> %.4f'
          % (sigma, old, new, taken, np.linalg.norm(q0 - planted), np.linalg.norm(q - planted)))
    assert new <= old
    assert taken is not None and np.linalg.norm(q - planted) < np.linalg.norm(q0 - planted)


# ---- the gain rule on the effective observation -------------------------------------------------------------------------------
@pytest.mark.parametrize('kappa', [0.0, 50.0])
def test_gain_rule_on_the_effective_observation_does_not_increase_the_objective(kappa):
    """4 096 seeded samples per slice, 8 slices with planted gains, signal at 1 - 3 sigma: from e0 = 1 (and from a
    second, generic start) the rule on x~ = x R(tau x e0 a) minimises the majoriser at e0 plus the ridge exactly, so
    F(e) = sum W [1/2 tau (x - e a)^2 + c(tau x e a)] + 1/2 kappa sum (e - 1)^2 does not increase - up to the rounding
    of the two evaluations of F, N 2^-53 sum |terms| each (a float64 sum of N terms in any order)."""
    from unires_amd._update import gain_rule
    S, n, tau = 8, 4096, 1.0
    gen = torch.Generator().manual_seed(41)
    a = (1.0 + 2.0 * torch.rand((S, n), generator=gen, dtype=torch.float64)).numpy()
    planted = gain64.gains(S, 'generic', seed=7).double().numpy()
    x = rician64.rice(torch.from_numpy(planted[:, None] * a), 1.0, (S, n), gen).numpy()
    x[torch.rand((S, n), generator=gen).numpy() < 0.1] = 0.0
    W = torch.rand((S, n), generator=gen, dtype=torch.float64).numpy()

    def F(e):
        p = e[:, None] * a
        terms = np.where(x != 0, W * (0.5 * tau * (x - p) ** 2 + rician64.c64(tau * x * p)), 0.0)
        return float(terms.sum() + 0.5 * kappa * ((e - 1.0) ** 2).sum()), float(np.abs(terms).sum())

    for e0 in (np.ones(S), gain64.gains(S, 'generic', seed=9).double().numpy()):
        xt = x * rician64.ratio64(tau * x * e0[:, None] * a)
        live = xt != 0  # (the rule's mask, read on x~: 0 exactly where x is)
        assert np.array_equal(live, x != 0)
        sums = np.concatenate([(W * xt * a * live).sum(1), (W * a * a * live).sum(1), (W * live).sum(1)])
        e1 = gain_rule(torch.from_numpy(sums), tau, kappa, 2.0).numpy()
        (f0, m0), (f1, m1) = F(e0), F(e1)
        slack = S * n * U53 * (m0 + m1)
        print('kappa %g: F %.6f -> %.6f (slack %.3g); max |e1 - planted| %.4f' % (kappa, f0, f1, slack, np.abs(e1 - planted).max()))
        assert f1 <= f0 + slack
        assert f1 < f0  # (and here it does decrease: e0 is not the minimiser)


# ---- the switch ----------------------------------------------------------------------------------------------------------------
def test_rician_gn_is_off_by_default():
    from unires_amd.struct import settings
    assert settings().rician_gn is False


def test_scaling_stays_refused_with_rician_gn():
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.max_iter = 3
    sett.noise_model, sett.rician_gn, sett.scaling = 'rician', True, True
    with pytest.raises(NotImplementedError, match=r"sett\.scaling with sett\.noise_model = 'rician'"):
        U.fit([[xn]], [y], sett)
    assert getattr(xn, '_rician_dat', None) is None


@pytest.mark.parametrize('user', [False, True])
def test_unified_rigid_with_gains_still_needs_gain_gn(user):
    """tests/test_gain.py's pinned refusal holds under the Rician model with the switch on."""
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.max_iter = 3
    sett.noise_model, sett.rician_gn, sett.unified_rigid = 'rician', True, True
    if user:
        xn.slice_gain = torch.ones(5)
    else:
        sett.slice_gain = True
    with pytest.raises(NotImplementedError, match='sett.unified_rigid') as err:
        U.fit([[xn]], [y], sett)
    assert 'sett.gain_gn' in str(err.value)


@pytest.mark.parametrize('names', [('unified_rigid',), ('slice_gain',), ('unified_rigid', 'slice_gain', 'gain_gn')])
def test_init_accepts_the_rigid_update_and_the_gain_estimate_with_rician_gn(names):
    """max_iter = 0: validation, no iteration, nothing on a device."""
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    sett.noise_model, sett.rician_gn = 'rician', True
    for name in names:
        setattr(sett, name, True)
    info = U.fit([[xn]], [y], sett)[3]
    assert info['n_iter'] == 0 and torch.equal(xn._rician_dat, xn.dat)
    assert (info['slice_gain'][0][0] is not None) == ('slice_gain' in names)


def test_the_switch_changes_nothing_under_the_gaussian_model():
    from unires_amd._update import _is_rician
    xn, y, sett = _cpu_structs()
    sett.rician_gn = True
    assert not _is_rician(xn, sett)
    sett.noise_model = 'rician'
    assert _is_rician(xn, sett)
    xn.ct = True
    assert not _is_rician(xn, sett)


# ---- the symbol, argument checks ----------------------------------------------------------------------------------------------
def test_symbol_declared_bound_and_exported(lib):
    from unires_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    assert re.search(r'\bint\s+unires_rigid_terms_r\s*\(', hdr)
    assert 'unires_rigid_terms_r' in _lib.SIGNATURES and len(_lib.SIGNATURES['unires_rigid_terms_r'][1]) == 11
    assert getattr(lib, 'unires_rigid_terms_r') is not None
    assert lib.unires_abi_version() == 1


def test_argument_errors_before_device_work(lib):
    """unires_slice_sums' codes for the same mistakes; g, u, e and out may be NULL."""
    from unires_amd import _lib
    buf, other = np.zeros(64, dtype=np.float32), np.zeros(64, dtype=np.float32)
    out = np.zeros(12, dtype=np.float64)
    p, q, o = buf.ctypes.data, other.ctypes.data, out.ctypes.data
    ok = _lib.i3((4, 4, 4))
    f = lib.unires_rigid_terms_r
    assert f(None, p, None, None, None, ok, 2, 1.0, o, None, None) == lib.unires_slice_sums(None, p, ok, 2, o, None) == 1
    assert f(p, None, None, None, None, ok, 2, 1.0, o, None, None) == lib.unires_slice_sums(p, None, ok, 2, o, None) == 1
    assert f(p, p, None, None, None, ok, 2, 1.0, None, None, None) == lib.unires_slice_sums(p, p, ok, 2, None, None) == 1
    for bad in (-1, 3):
        assert f(p, p, None, None, None, ok, bad, 1.0, o, None, None) == lib.unires_slice_sums(p, p, ok, bad, o, None) == 3
    for dims in ((0, 4, 4), (4, -1, 4)):
        d = _lib.i3(dims)
        assert f(p, p, None, None, None, d, 2, 1.0, o, None, None) == lib.unires_slice_sums(p, p, d, 2, o, None) == 2
    # the inputs are only read: out may be ay, not x or g
    assert f(p, q, None, None, None, ok, 1, 1.0, o, p, None) == 3
    assert b'out must not be' in lib.unires_last_error()
    assert f(q, q, p, None, None, ok, 1, 1.0, o, p, None) == 3
