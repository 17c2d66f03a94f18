"""The host side of the bias field (sett.bias, _input.bias_coef) without a GPU: the product identity
behind the Hessian, the gradient, the step rule, the orders, the prior, the defaults, the refusals and the validation of
a user's coefficients.  The float64 side is tests/bias64.py.  Every test here fails on the commit before the feature: the
package has no ``bias_step``, no ``bias_orders`` and no ``_init_bias``."""
import os

import numpy as np
import pytest
import torch

from tests import bias64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (5, 4, 6)


def _data(shape=SHAPE, seed=3, zeros=True):
    rng = np.random.default_rng(seed)
    mu = (50.0 + 30.0 * rng.random(shape)).astype(np.float32)
    x = (mu * (1.0 + 0.2 * rng.standard_normal(shape))).astype(np.float32)
    if zeros:
        x[rng.random(shape) < 0.1] = 0
    g = rng.random(shape).astype(np.float32)
    u = rng.random(shape[2]).astype(np.float32)
    return x, mu, g, u


@pytest.mark.parametrize('orders', [(1, 1, 1), (3, 1, 2), SHAPE])
def test_hessian_from_the_projection_is_the_dense_one(orders):
    """sum_v f Phi_k Phi_l assembled by ``bias_hessian`` from the projection of f onto the orders < 2 k - 1 against the
    dense basis, 1e-12 relative to the largest entry: k = 1 everywhere, a mixed case, and the complete basis k_d = n_d
    (orders up to 2 n - 2, beyond the grid's own n cosines: the identity is trigonometric, it needs no orthogonality)."""
    from unires_amd._update import bias_hessian, bias_tables
    rng = np.random.default_rng(7)
    f = rng.random(SHAPE) + 0.1
    tabs = bias_tables(SHAPE, orders)
    assert all(np.array_equal(a, b) for a, b in zip(tabs, bias64.tables64(SHAPE, orders)))  # the same bits
    assert all((t[0] == 1.0).all() for t in tabs)
    P = np.einsum('ijk,ai,bj,ck->abc', f, *tabs)
    _, dense = bias64.dense_terms64(f, f, SHAPE, orders)
    got = bias_hessian(P, orders)
    assert got.shape == dense.shape
    assert np.abs(got - dense).max() <= 1e-12 * np.abs(dense).max()
    assert np.abs(bias64.hessian_from_projection64(P, orders) - dense).max() <= 1e-12 * np.abs(dense).max()
    assert np.linalg.eigvalsh(got).min() > -1e-9 * np.abs(dense).max()  # (the Gauss-Newton curvature: f > 0)


def test_gradient_against_central_differences():
    """tau G + Lambda c of ``bias_step``, G the projection of W m r, against central differences of the float64
    objective at a generic c (inside the clamp), with voxel weights, slice weights and zeros in x."""
    from unires_amd._update import bias_step
    x, mu, g, u = _data()
    orders, tau = (3, 2, 2), 0.01
    rng = np.random.default_rng(5)
    c = 0.1 * rng.standard_normal(orders)
    lam = bias64.lambda64(SHAPE, (1.0, 1.0, 2.0), orders, tau * float((x.astype(np.float64) ** 2).sum()), 0.01, 60.0)
    b = np.exp(bias64.beta64(c, SHAPE))
    W = bias64.weights64(SHAPE, g, u, 2) * (x != 0)
    m = b * mu
    tabs = bias64.tables64(SHAPE, orders)
    G = np.einsum('ijk,ai,bj,ck->abc', W * m * (m - x), *[t[:k] for t, k in zip(tabs, orders)])
    P = np.einsum('ijk,ai,bj,ck->abc', W * m * m, *tabs)
    cands, grad, H = bias_step(c, G, P, lam, tau)
    assert np.allclose(grad, bias64.gradient64(c, x, mu, g, u, 2, lam, tau), rtol=1e-12, atol=0)
    E = lambda cc: bias64.objective64(cc, x, mu, g, u, 2, lam, tau)
    h = 1e-5
    for idx in np.ndindex(*orders):
        e = np.zeros(orders)
        e[idx] = h
        fd = (E(c + e) - E(c - e)) / (2 * h)
        assert abs(fd - grad[idx]) <= 1e-6 * max(np.abs(grad).max(), 1.0), (idx, fd, grad[idx])
    # the restated rule gives the same step, and the candidates are c + s Delta in the line search's order
    delta, grad2, H2 = bias64.step64(c, G, P, lam, tau)
    assert np.allclose(H, H2, rtol=1e-12, atol=0) and np.allclose(grad, grad2, rtol=1e-13, atol=0)
    assert len(cands) == 6
    for s, cand in zip(bias64.STEPS, cands):
        assert np.allclose(cand, c + s * delta, rtol=1e-9, atol=1e-12)


def test_accepted_step_never_raises_the_objective():
    """From c = 0 on data with a planted field, five steps of the rule with the float64 objective as the line search's
    E: the accepted E never rises, and falls at the first; where no candidate is accepted c stays."""
    from unires_amd._update import BIAS_STEPS, bias_energy, bias_step
    x, mu, g, u = _data(seed=11)
    orders, tau = (2, 2, 2), 0.02
    planted = np.zeros(orders)
    planted[0, 0, 0], planted[1, 0, 0], planted[0, 1, 1] = 0.1, 0.15, -0.1
    x = (x * np.exp(bias64.beta64(planted, SHAPE))).astype(np.float32)
    lam = bias64.lambda64(SHAPE, (1.0, 1.0, 2.0), orders, tau * float((x.astype(np.float64) ** 2).sum()), 0.01, 60.0)
    assert BIAS_STEPS == bias64.STEPS
    c = np.zeros(orders)
    E = lambda cc: bias64.objective64(cc, x, mu, g, u, 2, lam, tau)
    tabs = bias64.tables64(SHAPE, orders)
    trace = [E(c)]
    for it in range(5):
        b = np.exp(bias64.beta64(c, SHAPE))
        W = bias64.weights64(SHAPE, g, u, 2) * (x != 0)
        m = b * mu
        S = float((W * (m - x) ** 2).sum())
        assert abs(bias_energy(S, c, lam, tau) - E(c)) <= 1e-12 * E(c)
        G = np.einsum('ijk,ai,bj,ck->abc', W * m * (m - x), *[t[:k] for t, k in zip(tabs, orders)])
        P = np.einsum('ijk,ai,bj,ck->abc', W * m * m, *tabs)
        cands, _, _ = bias_step(c, G, P, lam, tau)
        for cand in cands:
            if E(cand) <= trace[-1]:
                c = cand
                break
        trace.append(E(c))
    assert all(b_ <= a_ for a_, b_ in zip(trace, trace[1:])), trace
    assert trace[1] < trace[0]
    # a singular system (no data, no prior): no candidates, c stays
    cands, _, _ = bias_step(np.zeros(orders), np.zeros(orders), np.zeros((3, 3, 3)), np.zeros(orders), tau)
    assert cands == []


def test_bias_orders_at_their_clamps():
    """k_d = clamp(ceil(2 n_d vx_d / cutoff), 1, min(8, n_d)): a 3-slice axis stops at 3; a cut-off longer than twice
    the field of view gives 1; a field of view that would give more than 8 stops at 8; and an unclamped case."""
    import unires_amd as U
    from unires_amd._update import bias_orders, bias_orders_of
    assert bias_orders_of((256, 256, 3), (1.0, 1.0, 50.0), 60.0) == (8, 8, 3)       # ceil(8.53) -> 8; ceil(5) -> 3 slices
    assert bias_orders_of((20, 20, 20), (1.0, 1.0, 1.0), 60.0) == (1, 1, 1)          # 2 * 20 / 60 < 1
    assert bias_orders_of((300, 100, 42), (1.0, 1.0, 4.0), 60.0) == (8, 4, 6)        # 10 -> 8; ceil(3.33); ceil(5.6)
    assert bias_orders_of((90, 91, 1), (1.0, 1.0, 1.0), 60.0) == (3, 4, 1)           # exactly 3 stays 3; 3.03 -> 4
    sett = U.settings()
    xn = U._input(torch.zeros(64, 48, 10), torch.diag(torch.tensor([2.0, 1.5, 6.0, 1.0], dtype=torch.float64)), 1.0)
    assert bias_orders(xn, sett) == bias64.orders64((64, 48, 10), (2.0, 1.5, 6.0), 60.0) == (5, 3, 2)
    sett.bias_cutoff = 30.0
    assert bias_orders(xn, sett) == (8, 5, 4)


def test_prior_against_its_formulas():
    """Lambda = kappa bias_reg (1 + sum_d (cutoff m_d / (2 n_d vx_d))^2) entry by entry, kappa = tau sum x^2."""
    import unires_amd as U
    from unires_amd._update import bias_kappa, bias_lambda
    sett = U.settings()
    shape, vx, orders = (12, 10, 9), (1.0, 2.0, 3.0), (3, 2, 4)
    got = bias_lambda(shape, vx, orders, 7.5, sett)
    want = bias64.lambda64(shape, vx, orders, 7.5, 0.01, 60.0)
    assert got.shape == orders and np.allclose(got, want, rtol=1e-14, atol=0)
    assert got[0, 0, 0] == 7.5 * 0.01
    assert np.isclose(got[2, 1, 3], 7.5 * 0.01 * (1 + (60 * 2 / 24.0) ** 2 + (60 * 1 / 40.0) ** 2 + (60 * 3 / 54.0) ** 2), rtol=1e-14)
    x = torch.tensor([[[0.0, 2.0], [3.0, 0.0]]])
    xn = U._input(x, torch.eye(4, dtype=torch.float64), 0.5)
    k = bias_kappa(xn)
    assert k.dtype == torch.float64 and float(k) == 0.5 * 13.0


def test_defaults():
    import unires_amd as U
    s = U.settings()
    assert s.bias is False and s.bias_cutoff == 60.0 and s.bias_reg == 0.01 and s.bias_max == 4.0
    assert U._input().bias_coef is None
    assert callable(U.bias_field) and callable(U._update_bias)
    from unires_amd import _lib
    for name in ('unires_bias_field', 'unires_bias_terms'):
        assert name in _lib.SIGNATURES
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert "'bias.hip'" in entry and "'bias.hpp'" in entry


def _structs(coef=None):
    import unires_amd as U
    xn = U._input(torch.ones(6, 5, 4), torch.eye(4, dtype=torch.float64), 1.0)
    xn.bias_coef = coef
    return [[xn]], U.settings()


@pytest.mark.parametrize('name,value', [('noise_model', 'rician'), ('scaling', True), ('unified_rigid', True),
                                        ('slice_gain', True)])
@pytest.mark.parametrize('how', ['sett', 'coef'])
def test_refused_by_name(name, value, how):
    """sett.bias, or a user's bias_coef alone, with each of the four settings: NotImplementedError naming it, before
    anything touches a device."""
    from unires_amd.run import _init_bias
    x, sett = _structs(torch.zeros(2, 2, 1, dtype=torch.float64) if how == 'coef' else None)
    sett.bias = how == 'sett'
    setattr(sett, name, value)
    with pytest.raises(NotImplementedError, match=name if name != 'noise_model' else 'rician'):
        _init_bias(x, sett, torch.device('cpu'))


@pytest.mark.parametrize('coef,msg', [
    (torch.zeros(2, 2), 'shape'), (torch.zeros(9, 1, 1), 'shape'), (torch.zeros(2, 2, 5), 'shape'),
    (torch.zeros(0, 1, 1), 'shape'), (torch.tensor([[[float('nan')]]]), 'finite'),
    (torch.tensor([[[float('inf')]]]), 'finite'), (torch.zeros(1, 1, 1, dtype=torch.complex64), 'real'),
    (torch.zeros(1, 1, 1, dtype=torch.bool), 'real')])
def test_validation_of_bias_coef(coef, msg):
    """A wrong rank, more than 8 or more than n_d orders, an empty axis, a non-finite or non-real value: ValueError
    naming channel and repeat, before anything touches a device."""
    from unires_amd.run import _init_bias
    x, sett = _structs(coef)
    with pytest.raises(ValueError, match=r'x\[0\]\[0\]\.bias_coef.*' + msg):
        _init_bias(x, sett, torch.device('cpu'))


def test_bad_settings_and_no_field_leaves_no_state():
    from unires_amd.run import _init_bias
    for name, bad in (('bias_cutoff', 0.0), ('bias_reg', -1.0), ('bias_max', 1.0)):
        x, sett = _structs()
        sett.bias = True
        setattr(sett, name, bad)
        with pytest.raises(ValueError, match=name):
            _init_bias(x, sett, torch.device('cpu'))
    x, sett = _structs()
    x[0][0]._bias_b = 'stale'
    _init_bias(x, sett, torch.device('cpu'))  # off and no coefficients: an earlier fit()'s field is forgotten
    assert x[0][0]._bias_b is None and x[0][0]._bias_dat is None and x[0][0]._bias_weight is None
    with pytest.raises(ValueError, match='coef'):
        import unires_amd as U
        U.bias_field(torch.zeros(9, 1, 1), (16, 4, 4))
