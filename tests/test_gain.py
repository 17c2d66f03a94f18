"""Per-slice intensity gains without a device: the gain rule against the dense 1-D quadratic it
minimises (the library's tensor form against tests/gain64.py's restatement), the algebra of the gained y-update system
on dense float64 matrices built from tests/ref64.py's Operator64, the composed tables, and the host side: settings,
fit()'s refusals and validation, the new symbols.

The system is  sum_n tau_n A_n^T diag(W_n e_n^2) A_n + rho lam^2 D^T D  with the right-hand side
sum_n tau_n A_n^T (W_n e_n x_n), e_n constant over each slice along ``po.dim_thick``.  The reference has no counterpart.
"""
import os

import numpy as np
import pytest
import torch

from tests import diff64, gain64, ref64, slice64
from tests.helpers import make_problem, oracle_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM_Y = (6, 5, 4)
GMAX = 3.0  # (no test depends on the defaults of sett.gain_reg and sett.gain_max)


# ---- the rule ---------------------------------------------------------------------------------------------------------
# (P_s, Q_s, kappa) with tau = 1: interior, both clamps, Q = 0 with and without a prior, kappa = 0, a negative P
RULE_CASES = [(9.0, 10.0, 1.0), (11.5, 10.0, 1.0), (100.0, 10.0, 1.0), (0.1, 10.0, 1.0), (0.0, 0.0, 1.0),
              (0.0, 0.0, 0.0), (8.5, 10.0, 0.0), (50.0, 10.0, 0.0), (-3.0, 10.0, 0.5), (3.0, 10.0, 1e6)]


def _both(P, Q, kappa, tau=1.0, gmax=GMAX):
    from unires_amd._update import gain_rule
    S = len(P)
    sums = np.array(list(P) + list(Q) + [1.0] * S, np.float64)
    got = gain_rule(torch.from_numpy(sums), tau, kappa, gmax).numpy()
    want = gain64.rule64(sums, tau, kappa, gmax)
    assert got.dtype == np.float64 and np.array_equal(got, want), (got, want)
    got_t = gain_rule(torch.from_numpy(sums), tau, torch.tensor(kappa, dtype=torch.float64), gmax).numpy()
    assert np.array_equal(got_t, want)  # (kappa as the 0-d device tensor fit() keeps)
    return got


@pytest.mark.parametrize('P, Q, kappa', RULE_CASES)
def test_rule_is_the_arg_min_of_the_dense_quadratic(P, Q, kappa):
    """f(e) = 1/2 (Q e^2 - 2 P e) + 1/2 kappa (e - 1)^2 on a grid of 20 001 points over [1 / gmax, gmax]: the rule's
    value is no worse than the best grid point, and lies within one grid step of it where the minimiser is unique."""
    e = float(_both([P], [Q], kappa)[0])
    assert 1.0 / GMAX <= e <= GMAX
    grid = np.linspace(1.0 / GMAX, GMAX, 20001)
    f = lambda t: 0.5 * (Q * t * t - 2.0 * P * t) + 0.5 * kappa * (t - 1.0) ** 2
    best = grid[np.argmin(f(grid))]
    assert f(e) <= f(grid).min() + 1e-12 * max(1.0, abs(f(grid)).max())
    if Q + kappa > 0:
        assert abs(e - best) <= grid[1] - grid[0]
    else:
        assert e == 1.0  # (no data and no prior: f is flat, the gain stays 1)


def test_rule_clamps_at_both_ends_and_keeps_empty_slices_at_one():
    e = _both([100.0, 0.1, 0.0, 9.0], [10.0, 10.0, 0.0, 10.0], 1.0)
    assert e[0] == GMAX and e[1] == 1.0 / GMAX and e[2] == 1.0
    assert e[3] == (9.0 + 1.0) / (10.0 + 1.0)
    # all-zero weights (every sum 0) and an all-zero observation (kappa = 0 too): ones
    assert list(_both([0.0] * 3, [0.0] * 3, 0.7)) == [1.0] * 3
    assert list(_both([0.0] * 3, [0.0] * 3, 0.0)) == [1.0] * 3
    # tau scales the sums, not kappa
    assert _both([9.0], [10.0], 1.0, tau=2.0)[0] == 19.0 / 21.0


@pytest.mark.parametrize('seed', range(5))
def test_one_gain_step_never_increases_the_energy(seed):
    """At a fixed y and W: E(rule) <= E(e0) for any start e0 in the interval, on seeded slices (one of them empty)."""
    rng = np.random.default_rng(seed)
    S, n = 7, 40
    x = rng.normal(100.0, 30.0, (S, n))
    a = x / rng.uniform(0.7, 1.4, (S, 1)) + rng.normal(0.0, 5.0, (S, n))
    W = rng.uniform(0.0, 1.0, (S, n))
    W[3] = 0.0
    tau, kappa = 0.02, rng.uniform(0.0, 50.0)
    X, P, Q = tau * (W * x * x).sum(1), tau * (W * x * a).sum(1), tau * (W * a * a).sum(1)
    sums = np.concatenate([P / tau, Q / tau, W.sum(1)])
    e1 = gain64.rule64(sums, tau, kappa, GMAX)
    for _ in range(20):
        e0 = rng.uniform(1.0 / GMAX, GMAX, S)
        E0, E1 = gain64.energy64(e0, P, Q, X, kappa), gain64.energy64(e1, P, Q, X, kappa)
        assert E1 <= E0 + 1e-12 * abs(E0)
    assert e1[3] == 1.0 or kappa == 0.0


# ---- the system -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny():
    """One thick-slice repeat at 6 x 5 x 4 (thick 2 along z, a general rigid): the dense matrix of A."""
    prob = make_problem(seed=3, dim_y=DIM_Y, thick=2, thick_axes=[2], rot=0.1, trans=0.4, scl=0.0)
    xs, ys = oracle_structs(prob)
    po = xs[0][0].po
    op = ref64.Operator64(po, 'super-resolution')
    ny = int(np.prod(DIM_Y))
    eye = lambda n, i: torch.nn.functional.one_hot(torch.tensor(i), n).double()
    A = torch.stack([op.A(eye(ny, j).reshape(DIM_Y)).reshape(-1) for j in range(ny)], 1).numpy()
    from unires_amd._project import _slice_axis
    axis = _slice_axis(xs[0][0])
    assert axis == int(po.dim_thick) == 2
    S = int(op.dim_x[axis])
    g = torch.rand(tuple(op.dim_x), generator=torch.Generator().manual_seed(5)).double()
    W = (g * slice64.spread(slice64.weights(S, 'ramp'), op.dim_x, axis)).numpy().reshape(-1)
    reg = 0.7 * float(ys[0].lam) ** 2 * diff64.dense_dtd(DIM_Y, [1.0, 1.0, 1.0], 'forward')
    return dict(op=op, A=A, axis=axis, S=S, W=W, reg=reg, tau=float(xs[0][0].tau),
                x=xs[0][0].dat.double().numpy().reshape(-1))


def _gained(t, e, W=None):
    """The dense matrix of A^T diag(W e^2) A, e the (S,) gains spread over x space."""
    ev = slice64.spread(e, t['op'].dim_x, t['axis']).numpy().reshape(-1)
    W = t['W'] if W is None else W
    return t['A'].T @ ((W * ev * ev)[:, None] * t['A']), ev


def test_gained_normal_matrix_is_symmetric_psd_and_is_the_weighted_one_at_unit_gains(tiny):
    H, _ = _gained(tiny, gain64.gains(tiny['S'], 'generic'))
    scale = np.abs(tiny['A'].T @ tiny['A']).max()
    assert np.abs(H - H.T).max() <= 1e-12 * scale
    assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-12 * scale
    H1, _ = _gained(tiny, gain64.gains(tiny['S'], 'ones'))
    assert np.array_equal(H1, tiny['A'].T @ (tiny['W'][:, None] * tiny['A']))


def test_gained_system_is_positive_definite_and_its_solution_is_stationary(tiny):
    """PD with the zero-bound D^T D, even with all weights 0; and the solution of H y = tau A^T (W e x) zeroes the
    gradient of 1/2 tau sum W (x - e A y)^2 + 1/2 y^T R y, written out on its own."""
    for pattern in ('generic', 'pow2', 'ones'):
        e = gain64.gains(tiny['S'], pattern)
        for W in (tiny['W'], np.zeros_like(tiny['W'])):
            H, ev = _gained(tiny, e, W)
            H = tiny['tau'] * H + tiny['reg']
            assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() > 0, pattern
    e = gain64.gains(tiny['S'], 'generic')
    H, ev = _gained(tiny, e)
    H = tiny['tau'] * H + tiny['reg']
    b = tiny['tau'] * (tiny['A'].T @ (tiny['W'] * ev * tiny['x']))
    y = np.linalg.solve(H, b)
    grad = -tiny['tau'] * (tiny['A'].T @ (tiny['W'] * ev * (tiny['x'] - ev * (tiny['A'] @ y)))) + tiny['reg'] @ y
    assert np.abs(grad).max() <= 1e-10 * np.abs(b).max()
    # ... and it is not the solution without gains
    y1 = np.linalg.solve(tiny['tau'] * _gained(tiny, gain64.gains(tiny['S'], 'ones'))[0] + tiny['reg'],
                         tiny['tau'] * (tiny['A'].T @ (tiny['W'] * tiny['x'])))
    assert np.abs(y - y1).max() > 1e-3 * np.abs(y).max()


# ---- the tables -------------------------------------------------------------------------------------------------------
def test_unit_gains_compose_to_the_weights_bit_for_bit():
    bits = lambda v: np.asarray(v, np.float32).view(np.uint32)
    for pattern in ('ramp', 'pow2', 'ones', 'zeros'):
        u = slice64.weights(37, pattern).numpy()
        w_mat, w_rhs = gain64.compose32(u, np.ones(37, np.float32))
        assert np.array_equal(bits(w_mat), bits(u)) and np.array_equal(bits(w_rhs), bits(u)), pattern
    e = gain64.gains(37, 'generic').numpy()
    w_mat, w_rhs = gain64.compose32(None, e)
    assert np.array_equal(bits(w_rhs), bits(e))
    assert np.array_equal(bits(w_mat), bits((e.astype(np.float64) ** 2).astype(np.float32)))  # fl32(e e): e e is exact in float64


# ---- the host side ----------------------------------------------------------------------------------------------------
def test_settings_and_struct_defaults():
    from unires_amd.struct import _input, settings
    s = settings()
    assert s.slice_gain is False
    assert isinstance(s.gain_reg, float) and s.gain_reg >= 0
    assert isinstance(s.gain_max, float) and s.gain_max > 1
    assert _input().slice_gain is None


def _cpu_structs():
    from unires_amd.struct import _input, _output, _proj_op, settings
    xn = _input(dat=torch.ones(4, 5, 6), mat=torch.eye(4, dtype=torch.float64))
    xn.po = _proj_op()
    xn.po.dim_thick = 1
    y = _output(dat=torch.zeros(4, 5, 6), mat=torch.eye(4, dtype=torch.float64), lam=1.0)
    sett = settings()
    sett.max_iter = 0
    return xn, y, sett


@pytest.mark.parametrize('user', [False, True])
def test_fit_refuses_scaling_and_unified_rigid_with_gains(user):
    """Before the first iteration, by name: with sett.slice_gain and with a user's gains alone."""
    import unires_amd as U
    for name, exc in (('scaling', ValueError), ('unified_rigid', NotImplementedError)):
        xn, y, sett = _cpu_structs()
        sett.max_iter = 3
        if user:
            xn.slice_gain = torch.ones(5)
        else:
            sett.slice_gain = True
        setattr(sett, name, True)
        with pytest.raises(exc, match='sett.%s' % name):
            U.fit([[xn]], [y], sett)
    # without gains both settings are left alone by the check
    from unires_amd.run import _init_slice_gains
    xn, y, sett = _cpu_structs()
    sett.scaling = sett.unified_rigid = True
    _init_slice_gains([[xn]], sett, torch.device('cpu'))
    assert xn.slice_gain is None


@pytest.mark.parametrize('bad, word', [(torch.ones(4), 'shape'), (torch.ones(5, 1), 'shape'),
                                       (torch.tensor([1.0, 1.0, float('nan'), 1.0, 1.0]), 'finite'),
                                       (torch.tensor([1.0, 1.0, float('inf'), 1.0, 1.0]), 'finite'),
                                       (torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0]), '> 0'),
                                       (torch.tensor([1.0, -0.5, 1.0, 1.0, 1.0]), '> 0'),
                                       (torch.ones(5, dtype=torch.bool), 'real')])
def test_fit_refuses_bad_user_gains_naming_channel_and_repeat(bad, word):
    """One gain per slice along po.dim_thick (axis 1 here: 5 slices), real, finite, > 0: checked before anything runs,
    and the message names x[channel][repeat]."""
    import unires_amd as U
    good, _, _ = _cpu_structs()
    xn, y, sett = _cpu_structs()
    xn.slice_gain = bad
    with pytest.raises(ValueError, match=word) as err:
        U.fit([[good, xn]], [y], sett)
    assert 'x[0][1].slice_gain' in str(err.value)


def test_fit_validation_accepts_good_gains_and_starts_estimated_fits_from_them_or_ones():
    from unires_amd.run import _init_slice_gains
    xn, y, sett = _cpu_structs()
    xn.slice_gain = [1, 0.9, 1.1, 1, 1]  # (anything torch.as_tensor takes)
    _init_slice_gains([[xn]], sett, torch.device('cpu'))
    assert xn.slice_gain.dtype == torch.float32 and xn.slice_gain.tolist() == torch.tensor([1, 0.9, 1.1, 1, 1]).tolist()
    assert xn._gain_kappa is None  # (estimation off: no prior)
    xn.slice_gain = None
    _init_slice_gains([[xn]], sett, torch.device('cpu'))
    assert xn.slice_gain is None  # off: nothing is made up
    sett.slice_gain = True
    user = torch.tensor([1.0, 0.9, 1.1, 1.0, 1.0])
    ct, _, _ = _cpu_structs()
    ct.ct = True
    xn.slice_gain = user
    _init_slice_gains([[xn, ct]], sett, torch.device('cpu'))
    assert torch.equal(xn.slice_gain, user) and xn.slice_gain.data_ptr() != user.data_ptr()  # (written in place later)
    assert ct.slice_gain is None and ct._gain_kappa is None  # (CT repeats are not estimated)
    # kappa = gain_reg tau sum x^2 / K: ones(4, 5, 6), 5 slices of 24 voxels
    assert float(xn._gain_kappa) == sett.gain_reg * xn.tau * 120.0 / 5.0
    zero, _, _ = _cpu_structs()
    zero.dat = torch.zeros(4, 5, 6)
    _init_slice_gains([[zero]], sett, torch.device('cpu'))
    assert zero.slice_gain.tolist() == [1.0] * 5 and float(zero._gain_kappa) == 0.0


def test_fit_reports_no_gains_with_the_feature_off():
    import unires_amd as U
    xn, y, sett = _cpu_structs()
    xn.po.rigid = torch.eye(4, dtype=torch.float64)
    sett.clean_fov = False
    info = U.fit([[xn]], [y], sett)[3]
    assert info['slice_gain'] == [[None]]


def test_new_symbols_are_in_the_header_and_in_the_ctypes_table():
    from unires_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'unires_hip.h')).read()
    for name in ('unires_gain_sums', 'unires_slice_apply', 'unires_plan_set_slice_gains'):
        assert 'int %s(' % name in header, name
        assert name in _lib.SIGNATURES, name
    assert 'gain.hip' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
