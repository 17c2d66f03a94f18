"""The deferred iterate update of tol = 0 solves (unires_plan_cg_ring; cg.hip k_update_p_ring / k_update_p_flush):
x takes the alpha p terms of a ring of K iterations at once, in iteration order, with the same roundings - so x must
be the same bits as with K = 1 (the iterate updated every iteration, the kernels of the solves outside the scope).
Covered: K in {2, 3, 8} and K >= max_iter, iteration counts that are not multiples of K, volumes whose size is not a
multiple of 4 (the kernels' scalar tails), graph-replayed and plain launches, the channels' joint solve on separate
streams and on one, the Jacobi preconditioner, the fallback to K = 1 when the ring does not fit its budget, and that
solves outside the scope report K = 1."""
import os

import pytest
import torch

from tests.helpers import gpu_structs, make_problem

pytestmark = pytest.mark.gpu

DIMS = {'even': (20, 18, 16), 'tail': (17, 13, 11)}  # 5 760 and 2 431 voxels


def _setup(dev, dims, n_channels=1, seed=91):
    prob = make_problem(seed=seed, dim_y=dims, n_channels=n_channels, thick=4, regime='sr', scl=0.1)
    xg, yg, sett = gpu_structs(prob, dev)
    torch.manual_seed(seed)
    bs = [torch.rand(dims, device=dev) - 0.5 for _ in range(n_channels)]
    x0s = [yg[c].dat.clone() for c in range(n_channels)]
    return prob, xg, yg, sett, bs, x0s


def _plan(xg, yg, sett, c, k):
    from unires_amd._project import _channel_plan
    yg[c]._plan = None  # (a plan of its own for every call: the cache would hand back the previous one)
    plan = _channel_plan(xg[c], yg[c], sett.method, sett.do_proj)
    plan.cg_ring(k)
    return plan


def _solve(plan, b, x0, rho, lam, max_iter, **kw):
    x = x0.clone()
    plan.cg(b, x, rho, lam, max_iter=max_iter, tolerance=0, **kw)
    torch.cuda.synchronize()
    return x


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('dims', list(DIMS))
@pytest.mark.parametrize('k,max_iter', [(2, 7), (3, 20), (3, 9), (8, 20), (8, 16), (8, 5), (8, 1)])
def test_ring_is_bit_identical_to_the_iterate_updated_every_iteration(dev, dims, k, max_iter):
    prob, xg, yg, sett, bs, x0s = _setup(dev, DIMS[dims])
    rho, lam = float(prob['rho']), float(yg[0].lam)
    p1, pk = _plan(xg, yg, sett, 0, 1), _plan(xg, yg, sett, 0, k)
    ref = _solve(p1, bs[0], x0s[0], rho, lam, max_iter)
    assert p1.cg_ring() == 1
    for rep in range(3):  # capture, replay, replay
        x = _solve(pk, bs[0], x0s[0], rho, lam, max_iter)
        assert pk.cg_ring() == k
        assert _same_bits(x, ref), (rep, (x - ref).abs().max().item())
    assert not _same_bits(ref, x0s[0])  # (the solve did move x)


@pytest.mark.parametrize('mode', [1, 2])
def test_plain_launches_agree_with_the_replayed_graph(dev, mode):
    """time_matvecs(1): the solve runs as plain launches with events; (2): every A(p) twice inside the graph."""
    prob, xg, yg, sett, bs, x0s = _setup(dev, DIMS['tail'], seed=92)
    rho, lam = float(prob['rho']), float(yg[0].lam)
    p1, pk = _plan(xg, yg, sett, 0, 1), _plan(xg, yg, sett, 0, 8)
    ref = _solve(p1, bs[0], x0s[0], rho, lam, 19)
    graph = _solve(pk, bs[0], x0s[0], rho, lam, 19)
    pk.time_matvecs(mode)
    plain = _solve(pk, bs[0], x0s[0], rho, lam, 19)
    assert pk.cg_ring() == 8
    if mode == 1:
        assert pk.matvec_time()[0] == 19
    pk.time_matvecs(False)
    again = _solve(pk, bs[0], x0s[0], rho, lam, 19)
    assert _same_bits(graph, ref) and _same_bits(plain, ref) and _same_bits(again, ref)


@pytest.mark.parametrize('streams', [True, False])
def test_joint_solve_of_the_channels(dev, streams):
    from unires_amd._plan import cg_many
    prob, xg, yg, sett, bs, x0s = _setup(dev, DIMS['even'], n_channels=3, seed=93)
    rho, lams = float(prob['rho']), [float(yc.lam) for yc in yg]
    refs = []
    for c in range(3):
        refs.append(_solve(_plan(xg, yg, sett, c, 1), bs[c], x0s[c], rho, lams[c], 13))
    plans = [_plan(xg, yg, sett, c, 8) for c in range(3)]
    sts = [torch.cuda.Stream(device=dev) for _ in range(3)] if streams else [torch.cuda.current_stream(dev)] * 3
    for rep in range(2):
        xs = [x0.clone() for x0 in x0s]
        torch.cuda.synchronize()
        cg_many(plans, bs, xs, rho, lams, sts, max_iter=13, tolerance=0)
        torch.cuda.synchronize()
        for c in range(3):
            assert plans[c].cg_ring() == 8
            assert _same_bits(xs[c], refs[c]), (rep, c)


def test_jacobi_preconditioned_solve(dev):
    prob, xg, yg, sett, bs, x0s = _setup(dev, DIMS['tail'], seed=94)
    rho, lam = float(prob['rho']), float(yg[0].lam)
    p1, pk = _plan(xg, yg, sett, 0, 1), _plan(xg, yg, sett, 0, 3)
    for p in (p1, pk):
        p.precond_build(rho, lam, mode='jacobi')
    ref = _solve(p1, bs[0], x0s[0], rho, lam, 11, precond='jacobi')
    x = _solve(pk, bs[0], x0s[0], rho, lam, 11, precond='jacobi')
    assert pk.cg_ring() == 3 and _same_bits(x, ref)


def test_ring_that_does_not_fit_its_budget_falls_back(dev, monkeypatch):
    prob, xg, yg, sett, bs, x0s = _setup(dev, DIMS['even'], seed=95)
    rho, lam = float(prob['rho']), float(yg[0].lam)
    ref = _solve(_plan(xg, yg, sett, 0, 1), bs[0], x0s[0], rho, lam, 10)
    monkeypatch.setenv('UNIRES_CG_RING_MB', '0')
    p0 = _plan(xg, yg, sett, 0, 8)
    x = _solve(p0, bs[0], x0s[0], rho, lam, 10)
    assert p0.cg_ring() == 1 and _same_bits(x, ref)
    # a budget of two direction buffers: K = 3 although 8 was asked for, and it stays so
    slot_mb = (DIMS['even'][0] * DIMS['even'][1] * DIMS['even'][2] * 4 + 255) // 256 * 256 / 1048576
    monkeypatch.setenv('UNIRES_CG_RING_MB', repr(2.5 * slot_mb))
    p2 = _plan(xg, yg, sett, 0, 8)
    x = _solve(p2, bs[0], x0s[0], rho, lam, 10)
    assert p2.cg_ring() == 3 and _same_bits(x, ref)
    monkeypatch.delenv('UNIRES_CG_RING_MB')
    x = _solve(p2, bs[0], x0s[0], rho, lam, 10)
    assert p2.cg_ring() == 3 and _same_bits(x, ref)


def test_solves_outside_the_scope_keep_the_iterate_updated_every_iteration(dev):
    prob, xg, yg, sett, bs, x0s = _setup(dev, DIMS['even'], seed=96)
    rho, lam = float(prob['rho']), float(yg[0].lam)
    plan = _plan(xg, yg, sett, 0, 8)
    _solve(plan, bs[0], x0s[0], rho, lam, 6)
    assert plan.cg_ring() == 8
    for stop in ('max_gain', 'max_gain_fresh', 'max_gain_recurred', 'e'):
        x = x0s[0].clone()
        plan.cg(bs[0], x, rho, lam, max_iter=6, tolerance=1e-3, stop=stop)
        assert plan.cg_ring() == 1, stop
    plan.precond_build(rho, lam, mode='fft')
    _solve(plan, bs[0], x0s[0], rho, lam, 6, precond='fft')
    assert plan.cg_ring() == 1
    _solve(plan, bs[0], x0s[0], rho, lam, 6)
    assert plan.cg_ring() == 8


def test_default_ring_size(dev):
    if os.environ.get('UNIRES_CG_RING'):
        pytest.skip('UNIRES_CG_RING set')
    from unires_amd._project import _channel_plan
    prob, xg, yg, sett, bs, x0s = _setup(dev, DIMS['even'], seed=97)
    yg[0]._plan = None
    plan = _channel_plan(xg[0], yg[0], sett.method, sett.do_proj)
    assert plan.cg_ring() == 1  # (no solve yet)
    _solve(plan, bs[0], x0s[0], float(prob['rho']), float(yg[0].lam), 4)
    assert plan.cg_ring() == 8
