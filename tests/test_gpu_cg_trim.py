"""The trimmed last iteration of a fixed-iteration solve (api_cg.hip: cg_enqueue_iters; cg.hip: k_sc_alpha's
iteration count, k_update_p_flush<false>, k_update_x): iteration N of a tol = 0 solve is the operator, alpha and the
iterate alone, so x must be the same bits as with UNIRES_CG_TRIM=0 and the solve must still report N iterations.
The switch is read once per process: the references come from ONE child process that runs every case with it off
(tests/switch_reference.py).  Covered: both volumes of test_gpu_cg_ring (the second for the scalar tails), K in
{1, 2, 3, 8}, iteration counts around the ring sizes, capture and two replays, Jacobi, plain launches with events and the
doubled operator, the channels' joint solve; and that nothing of a trimmed solve's state (r, r.z and beta are those of
iteration N - 1) leaks into the next solve on the plan."""
import functools

import pytest
import torch

from tests.helpers import gpu_structs, make_problem
from tests.switch_reference import cg_ends, child_main, from_child, same_bits, switch_on

pytestmark = pytest.mark.gpu

DIMS = {'even': (20, 18, 16), 'tail': (17, 13, 11)}
RINGS = (1, 2, 3, 8)
ITERS = (1, 2, 7, 8, 9, 16, 20)
STOPS = ('max_gain', 'max_gain_fresh', 'max_gain_recurred', 'e')


@functools.lru_cache(maxsize=None)
def _setup(dev, dims, n_channels=1, seed=191):
    prob = make_problem(seed=seed, dim_y=DIMS[dims], n_channels=n_channels, thick=4, regime='sr', scl=0.1)
    xg, yg, sett = gpu_structs(prob, dev)
    torch.manual_seed(seed)
    bs = [torch.rand(DIMS[dims], device=dev) - 0.5 for _ in range(n_channels)]
    x0s = [yg[c].dat.clone() for c in range(n_channels)]
    rho, lams = float(prob['rho']), [float(yc.lam) for yc in yg]
    return xg, yg, sett, bs, x0s, rho, lams


def _plan(xg, yg, sett, c, k):
    from unires_amd._project import _channel_plan
    yg[c]._plan = None  # (a plan of its own for every call)
    plan = _channel_plan(xg[c], yg[c], sett.method, sett.do_proj)
    plan.cg_ring(k)
    return plan


def _solve(plan, b, x0, rho, lam, max_iter, **kw):
    x = x0.clone()
    it, _ = plan.cg(b, x, rho, lam, max_iter=max_iter, tolerance=0, **kw)
    torch.cuda.synchronize()
    return x, it


# ---- the cases: each returns the iterates it produced (and asserts what does not depend on the switch) ----
def case_grid(dev, dims, k, max_iter):
    xg, yg, sett, bs, x0s, rho, lams = _setup(dev, dims)
    plan = _plan(xg, yg, sett, 0, k)
    out = []
    for rep in range(3):  # capture, replay, replay
        x, it = _solve(plan, bs[0], x0s[0], rho, lams[0], max_iter)
        assert it == max_iter, (rep, it)
        assert plan.cg_ring() == k  # (a trimmed solve leaves the ring size as it was)
        assert cg_ends(plan)[0] == switch_on('UNIRES_CG_TRIM'), rep  # (the path under test did run, replays included)
        out.append(x.cpu())
    return out


def case_jacobi(dev, dims, max_iter):
    xg, yg, sett, bs, x0s, rho, lams = _setup(dev, dims)
    plan = _plan(xg, yg, sett, 0, 3)
    plan.precond_build(rho, lams[0], mode='jacobi')
    out = []
    for rep in range(3):
        x, it = _solve(plan, bs[0], x0s[0], rho, lams[0], max_iter, precond='jacobi')
        assert it == max_iter and plan.cg_ring() == 3
        out.append(x.cpu())
    return out


def case_timed(dev, mode, k):
    xg, yg, sett, bs, x0s, rho, lams = _setup(dev, 'tail')
    plan = _plan(xg, yg, sett, 0, k)
    out = [_solve(plan, bs[0], x0s[0], rho, lams[0], 9)[0].cpu()]
    plan.time_matvecs(mode)
    x, it = _solve(plan, bs[0], x0s[0], rho, lams[0], 9)
    assert it == 9
    if mode == 1:
        assert plan.matvec_time()[0] == 9  # (one operator application per iteration, the start's not among them)
    out.append(x.cpu())
    plan.time_matvecs(False)
    out.append(_solve(plan, bs[0], x0s[0], rho, lams[0], 9)[0].cpu())
    return out


def case_many(dev, streams):
    from unires_amd._plan import cg_many
    xg, yg, sett, bs, x0s, rho, lams = _setup(dev, 'even', 3, 193)
    plans = [_plan(xg, yg, sett, c, 8) for c in range(3)]
    sts = [torch.cuda.Stream(device=dev) for _ in range(3)] if streams else [torch.cuda.current_stream(dev)] * 3
    out = []
    for rep in range(2):
        xs = [x0.clone() for x0 in x0s]
        torch.cuda.synchronize()
        res = cg_many(plans, bs, xs, rho, lams, sts, max_iter=13, tolerance=0, sync=True)
        torch.cuda.synchronize()
        assert [r[0] for r in res] == [13, 13, 13]
        out += [x.cpu() for x in xs]
    return out


GRID = [(d, k, n) for d in DIMS for k in RINGS for n in ITERS]
JACOBI = [('even', 11), ('tail', 3), ('tail', 1)]
TIMED = [(1, 8), (2, 8), (1, 1), (2, 1)]


def reference(dev):
    out = {}
    for c in GRID:
        out[('grid',) + c] = case_grid(dev, *c)
    for c in JACOBI:
        out[('jacobi',) + c] = case_jacobi(dev, *c)
    for c in TIMED:
        out[('timed',) + c] = case_timed(dev, *c)
    for s in (True, False):
        out[('many', s)] = case_many(dev, s)
    return out


@pytest.fixture(scope='module')
def untrimmed(dev, tmp_path_factory):
    """Every case with UNIRES_CG_TRIM=0, computed once in a child process."""
    return from_child('tests.test_gpu_cg_trim', {'UNIRES_CG_TRIM': '0'}, tmp_path_factory.mktemp('trim') / 'ref.pt')


def _check(got, ref):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert same_bits(a, b), (i, (a - b).abs().max().item())


@pytest.mark.parametrize('dims,k,max_iter', GRID)
def test_trimmed_solve_is_bit_identical(dev, untrimmed, dims, k, max_iter):
    got = case_grid(dev, dims, k, max_iter)
    _check(got, untrimmed[('grid', dims, k, max_iter)])
    assert not same_bits(got[0], _setup(dev, dims)[4][0].cpu())  # (the solve did move x)


@pytest.mark.parametrize('dims,max_iter', JACOBI)
def test_jacobi_preconditioned_solve(dev, untrimmed, dims, max_iter):
    _check(case_jacobi(dev, dims, max_iter), untrimmed[('jacobi', dims, max_iter)])


@pytest.mark.parametrize('mode,k', TIMED)
def test_plain_launches_and_doubled_operator(dev, untrimmed, mode, k):
    _check(case_timed(dev, mode, k), untrimmed[('timed', mode, k)])


@pytest.mark.parametrize('streams', [True, False])
def test_joint_solve_of_the_channels(dev, untrimmed, streams):
    _check(case_many(dev, streams), untrimmed[('many', streams)])


@pytest.mark.parametrize('k', [1, 8])
@pytest.mark.parametrize('stop', STOPS)
def test_nothing_leaks_into_the_next_solve(dev, stop, k):
    """A solve with a tolerance straight after a trimmed one, on the same plan, is the solve of a fresh plan: iterate
    bits, iteration count and objective trace."""
    xg, yg, sett, bs, x0s, rho, lams = _setup(dev, 'tail')
    fresh, used = _plan(xg, yg, sett, 0, k), _plan(xg, yg, sett, 0, k)
    _solve(used, bs[0], x0s[0], rho, lams[0], 7)
    xa, xb = x0s[0].clone(), x0s[0].clone()
    ita, tra = fresh.cg(bs[0], xa, rho, lams[0], max_iter=12, tolerance=1e-3, stop=stop)
    itb, trb = used.cg(bs[0], xb, rho, lams[0], max_iter=12, tolerance=1e-3, stop=stop)
    torch.cuda.synchronize()
    assert ita == itb and tra == trb and same_bits(xa, xb)
    assert not cg_ends(used)[0]  # (a solve with a stopping rule is never trimmed)
    assert used.cg_ring() == 1
    x, it = _solve(used, bs[0], x0s[0], rho, lams[0], 7)  # ... and the trimmed solve after it is what it was
    ref, _ = _solve(_plan(xg, yg, sett, 0, k), bs[0], x0s[0], rho, lams[0], 7)
    assert it == 7 and used.cg_ring() == k and same_bits(x, ref) and cg_ends(used)[0]


def test_every_solve_reports_its_own_path(dev):
    """Whole (captured), chunked, whole again (replayed) on one plan: after each solve the plan reports that solve's
    trim and ring size, not the one before's, and the replay gives the capture's bits."""
    xg, yg, sett, bs, x0s, rho, lams = _setup(dev, 'tail')
    plan = _plan(xg, yg, sett, 0, 3)
    x1, it = _solve(plan, bs[0], x0s[0], rho, lams[0], 9)
    assert it == 9 and cg_ends(plan)[0] and plan.cg_ring() == 3
    x = x0s[0].clone()
    plan.cg(bs[0], x, rho, lams[0], max_iter=9, tolerance=1e-3)
    torch.cuda.synchronize()
    assert not cg_ends(plan)[0] and plan.cg_ring() == 1
    x3, it = _solve(plan, bs[0], x0s[0], rho, lams[0], 9)
    assert it == 9 and cg_ends(plan)[0] and plan.cg_ring() == 3
    assert same_bits(x1, x3)


if __name__ == '__main__':
    child_main(reference)
