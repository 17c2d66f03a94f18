"""The start of a CG solve fused into the push (splat2.hip: k_splat2's residual mode; api_operator.hip: push_any serves
or declines it; api_cg.hip: cg_enqueue_start): where the last repeat's push is k_splat2, a forward-difference plan
without masks writes r = b - A(x0), the first direction and the partials of r.z from the push's epilogue instead of
storing A(x0) for k_residual_init; for a solve with a tolerance also the partials of obj[0].  Compared with
UNIRES_CG_START_FUSED=0 (read once per process: the references come from ONE child process that runs every case with it
off): the iterate bit for bit, the iteration count, and the objective trace bit for bit from obj[1] on.  obj[0] itself
is the float64 sum of the SAME float32 terms (the test checks x, so r and the terms are the same) grouped by the push's
waves instead of k_residual_init's blocks.  A float64 sum of n terms t_i, in any order, is within (n - 1) 2^-53 sum |t_i|
of the exact sum (Higham, Accuracy and Stability, eq. 4.4, first order), so two groupings differ by at most twice that
and obj[0] = sum / 2 by (n - 1) 2^-53 sum |t_i|: the bound asserted, with sum |t_i| from a float64 evaluation of
(A(x0) - 2 b) x0 (1 % added for that evaluation's own rounding of the terms).  The routes that decline the mode
(k_ata1, a masked repeat, a central difference) must give every value, obj[0] included, bit for bit.

Shapes: (37, 30, 61) with slices 6 thick has partial tiles in x and y (tiles are 8 x 4) and a last z tile of one
plane - the generic epilogue next to the whole-tile one; (40, 36, 64) is whole tiles only."""
import functools

import pytest
import torch

from tests.helpers import gpu_structs, make_problem
from tests.switch_reference import cg_ends, child_main, from_child, same_bits, switch_on

pytestmark = pytest.mark.gpu

# name -> (make_problem arguments, splat2_axis expected of the last repeat)
PROBLEMS = {
    'z_odd': (dict(dim_y=(37, 30, 61), thick=6, rot=0.12, trans=2.5, thick_axes=[2], scl=0.1), 2),
    'z_even': (dict(dim_y=(40, 36, 64), thick=6, rot=0.12, trans=2.5, thick_axes=[2], scl=0.1), 2),
    'x_odd': (dict(dim_y=(61, 30, 37), thick=6, rot=0.12, trans=2.5, thick_axes=[0], scl=0.1), 0),
    'y_odd': (dict(dim_y=(37, 61, 30), thick=6, rot=0.12, trans=2.5, thick_axes=[1], scl=0.1), 1),
    'two_repeats': (dict(dim_y=(37, 30, 61), thick=6, rot=0.12, trans=2.5, n_repeats=2, scl=0.1), None),
}
SOLVES = [(1, 0.0), (3, 0.0), (12, 1e-3)]  # (max_iter, tolerance)


@functools.lru_cache(maxsize=None)
def _setup(dev, name, regime='sr', seed=291):
    kw = dict(PROBLEMS[name][0]) if name in PROBLEMS else dict(dim_y=(20, 18, 33), rot=0.08, trans=1.5)
    prob = make_problem(seed=seed, n_channels=1, regime=regime, **kw)
    xg, yg, sett = gpu_structs(prob, dev)
    torch.manual_seed(seed)
    b = torch.rand(prob['dim_y'], device=dev) - 0.5
    return xg, yg, sett, b, yg[0].dat.clone(), float(prob['rho']), float(yg[0].lam)


def _plan(xg, yg, sett, **kw):
    from unires_amd._project import _channel_plan
    yg[0]._plan = None  # (a plan of its own for every call)
    return _channel_plan(xg[0], yg[0], sett.method, sett.do_proj, **kw)


def _solves(plan, b, x0, rho, lam, precond='none', fused=False):
    """Every solve of SOLVES twice (capture, replay): [(x, iters, trace), ...]; ``fused``: whether the start's residual
    must have come from the push."""
    out = []
    for max_iter, tol in SOLVES:
        for rep in range(2):
            x = x0.clone()
            it, tr = plan.cg(b, x, rho, lam, max_iter=max_iter, tolerance=tol, precond=precond)
            torch.cuda.synchronize()
            if tol == 0:
                assert it == max_iter
            assert cg_ends(plan)[1] == fused, (max_iter, tol, rep)  # (the path under test did run / was declined)
            out.append((x.cpu(), it, tr))
    return out


def case_splat2(dev, name, precond):
    xg, yg, sett, b, x0, rho, lam = _setup(dev, name)
    plan = _plan(xg, yg, sett)
    last = plan.repeat_info(plan.n_repeats - 1)
    assert last['pull2'] and last['splat2_axis'] is not None and not last['masked'], last
    if PROBLEMS[name][1] is not None:
        assert last['splat2_axis'] == PROBLEMS[name][1], last
    if precond == 'jacobi':
        plan.precond_build(rho, lam, mode='jacobi')
    return _solves(plan, b, x0, rho, lam, precond, fused=switch_on('UNIRES_CG_START_FUSED'))


def obj0_bound(dev, name):
    """(n - 1) 2^-53 sum |t_i| for the terms of obj[0] (see the module's docstring)."""
    xg, yg, sett, b, x0, rho, lam = _setup(dev, name)
    ax = _plan(xg, yg, sett).matvec(x0, rho, lam)
    t = (ax.double() - 2 * b.double()) * x0.double()
    return 1.01 * (t.numel() - 1) * 2.0 ** -53 * t.abs().sum().item()


def case_declined(dev, route):
    if route == 'ata1':
        xg, yg, sett, b, x0, rho, lam = _setup(dev, 'dn', 'dn')
        plan = _plan(xg, yg, sett)
        assert plan.repeat_info(0)['fused']
    elif route == 'masked':
        xg, yg, sett, b, x0, rho, lam = _setup(dev, 'z_odd', 'sr', 292)  # (a problem of its own: it is changed below)
        dat = xg[0][0].dat
        dat.view(-1)[::7] = 0  # (the same voxels in either process; an in-place change the plan's mask follows)
        plan = _plan(xg, yg, sett, mask_zeros=True)
        assert plan.repeat_info(0)['masked']
    else:
        xg, yg, sett, b, x0, rho, lam = _setup(dev, 'z_even')
        plan = _plan(xg, yg, sett, diff='central')
    return _solves(plan, b, x0, rho, lam)


SPLAT2 = [(n, 'none') for n in PROBLEMS] + [(n, 'jacobi') for n in PROBLEMS if n != 'two_repeats']
DECLINED = ['ata1', 'central', 'masked']


def reference(dev):
    out = {}
    for c in SPLAT2:
        out[('splat2',) + c] = case_splat2(dev, *c)
    for r in DECLINED:
        out[('declined', r)] = case_declined(dev, r)
    return out


@pytest.fixture(scope='module')
def unfused(dev, tmp_path_factory):
    """Every case with UNIRES_CG_START_FUSED=0, computed once in a child process."""
    return from_child('tests.test_gpu_cg_start', {'UNIRES_CG_START_FUSED': '0'},
                      tmp_path_factory.mktemp('start') / 'ref.pt')


def _check(got, ref, obj0_tol=0.0):
    assert len(got) == len(ref)
    for i, ((xa, ita, tra), (xb, itb, trb)) in enumerate(zip(got, ref)):
        assert ita == itb, (i, ita, itb)
        assert same_bits(xa, xb), (i, (xa - xb).abs().max().item())
        assert (tra is None) == (trb is None)
        if tra is not None:
            print('obj[0]: fused %r unfused %r diff %.3g bound %.3g' % (tra[0], trb[0], abs(tra[0] - trb[0]), obj0_tol))
            assert abs(tra[0] - trb[0]) <= obj0_tol, (i, tra[0], trb[0], obj0_tol)
            assert tra[1:] == trb[1:], (i, tra, trb)


@pytest.mark.parametrize('name,precond', SPLAT2)
def test_fused_start_is_bit_identical(dev, unfused, name, precond):
    got = case_splat2(dev, name, precond)
    _check(got, unfused[('splat2', name, precond)], obj0_bound(dev, name))
    assert not same_bits(got[0][0], _setup(dev, name)[4].cpu())  # (the solve did move x)


@pytest.mark.parametrize('route', DECLINED)
def test_routes_that_decline_the_mode_solve_as_before(dev, unfused, route):
    _check(case_declined(dev, route), unfused[('declined', route)])


if __name__ == '__main__':
    child_main(reference)
