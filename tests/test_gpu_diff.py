"""sett.diff = 'backward' / 'central' on the GPU: the regulariser's kernel family per voxel against the float64
restatement tests/diff64.py (bounds derived there, none fitted), the plan's matvec / CG / captured graph with a
non-forward D, and the whole y-update / ADMM iteration / fit() / preproc() with the setting.

nitorch is not available to this project: the definitions are restated from its published diff1d / div1d
[recalled] (tests/diff64.py); what these tests pin is the project's own statement of them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nitorch_restated as N
from oracle import unires_restated as O
from tests import admm64, diff64, ref64
from tests.helpers import gpu_structs, make_problem, oracle_structs, rel_err

pytestmark = pytest.mark.gpu

GATE = 1e-4
NONFWD = ('backward', 'central')
# axes of length 1, 2, 3 (central's reach); lines shorter than 4 (the flat kernel declines); lines across the 64 and
# 256 boundaries; a volume longer than one flat chunk (1024 voxels) with x faces inside it
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 1, 5), (3, 4, 2), (5, 3, 1), (4, 5, 66), (3, 7, 130), (2, 3, 259), (9, 10, 67)]
VX = {'iso': (1.0, 1.0, 1.0), 'aniso': (0.8, 1.25, 2.0)}
RHO = 0.37


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _cmp(out, ref, tol, what):
    r = ref64.compare(out.cpu(), _t(ref), _t(tol))
    assert r['ok'], (what, r)
    return r['max_ratio']


def _id_plan(dev, dim, vx, tau, diff):
    from unires_amd._plan import ChannelPlan
    return ChannelPlan(dim, vx, [(None, tau)], 'denoising', False, device=dev, diff=diff)


def _id_matvec(dev, p, vx, tau, rho, lam, diff, out=None):
    """(q, dot) of the A = I plan's matvec: the flat streaming kernel where the shape is in its domain."""
    plan = _id_plan(dev, tuple(p.shape), vx, tau, diff)
    dot = torch.zeros((), dtype=torch.float64, device=dev)
    q = plan.matvec(p, rho, lam, out=out, dot=dot)
    torch.cuda.synchronize()
    res = q.clone(), float(dot)
    plan.close()
    return res


# ---- op level -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vx', list(VX))
@pytest.mark.parametrize('dim', SHAPES)
def test_gradient_divergence_and_stencil_per_voxel(dev, dim, vx):
    """im_gradient, im_divergence and a src + c DtD (the op-level kernel AND the A = I plan's matvec: the flat
    streaming kernel, its fallback below nz = 4 / 64 voxels) against diff64 within the derived bounds; adjointness."""
    from unires_amd import _ops
    g = torch.Generator().manual_seed(sum(dim) + len(vx))
    y = ((torch.rand(dim, generator=g) - 0.3) * 100).float()
    g3 = ((torch.rand((3,) + dim, generator=g) - 0.5) * 10).float()
    yd, gd = y.to(dev), g3.to(dev)
    worst = {}
    for which in NONFWD:
        Dy = _ops.grad(yd, VX[vx], which)
        worst['grad ' + which] = _cmp(Dy, *diff64.gradient(y.numpy(), VX[vx], which), ('grad', which))
        Dtg = _ops.div(gd, VX[vx], which)
        worst['div ' + which] = _cmp(Dtg, *diff64.divergence(g3.numpy(), VX[vx], which), ('div', which))
        # <D y, g> = <y, D^T g>, float64 sums of the kernels' float32 outputs
        lhs = float((Dy.double() * gd.double()).sum())
        rhs = float((yd.double() * Dtg.double()).sum())
        scale = float((Dy.double().abs() * gd.double().abs()).sum()) + 1e-300
        assert abs(lhs - rhs) <= 1e-6 * scale, (which, lhs, rhs)
        a, c = 0.7, 1.3
        ref, tol = diff64.a_plus_c_dtd(y.numpy(), VX[vx], which, a, c)
        worst['dtd ' + which] = _cmp(_ops.dtd(yd, VX[vx], a, c, which), ref, tol, ('dtd', which))
        # the plan's matvec with A = I: q = tau p + rho lam^2 DtD p; c is formed as rho * (lam * lam) in float32
        tau, lam = 0.7, 0.9
        cc = float(np.float32(RHO) * (np.float32(lam) * np.float32(lam)))
        ref, tol = diff64.a_plus_c_dtd(y.numpy(), VX[vx], which, tau, cc)
        q, dot = _id_matvec(dev, yd, VX[vx], tau, RHO, lam, which)
        worst['flat ' + which] = _cmp(q, ref, tol, ('matvec A = I', which))
        ref_dot = float((y.double() * q.cpu().double()).sum())
        mag = float((y.double().abs() * q.cpu().double().abs()).sum())
        # (the kernel sums float32 products in float64: u per term, and the sum's own float64 slack)
        assert abs(dot - ref_dot) <= (diff64.U + (y.numel() + 32) * diff64.U64) * mag, (which, dot, ref_dot)
    print('diff ops %s %s: max err/tol %s' % (dim, vx, {k: round(v, 3) for k, v in worst.items()}), flush=True)


@pytest.mark.parametrize('dim', [(4, 5, 66), (9, 10, 67)])
def test_flat_kernel_with_an_unaligned_output(dev, dim):
    """q 4, 8 and 12 bytes off a 16-byte boundary: the flat kernel's head voxels and a shifted vector grid."""
    g = torch.Generator().manual_seed(11)
    y = ((torch.rand(dim, generator=g) - 0.3) * 100).float()
    n = y.numel()
    cc = float(np.float32(RHO) * (np.float32(0.9) * np.float32(0.9)))
    for which in NONFWD:
        ref, tol = diff64.a_plus_c_dtd(y.numpy(), VX['aniso'], which, 0.7, cc)
        for off in (1, 2, 3):
            buf = torch.full((n + 8,), -7.75e37, dtype=torch.float32, device=dev)
            out = buf[off:off + n].view(dim)
            q, _ = _id_matvec(dev, y.to(dev), VX['aniso'], 0.7, RHO, 0.9, which, out=out)
            _cmp(q, ref, tol, (which, off))
            assert bool((buf[:off] == -7.75e37).all()) and bool((buf[off + n:] == -7.75e37).all())


@pytest.mark.parametrize('vx', list(VX))
@pytest.mark.parametrize('dim', SHAPES)
def test_forward_through_the_new_entry_points_is_bit_identical(dev, lib, dim, vx):
    from unires_amd._lib import check, f3, i3
    from unires_amd._ops import _ptr, _stream
    g = torch.Generator().manual_seed(3)
    y = ((torch.rand(dim, generator=g) - 0.3) * 100).float().to(dev)
    g3 = ((torch.rand((3,) + dim, generator=g) - 0.5) * 10).float().to(dev)
    d, v = i3(dim), f3(VX[vx])
    a3, b3 = torch.empty_like(g3), torch.empty_like(g3)
    check(lib.unires_grad_fwd_zero(_ptr(y), d, v, _ptr(a3), _stream()))
    check(lib.unires_grad_which(_ptr(y), d, v, 0, _ptr(b3), _stream()))
    assert torch.equal(a3, b3)
    a, b = torch.empty_like(y), torch.empty_like(y)
    check(lib.unires_div_fwd_zero(_ptr(g3), d, v, _ptr(a), _stream()))
    check(lib.unires_div_which(_ptr(g3), d, v, 0, _ptr(b), _stream()))
    assert torch.equal(a, b)
    check(lib.unires_dtd(_ptr(y), d, v, 0.7, 1.3, _ptr(a), _stream()))
    check(lib.unires_dtd_which(_ptr(y), d, v, 0, 0.7, 1.3, _ptr(b), _stream()))
    assert torch.equal(a, b)
    assert lib.unires_dtd_which(_ptr(y), d, v, 5, 0.7, 1.3, _ptr(b), _stream()) == 3  # UNIRES_ERR_ARG
    # a plan told 'forward' explicitly is a plan left at its default
    p0, p1 = _id_matvec(dev, y, VX[vx], 0.7, RHO, 0.9, 'forward'), None
    from unires_amd._plan import ChannelPlan
    plan = ChannelPlan(dim, VX[vx], [(None, 0.7)], 'denoising', False, device=dev)
    dot = torch.zeros((), dtype=torch.float64, device=dev)
    p1 = plan.matvec(y, RHO, 0.9, dot=dot)
    assert torch.equal(p0[0], p1) and p0[1] == float(dot)
    plan.close()


# ---- z / w update and the prior term ---------------------------------------------------------------------------------
def _run_zw(dev, lib, which, ys, lam, vx, alpha, z, w):
    from unires_amd._lib import check, f3, i3, diff_code
    from unires_amd._ops import _ptr, _stream
    Cn, dim = len(lam), tuple(ys.shape[1:])
    yd = [ys[c].contiguous().to(dev) for c in range(Cn)]
    ptrs = (C.c_void_p * Cn)(*[t.data_ptr() for t in yd])
    lams = (C.c_float * Cn)(*lam)
    zv, wv = z.clone().to(dev), w.clone().to(dev)
    jv = torch.full(dim, -7.75e37, dtype=torch.float32, device=dev)  # (every voxel of s must be written)
    nv = torch.zeros(1, dtype=torch.float64, device=dev)
    code = diff_code(which)
    check(lib.unires_zw_update_which(ptrs, lams, Cn, i3(dim), f3(vx), code, float(RHO), float(alpha), _ptr(zv), _ptr(wv),
                                     _ptr(jv), _stream()))
    check(lib.unires_nll_prior_which(ptrs, lams, Cn, i3(dim), f3(vx), code, _ptr(nv), _stream()))
    torch.cuda.synchronize()
    return jv.cpu().numpy(), zv.cpu().numpy(), wv.cpu().numpy(), float(nv.cpu()[0])


@pytest.mark.parametrize('vx', list(VX))
@pytest.mark.parametrize('dim', SHAPES)
def test_zw_update_and_prior_per_voxel(dev, lib, monkeypatch, dim, vx):
    """unires_zw_update_which / unires_nll_prior_which against admm64's zw_update / nll_prior - its bounds unchanged -
    fed with the generalised gradient; C = 1, 3, 9, alpha = 1 and 0.7."""
    worst = 0.0
    for which in NONFWD:
        monkeypatch.setattr(admm64, 'grad64', lambda y, s, which=which: diff64.grad64(y, s, which))
        for Cn in (1, 3, 9):
            for alpha in (1.0, 0.7):
                ys, lam, z, w = admm64.zw_inputs(dim, Cn, RHO, alpha, vx=VX[vx])
                s, zo, wo, nll = _run_zw(dev, lib, which, ys, lam, VX[vx], alpha, z, w)
                B = admm64.zw_update(ys.numpy(), lam, VX[vx], RHO, alpha, z.numpy(), w.numpy())

                def check(key, out, ref, tol):
                    err = np.abs(out.astype(np.float64) - ref)
                    bad = err > tol
                    assert not bad.any(), (which, Cn, alpha, key, tuple(int(i) for i in np.argwhere(bad)[0]), int(bad.sum()))
                    return float((err / np.maximum(tol, 1e-300)).max())

                worst = max(worst, check('s', s, *B['s']))
                for c in range(Cn):
                    Bc = B['chan'](c)
                    worst = max(worst, check('z%d' % c, zo[c], *Bc['z']), check('w%d' % c, wo[c], *Bc['w']))
                ref, tol = admm64.nll_prior(ys.numpy(), lam, VX[vx])
                assert abs(nll - ref) <= tol, (which, Cn, 'nll', nll, ref, tol)
    print('diff zw %s %s: max err/tol %.3f' % (dim, vx, worst), flush=True)


# ---- mirror checks (no oracle: forward is the parent commit's behaviour) --------------------------------------------
@pytest.mark.parametrize('vx', list(VX))
@pytest.mark.parametrize('dim', SHAPES)
def test_backward_stencil_is_the_mirrored_forward_stencil(dev, dim, vx):
    """DtD_backward y = flip(DtD_forward flip(y)) per voxel, within the sum of both sides' bounds."""
    g = torch.Generator().manual_seed(5)
    y = ((torch.rand(dim, generator=g) - 0.3) * 100).float()
    tau, lam = 0.7, 0.9  # (the plan wants tau > 0; tau p mirrors like the stencil)
    cc = float(np.float32(RHO) * (np.float32(lam) * np.float32(lam)))
    qb, _ = _id_matvec(dev, y.to(dev), VX[vx], tau, RHO, lam, 'backward')
    qf, _ = _id_matvec(dev, y.flip(0, 1, 2).contiguous().to(dev), VX[vx], tau, RHO, lam, 'forward')
    _, tol_b = diff64.a_plus_c_dtd(y.numpy(), VX[vx], 'backward', tau, cc)
    _, tol_f = diff64.a_plus_c_dtd(y.flip(0, 1, 2).numpy(), VX[vx], 'forward', tau, cc)
    tol = tol_b + np.ascontiguousarray(tol_f[::-1, ::-1, ::-1])
    _cmp(qb, qf.cpu().flip(0, 1, 2).double().numpy(), tol, 'mirror')


def _fit_identity(dev, monkeypatch, prob, diff, flip):
    """fit() on an A = I problem (optionally with every volume flipped along the three axes); returns the image
    (C, *dim), the trace, the iteration count and the last z, w."""
    import unires_amd as U
    from unires_amd import run
    fl = (lambda t: t.flip(-3, -2, -1).contiguous()) if flip else (lambda t: t)
    xg, yg, sett = gpu_structs(prob, dev)
    for xc in xg:
        for xn in xc:
            xn.dat = fl(xn.dat)
    for yc in yg:
        yc.dat = fl(yc.dat)
        yc.lam0 = float(yc.lam) / 4.0
    sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = 12, 1e-4, 4.0, 3
    sett.clean_fov = False
    sett.diff = diff
    kept = {}
    inner = run._update_admm

    def spy(*a, **k):
        out = inner(*a, **k)
        kept['z'], kept['w'] = out[1], out[2]
        return out

    monkeypatch.setattr(run, '_update_admm', spy)
    dat, _, _, info = U.fit(xg, yg, sett)
    torch.cuda.synchronize()
    return dat.cpu(), info, kept['z'].cpu(), kept['w'].cpu()


def test_fit_backward_is_the_mirror_of_fit_forward(dev, monkeypatch):
    """The whole fit() with A = I, two repeats, sett.diff = 'backward', 12 ADMM iterations: the flip of fit() with
    forward differences on the flipped data, z and w flipped and negated (D_b = -P D_f P).  Gates: tests/test_gpu_path.py's
    for the same quantities."""
    prob = make_problem(seed=71, dim_y=(20, 18, 16), n_channels=2, regime='id', n_repeats=2)
    dat_b, info_b, z_b, w_b = _fit_identity(dev, monkeypatch, prob, 'backward', False)
    dat_f, info_f, z_f, w_f = _fit_identity(dev, monkeypatch, prob, 'forward', True)
    assert info_b['n_iter'] == info_f['n_iter'] == 12
    assert torch.allclose(info_b['obj'], info_f['obj'], rtol=5e-4)
    for c in range(2):
        assert rel_err(dat_b[..., c], dat_f[..., c].flip(0, 1, 2)) < GATE
    assert rel_err(z_b, -z_f.flip(-3, -2, -1)) < 5e-4 and rel_err(w_b, -w_f.flip(-3, -2, -1)) < 5e-4
    assert float(z_b.abs().max()) > 0
    # ... and it is not the forward result
    dat_0, _, _, _ = _fit_identity(dev, monkeypatch, prob, 'forward', False)
    assert rel_err(dat_b, dat_0) > 1e-5


# ---- the plan's matvec ------------------------------------------------------------------------------------------------
MATVEC_CASES = {
    'id_1ch': dict(dim_y=(18, 17, 13), n_channels=1, regime='id'),
    'dn_2ch': dict(dim_y=(15, 13, 11), n_channels=2, regime='dn', rot=0.1, trans=1.5),
    'sr_2rep': dict(dim_y=(14, 12, 15), n_channels=2, thick=2, regime='sr', n_repeats=2, scl=0.05),
}


@pytest.mark.parametrize('which', NONFWD)
@pytest.mark.parametrize('case', list(MATVEC_CASES))
def test_matvec_equals_the_composed_operator(dev, case, which):
    """unires_ata_matvec on a non-forward plan against sum_n tau_n _proj_apply('AtA') + rho lam^2 _DtD(diff) composed
    from the op-level calls; the returned dot against the float64 dot of the stored vectors."""
    import unires_amd as U
    from unires_amd._project import _channel_plan
    prob = make_problem(seed=12, **MATVEC_CASES[case])
    xg, yg, sett = gpu_structs(prob, dev)
    vx = N.voxel_size(prob['mat_y']).float()
    rho = float(prob['rho'])
    torch.manual_seed(6)
    for c in range(len(xg)):
        p = (torch.rand(prob['dim_y']) * 100).to(dev)
        lam = float(yg[c].lam)
        plan = _channel_plan(xg[c], yg[c], prob['method'], prob['do_proj'], vx, diff=which)
        assert plan.diff == which
        dot = torch.zeros((), dtype=torch.float64, device=dev)
        q = plan.matvec(p, rho, lam, dot=dot)
        op = 'AtA' if prob['do_proj'] else 'none'
        ref = rho * lam ** 2 * U._DtD(p, vx, diff=which).double()
        for xn in xg[c]:
            ref = ref + float(xn.tau) * U._proj_apply(op, p[None, None], xn.po, method=prob['method'])[0, 0].double()
        err = rel_err(q.cpu(), ref.cpu())
        ref_dot = float((p.double() * q.double()).sum())
        print('diff matvec %s %s c%d: rel_err %.3g, dot rel %.3g' % (case, which, c, err, abs(float(dot) - ref_dot) / abs(ref_dot)),
              flush=True)
        assert err < GATE
        assert abs(float(dot) - ref_dot) <= 1e-9 * abs(ref_dot)
        # U._proj('AtA') is the same call
        q2 = U._proj('AtA', p, xg[c], yg[c], method=prob['method'], do=prob['do_proj'], rho=rho, vx_y=vx, diff=which)
        assert torch.equal(q, q2)


# ---- CG ---------------------------------------------------------------------------------------------------------------
def _dense_system(dim, vx, which, tau, rho, lam):
    tau, c = float(np.float32(tau)), float(np.float32(rho) * (np.float32(lam) * np.float32(lam)))
    return tau * np.eye(int(np.prod(dim))) + c * diff64.dense_dtd(dim, vx, which)


@pytest.mark.parametrize('which', NONFWD)
def test_cg_against_a_dense_float64_system(dev, which):
    dim, vx, tau, rho, lam = (6, 5, 7), VX['aniso'], 0.8, 0.9, 1.1
    A = _dense_system(dim, vx, which, tau, rho, lam)
    g = torch.Generator().manual_seed(9)
    b = (torch.rand(dim, generator=g) * 10).float()
    want = np.linalg.solve(A, b.double().numpy().ravel()).reshape(dim)
    plan = _id_plan(dev, dim, vx, tau, which)
    x = torch.zeros(dim, device=dev)
    # enough iterations to converge, and no more: the A-norm error of CG falls by r = (sqrt(k) - 1) / (sqrt(k) + 1) per
    # iteration at least (k: the condition number), so 2 r^n <= 1e-6 after n iterations.  (A fixed-iteration solve run
    # far past convergence divides 0 by 0 in float32, whatever the difference.)
    sk = float(np.sqrt(np.linalg.cond(A)))
    n_it = int(np.ceil(np.log(0.5e-6) / np.log((sk - 1.0) / (sk + 1.0))))
    assert 4 <= n_it <= 40
    plan.cg(b.to(dev), x, rho, lam, max_iter=n_it, tolerance=0.0)
    assert rel_err(x.cpu(), _t(want)) < GATE
    # the objective trace and the stopping iteration against a float64 CG on the same dense system
    At = _t(A)
    x64, n_ref, obj_ref = N.cg(lambda v: (At @ v.reshape(-1)).reshape(dim), b.double(), torch.zeros(dim, dtype=torch.float64),
                               max_iter=40, tolerance=1e-3, stop='max_gain', return_info=True)
    x = torch.zeros(dim, device=dev)
    n_gpu, obj = plan.cg(b.to(dev), x, rho, lam, max_iter=40, tolerance=1e-3, stop='max_gain')
    assert n_gpu == n_ref
    assert torch.allclose(torch.tensor(obj, dtype=torch.float64), obj_ref, rtol=1e-5, atol=0)
    plan.close()


@pytest.mark.parametrize('case', ['id_1ch', 'dn_2ch'])
def test_switching_the_difference_drops_the_captured_solve(dev, case):
    """Two tol = 0 solves on one plan (the second replays the captured graph), a switch of `which`, a third solve:
    the bits of a fresh plan built with that `which`; switching back gives the first result's bits."""
    from unires_amd._plan import ChannelPlan
    prob = make_problem(seed=23, **MATVEC_CASES[case])
    xg, yg, sett = gpu_structs(prob, dev)
    vx = [float(v) for v in N.voxel_size(prob['mat_y'])]
    reps = [(xn.po, xn.tau) for xn in xg[0]]
    rho, lam = float(prob['rho']), float(yg[0].lam)
    g = torch.Generator().manual_seed(2)
    b = (torch.rand(prob['dim_y'], generator=g) * 0.1).to(dev)
    x0 = prob['y0'][0].to(dev)

    def solve(plan, x):
        x.copy_(x0)
        plan.cg(b, x, rho, lam, max_iter=6, tolerance=0.0)
        torch.cuda.synchronize()
        return x.clone()

    plan = ChannelPlan(prob['dim_y'], vx, reps, prob['method'], prob['do_proj'], device=dev)
    x = torch.empty_like(x0)
    first = solve(plan, x)
    assert torch.equal(solve(plan, x), first)
    res = {'forward': first}
    for which in ('central', 'backward', 'central'):
        plan.set_diff(which)
        got = solve(plan, x)
        assert torch.equal(solve(plan, x), got)
        fresh = ChannelPlan(prob['dim_y'], vx, reps, prob['method'], prob['do_proj'], device=dev, diff=which)
        xf = torch.empty_like(x0)
        assert torch.equal(solve(fresh, xf), got), which
        fresh.close()
        assert not torch.equal(got, first)
        res.setdefault(which, got)
        assert torch.equal(res[which], got)
    plan.set_diff('forward')
    assert torch.equal(solve(plan, x), first)
    plan.close()


# ---- end to end against the oracle ---------------------------------------------------------------------------------
def _patch_oracle(monkeypatch, which):
    """oracle.unires_restated's im_gradient / im_divergence replaced by diff64-backed functions that ignore the
    caller's `which` (no file under oracle/ changes)."""
    def grad(dat, vx=None, which_=None, bound='zero', **kw):
        v = [1.0] * 3 if vx is None else [float(t) for t in torch.as_tensor(vx, dtype=dat.dtype)]
        y = dat.double().numpy()
        g = np.stack([diff64._apply(y, d, which, False, False) / v[d] for d in range(3)])
        return _t(g).to(dat.dtype)

    def div(dat, vx=None, which_=None, bound='zero', **kw):
        v = [1.0] * 3 if vx is None else [float(t) for t in torch.as_tensor(vx, dtype=dat.dtype)]
        g3 = dat.double().numpy()
        out = sum(diff64._apply(g3[d], d, which, True, False) / v[d] for d in range(3))
        return _t(out).to(dat.dtype)

    monkeypatch.setattr(O, 'im_gradient', grad)
    monkeypatch.setattr(O, 'im_divergence', div)


E2E_CASES = {
    'sr_3ch_axes': dict(dim_y=(20, 18, 16), n_channels=3, thick=4, regime='sr', scl=0.1),
    'dn_2ch': dict(dim_y=(15, 13, 11), n_channels=2, regime='dn', rot=0.1, trans=1.5),
}


@pytest.mark.parametrize('which', NONFWD)
@pytest.mark.parametrize('case', list(E2E_CASES))
def test_full_admm_iterations_track_the_oracle(dev, monkeypatch, case, which):
    """tests/test_gpu_path.py's test of the same name with sett.diff = `which`, its gates unchanged."""
    import unires_amd as U
    _patch_oracle(monkeypatch, which)
    prob = make_problem(seed=18, **E2E_CASES[case])
    xo, yo = oracle_structs(prob)
    xg, yg, sett = gpu_structs(prob, dev)
    sett.diff = which
    rho = torch.tensor(prob['rho'])
    zo, wo = prob['z'].clone(), prob['w'].clone()
    zg, wg = zo.clone().to(dev), wo.clone().to(dev)
    tmp = torch.zeros_like(yg[0].dat)
    obj = torch.zeros((3, 3), dtype=torch.float64, device=dev)
    for it in range(3):
        yo = O.update_y(xo, yo, zo, wo, rho, prob['method'], prob['do_proj'])
        ref_obj = O.compute_nll(xo, yo, prob['method'], prob['do_proj'])
        zo, wo, _ = O.update_zw(yo, zo, wo, rho)
        yg, zg, wg, tmp, obj = U._update_admm(xg, yg, zg, wg, float(rho), tmp, obj, it, sett)
        for c in range(len(yo)):
            assert rel_err(yg[c].dat.cpu(), yo[c].dat) < GATE, (it, c)
        assert abs(obj[it, 0].item() - ref_obj[0].item()) < 1e-4 * abs(ref_obj[0].item())
    assert rel_err(zg.cpu(), zo) < 5e-4 and rel_err(wg.cpu(), wo) < 5e-4


def test_preproc_with_central_differences(dev, monkeypatch):
    """One preproc() from [dat, mat] pairs with sett.diff = 'central', max_iter = 3: the setting reaches the plan, the
    z / w update and the prior term, and changes the result."""
    import unires_amd as U
    from unires_amd import _plan
    from unires_amd.run import preproc
    from tests import coreg_phantom as P
    dim = (48, 56, 40)  # (the phantom and size of tests/test_gpu_init.py::test_demo_call_shape)
    dat = P.observation(dim, (1.0, 1.0, 1.0), 0, 3, dev, scale=0.35)[0].abs()
    seen = []
    inner = _plan.ChannelPlan.set_diff
    monkeypatch.setattr(_plan.ChannelPlan, 'set_diff', lambda self, diff: (seen.append(diff), inner(self, diff))[1])
    out = {}
    for diff in ('forward', 'central'):
        sett = U.settings()
        sett.device = dev
        for k, v in dict(vx=1.0, write_out=False, reg_scl=1.0, ct=False, max_iter=3, diff=diff).items():
            setattr(sett, k, v)
        out[diff] = preproc([[dat.clone(), torch.eye(4, device=dev)]], sett)[0]
        assert out[diff].shape == dim + (1,) and bool(torch.isfinite(out[diff]).all())
    assert 'central' in seen
    assert rel_err(out['central'], out['forward']) > 1e-5
    sett = U.settings()
    sett.device, sett.diff = dev, 'upwind'
    with pytest.raises(ValueError, match='diff'):
        for k, v in dict(vx=1.0, write_out=False, reg_scl=1.0, ct=False, max_iter=3).items():
            setattr(sett, k, v)
        preproc([[dat.clone(), torch.eye(4, device=dev)]], sett)


# ---- FFT preconditioner ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['id_1ch', 'dn_2ch'])
def test_fft_preconditioner_with_central_differences(dev, monkeypatch, case):
    """The FFT-diagonal preconditioner of a central plan (per-axis symbol sin^2(2 pi k / n)): operator parity with a
    torch.fft restatement, symmetry / positivity, and tests/test_gpu_path.py::test_fft_preconditioner's own criterion
    - a smaller residual than plain CG after the same number of iterations.  The iteration count of a tolerance
    solve is printed, not gated."""
    import math
    from unires_amd._project import _channel_plan
    _patch_oracle(monkeypatch, 'central')
    prob = make_problem(seed=61, **MATVEC_CASES[case])
    xo, yo = oracle_structs(prob)
    xg, yg, sett = gpu_structs(prob, dev)
    rho = torch.tensor(prob['rho'])
    dim = prob['dim_y']
    vx = N.voxel_size(prob['mat_y']).float()
    torch.manual_seed(3)
    for c in range(len(xo)):
        plan = _channel_plan(xg[c], yg[c], sett.method, sett.do_proj, diff='central')
        plan.precond_build(float(rho), float(yg[c].lam), mode='fft')
        if prob['do_proj']:
            acc = torch.zeros(dim)
            for xn in xo[c]:
                acc += xn.tau * O.proj_apply('AtA', torch.ones(dim)[None, None], xn.po, method=prob['method'])[0, 0]
            a = float(acc.double().mean())
        else:
            a = float(sum(float(xn.tau) for xn in xo[c]))
        cc = [float(rho) * float(yo[c].lam) ** 2 / float(vx[d]) ** 2 for d in range(3)]
        sym = [torch.sin(2.0 * math.pi * torch.arange(n, dtype=torch.float64) / n) ** 2 for n in dim]
        den = a + cc[0] * sym[0][:, None, None] + cc[1] * sym[1][None, :, None] + cc[2] * sym[2][None, None, :dim[2] // 2 + 1]
        pre_o = lambda v: torch.fft.irfftn(torch.fft.rfftn(v.double()) / den, s=dim).float()
        u, v = torch.rand(dim), torch.rand(dim)
        Pu, Pv = plan.precond_apply(u.to(dev)).cpu(), plan.precond_apply(v.to(dev)).cpu()
        assert rel_err(Pu, pre_o(u)) < 2e-5
        s1, s2 = (Pu.double() * v.double()).sum(), (u.double() * Pv.double()).sum()
        assert abs(s1 - s2) < 1e-5 * abs(s1) and (Pu.double() * u.double()).sum() > 0

    def run(precond, max_iter, tol):
        x, y, s = gpu_structs(prob, dev)
        s.diff, s.cgs_max_iter, s.cgs_tol, s.cgs_stop, s.cgs_precond = 'central', max_iter, tol, 'max_gain', precond
        import unires_amd as U
        info = []
        U._update_y(x, y, prob['z'].to(dev), prob['w'].to(dev), prob['rho'], torch.zeros_like(y[0].dat), s, info=info)
        torch.cuda.synchronize()
        return [yc.dat.cpu() for yc in y], info

    y_pcg, _ = run('fft', 8, 0.0)
    y_cg, _ = run('none', 8, 0.0)
    for c in range(len(xo)):
        b = O.y_rhs(xo[c], yo[c], prob['z'][c], prob['w'][c], rho, vx, prob['method'], prob['do_proj'])
        lhs = lambda d: O.proj('AtA', d, xo[c], yo[c], method=prob['method'], do=prob['do_proj'], rho=rho, vx_y=vx)
        r_pcg, r_cg = (b - lhs(y_pcg[c])).norm(), (b - lhs(y_cg[c])).norm()
        assert r_pcg < r_cg, (c, float(r_pcg), float(r_cg))
    it_pcg, it_cg = [i[0] for i in run('fft', 40, 1e-3)[1]], [i[0] for i in run('none', 40, 1e-3)[1]]
    print('diff fft central %s: iterations with the FFT preconditioner %s, without %s' % (case, it_pcg, it_cg), flush=True)
