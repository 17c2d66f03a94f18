"""The per-voxel comparator of tests/ref64.py, checked on the CPU: it is sound (the float32 oracle, a correct
float32 implementation of the same operator, passes it for A, At, AtA and the matvec) and sharp (one voxel off by
10x its tolerance, one 8x4x30 tile off by 1e-3 and one non-zero value outside the operator's support all fail it,
while the relative-L2 gates of the GPU parity tests pass the first two)."""
import pytest
import torch

from oracle import nitorch_restated as N
from oracle import unires_restated as O
from tests import ref64
from tests.helpers import make_problem, oracle_structs, rel_err

PROBLEMS = {
    'small_thick3': dict(dim_y=(16, 14, 12), thick=3, rot=0.1, trans=0.7),
    'mid_thick6z_scl': dict(dim_y=(41, 38, 61), thick=6, thick_axes=[2], rot=0.12, trans=2.0, scl=0.1),
    'mid_iso2_gauss': dict(dim_y=(34, 30, 36), thick=2, iso=(2, 2, 2), prof_ip=2, rot=0.1, trans=1.0),
    'mid_denoise': dict(dim_y=(33, 29, 40), regime='dn', rot=0.1, trans=2.0),
}


def _setup(kw, seed=3):
    prob = make_problem(seed=seed, **kw)
    xs, ys = oracle_structs(prob)
    xc, yc = xs[0], ys[0]
    po = xc[0].po
    op = ref64.Operator64(po, prob['method'])
    gen = torch.Generator().manual_seed(seed + 1)
    p = (torch.rand(prob['dim_y'], generator=gen) * 10 - 2).float()
    v = (torch.rand(tuple(po.dim_x), generator=gen) * 10 - 2).float()
    return prob, xc, yc, po, op, p, v


def _oracle32(op_name, dat, po, method):
    return O.proj_apply(op_name, dat[None, None], po, method=method)[0, 0]


@pytest.mark.parametrize('name', list(PROBLEMS))
def test_float32_oracle_passes_the_per_voxel_bound(name):
    prob, xc, yc, po, op, p, v = _setup(PROBLEMS[name])
    m = prob['method']
    mx, my, myy, _ = op.tie_masks(po)
    ref, tol = op.bound_A(p)
    r = ref64.compare(_oracle32('A', p, po, m), ref, tol, mx)
    assert r['ok'], ('A', r)
    ref, tol = op.bound_At(v)
    r = ref64.compare(_oracle32('At', v, po, m), ref, tol, my)
    assert r['ok'], ('At', r)
    ref, tol = op.bound_AtA(p)
    r = ref64.compare(_oracle32('AtA', p, po, m), ref, tol, myy)
    assert r['ok'], ('AtA', r)
    rho = torch.tensor(prob['rho'], dtype=torch.float32)
    vx = N.voxel_size(prob['mat_y']).float()
    q32 = O.proj('AtA', p, xc, yc, method=m, do=True, rho=rho, vx_y=vx)
    ref, tol = op.bound_matvec(p, xc[0].tau, rho, yc.lam, vx)
    r = ref64.compare(q32, ref, tol, myy)
    assert r['ok'], ('matvec', r)
    assert r['max_ratio'] > 0.0  # (the oracle's float32 result really differs from the float64 one)


def test_comparator_catches_one_voxel_and_one_tile_that_l2_gates_pass():
    # mid-size, a partial tile on every axis: 97 = 12 * 8 + 1, 90 = 22 * 4 + 2, 121 = 4 * 30 + 1
    prob, xc, yc, po, op, p, v = _setup(dict(dim_y=(97, 90, 121), thick=6, thick_axes=[2], rot=0.12, trans=2.0,
                                             scl=0.1))
    ref, tol = op.bound_AtA(p)
    out = ref.clone()
    assert ref64.compare(out, ref, tol)['ok']
    # (b) one voxel 10x its tolerance off: the relative-L2 gate of the mid-size tests (2e-5) cannot see it
    c = tuple(s // 2 for s in prob['dim_y'])
    bad = out.clone()
    bad[c] += 10 * tol[c]
    assert rel_err(bad, ref) < 2e-5
    r = ref64.compare(bad, ref, tol)
    assert not r['ok'] and r['n_bad'] == 1 and r['first'] == c
    # (c) one 8 x 4 x 30 tile (k_splat2 / k_ata1) scaled by 1 + 1e-3: the 256^3 gate (1e-4) passes it
    bad = out.clone()
    bad[40:48, 44:48, 60:90] *= 1 + 1e-3
    assert rel_err(bad, ref) < 1e-4
    r = ref64.compare(bad, ref, tol)
    assert not r['ok'] and r['n_bad'] > 100


def test_comparator_demands_exact_zero_outside_the_support():
    # one impulse: A^T A e_j is confined to the voxels within reach of the grid points e_j's x voxels read
    prob, xc, yc, po, op, p, v = _setup(PROBLEMS['mid_thick6z_scl'])
    e = torch.zeros(prob['dim_y'])
    e[20, 19, 30] = 1.0
    ref, tol = op.bound_AtA(e)
    assert (tol == 0).any() and (tol > 0).any()
    r = ref64.compare(_oracle32('AtA', e, po, prob['method']), ref, tol)
    assert r['ok'], r
    far = tuple(int(i) for i in torch.nonzero(tol == 0)[0])
    bad = ref.clone()
    bad[far] = 1e-30  # (d) a single non-zero value outside the support
    r = ref64.compare(bad, ref, tol)
    assert not r['ok'] and r['first'] == far
