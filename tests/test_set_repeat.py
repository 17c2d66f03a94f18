"""The chains of tests/test_gpu_set_repeat.py held to their conditions on the CPU, on the float64 reference alone: every
stage within the tie cap (fewer than 1 % of the volume excluded; with the seeds and angles of the chains: none), the
orient chain's relabelling as stated, consecutive stage references further apart than the per-voxel bound (an operator
that did not move would be caught), and a stage-k reference with one 8 x 4 x 30 tile of stage k - 1 planted into it
caught by ``ref64.compare`` while the 2e-5 relative-L2 gate of ``test_plan_rebuilds_when_the_rigid_changes`` passes it."""
import pytest
import torch

from tests import ref64
from tests.helpers import rel_err
from tests.test_gpu_set_repeat import (CHAINS, MW_CHAINS, ORIENT_STAGES, matvec64, mw_matvec64, stage_problems,
                                       stage_reference, tie_cap_ok, tie_counts)

STAGES = [(name, k) for name, ch in CHAINS.items() for k in range(len(ch['stages']))]


def test_a_stage_replaces_the_moved_repeats_rigid_and_nothing_else():
    for name, ch in CHAINS.items():
        probs = stage_problems(name)
        assert len(probs) == len(ch['stages'])
        r0 = probs[0]['chans'][0]['reps']
        for k, prob in enumerate(probs[1:], 1):
            assert prob['rho'] == probs[0]['rho'] and prob['chans'][0]['lam'] == probs[0]['chans'][0]['lam']
            for i, (a, b) in enumerate(zip(r0, prob['chans'][0]['reps'])):
                assert a['dat'] is b['dat'] and a['tau'] == b['tau'] and a['dim_x'] == b['dim_x'], (name, k, i)
                assert torch.equal(a['mat_x'], b['mat_x']) and a['scl'] == b['scl'], (name, k, i)
                if i != ch['moved']:
                    assert a['rigid'] is b['rigid'], (name, k, i)
            moved = prob['chans'][0]['reps'][ch['moved']]['rigid']
            before = probs[k - 1]['chans'][0]['reps'][ch['moved']]['rigid']
            assert not torch.equal(moved, before), (name, k)
            # a rigid: orthonormal, det + 1
            Rm = moved[:3, :3]
            assert torch.allclose(Rm @ Rm.T, torch.eye(3, dtype=Rm.dtype), atol=1e-12) and float(torch.det(Rm)) > 0


@pytest.mark.parametrize('name,k', STAGES)
def test_tie_cap_of_every_stage(name, k):
    R = stage_reference(name, k)
    print('ties %s stage %d: %s of x %d / y %d' % (name, k, tie_counts(R), R['v'].numel(), R['p'].numel()))
    assert tie_cap_ok(R), (name, k, tie_counts(R))
    if name == 'orient':
        assert R['reps'][0]['orient'] == ORIENT_STAGES[k], (k, R['reps'][0]['orient'])
        assert tuple(R['reps'][0]['po'].dim_x) == tuple(stage_reference(name, 0)['reps'][0]['po'].dim_x)


@pytest.mark.parametrize('name', list(CHAINS))
def test_consecutive_stage_references_differ_beyond_the_bound(name):
    """What ``test_every_stage_per_voxel`` asserts of the kernel's q, shown of the references: stage k - 1's matvec, cast
    to float32, fails stage k's bound (so a plan whose operator did not move cannot pass), and stage k's own passes."""
    prev = None
    for k in range(len(CHAINS[name]['stages'])):
        R = stage_reference(name, k)
        refq, tolq = matvec64(R)
        assert ref64.compare(refq.float(), refq, tolq, R['myy'])['ok'], (name, k)
        if prev is not None:
            c = ref64.compare(matvec64(prev)[0].float(), refq, tolq, R['myy'] | prev['myy'])
            assert not c['ok'] and c['n_bad'] > 100, (name, k, c)
        prev = R


@pytest.mark.parametrize('name', list(MW_CHAINS))
def test_masked_weighted_stage_references_differ_from_the_plain_ones(name):
    for k in range(MW_CHAINS[name]):
        R = stage_reference(name, k)
        refq, tolq = mw_matvec64(R)
        assert ref64.compare(refq.float(), refq, tolq, R['myy'])['ok'], (name, k)
        assert not ref64.compare(matvec64(R)[0].float(), refq, tolq, R['myy'])['ok'], (name, k)


def test_one_stale_tile_is_caught_and_the_l2_gate_is_blind_to_a_stale_share_of_it():
    """The z chain's stage 1 (rot 0.0) with one k_splat2 tile (8 x 4 x 30) of stage 0 (rot 0.1) left in place - a tile
    whose schedule was not rebuilt: ``ref64.compare`` fails it, in that tile alone.  With the random input of these
    tests a whole tile of another operator is visible to the relative-L2 gate of tests/test_gpu_path.py's rebuild test
    as well (2e-5; measured 9.3e-4: the tile is 1 % of the volume and differs by 9 % in it), so that gate is held against
    what a stale tail leaves instead: the same tile with 1 % of its value still the old operator's (one stale segment
    among the about hundred that reach a tile).  The gate passes that (9.3e-6); the per-voxel bound fails it."""
    R0, R1 = stage_reference('z', 0), stage_reference('z', 1)
    ref0, (ref1, tol1) = matvec64(R0)[0], matvec64(R1)
    tile = (slice(16, 24), slice(16, 20), slice(0, 30))
    for share, l2_passes in ((1.0, False), (0.01, True)):
        bad = ref1.clone()
        bad[tile] += share * (ref0[tile] - ref1[tile])
        bad = bad.float()
        l2 = rel_err(bad, ref1)
        c = ref64.compare(bad, ref1, tol1, R1['myy'])
        print('stale tile, share %g: n_bad %d max err/tol %.3g rel_err %.3g' % (share, c['n_bad'], c['max_ratio'], l2))
        assert not c['ok'] and 100 < c['n_bad'] <= 8 * 4 * 30, c
        outside = torch.ones_like(R1['myy'])
        outside[tile] = False
        assert ref64.compare(bad, ref1, tol1, R1['myy'] | ~outside)['ok']  # (nothing outside the tile)
        assert (l2 < 2e-5) == l2_passes, (share, l2)
