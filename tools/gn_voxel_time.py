"""What voxel weights cost in the two Gauss-Newton updates.

Config 3's observation shape (256^3 output, x space 256 x 256 x 42, tools/mask_time.py's workload), first channel: one
`_update_scaling` pass and one `_update_rigid` pass (one Gauss-Newton step with its line search, `sett.rigid_samp`), wall
clock around the call with the device idle before and after - both updates read their sums back, so host and device
time are one - divided by the number of repeats.  Four arms, alternated within one run `--rounds` times after one
untimed round: `off` (no weights) and `slice` (a third of every observation's slices at weight 1/2) - the two
yardsticks, paths this work does not change - `voxel` (a map with a third of the voxels at 1/2, `sett.voxel_gn`) and
`both` (the map beside the slice weights).  Scaling, rigid_q and po.rigid are put back after every call, so every call
does the same work.

Also the two kernels alone against their slice-weighted siblings at 256 x 256 x 42: HIP events around 20 calls, median
of the rounds.  The expectation to confirm or refute: every evaluation reads one more volume (g: 11 MB here).

    python tools/gn_voxel_time.py [--rounds 5] [--out profiles/gn_voxel_time.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gn_weight_time import stats  # noqa: E402
from mask_time import SHAPES  # noqa: E402

ARMS = ('off', 'slice', 'voxel', 'both')


def measure_updates(rounds, device):
    from workloads import WORKLOADS, build_subject
    from unires_amd._project import _channel_plan, _slice_axis
    from unires_amd._rigid import _logq, _update_rigid, affine_basis
    from unires_amd._update import _update_scaling, _update_y
    wl = WORKLOADS[SHAPES['cfg3']]
    x, y, z, w, rho, sett = build_subject(wl, device, seed=1234)
    x, y = [x[0]], [y[0]]
    # the subject starts from y = 0: one y-update (20 CG iterations) gives both updates an image to work on
    _update_y(x, y, z[:1], w[:1], rho, torch.zeros_like(y[0].dat), sett)
    sett.voxel_gn = True
    weights, maps = [], []
    gen = torch.Generator().manual_seed(7)
    for xn in x[0]:
        S = int(xn.dat.shape[_slice_axis(xn)])
        u = torch.ones(S, dtype=torch.float32, device=device)
        u[:max(1, S // 3)] = 0.5
        weights.append(u)
        g = torch.ones(tuple(xn.dat.shape), dtype=torch.float32)
        g[torch.rand(tuple(xn.dat.shape), generator=gen) < 1.0 / 3.0] = 0.5
        maps.append(g.to(device).contiguous())
        if xn.rigid_q is None:
            xn.rigid_q = _logq(xn.po.rigid, affine_basis('SE'))
    saved = [(xn.po.scl, xn.rigid_q.clone(), xn.po.rigid.clone()) for xn in x[0]]
    calls = {'scaling': lambda: _update_scaling(x, y, sett, max_niter_gn=1, num_linesearch=6),
             'rigid': lambda: _update_rigid(x, y, sett, mean_correct=False, max_niter_gn=1, num_linesearch=6,
                                            samp=sett.rigid_samp)}
    per = {k: {a: [] for a in ARMS} for k in calls}
    for r in range(rounds + 1):
        for a in ARMS:  # alternated: drift of the clocks / the neighbours' load lands on every arm alike
            for xn, u, g in zip(x[0], weights, maps):
                xn.slice_w = u if a in ('slice', 'both') else None
                xn.weight = g if a in ('voxel', 'both') else None
            # (the plan takes or drops the arm's weights here, outside the timed calls: that is the y-update's cost)
            _channel_plan(x[0], y[0], sett.method, sett.do_proj)
            for k, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0) / len(x[0])
                for xn, (scl, q, rigid) in zip(x[0], saved):
                    xn.po.scl, xn.rigid_q, xn.po.rigid = scl, q.clone(), rigid.clone()
                if r > 0:  # (round 0: warm-up)
                    per[k][a].append(ms)
    return {'workload': SHAPES['cfg3'], 'dim_y': list(wl['dim_y']), 'dim_x': [list(xn.dat.shape) for xn in x[0]],
            'repeats': len(x[0]), 'rigid_samp': sett.rigid_samp, 'unit': 'ms per repeat', 'rounds': rounds,
            **{k: {a: stats(v) for a, v in per[k].items()} for k in per}}


def measure_kernels(rounds, device, calls=20, shape=(256, 256, 42), axis=2):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=gen)
    x[torch.rand(shape, generator=gen) < 0.3] = 0
    x, ay = x.to(device), torch.randn(shape, generator=gen).to(device)
    g = torch.ones(shape)
    g[torch.rand(shape, generator=gen) < 1.0 / 3.0] = 0.5
    g = g.to(device)
    u = torch.ones(shape[axis], dtype=torch.float32, device=device)
    u[:shape[axis] // 3] = 0.5
    out = torch.empty_like(ay)
    sums = torch.empty(5, dtype=torch.float64, device=device)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    forms = {
        'resid': lambda: check(lib.unires_rigid_resid(P(x), P(ay), i3(shape), axis, None, P(out), st)),
        'resid_slice': lambda: check(lib.unires_rigid_resid(P(x), P(ay), i3(shape), axis, P(u), P(out), st)),
        'resid_voxel': lambda: check(lib.unires_rigid_resid_g(P(x), P(ay), P(g), i3(shape), axis, None, P(out), st)),
        'resid_both': lambda: check(lib.unires_rigid_resid_g(P(x), P(ay), P(g), i3(shape), axis, P(u), P(out), st)),
        'sums': lambda: check(lib.unires_scaling_sums(P(x), P(ay), i3(shape), axis, P(sums), st)),
        'sums_slice': lambda: check(lib.unires_scaling_sums_w(P(x), P(ay), i3(shape), axis, P(u), P(sums), st)),
        'sums_voxel': lambda: check(lib.unires_scaling_sums_g(P(x), P(ay), i3(shape), axis, P(g), None, P(sums), st)),
        'sums_both': lambda: check(lib.unires_scaling_sums_g(P(x), P(ay), i3(shape), axis, P(g), P(u), P(sums), st)),
    }
    per = {k: [] for k in forms}
    for r in range(rounds + 1):
        for k, f in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                f()
            t1.record()
            torch.cuda.synchronize()
            if r > 0:
                per[k].append(1e3 * t0.elapsed_time(t1) / calls)
    return {'shape': list(shape), 'axis': axis, 'unit': 'us per call', 'calls': calls,
            'volume_MB': round(4e-6 * x.numel(), 2), **{k: stats(v) for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gn_voxel_time.json'))
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'one _update_scaling pass and one _update_rigid pass per repeat, wall clock: no weights and slice '
                   'weights (the yardsticks) against a voxel map and both, alternated after one warm-up round; the two '
                   'kernels alone beside their siblings, HIP events around 20 calls; median, min, max over the rounds',
           'device': torch.cuda.get_device_name(0)}
    out['kernels'] = measure_kernels(args.rounds, device)
    print(json.dumps(out['kernels']), flush=True)
    out['updates'] = measure_updates(args.rounds, device)
    print(json.dumps(out['updates']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
