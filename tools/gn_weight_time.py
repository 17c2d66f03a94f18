"""What slice weights cost in the two Gauss-Newton updates.

Config 3's observation shape (256^3 output, x space 256 x 256 x 42, tools/mask_time.py's workload), first channel: one
`_update_scaling` pass and one `_update_rigid` pass (one Gauss-Newton step with its line search, `sett.rigid_samp`), wall
clock around the call with the device idle before and after - both updates read their sums back, so host and device
time are one - divided by the number of repeats.  Two arms, alternated within one run `--rounds` times after one
untimed round: `off` (no weights: the yardstick, the same build) and `on` (a third of every observation's slices at
weight 1/2).  Scaling, rigid_q and po.rigid are put back after every call, so every call does the same work.

Also `unires_rigid_resid` alone against the four tensor passes it replaces (difference, two comparisons joined, masked
store) at 256 x 256 x 42: HIP events around 20 calls, median of the rounds.

    python tools/gn_weight_time.py [--rounds 5] [--out profiles/gn_weight_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from mask_time import SHAPES  # noqa: E402

ARMS = ('off', 'on')


def stats(v):
    return {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}


def measure_updates(rounds, device):
    from workloads import WORKLOADS, build_subject
    from unires_amd._project import _slice_axis
    from unires_amd._rigid import _logq, _update_rigid, affine_basis
    from unires_amd._update import _update_scaling, _update_y
    wl = WORKLOADS[SHAPES['cfg3']]
    x, y, z, w, rho, sett = build_subject(wl, device, seed=1234)
    x, y = [x[0]], [y[0]]
    # the subject starts from y = 0: one y-update (20 CG iterations) gives both updates an image to work on
    _update_y(x, y, z[:1], w[:1], rho, torch.zeros_like(y[0].dat), sett)
    weights = []
    for xn in x[0]:
        S = int(xn.dat.shape[_slice_axis(xn)])
        u = torch.ones(S, dtype=torch.float32, device=device)
        u[:max(1, S // 3)] = 0.5
        weights.append(u)
        if xn.rigid_q is None:
            xn.rigid_q = _logq(xn.po.rigid, affine_basis('SE'))
    saved = [(xn.po.scl, xn.rigid_q.clone(), xn.po.rigid.clone()) for xn in x[0]]
    calls = {'scaling': lambda: _update_scaling(x, y, sett, max_niter_gn=1, num_linesearch=6),
             'rigid': lambda: _update_rigid(x, y, sett, mean_correct=False, max_niter_gn=1, num_linesearch=6,
                                            samp=sett.rigid_samp)}
    per = {k: {a: [] for a in ARMS} for k in calls}
    for r in range(rounds + 1):
        for a in ARMS:  # alternated: drift of the clocks / the neighbours' load lands on both arms alike
            for xn, u in zip(x[0], weights):
                xn.slice_w = u if a == 'on' else None
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


def measure_resid(rounds, device, calls=20, shape=(256, 256, 42), axis=2):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=gen)
    x[torch.rand(shape, generator=gen) < 0.3] = 0
    x, ay = x.to(device), torch.randn(shape, generator=gen).to(device)
    u = torch.ones(shape[axis], dtype=torch.float32, device=device)
    u[:shape[axis] // 3] = 0.5
    out = torch.empty_like(ay)
    st = torch.cuda.current_stream().cuda_stream

    def tensor_form():
        d = ay - x
        d[(x == 0) | (ay == 0)] = 0
        return d

    forms = {'tensor_passes': tensor_form,
             'kernel': lambda: check(lib.unires_rigid_resid(x.data_ptr(), ay.data_ptr(), i3(shape), axis, None,
                                                            out.data_ptr(), st)),
             'kernel_weighted': lambda: check(lib.unires_rigid_resid(x.data_ptr(), ay.data_ptr(), i3(shape), axis,
                                                                     u.data_ptr(), out.data_ptr(), st))}
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
            **{k: stats(v) for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gn_weight_time.json'))
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'one _update_scaling pass and one _update_rigid pass per repeat, wall clock, weights off against on '
                   '(a third of the slices at 1/2), alternated after one warm-up round; unires_rigid_resid alone '
                   'against the tensor passes it replaces, HIP events around 20 calls; median, min, max over the rounds',
           'device': torch.cuda.get_device_name(0)}
    out['resid'] = measure_resid(args.rounds, device)
    print(json.dumps(out['resid']), flush=True)
    out['updates'] = measure_updates(args.rounds, device)
    print(json.dumps(out['updates']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
