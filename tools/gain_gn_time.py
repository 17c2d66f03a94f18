"""What carrying the slice gains through the rigid Gauss-Newton update costs.

kernels: unires_rigid_terms_e - without `out` (a line-search evaluation) and with it (the Gauss-Newton evaluation),
without and with a voxel map g - against the composition of existing calls it
replaces, in the same process: unires_slice_apply (the gained prediction into a temporary), unires_slice_sums /
unires_voxel_sums on it and, with `out`, unires_rigid_resid / unires_rigid_resid_g on it in place.  Shapes:
tools/gain_time.py's - 256 x 256 x 42 with the 42 slices along axis 2, and its transposes with them along axes 1 and 0 -
and the decimated shape the rigid update sees for config 3's observations at samp = 3 (sk = max(1, floor(samp / vx +
1/2)) per axis, dim_x <- floor(dim_x / sk): 85 x 85 x 42).  HIP events around 20 calls after a warm-up round, arms
alternated within a round, median with min - max over the rounds.

update: one `_update_rigid` call (one Gauss-Newton step with its line search, samp = 0) on DESIGN 8.6's phantom
(48 x 48 x 40, two repeats with 3 mm slices) with user gains beside slice weights on the second repeat against the same
call with the slice weights alone; wall clock around the call with the device idle before and after (the update reads
its sums back), rigid_q and po.rigid put back after every call, arms alternated.

    python tools/gain_gn_time.py [--rounds 5] [--out profiles/gain_gn_time.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gain_time import SUM_SHAPES  # noqa: E402


def decimated(dim, vx, samp):
    """_proj_info's sub-sampling rule."""
    sk = [max(1, int(math.floor(samp / v + 0.5))) for v in vx]
    return tuple(int(math.floor(d / k)) for d, k in zip(dim, sk))


SHAPES = SUM_SHAPES + [(decimated((256, 256, 42), (1.0, 1.0, 6.0), 3.0), 2)]


def stats(v):
    return {'median': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}


def measure_kernels(rounds, device, calls=20):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    P = lambda t: t.data_ptr()
    rows = []
    for shape, axis in SHAPES:
        S = shape[axis]
        x = torch.randn(shape, generator=gen)
        x[torch.rand(shape, generator=gen) < 0.3] = 0
        x, ay = x.to(device), torch.randn(shape, generator=gen).to(device)
        g = torch.rand(shape, generator=gen).to(device)
        u = torch.rand(S, generator=gen).to(device)
        e = (0.5 + 1.5 * torch.rand(S, generator=gen)).to(device)
        t = (u.double() * e.double()).float()
        tmp, work = torch.empty_like(ay), ay.clone()
        sums = torch.empty(2 * S, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream().cuda_stream
        d = i3(shape)

        def fused(gp, out):
            return lambda: check(lib.unires_rigid_terms_e(P(x), P(work), gp, P(u), P(e), d, axis, P(sums), out, st))

        def composed(with_g, with_out):
            def run():
                check(lib.unires_slice_apply(P(work), P(tmp), P(e), d, axis, st))
                if with_g:
                    check(lib.unires_voxel_sums(P(x), P(tmp), P(g), d, axis, P(sums), st))
                    if with_out:
                        check(lib.unires_rigid_resid_g(P(x), P(tmp), P(g), d, axis, P(t), P(tmp), st))
                else:
                    check(lib.unires_slice_sums(P(x), P(tmp), d, axis, P(sums), st))
                    if with_out:
                        check(lib.unires_rigid_resid(P(x), P(tmp), d, axis, P(t), P(tmp), st))
            return run

        # (the fused call with `out` writes beside ay here, not over it as _rigid_terms does: repeated calls in place
        # would feed residuals back in as predictions; the traffic - one volume stored - is the same)
        arms = {'fused_ls': fused(None, None), 'composed_ls': composed(False, False),
                'fused_gn': fused(None, P(tmp)), 'composed_gn': composed(False, True),
                'fused_ls_g': fused(P(g), None), 'composed_ls_g': composed(True, False),
                'fused_gn_g': fused(P(g), P(tmp)), 'composed_gn_g': composed(True, True)}
        per = {k: [] for k in arms}
        for r in range(rounds + 1):
            for k, call in arms.items():  # alternated within a round
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(calls):
                    call()
                t1.record()
                torch.cuda.synchronize()
                if r > 0:  # (round 0: warm-up)
                    per[k].append(1e3 * t0.elapsed_time(t1) / calls)
        row = {'shape': list(shape), 'axis': axis, 'unit': 'us per call', 'volume_MB': round(4e-6 * x.numel(), 2),
               **{k: stats(v) for k, v in per.items()}}
        for k in ('ls', 'gn', 'ls_g', 'gn_g'):
            row['fused_over_composed_' + k] = round(row['fused_' + k]['median'] / row['composed_' + k]['median'], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def measure_update(rounds, device):
    from tests.helpers import gpu_structs, make_problem
    from unires_amd._rigid import _update_rigid
    prob = make_problem(seed=5, dim_y=(48, 48, 40), thick=3, n_repeats=2, rot=0.0, trans=0.0, noise_sd=5.0,
                        thick_axes=None, shift=(0.0, 0.0, 0.0))
    x, y, sett = gpu_structs(prob, device)
    sett.gain_gn = True
    x1 = x[0][1]
    S = int(x1.dat.shape[1])
    u = torch.ones(S, dtype=torch.float32, device=device)
    u[:max(1, S // 3)] = 0.5
    e = torch.tensor([(1.0, 0.85, 1.15)[s % 3] for s in range(S)], dtype=torch.float32, device=device)
    for xn in x[0]:
        xn.rigid_q = torch.zeros(6, dtype=torch.float64)
    saved = [(xn.rigid_q.clone(), xn.po.rigid.clone()) for xn in x[0]]
    per = {'slice_weights': [], 'slice_weights_and_gains': []}
    for r in range(rounds + 1):
        for arm in per:  # alternated
            x1.slice_w = u
            x1.slice_gain = e if arm == 'slice_weights_and_gains' else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _update_rigid(x, y, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            for xn, (q, rigid) in zip(x[0], saved):
                xn.rigid_q, xn.po.rigid = q.clone(), rigid.clone()
            if r > 0:  # (round 0: warm-up)
                per[arm].append(ms)
    return {'phantom': 'DESIGN 8.6: 48 x 48 x 40, two repeats with 3 mm slices', 'unit': 'ms per _update_rigid call',
            'rounds': rounds, **{k: stats(v) for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gain_gn_time.json'))
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'unires_rigid_terms_e (fused) against unires_slice_apply + unires_slice_sums / unires_voxel_sums '
                   '[+ unires_rigid_resid / unires_rigid_resid_g] (composed): ls - no out, a line-search evaluation; gn - '
                   'with out in place; _g - with a voxel map; HIP events around 20 calls, median, min, max over the '
                   'rounds after one warm-up round, arms alternated.  update: one _update_rigid call, wall clock',
           'device': torch.cuda.get_device_name(0)}
    out['kernels'] = measure_kernels(args.rounds, device)
    out['update'] = measure_update(args.rounds, device)
    print(json.dumps(out['update']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
