"""What per-slice gains cost: the estimator's reduction, and the in-solve matvec with gains on.

sums: unires_gain_sums alone at 256 x 256 x 42 with the 42 slices along axis 2, and at 256 x 42 x 256 and 42 x 256 x 256
with them along axes 1 and 0 - without weights and with g and u - and unires_slice_sums on the same shapes in the same
process as the yardstick (an existing kernel that reads the same two volumes).  HIP events around 20 calls after a
warm-up round; median with min - max over the rounds, the kernels alternated within a round.

matvec: the in-solve matvec time at config 3 (256^3 x 3 with 6 mm slices) - every A(p) of the CG solves of one y-update
bracketed with HIP events by the library (unires_plan_time_matvecs; tol = 0), tools/slice_time.py's measurement - with
every observation weighted (`weights`) and with every observation weighted and gained (`gains`): the same pass, handed
another table.  The arms alternate within one run, `--rounds` times after one untimed round.

    python tools/gain_time.py [--rounds 5] [--out profiles/gain_time.json] [--sums | --matvec]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from mask_time import SHAPES, one_update  # noqa: E402

SUM_SHAPES = [((256, 256, 42), 2), ((256, 42, 256), 1), ((42, 256, 256), 0)]
ARMS = ('weights', 'gains')


def measure_sums(rounds, device, calls=20):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    lib = _lib.load()
    out = []
    gen = torch.Generator().manual_seed(3)
    for shape, axis in SUM_SHAPES:
        x = torch.randn(shape, generator=gen).to(device)
        ay = torch.randn(shape, generator=gen).to(device)
        g = torch.rand(shape, generator=gen).to(device)
        u = torch.rand(shape[axis], generator=gen).to(device)
        S = shape[axis]
        s2 = torch.empty(2 * S, dtype=torch.float64, device=device)
        s3 = torch.empty(3 * S, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream().cuda_stream
        kernels = {
            'slice_sums': lambda: lib.unires_slice_sums(x.data_ptr(), ay.data_ptr(), i3(shape), axis, s2.data_ptr(), st),
            'gain_sums': lambda: lib.unires_gain_sums(x.data_ptr(), ay.data_ptr(), None, None, i3(shape), axis, s3.data_ptr(), st),
            'gain_sums_gu': lambda: lib.unires_gain_sums(x.data_ptr(), ay.data_ptr(), g.data_ptr(), u.data_ptr(), i3(shape), axis,
                                                         s3.data_ptr(), st),
        }
        per = {k: [] for k in kernels}
        for r in range(rounds + 1):
            for k, call in kernels.items():  # alternated within a round
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(calls):
                    check(call())
                t1.record()
                torch.cuda.synchronize()
                if r > 0:  # (round 0: warm-up)
                    per[k].append(1e3 * t0.elapsed_time(t1) / calls)
        row = {'shape': list(shape), 'axis': axis, 'read_MB': round(2 * 4 * x.numel() / 1e6, 2),
               'read_MB_gu': round(3 * 4 * x.numel() / 1e6, 2)}
        for k, v in per.items():
            row[k] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
        row['gain_over_slice'] = round(row['gain_sums']['median_us'] / row['slice_sums']['median_us'], 3)
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def measure_matvec(name, rounds, device):
    import unires_amd as U
    from workloads import WORKLOADS, build_subject
    from unires_amd._project import _channel_plan, _slice_axis
    wl = WORKLOADS[name]
    x, y, z, w, rho, sett = build_subject(wl, device, seed=1234)
    sett.channel_streams = False  # one channel after the other: a launch's time is the kernel's own
    sett.cgs_tol = 0.0
    data = {}
    for c, xc in enumerate(x):
        for n, xn in enumerate(xc):
            S = int(xn.dat.shape[_slice_axis(xn)])
            u = torch.ones(S, dtype=torch.float32, device=device)
            u[:max(1, S // 3)] = 0.5
            e = torch.tensor([(1.0, 0.85, 1.15)[s % 3] for s in range(S)], dtype=torch.float32, device=device)
            data[(c, n)] = (u, e)
    tmp = torch.zeros_like(y[0].dat)
    plans_of = lambda: [_channel_plan(x[c], y[c], sett.method, sett.do_proj) for c in range(len(x))]
    per = {a: [] for a in ARMS}
    infos, napp = {}, 0
    for r in range(rounds + 1):
        for a in ARMS:  # alternated: drift of the clocks / the neighbours' load lands on every arm alike
            for (c, n), (u, e) in data.items():
                x[c][n].slice_w = u
                x[c][n].slice_gain = e if a == 'gains' else None
            one_update(U, plans_of, x, y, z, w, rho, tmp, sett, False)  # (the plan switches; the new graph is captured)
            us, napp = one_update(U, plans_of, x, y, z, w, rho, tmp, sett, True)
            if r > 0:  # (round 0: warm-up)
                per[a].append(us)
            infos[a] = plans_of()[0].repeat_info(0)
    res = {'workload': name, 'dim_y': list(wl['dim_y']), 'channels': wl['C'], 'applications_per_update': napp,
           'rounds': rounds,
           'forms': {a: {k: infos[a][k] for k in ('pull2', 'splat2_axis', 'shift', 'fused', 'weighted', 'gained')} for a in ARMS}}
    for a, v in per.items():
        res[a] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gain_time.json'))
    ap.add_argument('--sums', action='store_true', help='the reduction kernels alone')
    ap.add_argument('--matvec', action='store_true', help='the in-solve matvec at config 3 alone')
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'gain_sums / slice_sums: HIP events around 20 calls, median (min - max) over the rounds after one '
                   'warm-up round, kernels alternated; matvec: in-solve time per application '
                   '(unires_plan_time_matvecs), every observation weighted against weighted and gained, arms alternated',
           'device': torch.cuda.get_device_name(0)}
    if not args.matvec:
        out['sums'] = measure_sums(args.rounds, device)
    if not args.sums:
        out['matvec'] = measure_matvec(SHAPES['cfg3'], args.rounds, device)
        print(json.dumps(out['matvec']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
