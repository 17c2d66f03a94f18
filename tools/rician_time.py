"""What the Rician data term costs (sett.noise_model = 'rician').

kernel: unires_rician_terms alone in its three forms - xt only (an iteration without an objective), sums only (an
objective evaluation on its own) and both (an iteration with one) - without and with a voxel map g, at 256 x 256 x 43
(config 3's observation, the 43 slices along axis 2) and at 256^3.  HIP events around 20 calls after a warm-up round,
arms alternated within a round, median with min - max over the rounds; the bytes a form has to move (x and ay read, g
read with sums, xt written) give the bandwidth it reaches.

fit: fit() on the config-3 workload (256^3, three channels of 6 mm slices; magnitudes of its observations, which carry
Gaussian noise), fixed ADMM iterations of 20 CG iterations (cgs_tol = 0), under 'gaussian' and under 'rician', with the
objective (tolerance > 0) and without (tolerance = 0); wall clock around fit() with the device idle before and after,
divided by the iterations, after a warm-up fit; arms alternated.

    python tools/rician_time.py [--rounds 5] [--iters 8] [--out profiles/rician_time.json]
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

SHAPES = [((256, 256, 43), 2), ((256, 256, 256), 2)]
WORKLOAD = 'cfg3_256c3_thick6z'


def stats(v):
    return {'median': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}


def measure_kernel(rounds, device, calls=20):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    P = lambda t: t.data_ptr()
    rows = []
    for shape, axis in SHAPES:
        S = shape[axis]
        sd = 75.0
        x = (torch.rand(shape, generator=gen) * 400.0).to(device)
        ay = (torch.rand(shape, generator=gen) * 400.0).to(device)
        g = torch.rand(shape, generator=gen).to(device)
        xt = torch.empty_like(x)
        L = torch.empty(S, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream().cuda_stream
        d, tau = i3(shape), 1.0 / sd ** 2
        call = lambda gp, o, s: (lambda: check(lib.unires_rician_terms(P(x), P(ay), gp, None, d, axis, tau, o, s, st)))
        arms = {'xt': call(None, P(xt), None), 'sums': call(None, None, P(L)), 'both': call(None, P(xt), P(L)),
                'sums_g': call(P(g), None, P(L)), 'both_g': call(P(g), P(xt), P(L))}
        volumes = {'xt': 3, 'sums': 2, 'both': 3, 'sums_g': 3, 'both_g': 4}
        per = {k: [] for k in arms}
        for r in range(rounds + 1):
            for k, run in arms.items():  # alternated within a round
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(calls):
                    run()
                t1.record()
                torch.cuda.synchronize()
                if r > 0:  # (round 0: warm-up)
                    per[k].append(1e3 * t0.elapsed_time(t1) / calls)
        mb = 4e-6 * x.numel()
        row = {'shape': list(shape), 'axis': axis, 'unit': 'us per call', 'volume_MB': round(mb, 2)}
        for k, v in per.items():
            row[k] = stats(v)
            row[k]['GB_per_s'] = round(volumes[k] * mb * 1e-3 / (row[k]['median'] * 1e-6), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def measure_fit(rounds, iters, device):
    import unires_amd as U
    from workloads import WORKLOADS, build_subject
    wl = WORKLOADS[WORKLOAD]

    def one(model, tolerance):
        x, y, z, w, rho, sett = build_subject(wl, device, seed=1234)
        for xc in x:
            for xn in xc:
                xn.dat = xn.dat.abs()
        for yc in y:
            yc.lam0 = float(yc.lam)
        sett.scaling, sett.unified_rigid, sett.clean_fov = False, False, False
        sett.max_iter, sett.tolerance, sett.reg_scl, sett.sched_num = iters, tolerance, 1.0, 0
        sett.cgs_max_iter, sett.cgs_tol = 20, 0.0
        sett.noise_model = model
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = U.fit(x, y, sett)[3]
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        assert info['n_iter'] == iters, info['n_iter']
        return ms / iters

    arms = [(m, t) for t in (1e-4, 0.0) for m in ('gaussian', 'rician')]
    name = lambda m, t: '%s_%s' % (m, 'objective' if t > 0 else 'no_objective')
    per = {name(m, t): [] for m, t in arms}
    for r in range(rounds + 1):
        for m, t in arms:  # alternated
            ms = one(m, t)
            if r > 0:  # (round 0: warm-up - plans, captured solves)
                per[name(m, t)].append(ms)
    out = {'workload': WORKLOAD, 'dim_y': list(wl['dim_y']), 'channels': wl['C'], 'admm_iterations': iters,
           'cg': '20 iterations, cgs_tol = 0', 'unit': 'ms per ADMM iteration (wall clock of fit() / iterations)',
           'rounds': rounds, **{k: stats(v) for k, v in per.items()}}
    for k in ('objective', 'no_objective'):
        out['rician_over_gaussian_' + k] = round(out['rician_' + k]['median'] / out['gaussian_' + k]['median'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rician_time.json'))
    ap.add_argument('--kernel', action='store_true', help='the kernel alone')
    ap.add_argument('--fit', action='store_true', help='fit() alone')
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'unires_rician_terms: HIP events around 20 calls, median, min, max over the rounds after one warm-up '
                   'round, arms alternated; fit: wall clock of fit() per ADMM iteration on config 3 under both noise '
                   'models, with and without the objective',
           'device': torch.cuda.get_device_name(0)}
    if not args.fit:
        out['kernel'] = measure_kernel(args.rounds, device)
    if not args.kernel:
        out['fit'] = measure_fit(args.rounds, args.iters, device)
        print(json.dumps(out['fit']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
