"""What the bias field costs: its two launchers alone, and an ADMM iteration with sett.bias on and off.

launchers: unires_bias_field (b, g b^2 and x / b written) and unires_bias_terms (full, and for the objective alone) at
the 256 x 256 x 42 observation of config 3, for orders (4, 4, 2) and (8, 8, 8), without weights and with g and u; HIP
events around 20 calls after a warm-up round, median with min - max over the rounds, the calls alternated within a round.

iteration: `_update_admm` at config 3 (256^3 x 3 with 6 mm slices; tol = 0, no objective), wall clock around 3 iterations
with the device idle before and after, sett.bias off and on alternated within a round on one set of structs; the orders
are those of sett.bias_cutoff = 60 mm on the observation's grid.

    python tools/bias_time.py [--rounds 5] [--out profiles/bias_time.json] [--launchers | --iteration]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (256, 256, 42)
ORDERS = [(4, 4, 2), (8, 8, 8)]


def _stats(v, nd=2):
    return {'median': round(statistics.median(v), nd), 'min': round(min(v), nd), 'max': round(max(v), nd)}


def measure_launchers(rounds, device, calls=20):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    from unires_amd._update import bias_tables
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    mu = (50.0 + 30.0 * torch.rand(SHAPE, generator=gen)).to(device)
    x = (mu.cpu() * (1.0 + 0.1 * torch.randn(SHAPE, generator=gen))).to(device)
    g = torch.rand(SHAPE, generator=gen).to(device)
    u = torch.rand(SHAPE[2], generator=gen).to(device)
    b, gb2, xb = (torch.empty(SHAPE, device=device) for _ in range(3))
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: None if t is None else t.data_ptr()
    out = []
    for k in ORDERS:
        tabs = [torch.from_numpy(t).to(device) for t in bias_tables(SHAPE, k)]
        coef = torch.from_numpy(0.05 * np.random.default_rng(1).standard_normal(k)).to(device)
        K, Q = int(np.prod(k)), int(np.prod([2 * v - 1 for v in k]))
        o = torch.empty(1 + K + Q, dtype=torch.float64, device=device)
        field = lambda gg, full: lib.unires_bias_field(P(coef), P(tabs[0]), P(tabs[1]), P(tabs[2]), i3(k), i3(SHAPE),
                                                       float(np.log(4.0)), P(gg), P(x), P(b), P(gb2) if full else None,
                                                       P(xb) if full else None, st)
        terms = lambda gg, uu, kk: lib.unires_bias_terms(P(x), P(mu), P(b), P(gg), P(uu), 2, P(tabs[0]), P(tabs[1]),
                                                         P(tabs[2]), i3(kk), i3(SHAPE), P(o), st)
        kernels = {
            'field_b': lambda: field(None, False),
            'field_all': lambda: field(None, True),
            'field_all_g': lambda: field(g, True),
            'terms': lambda: terms(None, None, k),
            'terms_gu': lambda: terms(g, u, k),
            'terms_objective': lambda: terms(None, None, (0, 0, 0)),
        }
        check(field(None, True))
        per = {name: [] for name in kernels}
        for r in range(rounds + 1):
            for name, call in kernels.items():  # alternated within a round
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(calls):
                    check(call())
                t1.record()
                torch.cuda.synchronize()
                if r > 0:  # (round 0: warm-up)
                    per[name].append(1e3 * t0.elapsed_time(t1) / calls)
        row = {'shape': list(SHAPE), 'orders': list(k), 'volume_MB': round(4 * x.numel() / 1e6, 2)}
        for name, v in per.items():
            s = _stats(v)
            row[name] = {'median_us': s['median'], 'min_us': s['min'], 'max_us': s['max']}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def measure_iteration(rounds, device, iters=3):
    import unires_amd as U
    from workloads import WORKLOADS, build_subject
    from unires_amd.run import _init_bias
    from unires_amd._update import bias_orders
    wl = WORKLOADS['cfg3_256c3_thick6z']
    x, y, z, w, rho, sett = build_subject(wl, device, seed=1234)
    sett.cgs_tol, sett.tolerance = 0.0, 0.0
    tmp = torch.zeros_like(y[0].dat)
    per = {'off': [], 'on': []}
    orders = [list(bias_orders(xc[0], sett)) for xc in x]
    for r in range(rounds + 1):
        for arm in ('off', 'on'):  # alternated: drift lands on both arms alike
            sett.bias = arm == 'on'
            _init_bias(x, sett, device)  # (on: from zeros again; off: the fields are forgotten)
            U._update_admm(x, y, z, w, rho, tmp, None, 0, sett)  # (untimed: the plans switch their kernels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(iters):
                U._update_admm(x, y, z, w, rho, tmp, None, it, sett)
            torch.cuda.synchronize()
            if r > 0:  # (round 0: warm-up)
                per[arm].append(1e3 * (time.perf_counter() - t0) / iters)
    res = {'workload': 'cfg3_256c3_thick6z', 'dim_y': list(wl['dim_y']), 'channels': wl['C'],
           'observation': list(x[0][0].dat.shape), 'orders': orders, 'cgs_max_iter': int(sett.cgs_max_iter),
           'iterations_timed': iters, 'rounds': rounds}
    for arm, v in per.items():
        s = _stats(v, 3)
        res[arm] = {'median_ms': s['median'], 'min_ms': s['min'], 'max_ms': s['max']}
    res['on_over_off'] = round(res['on']['median_ms'] / res['off']['median_ms'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bias_time.json'))
    ap.add_argument('--launchers', action='store_true', help='the two launchers alone')
    ap.add_argument('--iteration', action='store_true', help='the ADMM iteration at config 3 alone')
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'launchers: HIP events around 20 calls, median (min - max) over the rounds after one warm-up round, '
                   'calls alternated; iteration: wall clock per _update_admm call over 3 calls, device idle before and '
                   'after, sett.bias off / on alternated',
           'device': torch.cuda.get_device_name(0)}
    if not args.iteration:
        out['launchers'] = measure_launchers(args.rounds, device)
    if not args.launchers:
        out['iteration'] = measure_iteration(args.rounds, device)
        print(json.dumps(out['iteration']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
