"""What sett.diff = 'backward' / 'central' costs per operator application.

The in-solve matvec time - every A(p) of the CG solves of one y-update bracketed with HIP events by the library
(unires_plan_time_matvecs; the solves then run as plain launches, tol = 0) - for forward, backward and central
differences on

- the config-3 shape (256^3 x 3, 6 mm slices along z, general rigid): the projected regime, where a non-forward
  matvec is every A^T A kernel without its stencil epilogue plus one accumulating stencil pass (k_dtd_flat_w);
- the config-1 shape (181 x 217 x 181, A = I): the stencil pass alone (k_dtd_flat against k_dtd_flat_w).

The three differences alternate within one run, `--rounds` times after one untimed round; the figure of a
difference is the median over the rounds of its per-application mean (and the spread: min / max).  The bytes an
A = I application must move (read p, write q: 8 bytes per voxel) over the time give the share of the 8 TB/s HBM peak.

    python tools/diff_time.py [--rounds 7] [--out profiles/diff_time.json] [--only cfg1]

--only cfg1 / cfg3: one shape (for a rocprofv3 --kernel-trace --stats run of its own).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12
DIFFS = ('forward', 'backward', 'central')
SHAPES = {'cfg3': 'cfg3_256c3_thick6z', 'cfg1': 'cfg1_181c1_denoise'}


def one_update(U, plans_of, x, y, z, w, rho, tmp, sett, timed):
    """One y-update, channels one after the other; returns (microseconds per A(p), applications) when timed."""
    for yc in y:
        yc.dat.zero_()
    if not timed:
        U._update_y(x, y, z, w, rho, tmp, sett)
        torch.cuda.synchronize()
        return None
    plans = plans_of()
    for pl in plans:
        pl.time_matvecs(True)
    try:
        U._update_y(x, y, z, w, rho, tmp, sett)
        torch.cuda.synchronize()
        n, us = 0, 0.0
        for pl in plans:
            k, t = pl.matvec_time()
            n, us = n + k, us + t
    finally:
        for pl in plans:
            pl.time_matvecs(False)
    return us / max(n, 1), n


def measure(name, rounds, device):
    import unires_amd as U
    from unires_amd._project import _channel_plan
    from workloads import WORKLOADS, build_subject
    wl = WORKLOADS[name]
    x, y, z, w, rho, sett = build_subject(wl, device, seed=1234)
    sett.channel_streams = False  # one channel after the other: a launch's time is the kernel's own
    tmp = torch.zeros_like(y[0].dat)
    plans_of = lambda: [_channel_plan(x[c], y[c], sett.method, sett.do_proj) for c in range(len(x))]
    per = {d: [] for d in DIFFS}
    napp = 0
    for r in range(rounds + 1):
        for d in DIFFS:  # alternated: drift of the clocks / the neighbours' load lands on all three alike
            sett.diff = d
            one_update(U, plans_of, x, y, z, w, rho, tmp, sett, False)  # (the plan switches; the new graph is captured)
            us, napp = one_update(U, plans_of, x, y, z, w, rho, tmp, sett, True)
            if r > 0:  # (round 0: warm-up)
                per[d].append(us)
    nvox = 1
    for n in wl['dim_y']:
        nvox *= n
    res = {'workload': name, 'dim_y': list(wl['dim_y']), 'channels': wl['C'], 'applications_per_update': napp,
           'rounds': rounds}
    for d in DIFFS:
        med = statistics.median(per[d])
        res[d] = {'median_us': round(med, 2), 'min_us': round(min(per[d]), 2), 'max_us': round(max(per[d]), 2)}
        if wl.get('regime') == 'id':
            res[d]['share_of_hbm_peak'] = round(8.0 * nvox / (med * 1e-6) / HBM, 3)
    for d in DIFFS[1:]:
        res[d]['over_forward_us'] = round(res[d]['median_us'] - res['forward']['median_us'], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'diff_time.json'))
    ap.add_argument('--only', choices=list(SHAPES), default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    device = torch.device('cuda:0')
    out = {'what': 'in-solve matvec time per application (unires_plan_time_matvecs, HIP events), median over rounds; '
                   'forward / backward / central alternated within one run after one warm-up round',
           'device': torch.cuda.get_device_name(0), 'shapes': {}}
    for key, name in SHAPES.items():
        if args.only in (None, key):
            out['shapes'][key] = measure(name, args.rounds, device)
            print(json.dumps(out['shapes'][key]), flush=True)
    if args.only is None:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
