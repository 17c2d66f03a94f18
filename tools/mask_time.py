"""What sett.mask_zeros costs per operator application.

The in-solve matvec time - every A(p) of the CG solves of one y-update bracketed with HIP events by the library
(unires_plan_time_matvecs; the solves then run as plain launches, tol = 0) - with the setting off and on, on

- the config-3 shape (256^3 x 3, 6 mm slices along z, general rigid): forward -> k_mask_apply -> push against the same
  forward -> push: the difference is the mask pass;
- the config-2 shape (181 x 217 x 181 x 3, 1 mm, general rigid): pull -> k_mask_apply -> push against the single-pass
  k_ata1;
- the config-1 shape (181 x 217 x 181, A = I): a denoising-regime plan with the identity affine, pull ->
  k_mask_apply -> push, against the flat stencil alone.

For configs 1 and 2 a third arm, `pair`, runs the UNMASKED operator on the two-kernel form the masked one takes, in a
process of its own with UNIRES_NO_ATA1=1 UNIRES_NO_ALIGNED=1 (--arm pair; config 2: the plain plan; config 1: the
denoising-regime plan with the identity affine, its masks never set - without UNIRES_NO_ALIGNED that plan takes the
one-kernel shift form): on - pair is the mask pass, pair - off the forgone single-pass form.

A third of every observation's slices are zeroed.  Off and on alternate within one run, `--rounds` times after one
untimed round; the figure of an arm is the median over the rounds of its per-application mean (and min / max).

    python tools/mask_time.py [--rounds 5] [--out profiles/mask_time.json] [--only cfg2]
    UNIRES_NO_ATA1=1 UNIRES_NO_ALIGNED=1 python tools/mask_time.py --arm pair > profiles/mask_time_pair.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'cfg3': 'cfg3_256c3_thick6z', 'cfg2': 'cfg2_181c3_1mm', 'cfg1': 'cfg1_181c1_denoise'}


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


def subject(name, device):
    from workloads import WORKLOADS, build_subject
    wl = WORKLOADS[name]
    x, y, z, w, rho, sett = build_subject(wl, device, seed=1234)
    sett.channel_streams = False  # one channel after the other: a launch's time is the kernel's own
    sett.cgs_tol = 0.0
    for xc in x:  # a third of the slices (planes of constant last index) are missing
        for xn in xc:
            xn.dat[:, :, :xn.dat.shape[2] // 3] = 0
    return wl, x, y, z, w, rho, sett


def summary(name, wl, napp, rounds, info, per):
    res = {'workload': name, 'dim_y': list(wl['dim_y']), 'channels': wl['C'], 'applications_per_update': napp,
           'rounds': rounds, 'last_arm_info': {k: info[k] for k in ('pull2', 'splat2_axis', 'shift', 'fused', 'masked')}}
    for a, v in per.items():
        res[a] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
    return res


def measure(name, rounds, device):
    import unires_amd as U
    from unires_amd._project import _channel_plan
    wl, x, y, z, w, rho, sett = subject(name, device)
    tmp = torch.zeros_like(y[0].dat)
    plans_of = lambda: [_channel_plan(x[c], y[c], sett.method, sett.do_proj) for c in range(len(x))]
    arms = ['off', 'on']
    per = {a: [] for a in arms}
    napp = 0
    for r in range(rounds + 1):
        for a in arms:  # alternated: drift of the clocks / the neighbours' load lands on every arm alike
            sett.mask_zeros = a == 'on'
            one_update(U, plans_of, x, y, z, w, rho, tmp, sett, False)  # (the plan switches; the new graph is captured)
            us, napp = one_update(U, plans_of, x, y, z, w, rho, tmp, sett, True)
            if r > 0:  # (round 0: warm-up)
                per[a].append(us)
    return summary(name, wl, napp, rounds, plans_of()[0].repeat_info(0), per)  # (info: the last arm's, `on`)


def measure_pair(name, rounds, device):
    """The unmasked operator of the plan the setting builds (A = I: the denoising regime with the identity affine),
    built here and never given a mask: right-hand side and a 20-iteration solve per channel, as a y-update runs them."""
    from unires_amd._plan import ChannelPlan
    from unires_amd._project import _plan_regime, _plan_repeats
    from unires_amd.spatial import voxel_size
    wl, x, y, z, w, rho, sett = subject(name, device)
    method, do = _plan_regime(sett.method, sett.do_proj, True)
    vx = [float(v) for v in voxel_size(y[0].mat).tolist()]
    plans = [ChannelPlan(y[c].dim, vx, _plan_repeats(x[c], y[c], sett.do_proj, True), method, do, device=device)
             for c in range(len(x))]
    b = torch.zeros_like(y[0].dat)
    per, napp = [], 0
    for r in range(rounds + 1):
        for timed in (False, True):
            napp, us = 0, 0.0
            for c, pl in enumerate(plans):
                y[c].dat.zero_()
                pl.time_matvecs(timed)
                pl.rhs([xn.dat for xn in x[c]], w[c], z[c], rho, float(y[c].lam), out=b)
                pl.cg(b, y[c].dat, rho, float(y[c].lam), max_iter=sett.cgs_max_iter, tolerance=0.0, sync=False)
                torch.cuda.synchronize()
                if timed:
                    k, t = pl.matvec_time()
                    napp, us = napp + k, us + t
                    pl.time_matvecs(False)
        if r > 0:
            per.append(us / max(napp, 1))
    return summary(name, wl, napp, rounds, plans[0].repeat_info(0), {'pair': per})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mask_time.json'))
    ap.add_argument('--only', choices=list(SHAPES), default=None)
    ap.add_argument('--arm', choices=['pair'], default=None,
                    help='pair: the unmasked two-kernel operator of configs 1 and 2 alone; run with UNIRES_NO_ATA1=1 UNIRES_NO_ALIGNED=1')
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'in-solve matvec time per application (unires_plan_time_matvecs, HIP events), median over rounds; '
                   'mask_zeros off / on alternated within one run after one warm-up round; a third of the slices zeroed',
           'device': torch.cuda.get_device_name(0), 'shapes': {}}
    for key, name in SHAPES.items():
        if args.only in (None, key) and not (args.arm == 'pair' and key == 'cfg3'):
            out['shapes'][key] = (measure_pair if args.arm == 'pair' else measure)(name, args.rounds, device)
            print(json.dumps(out['shapes'][key]), flush=True)
    if args.only is None and args.arm is None:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
