"""What per-slice weights cost per operator application, and what the slice sums cost.

The in-solve matvec time - every A(p) of the CG solves of one y-update bracketed with HIP events by the library
(unires_plan_time_matvecs; the solves then run as plain launches, tol = 0) - on the shapes of tools/mask_time.py
(config 3: 256^3 x 3 with 6 mm slices; config 2: 181 x 217 x 181 x 3 at 1 mm; config 1: 181 x 217 x 181, A = I), in four
arms that alternate within one run, `--rounds` times after one untimed round:

    off       the unweighted plan of the same build
    on        every observation weighted: forward -> k_slice_apply -> push
    mask      sett.mask_zeros alone: forward -> k_mask_apply -> push
    mask_on   mask and weights: forward -> k_slice_apply<MASK> -> push - the yardstick is `mask`: one pass, not two

A third of every observation's slices (along po.dim_thick) carry the weight 1/2, the rest 1; for the mask arms the
first third of the planes of constant last index are zeroed, as in tools/mask_time.py.  The `pair` arm of that tool
(the unweighted operator on the two-kernel form, UNIRES_NO_ATA1=1 UNIRES_NO_ALIGNED=1, a process of its own) separates
the pass from the forgone single-pass forms for configs 1 and 2: --arm pair runs it from here.

--sums times unires_slice_sums alone: 256 x 256 x 42 and its transposes with the 42 slices along axis 2, 1 and 0, and
256 slices along axis 2; HIP events around 20 calls, median of the rounds.

    python tools/slice_time.py [--rounds 5] [--out profiles/slice_time.json] [--only cfg2]
    UNIRES_NO_ATA1=1 UNIRES_NO_ALIGNED=1 python tools/slice_time.py --arm pair > profiles/slice_time_pair.jsonl
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

from mask_time import SHAPES, measure_pair, one_update  # noqa: E402

ARMS = ('off', 'on', 'mask', 'mask_on')
SUM_SHAPES = [((256, 256, 42), 2), ((256, 42, 256), 1), ((42, 256, 256), 0), ((42, 256, 256), 2)]


def subject(name, device):
    from workloads import WORKLOADS, build_subject
    from unires_amd._project import _slice_axis
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
            zeroed = xn.dat.clone()
            zeroed[:, :, :zeroed.shape[2] // 3] = 0
            data[(c, n)] = (xn.dat, zeroed, u)
    return wl, x, y, z, w, rho, sett, data


def set_arm(arm, x, sett, data):
    sett.mask_zeros = arm.startswith('mask')
    for (c, n), (full, zeroed, u) in data.items():
        x[c][n].dat = zeroed if sett.mask_zeros else full
        x[c][n].slice_w = u if arm.endswith('on') else None


def measure(name, rounds, device):
    import unires_amd as U
    from unires_amd._project import _channel_plan
    wl, x, y, z, w, rho, sett, data = subject(name, device)
    tmp = torch.zeros_like(y[0].dat)
    plans_of = lambda: [_channel_plan(x[c], y[c], sett.method, sett.do_proj) for c in range(len(x))]
    per = {a: [] for a in ARMS}
    infos, napp = {}, 0
    for r in range(rounds + 1):
        for a in ARMS:  # alternated: drift of the clocks / the neighbours' load lands on every arm alike
            set_arm(a, x, sett, data)
            one_update(U, plans_of, x, y, z, w, rho, tmp, sett, False)  # (the plan switches; the new graph is captured)
            us, napp = one_update(U, plans_of, x, y, z, w, rho, tmp, sett, True)
            if r > 0:  # (round 0: warm-up)
                per[a].append(us)
            infos[a] = plans_of()[0].repeat_info(0)
    res = {'workload': name, 'dim_y': list(wl['dim_y']), 'channels': wl['C'], 'applications_per_update': napp,
           'rounds': rounds, 'dim_x': [list(x[0][0].dat.shape)],
           'forms': {a: {k: infos[a][k] for k in ('pull2', 'splat2_axis', 'shift', 'fused', 'masked', 'weighted')} for a in ARMS}}
    for a, v in per.items():
        res[a] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
    return res


def measure_sums(rounds, device, calls=20):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    lib = _lib.load()
    out = []
    gen = torch.Generator().manual_seed(3)
    for shape, axis in SUM_SHAPES:
        x = torch.randn(shape, generator=gen).to(device)
        ay = torch.randn(shape, generator=gen).to(device)
        sums = torch.empty(2 * shape[axis], dtype=torch.float64, device=device)
        st = torch.cuda.current_stream().cuda_stream
        per = []
        for r in range(rounds + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                check(lib.unires_slice_sums(x.data_ptr(), ay.data_ptr(), i3(shape), axis, sums.data_ptr(), st))
            t1.record()
            torch.cuda.synchronize()
            if r > 0:
                per.append(1e3 * t0.elapsed_time(t1) / calls)
        mb = 2 * 4 * x.numel() / 1e6
        out.append({'shape': list(shape), 'axis': axis, 'median_us': round(statistics.median(per), 2), 'min_us': round(min(per), 2),
                    'max_us': round(max(per), 2), 'read_MB': round(mb, 2)})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'slice_time.json'))
    ap.add_argument('--only', choices=list(SHAPES), default=None)
    ap.add_argument('--arm', choices=['pair'], default=None,
                    help='pair: the unweighted two-kernel operator of configs 1 and 2 alone (tools/mask_time.py\'s arm); run with UNIRES_NO_ATA1=1 UNIRES_NO_ALIGNED=1')
    ap.add_argument('--sums', action='store_true', help='time unires_slice_sums alone')
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'in-solve matvec time per application (unires_plan_time_matvecs, HIP events), median over rounds; the '
                   'arms alternated within one run after one warm-up round; a third of the slices at weight 1/2; '
                   'slice_sums: unires_slice_sums alone, HIP events around 20 calls',
           'device': torch.cuda.get_device_name(0), 'shapes': {}}
    if args.sums or (args.only is None and args.arm is None):
        out['slice_sums'] = measure_sums(args.rounds, device)
    if not args.sums:
        for key, name in SHAPES.items():
            if args.only in (None, key) and not (args.arm == 'pair' and key == 'cfg3'):
                out['shapes'][key] = (measure_pair if args.arm == 'pair' else measure)(name, args.rounds, device)
                print(json.dumps(out['shapes'][key]), flush=True)
    if args.only is None and args.arm is None and not args.sums:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
