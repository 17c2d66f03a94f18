"""What per-voxel weights cost per operator application.

The in-solve matvec time - every A(p) of the CG solves of one y-update bracketed with HIP events by the library
(unires_plan_time_matvecs; the solves then run as plain launches, tol = 0) - on the shapes of tools/mask_time.py
(config 3: 256^3 x 3 with 6 mm slices; config 2: 181 x 217 x 181 x 3 at 1 mm; config 1: 181 x 217 x 181, A = I), in four
arms that alternate within one run, `--rounds` times after one untimed round:

    off       the unweighted plan of the same build
    slice     every observation slice-weighted: forward -> k_slice_apply -> push - the second yardstick
    voxel     every observation voxel-weighted: forward -> k_voxel_apply -> push
    all       mask, slice weights and voxel weights: forward -> k_voxel_apply<MASK, SLICE> -> push - one pass, not three

A third of every observation's voxels (the first third of the planes of constant last index) carry the weight 1/2, the
rest 1; the slice weights and the mask are tools/slice_time.py's.  For configs 1 and 2 `off` runs a single-pass form the
weighted arms forgo: tools/mask_time.py's `pair` arm separates that from the pass.

    python tools/voxel_time.py [--rounds 5] [--out profiles/voxel_time.json] [--only cfg2]
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
from slice_time import subject  # noqa: E402

ARMS = ('off', 'slice', 'voxel', 'all')


def voxel_maps(data, device):
    """Per observation a weight map: 1/2 over the first third of the planes of constant last index, else 1."""
    maps = {}
    for key, (full, _, _) in data.items():
        g = torch.ones(tuple(full.shape), dtype=torch.float32, device=device)
        g[:, :, :max(1, g.shape[2] // 3)] = 0.5
        maps[key] = g
    return maps


def set_arm(arm, x, sett, data, maps):
    sett.mask_zeros = arm == 'all'
    for (c, n), (full, zeroed, u) in data.items():
        x[c][n].dat = zeroed if sett.mask_zeros else full
        x[c][n].slice_w = u if arm in ('slice', 'all') else None
        x[c][n].weight = maps[(c, n)] if arm in ('voxel', 'all') else None


def measure(name, rounds, device):
    import unires_amd as U
    from unires_amd._project import _channel_plan
    wl, x, y, z, w, rho, sett, data = subject(name, device)
    maps = voxel_maps(data, device)
    tmp = torch.zeros_like(y[0].dat)
    plans_of = lambda: [_channel_plan(x[c], y[c], sett.method, sett.do_proj) for c in range(len(x))]
    per = {a: [] for a in ARMS}
    infos, napp = {}, 0
    for r in range(rounds + 1):
        for a in ARMS:  # alternated: drift of the clocks / the neighbours' load lands on every arm alike
            set_arm(a, x, sett, data, maps)
            one_update(U, plans_of, x, y, z, w, rho, tmp, sett, False)  # (the plan switches; the new graph is captured)
            us, napp = one_update(U, plans_of, x, y, z, w, rho, tmp, sett, True)
            if r > 0:  # (round 0: warm-up)
                per[a].append(us)
            infos[a] = plans_of()[0].repeat_info(0)
    keys = ('pull2', 'splat2_axis', 'shift', 'fused', 'masked', 'weighted', 'voxel_weighted')
    res = {'workload': name, 'dim_y': list(wl['dim_y']), 'channels': wl['C'], 'applications_per_update': napp,
           'rounds': rounds, 'dim_x': [list(x[0][0].dat.shape)],
           'forms': {a: {k: infos[a][k] for k in keys} for a in ARMS}}
    for a, v in per.items():
        res[a] = {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voxel_time.json'))
    ap.add_argument('--only', choices=list(SHAPES), default=None)
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'in-solve matvec time per application (unires_plan_time_matvecs, HIP events), median over rounds; the '
                   'arms alternated within one run after one warm-up round; a third of the voxels at weight 1/2',
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
