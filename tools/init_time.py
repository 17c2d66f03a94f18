"""init() at the demo's full size: three contrasts of a 181 x 217 x 181 anatomy at 1 mm in 4 mm slices
along x, y and z, planted rigids of +-5 mm / +-0.1 rad, given as [dat, mat] pairs on the device.  Wall
time of init() as a whole and of each of its steps (the device drained after every step), and of
_write_data with and without the files (float32 .nii.gz, into a temporary directory); medians of
`--reps` runs after `--warmup` runs.  Writes the JSON to `--out`.

    python tools/init_time.py [--reps 5] [--warmup 1] [--out profiles/init_time.json]
    python tools/init_time.py --once     # one init() + one _write_data (no files), nothing timed:
                                         # for a rocprofv3 --kernel-trace --stats run of its own
                                         # (profiles/init_kernel_stats.csv)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM = (181, 217, 181)
STEPS = ('_read_data', '_estimate_hyperpar', '_fix_affine', '_resample_inplane', '_init_reg', '_format_y',
         '_proj_info_add', '_init_y_dat', '_init_y_label')


def subject(dev):
    from tests import coreg_phantom as P
    rng = np.random.default_rng(3)
    data = []
    for c, ax in enumerate((0, 1, 2)):
        v, d = [1.0, 1.0, 1.0], list(DIM)
        v[ax], d[ax] = 4.0, int(round(DIM[ax] / 4.0))
        dat, mat = P.observation(tuple(d), tuple(v), c, 103 + c, dev, sub_axis=ax)
        Pl = np.eye(4) if c == 0 else P.random_rigid(rng, 5.0, 0.1)
        data.append([dat, torch.from_numpy(Pl @ mat)])
    return data


def stepwise(data, sett):
    """init()'s own sequence (unires_amd/run.py), one timed step at a time."""
    import unires_amd as U
    from unires_amd import _core
    t = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t[name] = time.perf_counter() - t0
        return out
    x = timed('_read_data', lambda: U._read_data(data, sett))
    x = timed('_estimate_hyperpar', lambda: U._estimate_hyperpar(x, sett))
    x = timed('_fix_affine', lambda: _core._fix_affine(x, sett))
    x = timed('_resample_inplane', lambda: U._resample_inplane(x, sett))
    x, sett = timed('_init_reg', lambda: U._init_reg(x, sett))
    y, sett = timed('_format_y', lambda: U._format_y(x, sett))
    x = timed('_proj_info_add', lambda: U._proj_info_add(x, y, sett))
    y = timed('_init_y_dat', lambda: U._init_y_dat(x, y, sett))
    y = timed('_init_y_label', lambda: U._init_y_label(x, y, sett))
    return x, y, sett, t


def settings(dev, **kw):
    import unires_amd as U
    sett = U.settings()
    sett.device = dev
    for k, v in kw.items():
        setattr(sett, k, v)
    return sett


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'init_time.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('init_time.py needs a GPU')
    import __graft_entry__ as g
    g.build()
    import unires_amd as U
    dev = torch.device('cuda:0')
    data = subject(dev)
    torch.cuda.synchronize()
    if args.once:
        x, y, sett = U.init(data, settings(dev))
        U._write_data(x, y, settings(dev, write_out=False))
        torch.cuda.synchronize()
        print(json.dumps({'dim_y': list(y[0].dim), 'method': sett.method}))
        return
    whole, steps, clamp, files = [], {k: [] for k in STEPS}, [], []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, y, sett = U.init(data, settings(dev))
        torch.cuda.synchronize()
        t_whole = time.perf_counter() - t0
        x, y, sett, t = stepwise(data, settings(dev))
        t0 = time.perf_counter()
        U._write_data(x, y, settings(dev, write_out=False))
        torch.cuda.synchronize()
        t_clamp = time.perf_counter() - t0
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            U._write_data(x, y, settings(dev, dir_out=tmp))
            t_files = time.perf_counter() - t0
        if i >= args.warmup:
            whole.append(t_whole)
            clamp.append(t_clamp)
            files.append(t_files)
            for k in STEPS:
                steps[k].append(t[k])

    def med(v):
        return {'median_s': round(statistics.median(v), 6), 'min_s': round(min(v), 6), 'n': len(v)}
    out = {'shape': {'truth': list(DIM), 'observations': [list(xc[0].dim) for xc in x], 'slices_mm': 4,
                     'misalignment': '+-5 mm / +-0.1 rad', 'input': '[dat, mat] pairs on the device'},
           'device': torch.cuda.get_device_name(0),
           'mean_space': {'dim': list(y[0].dim), 'vx': U.spatial.voxel_size(y[0].mat).tolist()},
           'method': sett.method, 'do_proj': sett.do_proj,
           'init_wall': med(whole), 'steps_wall': {k: med(v) for k, v in steps.items()},
           'steps_sum_median_s': round(sum(statistics.median(v) for v in steps.values()), 6),
           'write_data_clamp_only_wall': med(clamp), 'write_data_with_files_wall': med(files),
           'note': 'wall clock, the device drained after every step; files: three float32 .nii.gz of the mean-space size'}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
