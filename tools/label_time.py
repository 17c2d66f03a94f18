"""Label warping at full size (256^3 output from a 181 x 217 x 181 parcellation, a small rigid, as in
tests/test_gpu_label.py): the one-pass vote (k_warp_label) against the reference's form - one linear
pull of the indicator and one select pass per label value - at U = 4, 20 and 100 values, and one
linear pull of the same geometry.  HIP events around `--reps` calls after `--warmup` calls; prints one
JSON line (median / min of the per-call times, microseconds).

    python tools/label_time.py [--reps 20] [--warmup 3] [--vote-only]

--vote-only: warm-up and timed vote calls only (for a rocprofv3 --kernel-trace --stats run of its own).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SDIM, GDIM = (181, 217, 181), (256, 256, 256)


def per_label_form(lab, M12, gdim):
    """The reference's _warp_label (unires/_core.py:419-436) on the HIP linear pull (selects as
    torch.where: no host round trip per value)."""
    from unires_amd import _ops
    f = torch.zeros(gdim, dtype=torch.float32, device=lab.device)
    p = torch.zeros_like(f)
    for v in lab.unique():
        t = _ops.pull_affine((lab == v).float(), M12, gdim)
        m = t > p
        p = torch.where(m, t, p)
        f = torch.where(m, v, f)
    return f


def time_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return {'median_us': round(statistics.median(ts), 1), 'min_us': round(min(ts), 1), 'n': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--vote-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('label_time.py needs a GPU')
    import __graft_entry__ as g
    g.build()
    from unires_amd import _ops
    from unires_amd.spatial import _m12
    from tests.test_gpu_label import _labels, _rigid_case
    dev = torch.device('cuda:0')
    M12 = _m12(_rigid_case(21, SDIM, GDIM))
    labs = {u: _labels(SDIM, u, seed=21, device=dev) for u in ((100,) if args.vote_only else (4, 20, 100))}
    torch.cuda.synchronize()
    if args.vote_only:
        t = time_us(lambda: _ops.warp_label(labs[100], M12, GDIM), args.reps, args.warmup)
        print(json.dumps({'vote_U100': t}))
        return
    out = {'case': {'label_dim': SDIM, 'out_dim': GDIM, 'geometry': 'rigid (tests/test_gpu_label.py seed 21)'},
           'vote': {}, 'per_label_form': {}}
    for u, lab in labs.items():
        n = int(lab.unique().numel())
        out['vote']['U%d' % u] = dict(time_us(lambda: _ops.warp_label(lab, M12, GDIM), args.reps, args.warmup),
                                      distinct=n)
        out['per_label_form']['U%d' % u] = dict(time_us(lambda: per_label_form(lab, M12, GDIM),
                                                        max(3, args.reps // 4), 1), distinct=n)
    ind = (labs[100] == labs[100].flatten()[0]).float()
    out['linear_pull'] = time_us(lambda: _ops.pull_affine(ind, M12, GDIM), args.reps, args.warmup)
    v = out['vote']['U100']['median_us']
    out['vote_over_pull'] = round(v / out['linear_pull']['median_us'], 2)
    out['per_label_over_vote'] = {k: round(d['median_us'] / out['vote'][k]['median_us'], 1)
                                  for k, d in out['per_label_form'].items()}
    out['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
