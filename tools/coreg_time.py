"""Timing of the rigid coregistration (coreg.hip, preproc.affine_align, _core._init_reg).

The demo's shape: a 181 x 217 x 181 (1 mm) phantom anatomy (tests/coreg_phantom.py), three
contrasts, each observation with 4 mm slices along x, y and z in turn, sd 75 noise, the second and
third misaligned by random rigids of +-5 mm / +-0.1 rad.  Reports:

- the wall time of _init_reg (torch.cuda.synchronize() before and after), `--reps` runs after one
  warm-up, with the cost evaluations, Powell lockstep steps and launches per pair, and the RMS
  foreground displacement left;
- HIP-event times of one histogram launch (both pairs) and one cost launch (both histograms) at the
  final transforms, and of one single-pair histogram;
- the same evaluation (trilinear G and F at the jittered points, partial-volume bins) with torch
  ops on the GPU (grid_sample + bincount): the in-house baseline;
- the NumPy restatement (tests/coreg_restated.py) of one evaluation.

    python tools/coreg_time.py [--reps 3] [--out profiles/coreg_time.json] [--kernels-only]

--kernels-only: one _init_reg run and nothing else (for a rocprofv3 --kernel-trace --stats run).
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

DIM = (181, 217, 181)


def subject(dev, seed=3):
    import unires_amd as U
    from tests import coreg_phantom as P
    rng = np.random.default_rng(seed)
    x, truth = [], []
    for c, ax in enumerate((0, 1, 2)):
        v, d = [1.0, 1.0, 1.0], list(DIM)
        v[ax], d[ax] = 4.0, int(round(DIM[ax] / 4.0))
        dat, mat = P.observation(tuple(d), tuple(v), c, 100 + seed + c, dev, sub_axis=ax)
        Pl = np.eye(4) if c == 0 else P.random_rigid(rng)
        x.append([U._input(dat, torch.from_numpy(Pl @ mat))])
        truth.append((mat, tuple(d)))
    return x, truth


class Counter:
    def __init__(self, preproc):
        self.p, self.hist, self.cost, self.jobs = preproc, 0, 0, 0
        self.h0, self.c0 = preproc.coreg_hist, preproc.coreg_cost

    def __enter__(self):
        def hist(jobs):
            self.hist += 1
            self.jobs += len(jobs)
            return self.h0(jobs)

        def cost(*a, **k):
            self.cost += 1
            return self.c0(*a, **k)
        self.p.coreg_hist, self.p.coreg_cost = hist, cost
        return self

    def __exit__(self, *a):
        self.p.coreg_hist, self.p.coreg_cost = self.h0, self.c0


def ev_time_us(fn, reps=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {'median_us': statistics.median(out), 'min_us': min(out)}


def torch_eval(G, F, M, step):
    """One evaluation with torch ops: the jittered grid, grid_sample (trilinear, align_corners) of
    both volumes, partial-volume weights, bincount."""
    from unires_amd import preproc
    dev = G.device
    T = torch.from_numpy(preproc.jitter_table()).to(dev)
    ng = [int(np.floor((G.shape[d] - 1) / float(step[d]))) + 1 for d in range(3)]
    p = torch.arange(ng[0] * ng[1] * ng[2], device=dev)
    i = [p // (ng[1] * ng[2]), (p // ng[2]) % ng[1], p % ng[2]]
    k = (3 * (p % 97)) % 97
    x = torch.stack([(i[d].float() + T[(k + d) % 97]) * float(step[d]) for d in range(3)], -1)
    ok = ((x >= 0) & (x <= torch.tensor(G.shape, device=dev) - 1)).all(-1)
    x = x[ok]
    Mt = torch.as_tensor(M, dtype=torch.float32, device=dev).reshape(3, 4)
    y = x @ Mt[:, :3].T + Mt[:, 3]
    inf = ((y >= 0) & (y <= torch.tensor(F.shape, device=dev) - 1)).all(-1)

    def samp(V, c):
        n = torch.tensor(V.shape, device=dev, dtype=torch.float32) - 1
        g = (c / n * 2 - 1).flip(-1)[None, None, None]
        return torch.nn.functional.grid_sample(V.float()[None, None], g, 'bilinear', 'zeros', align_corners=True).reshape(-1)
    g = torch.round(samp(G, x)).clamp(0, 255).long()
    f = torch.where(inf, samp(F, y).clamp(0, 255), torch.zeros_like(x[:, 0]))  # outside F: f = 0
    fl = f.floor().long()
    whi = torch.round((f - fl) * 65536).long()
    H = torch.bincount(g * 256 + fl, weights=(65536 - whi).double(), minlength=65536)
    hi = fl < 255
    H += torch.bincount(g[hi] * 256 + fl[hi] + 1, weights=whi[hi].double(), minlength=65536)
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coreg_time.json'))
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import unires_amd as U
    from unires_amd import preproc
    from tests import coreg_phantom as P
    from tests import coreg_restated as R
    dev = torch.device('cuda:0')
    x, truth = subject(dev)
    rms_before = [P.rms_mm(x[c][0].mat.cpu().numpy(), truth[c][0], truth[c][1]) for c in range(3)]
    sett = U.settings()
    sett.device = dev
    if a.kernels_only:
        U._init_reg(x, sett)
        torch.cuda.synchronize()
        return
    walls = []
    for r in range(a.reps + 1):
        xr, _ = subject(dev)
        s = U.settings()
        s.device = dev
        with Counter(preproc) as cnt:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            U._init_reg(xr, s)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
        if r:
            walls.append(t)
        x, sett = xr, s
    errs = [P.rms_mm(x[c][0].mat.cpu().numpy(), truth[c][0], truth[c][1]) for c in range(3)]
    # per-launch times at the final transforms
    from unires_amd.spatial import _m12
    u8, _, _ = preproc.coreg_quantise([xc[0].dat for xc in x])
    mats0 = [np.asarray(torch.as_tensor(m).cpu()) for m in [xc[0].mat for xc in x]]
    step = (1.0 / np.array([4.0, 1.0, 1.0])).astype(np.float32)   # fixed: 4 mm along x, samp = 1 mm
    jobs = [(u8[0], u8[i], _m12(np.linalg.solve(mats0[i], mats0[0])), step) for i in (1, 2)]
    H = preproc.coreg_hist(jobs)
    t_hist2 = ev_time_us(lambda: preproc.coreg_hist(jobs))
    t_hist1 = ev_time_us(lambda: preproc.coreg_hist(jobs[:1]))
    t_cost2 = ev_time_us(lambda: preproc.coreg_cost(H))
    t_quant = ev_time_us(lambda: preproc.coreg_quantise([xc[0].dat for xc in x]), reps=10, warmup=2)
    Ht = torch_eval(*jobs[0])
    same = float((Ht.round().long().cpu() == H[0].reshape(-1).cpu()).float().mean())
    t_torch = ev_time_us(lambda: torch_eval(*jobs[0]), reps=10, warmup=2)
    Gn, Fn = u8[0].cpu().numpy(), u8[1].cpu().numpy()
    t0 = time.perf_counter()
    Hn = R.hist(Gn, Fn, jobs[0][2], step)
    cn = R.cost(Hn)
    t_np = time.perf_counter() - t0
    res = {
        'shape': {'truth': DIM, 'observations': [list(xc[0].dim) for xc in x], 'slices_mm': 4,
                  'misalignment': '+-5 mm / +-0.1 rad', 'coreg_params': sett.coreg_params},
        'device': torch.cuda.get_device_name(0),
        'init_reg_wall_s': {'runs': walls, 'median': statistics.median(walls)},
        'rms_before_mm': rms_before,
        'rms_after_mm': errs,
        'per_pair': {'cost_evaluations': cnt.jobs / 2, 'lockstep_steps': cnt.hist,
                     'hist_launches': cnt.hist, 'cost_launches': cnt.cost, 'quantise_calls': 1,
                     'note': 'lockstep: one histogram launch and one cost launch per step serve every pair still searching'},
        'sample_points_per_eval': int(np.prod([int(np.floor((Gn.shape[d] - 1) / float(step[d]))) + 1 for d in range(3)])),
        'hist_launch_2_pairs': t_hist2, 'hist_launch_1_pair': t_hist1, 'cost_launch_2_pairs': t_cost2,
        'quantise_3_obs': t_quant,
        'torch_ops_eval_1_pair_hist_only': dict(t_torch, fraction_of_bins_equal_to_the_kernels=same,
                                                note='grid_sample rounds differently from the kernel: its histogram is close to, not equal to, the kernel\'s'),
        'numpy_restatement_eval_1_pair_s': t_np,
        'numpy_restatement_matches_gpu_hist': bool((Hn == H[0].cpu().numpy().astype(np.uint64)).all()),
        'numpy_cost': cn, 'gpu_cost': float(preproc.coreg_cost(H)[0]),
        'reference_figure': '4.36 s for the alignment of three observations in the reference demo, on an RTX 6000 Ada (other hardware; not measured here)',
    }
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
