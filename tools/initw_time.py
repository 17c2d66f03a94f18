"""Cost of voxel weight maps in init(): each new entry point against the unmasked entry of the same
build, at config 3's observation shape, 256 x 256 x 42.

- unires_noise_hist_g against unires_noise_hist (one observation; a map that is 0 on 3 % of the voxels);
- unires_coreg_hist_m with NULL / NULL, one and two cell supports against unires_coreg_hist (one job, step 1, a small
  rigid between two volumes of the shape);
- unires_pull3d_support against one unires_pull3d_affine of the same geometry (256 x 256 x 126 output grid);
- unires_coreg_quantise_m against unires_coreg_quantise and unires_coreg_cellmask alone (once per level, not per step).

HIP events around each call; the arms of a group are alternated call by call after one warm-up round, `--rounds`
rounds; medians and min - max in microseconds.

    python tools/initw_time.py [--rounds 30] [--out profiles/initw_time.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM = (256, 256, 42)


def alternate(arms, rounds):
    """arms: {name: fn}.  One warm-up round, then ``rounds`` rounds with every arm once per round, in turn."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[k].append(a.elapsed_time(b) * 1e3)
    return {k: {'median_us': statistics.median(v), 'min_us': min(v), 'max_us': max(v)} for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'initw_time.json'))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from unires_amd import _lib, _ops, preproc, stats
    from unires_amd._ops import _stream
    from unires_amd._rigid import _expm, affine_basis
    from tests import coreg_phantom as P
    dev = torch.device('cuda:0')
    vx = (1.0, 1.0, 4.0)
    dat = P.observation(DIM, vx, 0, 1, dev, sub_axis=2, rician=True)[0].contiguous()
    mov = P.observation(DIM, vx, 1, 2, dev, sub_axis=2, rician=True)[0].contiguous()
    gen = torch.Generator().manual_seed(0)
    w = (torch.rand(DIM, generator=gen) > 0.03).float().to(dev).contiguous()
    res = {'shape': DIM, 'device': torch.cuda.get_device_name(0), 'rounds': a.rounds,
           'map': '0 on 3 % of the voxels, independently'}

    res['noise_hist'] = alternate({
        'unires_noise_hist': lambda: stats.noise_hist([dat], [False]),
        'unires_noise_hist_g': lambda: stats.noise_hist([dat], [False], [w])}, a.rounds)

    sup = (w > 0).to(torch.uint8).contiguous()
    res['quantise'] = alternate({
        'unires_coreg_quantise': lambda: preproc.coreg_quantise([dat, mov]),
        'unires_coreg_quantise_m': lambda: preproc.coreg_quantise([dat, mov], [sup, sup]),
        'unires_coreg_cellmask': lambda: preproc.coreg_cellmask(sup)}, a.rounds)

    u8, _, _ = preproc.coreg_quantise([dat, mov])
    cell = preproc.coreg_cellmask(sup)
    R = _expm(np.array([1.5, -2.0, 0.8, 0.02, -0.03, 0.04]), affine_basis()).numpy()
    mat = P.true_mat(DIM, vx)
    M = np.linalg.solve(mat, R @ mat)[:3].astype(np.float32).reshape(-1)
    step = np.ones(3, np.float32)
    lib = _lib.load()
    hist = torch.empty((1, 256, 256), dtype=torch.int64, device=dev)

    def hist_m_null():
        arr = (preproc.JobM * 1)(preproc._job(u8[0], u8[1], M, step, None, None, cls=preproc.JobM))
        _lib.check(lib.unires_coreg_hist_m(1, arr, C.c_void_p(hist.data_ptr()), _stream()))
    res['coreg_hist'] = alternate({
        'unires_coreg_hist': lambda: preproc.coreg_hist([(u8[0], u8[1], M, step)]),
        'unires_coreg_hist_m_null_null': hist_m_null,
        'unires_coreg_hist_m_one_mask': lambda: preproc.coreg_hist([(u8[0], u8[1], M, step, None, cell)]),
        'unires_coreg_hist_m_two_masks': lambda: preproc.coreg_hist([(u8[0], u8[1], M, step, cell, cell)])}, a.rounds)
    ng = [int(np.floor((DIM[d] - 1) / 1.0)) + 1 for d in range(3)]
    res['coreg_hist']['sample_points'] = int(np.prod(ng))
    res['coreg_hist']['kept_fraction_two_masks'] = float(
        preproc.coreg_hist([(u8[0], u8[1], M, step, cell, cell)]).sum().item()
        / preproc.coreg_hist([(u8[0], u8[1], M, step)]).sum().item())

    gdim = (256, 256, 126)
    A = np.linalg.solve(mat, R @ P.true_mat(gdim, (1.0, 1.0, 4.0 / 3.0)))[:3].astype(np.float32).reshape(-1)
    res['pull'] = alternate({
        'unires_pull3d_affine': lambda: _ops.pull_affine(dat, A, gdim),
        'unires_pull3d_support': lambda: _ops.pull_support(w, A, gdim)}, a.rounds)
    res['pull']['grid'] = gdim
    res['pull']['supported_fraction'] = float(_ops.pull_support(w, A, gdim).float().mean())

    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
