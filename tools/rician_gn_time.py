"""What carrying the Rician noise model through the rigid Gauss-Newton update costs.

kernels: unires_rigid_terms_r - without `out` (a line-search evaluation) and with it (the Gauss-Newton evaluation),
without and with a voxel map g, slice weights u and gains e in every arm - against the composition of existing calls it
replaces, in the same process: unires_slice_apply (the gained prediction into a temporary), unires_rician_terms (the
sums of g c(z), and with `out` the effective observation into a second temporary), unires_slice_sums /
unires_voxel_sums on the gained prediction and, with `out`, unires_rigid_resid / unires_rigid_resid_g on the two
temporaries.  `cheapest_ls`: the shortest line-search composition the library had with gains - unires_rician_terms for
the sums of g c(z) alone and unires_rigid_terms_e without `out`, no temporary.  Shapes: tools/gain_gn_time.py's - 256 x 256 x 42 with the 42 slices along each axis in turn, and the
decimated 85 x 85 x 42 the rigid update sees for config 3's observations at samp = 3.  HIP events around 20 calls after
a warm-up round, arms alternated within a round, median with min - max over the rounds.

update: one `_update_rigid` call (one Gauss-Newton step with its line search, samp = 0) on DESIGN 8.6's phantom under
'rician' with sett.rician_gn against the same call under 'gaussian'; wall clock around the call with the device idle
before and after (the update reads its sums back), rigid_q and po.rigid put back after every call, arms alternated.

    python tools/rician_gn_time.py [--rounds 5] [--out profiles/rician_gn_time.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gain_gn_time import SHAPES, stats  # noqa: E402


def measure_kernels(rounds, device, calls=20):
    from unires_amd import _lib
    from unires_amd._lib import check, i3
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    P = lambda t: t.data_ptr()
    rows = []
    for shape, axis in SHAPES:
        S = shape[axis]
        # magnitude data at a few sigma: z = tau x e ay on both sides of the branch of the float32 forms
        x = (torch.rand(shape, generator=gen) * 4).float()
        x[torch.rand(shape, generator=gen) < 0.3] = 0
        x, ay = x.to(device), (torch.rand(shape, generator=gen) * 4).float().to(device)
        g = torch.rand(shape, generator=gen).to(device)
        u = torch.rand(S, generator=gen).to(device)
        e = (0.5 + 1.5 * torch.rand(S, generator=gen)).to(device)
        t = (u.double() * e.double()).float()
        tau = 1.0
        tmp, xt, res = torch.empty_like(ay), torch.empty_like(ay), torch.empty_like(ay)
        sums = torch.empty(3 * S, dtype=torch.float64, device=device)
        st = torch.cuda.current_stream().cuda_stream
        d = i3(shape)

        def fused(gp, out):
            return lambda: check(lib.unires_rigid_terms_r(P(x), P(ay), gp, P(u), P(e), d, axis, tau, P(sums), out, st))

        def composed(with_g, with_out):
            gp = P(g) if with_g else None
            lik = sums.data_ptr() + 16 * S  # (the last S doubles)

            def run():
                check(lib.unires_slice_apply(P(ay), P(tmp), P(e), d, axis, st))
                check(lib.unires_rician_terms(P(x), P(ay), gp, P(e), d, axis, tau, P(xt) if with_out else None, lik, st))
                if with_g:
                    check(lib.unires_voxel_sums(P(x), P(tmp), gp, d, axis, P(sums), st))
                    if with_out:
                        check(lib.unires_rigid_resid_g(P(xt), P(tmp), gp, d, axis, P(t), P(tmp), st))
                else:
                    check(lib.unires_slice_sums(P(x), P(tmp), d, axis, P(sums), st))
                    if with_out:
                        check(lib.unires_rigid_resid(P(xt), P(tmp), d, axis, P(t), P(tmp), st))
            return run

        def cheapest_ls(with_g):
            # with gains the library already has a shorter line-search composition, without a temporary:
            # unires_rician_terms for the sums of g c(z) alone and unires_rigid_terms_e without out for SSE and count
            gp = P(g) if with_g else None
            lik = sums.data_ptr() + 16 * S

            def run():
                check(lib.unires_rician_terms(P(x), P(ay), gp, P(e), d, axis, tau, None, lik, st))
                check(lib.unires_rigid_terms_e(P(x), P(ay), gp, P(u), P(e), d, axis, P(sums), None, st))
            return run

        # (the fused call with `out` writes beside ay here, not over it as _rigid_terms does: repeated calls in place
        # would feed residuals back in as predictions; the traffic - one volume stored - is the same)
        arms = {'fused_ls': fused(None, None), 'composed_ls': composed(False, False),
                'fused_gn': fused(None, P(res)), 'composed_gn': composed(False, True),
                'fused_ls_g': fused(P(g), None), 'composed_ls_g': composed(True, False),
                'fused_gn_g': fused(P(g), P(res)), 'composed_gn_g': composed(True, True),
                'cheapest_ls': cheapest_ls(False), 'cheapest_ls_g': cheapest_ls(True)}
        per = {k: [] for k in arms}
        for r in range(rounds + 1):
            for k, call in arms.items():  # alternated within a round
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(calls):
                    call()
                t1.record()
                torch.cuda.synchronize()
                if r > 0:  # (round 0: warm-up)
                    per[k].append(1e3 * t0.elapsed_time(t1) / calls)
        row = {'shape': list(shape), 'axis': axis, 'unit': 'us per call', 'volume_MB': round(4e-6 * x.numel(), 2),
               **{k: stats(v) for k, v in per.items()}}
        for k in ('ls', 'gn', 'ls_g', 'gn_g'):
            row['fused_over_composed_' + k] = round(row['fused_' + k]['median'] / row['composed_' + k]['median'], 3)
        for k in ('ls', 'ls_g'):
            row['fused_over_cheapest_' + k] = round(row['fused_' + k]['median'] / row['cheapest_' + k]['median'], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def measure_update(rounds, device):
    from tests.helpers import gpu_structs, make_problem
    from unires_amd._rigid import _update_rigid
    prob = make_problem(seed=5, dim_y=(48, 48, 40), thick=3, n_repeats=2, rot=0.0, trans=0.0, noise_sd=5.0,
                        thick_axes=None, shift=(0.0, 0.0, 0.0))
    x, y, sett = gpu_structs(prob, device)
    sett.rician_gn = True
    for xn in x[0]:
        xn.dat = xn.dat.abs().contiguous()
        xn.rigid_q = torch.zeros(6, dtype=torch.float64)
    saved = [(xn.rigid_q.clone(), xn.po.rigid.clone()) for xn in x[0]]
    per = {'gaussian': [], 'rician': []}
    for r in range(rounds + 1):
        for arm in per:  # alternated
            sett.noise_model = arm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _update_rigid(x, y, sett, mean_correct=False, max_niter_gn=1, num_linesearch=4, samp=0)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            for xn, (q, rigid) in zip(x[0], saved):
                xn.rigid_q, xn.po.rigid = q.clone(), rigid.clone()
            if r > 0:  # (round 0: warm-up)
                per[arm].append(ms)
    return {'phantom': 'DESIGN 8.6: 48 x 48 x 40, two repeats with 3 mm slices', 'unit': 'ms per _update_rigid call',
            'rounds': rounds, **{k: stats(v) for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rician_gn_time.json'))
    args = ap.parse_args()
    from unires_amd import _lib
    _lib.load()  # (raises where the library has not been built)
    device = torch.device('cuda:0')
    out = {'what': 'unires_rigid_terms_r (fused) against unires_slice_apply + unires_rician_terms + unires_slice_sums / '
                   'unires_voxel_sums [+ unires_rigid_resid / unires_rigid_resid_g] (composed), u and e in every arm: ls - no '
                   'out, a line-search evaluation; gn - with out; _g - with a voxel map; cheapest_ls - unires_rician_terms (sums only) + '
                   'unires_rigid_terms_e without out, the shortest line-search composition there was; HIP events around 20 calls, '
                   'median, min, max over the rounds after one warm-up round, arms alternated.  update: one '
                   '_update_rigid call, wall clock',
           'device': torch.cuda.get_device_name(0)}
    out['kernels'] = measure_kernels(args.rounds, device)
    out['update'] = measure_update(args.rounds, device)
    print(json.dumps(out['update']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
