"""Timing of the noise / intensity hyper-parameter estimator (noise.hip).

- unires_noise_hist (range pass + histogram pass, one call) at 256^3 and at 256 x 256 x 43, on
  magnitude MRI-like data (an ellipsoid at 1000 on a zero background, complex noise sd 75) and on
  CT-like data (air at exactly -1000, the one-bin pile-up), for both histogram forms
  (UNIRES_NOISE_HIST_FORM 0: plain LDS atomics, 1: wave pre-aggregation), with the fraction of
  8 TB/s the two streaming reads reach;
- unires_noise_fit for a 3 x 1 subject (three 256 x 256 x 43 observations) and its M-step counts;
- the same EM driven from the host with torch ops on the GPU (the reference's form: one small kernel
  per operation, a host read at every convergence test and every Koay-Basser step);
- the float64 NumPy restatement (tests/noise_restated.py) on the same histograms.

HIP events around `--reps` calls after `--warmup`; medians (and minima) in microseconds.

    python tools/noise_time.py [--reps 20] [--warmup 3] [--out profiles/noise_time.json] [--hist-only]

--hist-only: warm-up and timed unires_noise_hist calls at 256^3 only (for a rocprofv3 --kernel-trace
--stats run of its own: that split gives the range and histogram kernels separately).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIG, THICK = (256, 256, 256), (256, 256, 43)
HBM = 8e12


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


def wall_us(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {'median_us': round(statistics.median(ts), 1), 'min_us': round(min(ts), 1), 'n': reps}


def mri(dim, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ax = [torch.linspace(-1, 1, d, device=dev) for d in dim]
    X, Y, Z = torch.meshgrid(*ax, indexing='ij')
    truth = 1000.0 * ((X / 0.7) ** 2 + (Y / 0.6) ** 2 + (Z / 0.8) ** 2 < 1).float()
    re = torch.randn(dim, generator=g, device=dev) * 75.0
    im = torch.randn(dim, generator=g, device=dev) * 75.0
    return torch.sqrt((truth + re) ** 2 + im ** 2)


def ct(dim, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ax = [torch.linspace(-1, 1, d, device=dev) for d in dim]
    X, Y, Z = torch.meshgrid(*ax, indexing='ij')
    body = ((X / 0.7) ** 2 + (Y / 0.6) ** 2 + (Z / 0.8) ** 2 < 1)
    return torch.where(body, 40.0 + torch.randn(dim, generator=g, device=dev) * 20.0, torch.full(dim, -1000.0, device=dev))


def torch_em(counts, mn, mx, max_iter=10000):
    """The EM of DESIGN 8.1 as the reference runs its estimator: torch ops on the device, the stop test
    and the Koay-Basser loop read on the host.  Returns the M-step count."""
    dev = counts.device
    gmm = mn < 0
    h = counts.double()
    x = torch.linspace(mn, mx, 1024, dtype=torch.float64, device=dev)
    sumh = float(h.sum())
    mg = torch.full((2,), 0.5, dtype=torch.float64, device=dev)
    if gmm:
        loc = torch.tensor([mn + (mx - mn) / 3.0, mn + 2.0 * (mx - mn) / 3.0], dtype=torch.float64, device=dev)
        sig = torch.full((2,), (mx - mn) / 20.0, dtype=torch.float64, device=dev)
    else:
        loc = torch.tensor([0.0, mx / 3.0], dtype=torch.float64, device=dev)
        sig = torch.full((2,), mx / 20.0, dtype=torch.float64, device=dev)
    rr = math.sqrt(math.pi / (4 - math.pi))

    def xi(th):
        t2 = th * th
        z = 0.25 * t2
        b = (2 + t2) * torch.special.i0e(z) + t2 * torch.special.i1e(z)
        return 2 + t2 - (math.pi / 8) * b * b

    ll_prev, it = -math.inf, 0
    while it < max_iter:
        s2 = sig[:, None] ** 2
        d = x[None] - loc[:, None]
        if gmm:
            pdf = torch.exp(-(d * d) / (2 * s2)) / torch.sqrt(2 * math.pi * s2)
        else:
            pdf = x[None] / s2 * torch.exp(-(d * d) / (2 * s2)) * torch.special.i0e(x[None] * loc[:, None] / s2)
        p = mg[:, None] * pdf + 2.220446049250313e-16
        s = p.sum(0)
        r = h[None] * (p / s[None])
        ll = float((h * torch.log(s)).sum())
        if ll - ll_prev < 1e-8 * sumh:
            break
        m0, m1, m2 = r.sum(1), (r * x[None]).sum(1), (r * x[None] ** 2).sum(1)
        mg = m0 / m0.sum()
        mean = m1 / m0
        var = (m2 - m1 * m1 / m0 + 1e-6) / (m0 + 1e-6)
        if gmm:
            loc, sig = mean, var.sqrt()
        else:
            nl, sl = [], []
            for k in range(2):
                r_k = mean[k] / var[k].sqrt()
                if not float(r_k) > rr:
                    nl.append(torch.zeros((), dtype=torch.float64, device=dev))
                    sl.append(((mean[k] ** 2 + var[k]) / 2).sqrt())
                    continue
                th = r_k
                for _ in range(256):
                    tn = (xi(th) * (1 + r_k * r_k) - 2).clamp_min(0).sqrt()
                    dd = float((tn - th).abs())
                    th = tn
                    if dd < 1e-6:
                        break
                xv = xi(th)
                sk = (var[k] / xv).sqrt()
                nl.append((mean[k] ** 2 + (xv - 2) * sk * sk).clamp_min(0).sqrt())
                sl.append(sk)
            loc, sig = torch.stack(nl), torch.stack(sl)
        ll_prev = ll
        it += 1
    return it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'noise_time.json'))
    ap.add_argument('--hist-only', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('noise_time.py needs a GPU')
    import __graft_entry__ as g
    g.build()
    from unires_amd import stats as S
    from tests import noise_restated as R
    dev = torch.device('cuda:0')
    if args.hist_only:
        vol = mri(BIG, dev, 1)
        t = time_us(lambda: S.noise_hist([vol], [False]), args.reps, args.warmup)
        print(json.dumps({'hist_256^3': t}))
        return
    out = {'device': torch.cuda.get_device_name(0), 'hist': {}, 'method': 'HIP events, median of %d after %d warm-up' % (args.reps, args.warmup)}
    for name, dim, make, is_ct in (('mri_256^3', BIG, mri, False), ('mri_256x256x43', THICK, mri, False),
                                   ('ct_256^3', BIG, ct, True), ('ct_256x256x43', THICK, ct, True)):
        vol = make(dim, dev, 1)
        nbytes = 2 * 4 * vol.numel()  # two streaming reads of the float32 volume
        row = {}
        for form in (0, 1):
            os.environ['UNIRES_NOISE_HIST_FORM'] = str(form)
            t = time_us(lambda: S.noise_hist([vol], [is_ct]), args.reps, args.warmup)
            t['fraction_of_8TBs'] = round(nbytes / (t['median_us'] * 1e-6) / HBM, 3)
            row['form%d' % form] = t
        os.environ.pop('UNIRES_NOISE_HIST_FORM')
        out['hist'][name] = row
    # EM: a 3 x 1 subject of thick-slice observations
    vols = [mri(THICK, dev, 10 + c) for c in range(3)]
    counts, rng = S.noise_hist(vols, [False] * 3)
    res = S.noise_fit(counts, rng).cpu()
    out['fit_3x1'] = time_us(lambda: S.noise_fit(counts, rng), args.reps, args.warmup)
    out['fit_3x1']['m_steps'] = [int(v) for v in res[:, S.ITERS]]
    out['fit_3x1']['per_m_step_us'] = round(out['fit_3x1']['median_us'] / max(1, max(out['fit_3x1']['m_steps'])), 1)
    rn = rng.cpu().tolist()
    its = []
    out['torch_em_3x1'] = wall_us(lambda: its.append([torch_em(counts[o], rn[o][0], rn[o][1]) for o in range(3)]), 3)
    out['torch_em_3x1']['m_steps'] = its[-1]
    cn = counts.cpu().numpy()
    t0 = time.perf_counter()
    np_its = [R.fit(cn[o], rn[o][0], rn[o][1])['iters'] for o in range(3)]
    out['numpy_3x1'] = {'wall_us': round((time.perf_counter() - t0) * 1e6, 1), 'm_steps': np_its}
    out['torch_em_over_fit'] = round(out['torch_em_3x1']['median_us'] / out['fit_3x1']['median_us'], 1)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
