"""Cost of the exact device medians: ``unires_median_absres`` (with and without a prior) and
``unires_median_hh`` (with and without a weight map) at config 3's observation shape, 256 x 256 x 42, and at 256^3, each
beside the obvious torch form of the same job on the same GPU: ``where`` + count + ``kthvalue``, with the read-back of
the count that ``kthvalue``'s k needs.  The Huber pass with its threshold on the device (``unires_voxel_huber_dev``)
beside the one that takes it as an argument.  Both forms of a median are checked to agree before they are timed.

HIP events around each call; the arms of a group are alternated call by call after one warm-up round, `--rounds`
rounds; medians and min - max in microseconds.

    python tools/median_time.py [--rounds 20] [--out profiles/median_time.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.initw_time import alternate  # noqa: E402

SHAPES = ((256, 256, 42), (256, 256, 256))
INF = float('inf')


def torch_absres(x, ay, prior):
    a = (x - ay).abs()
    ok = (x != 0) & torch.isfinite(a)
    if prior is not None:
        ok &= prior > 0
    n = int(ok.sum())  # (the read-back: kthvalue's k is a host integer)
    if n == 0:
        return 0.0, 0
    return torch.where(ok, a, torch.full_like(a, INF)).reshape(-1).kthvalue((n + 1) // 2).values, n


def torch_hh(x, w):
    a, b, c, d = x[:-1, :-1], x[1:, :-1], x[:-1, 1:], x[1:, 1:]
    t = (((a - b) - c) + d).abs()
    ok = torch.isfinite(x) & (x > 0)
    if w is not None:
        ok &= w > 0
    ok = ok[:-1, :-1] & ok[1:, :-1] & ok[:-1, 1:] & ok[1:, 1:]
    n = int(ok.sum())
    if n == 0:
        return 0.0, 0
    return torch.where(ok, t, torch.full_like(t, INF)).reshape(-1).kthvalue((n + 1) // 2).values, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'median_time.json'))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from unires_amd import _lib, stats
    from unires_amd._ops import _ptr, _stream
    lib = _lib.load()
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds,
           'data': 'x = 400 + 120 randn with 3 % zeros, ay = x + 5 randn, prior / weight map 0 on 3 % of the voxels'}
    for shape in SHAPES:
        gen = torch.Generator().manual_seed(sum(shape))
        x = (400.0 + 120.0 * torch.randn(shape, generator=gen)).float()
        x[torch.rand(shape, generator=gen) < 0.03] = 0.0
        ay = (x + 5.0 * torch.randn(shape, generator=gen)).float()
        w = (torch.rand(shape, generator=gen) > 0.03).float()
        x, ay, w = x.to(dev).contiguous(), ay.to(dev).contiguous(), w.to(dev).contiguous()
        work, out = stats.median_work(dev), torch.zeros(2, dtype=torch.float64, device=dev)
        gout = torch.empty_like(x)
        counts = {}
        for name, prior in (('', None), ('_prior', w)):  # the two forms agree
            got, want = stats.median_absres(x, ay, prior).cpu(), torch_absres(x, ay, prior)
            assert float(got[0]) == float(want[0]) and int(got[1]) == want[1], (shape, got, want)
            counts['absres' + name] = int(got[1])
            got, want = stats.median_hh(x, 2, False, prior).cpu(), torch_hh(x, prior)
            assert float(got[0]) == float(want[0]) and int(got[1]) == want[1], (shape, got, want)
            counts['hh' + name.replace('prior', 'weight')] = int(got[1])
        stats.median_absres(x, ay, w, work=work, out=out)
        c = float(out[0].cpu()) * 3.0 * 1.4826
        mult = 3.0 * 1.4826
        key = 'x'.join(map(str, shape))
        res[key] = {
            'median_absres': alternate({
                'unires_median_absres': lambda: stats.median_absres(x, ay, None, work=work, out=out),
                'unires_median_absres_prior': lambda: stats.median_absres(x, ay, w, work=work, out=out),
                'torch_where_count_kthvalue': lambda: torch_absres(x, ay, None),
                'torch_where_count_kthvalue_prior': lambda: torch_absres(x, ay, w)}, a.rounds),
            'median_hh': alternate({
                'unires_median_hh': lambda: stats.median_hh(x, 2, False, None, work=work, out=out),
                'unires_median_hh_weight': lambda: stats.median_hh(x, 2, False, w, work=work, out=out),
                'torch_where_count_kthvalue': lambda: torch_hh(x, None),
                'torch_where_count_kthvalue_weight': lambda: torch_hh(x, w)}, a.rounds),
            'huber': alternate({
                'unires_voxel_huber': lambda: _lib.check(lib.unires_voxel_huber(
                    _ptr(x), _ptr(ay), _ptr(w), c, x.numel(), _ptr(gout), _stream())),
                'unires_voxel_huber_dev': lambda: _lib.check(lib.unires_voxel_huber_dev(
                    _ptr(x), _ptr(ay), _ptr(w), _ptr(out), mult, x.numel(), _ptr(gout), _stream()))}, a.rounds),
            'voxels': x.numel(), 'eligible': counts}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
