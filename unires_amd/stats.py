"""Noise / intensity statistics of an image - the counterpart of nitorch's ``estimate_noise`` as the
reference calls it (unires/_core.py:123-125), on the estimator DESIGN 8.1 states: a 1024-bin
histogram of the finite, non-zero voxels, then a float64 EM fit of a two-class Rice mixture (all
values >= 0) or Gaussian mixture (any value < 0).  Both steps are HIP kernels (``noise.hip``): one
launch bins any number of observations, one launch fits all their histograms."""
import ctypes as C

import torch

from . import _lib
from ._lib import check
from ._ops import _stream, on_device

BINS = 1024  # unires_noise_hist's bin count
MAX_ITER = 10000
# columns of unires_noise_fit's output rows
MG, LOC, SIG, MEAN, LL, ITERS, SD, MU, MODEL, SUMH, MN, MX = (0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 14, 15)
NOUT = 16


def _flat(dat, name='dat'):
    if not isinstance(dat, torch.Tensor) or not dat.is_cuda:
        raise RuntimeError('unires_amd: %s must be a CUDA/HIP tensor (no CPU path)' % name)
    if dat.dtype != torch.float32:
        raise TypeError('unires_amd: %s must be float32' % name)
    if dat.numel() < 1:
        raise ValueError('unires_amd: %s is empty' % name)
    return dat.reshape(-1).contiguous()


@on_device
def noise_hist(dats, cts, weights=None):
    """Masked range and 1024-bin histogram of every volume of ``dats`` in one pass.  Returns
    ``(counts, rng)``: (N, 1024) int32 device (the kernel's uint32 counts; < 2^31 per bin here since
    a volume has < 2^31 voxels) and (N, 2) float32 device (min, max of the voxels taken).
    ``weights``: one float32 device map (of its volume's size) or None per volume; a voxel of a volume
    with a map is taken only where the map is > 0."""
    flats = [_flat(d) for d in dats]
    if any(f.numel() >= 2 ** 31 for f in flats):
        raise ValueError('unires_amd: noise_hist takes volumes of fewer than 2^31 voxels')
    n = len(flats)
    dev = flats[0].device
    counts = torch.empty((n, BINS), dtype=torch.int32, device=dev)
    rng = torch.empty((n, 2), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in flats])
    sizes = (C.c_int64 * n)(*[f.numel() for f in flats])
    ct = (C.c_int32 * n)(*[1 if c else 0 for c in cts])
    if weights is not None and any(w is not None for w in weights):
        if len(weights) != n:
            raise ValueError('unires_amd: noise_hist takes one weight map (or None) per volume')
        gs = [None if w is None else _flat(w, 'weight') for w in weights]
        if any(g is not None and g.numel() != f.numel() for g, f in zip(gs, flats)):
            raise ValueError('unires_amd: a weight map must have the size of its volume')
        gptrs = (C.c_void_p * n)(*[None if g is None else g.data_ptr() for g in gs])
        check(_lib.load().unires_noise_hist_g(n, ptrs, sizes, ct, gptrs, C.c_void_p(counts.data_ptr()),
                                              C.c_void_p(rng.data_ptr()), _stream()))
        return counts, rng
    check(_lib.load().unires_noise_hist(n, ptrs, sizes, ct, C.c_void_p(counts.data_ptr()),
                                        C.c_void_p(rng.data_ptr()), _stream()))
    return counts, rng


@on_device
def noise_fit(counts, rng, max_iter=MAX_ITER):
    """Two-class EM fit of every histogram row in one launch -> (N, 16) float64 device rows
    (columns: the constants above; ``include/unires_hip.h`` unires_noise_fit)."""
    n = counts.shape[0]
    if counts.shape != (n, BINS) or rng.shape != (n, 2):
        raise ValueError('unires_amd: counts must be (N, %d) and rng (N, 2)' % BINS)
    counts, rng = counts.contiguous(), rng.contiguous()
    out = torch.empty((n, NOUT), dtype=torch.float64, device=counts.device)
    check(_lib.load().unires_noise_fit(n, C.c_void_p(counts.data_ptr()), C.c_void_p(rng.data_ptr()),
                                       int(max_iter), C.c_void_p(out.data_ptr()), _stream()))
    return out


def _noise_params(row):
    """(prm_noise, prm_not_noise) of one fit row (CPU float64)."""
    bg = 1 if row[MEAN + 1] < row[MEAN] else 0
    fg = 1 - bg
    f64 = lambda v: torch.tensor(float(v), dtype=torch.float64)  # noqa: E731
    return ({'sd': f64(row[SIG + bg]), 'mean': f64(row[MEAN + bg])},
            {'sd': f64(row[SIG + fg]), 'mean': f64(row[MEAN + fg])})


def estimate_noise(dat, num_class=2, bins=1024, max_iter=10000, weight=None):
    """Noise and not-noise statistics of the finite, non-zero voxels of ``dat`` (a float32 device
    tensor of any shape), nitorch's call shape: returns ``(prm_noise, prm_not_noise)``, dicts with
    ``'sd'`` and ``'mean'`` (float64 CPU scalars) of the class with the smaller and the larger mean.
    Negative values select the Gaussian mixture.  Only two classes and 1024 bins are built.
    ``weight``: a float32 device map of ``dat``'s size; only voxels where it is > 0 are read."""
    if num_class != 2:
        raise NotImplementedError('estimate_noise: only num_class=2 is implemented')
    if bins != BINS:
        raise NotImplementedError('estimate_noise: only bins=%d is implemented' % BINS)
    counts, rng = noise_hist([dat], [True], None if weight is None else [weight])
    row = noise_fit(counts, rng, max_iter)[0].cpu()
    if row[MODEL] < 0:
        raise ValueError('estimate_noise: no finite non-zero voxels, or all of them equal')
    return _noise_params(row)
