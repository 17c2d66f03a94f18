"""Noise / intensity statistics of an image - the counterpart of nitorch's ``estimate_noise`` as the
reference calls it (unires/_core.py:123-125), on the estimator DESIGN 8.1 states: a 1024-bin
histogram of the finite, non-zero voxels, then a float64 EM fit of a two-class Rice mixture (all
values >= 0) or Gaussian mixture (any value < 0).  Both steps are HIP kernels (``noise.hip``): one
launch bins any number of observations, one launch fits all their histograms.

Exact medians of masked float32 magnitudes, on the device and without a read-back (``median.hip``):
``median_absres`` - the robust scale of the Huber rule's residuals - and ``median_hh`` / ``estimate_noise_mad`` - a noise
sd for volumes without an air background, which the mixture cannot give."""
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


MAD_TO_SD = 1.4826  # 1 / Phi^-1(3/4): the median of |t| of a centred Gaussian t, times this, is its sd


def median_work(device):
    """The device scratch of one median call (``UNIRES_MEDIAN_WORK_BYTES``); the entry points clear it themselves, so
    one buffer serves any number of calls on a stream."""
    return torch.empty(_lib.UNIRES_MEDIAN_WORK_BYTES // 4, dtype=torch.int32, device=device)


def _out(out, device):
    """The (2,) float64 device result of a median call: a new tensor, or the caller's, checked."""
    if out is None:
        return torch.empty(2, dtype=torch.float64, device=device)
    if not isinstance(out, torch.Tensor) or out.device != device or out.dtype != torch.float64 or out.numel() != 2 \
            or not out.is_contiguous():
        raise ValueError('unires_amd: out must be a contiguous float64 tensor of 2 elements on the data\'s device')
    return out


def _work(work, device):
    if work is None:
        return median_work(device)
    if not isinstance(work, torch.Tensor) or not work.is_cuda or work.device != device or not work.is_contiguous() \
            or work.numel() * work.element_size() < _lib.UNIRES_MEDIAN_WORK_BYTES:
        raise ValueError('unires_amd: work must be a contiguous device buffer of UNIRES_MEDIAN_WORK_BYTES on the data\'s device')
    return work


@on_device
def median_absres(x, ay, prior=None, work=None, out=None):
    """Exact lower median of |fl32(x - ay)| over the voxels with x != 0, a finite difference and (``prior`` given)
    prior > 0 - the Huber rule's conventions - by a radix select on the device (``unires_median_absres``).
    Returns the (2,) float64 DEVICE tensor (median, N); nothing is read back.  ``work`` (``median_work``) and ``out``
    may be handed in to be reused."""
    fx, fa = _flat(x, 'x'), _flat(ay, 'ay')
    fp = None if prior is None else _flat(prior, 'prior')
    if fa.numel() != fx.numel() or (fp is not None and fp.numel() != fx.numel()):
        raise ValueError('unires_amd: x, ay and prior must have one size')
    out = _out(out, fx.device)
    work = _work(work, fx.device)
    check(_lib.load().unires_median_absres(C.c_void_p(fx.data_ptr()), C.c_void_p(fa.data_ptr()),
                                           None if fp is None else C.c_void_p(fp.data_ptr()), fx.numel(),
                                           C.c_void_p(work.data_ptr()), C.c_void_p(out.data_ptr()), _stream()))
    return out


@on_device
def median_hh(dat, axis, ct=False, weight=None, work=None, out=None):
    """Exact lower median of the magnitude of the Haar diagonal detail ((a - b) - c) + d of every 2 x 2 cell of the
    planes orthogonal to ``axis`` of the (X, Y, Z) float32 device volume ``dat``, over the cells whose four voxels are
    finite, non-zero (``ct`` False: > 0) and (``weight`` given) of weight > 0 (``unires_median_hh``).
    Returns the (2,) float64 DEVICE tensor (median, N); nothing is read back."""
    if not isinstance(dat, torch.Tensor) or dat.dim() != 3:
        raise ValueError('unires_amd: dat must be an (X, Y, Z) tensor')
    if axis not in (0, 1, 2):
        raise ValueError('unires_amd: axis must be 0, 1 or 2')
    fd = _flat(dat)
    fw = None if weight is None else _flat(weight, 'weight')
    if fw is not None and tuple(weight.shape) != tuple(dat.shape):
        raise ValueError('unires_amd: a weight map must have the shape of its volume')
    out = _out(out, fd.device)
    work = _work(work, fd.device)
    check(_lib.load().unires_median_hh(C.c_void_p(fd.data_ptr()), _lib.i3(dat.shape), int(axis), 1 if ct else 0,
                                       None if fw is None else C.c_void_p(fw.data_ptr()), C.c_void_p(work.data_ptr()),
                                       C.c_void_p(out.data_ptr()), _stream()))
    return out


def mad_sd(med):
    """sd of the noise from the median of the Haar detail's magnitude, in float32: fl32(fl32(1.4826 med) 0.5) - the
    detail of i.i.d. noise of variance s^2 has variance 4 s^2.  ``med``: a CPU scalar tensor; returns a float32 one."""
    med = torch.as_tensor(med).detach().cpu().to(torch.float32)
    return (torch.tensor(MAD_TO_SD, dtype=torch.float32) * med) * torch.tensor(0.5, dtype=torch.float32)


def estimate_noise_mad(dat, axis, ct=False, weight=None):
    """Noise sd of ``dat`` without a background class: ``(sd, N)`` with sd = ``mad_sd`` of ``median_hh``'s median (a
    float32 CPU scalar) and N the number of cells ranked.  For background-free inputs (skull-stripped, masked, cropped);
    with an air background the Rayleigh region pulls the estimate down, towards 0.655 sd."""
    r = median_hh(dat, axis, ct, weight).cpu()
    return mad_sd(r[0]), int(r[1])


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
