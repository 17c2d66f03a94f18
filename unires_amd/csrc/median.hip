// median.hip - the exact lower median of a masked stream of float32 magnitudes |t(v)|, on the device and without a
// read-back: the robust scale of the Huber rule (sett.voxel_scale = 'mad') and of init()'s noise estimate
// (sett.noise_est = 'mad').
//
// The key of a magnitude is the bit pattern of fabsf(t): monotone in the value for non-negative floats (-0 becomes +0,
// +inf sorts above every finite value).  A radix select on it, from the most significant bits down, in three passes of
// 11 + 11 + 10 bits:
//   k_median_absres / k_median_hh  one pass over the stream: a workgroup bins the digit of every eligible key that
//                  shares the prefix chosen so far into a private 2048 x uint32 LDS histogram (hist_add: one LDS atomic
//                  per wave for the lanes that share a bin) and adds its non-zero bins to the pass's global counts with
//                  integer atomics - counts do not depend on the order, so the result has the same bits every run.
//   k_median_scan  one workgroup: the prefix sums of the pass's 2048 counts, the bin that holds the rank looked for,
//                  and the rank that remains inside it - for the next pass to filter on, or, after the last pass, the
//                  median and the count.  The first scan makes the rank from the count: ceil(N / 2).
// No workgroup waits on another: the passes and their scans are separate launches on one stream.
#include <float.h>

#include "api_internal.hpp"
#include "median.hpp"

namespace unires {

namespace {

constexpr int kBits0 = 11, kBits1 = 11, kBits2 = 10;
static_assert(kBits0 + kBits1 + kBits2 == 32 && (1 << kBits0) == kMedianBins && kMedianBins % kBlock == 0, "digits");

__device__ __forceinline__ uint32_t key_of(float t) { return __float_as_uint(fabsf(t)); }

// one key into the workgroup's histogram of pass PASS; prefix: the bits above the pass's digit, as the scans chose them
template <int PASS>
__device__ __forceinline__ void rank_key(uint32_t *h, bool ok, uint32_t key, uint32_t prefix) {
  if (PASS == 0)
    hist_add<1>(h, ok, (int)(key >> (kBits1 + kBits2)));
  else if (PASS == 1)
    hist_add<1>(h, ok && (key >> (kBits1 + kBits2)) == prefix, (int)((key >> kBits2) & ((1u << kBits1) - 1u)));
  else
    hist_add<1>(h, ok && (key >> kBits2) == prefix, (int)(key & ((1u << kBits2) - 1u)));
}

__device__ __forceinline__ void hist_clear(uint32_t *h) {
  for (int b = threadIdx.x; b < kMedianBins; b += kBlock) h[b] = 0;
}

// the workgroup's non-zero bins into the pass's global counts
__device__ __forceinline__ void hist_flush(const uint32_t *h, uint32_t *counts) {
  for (int b = threadIdx.x; b < kMedianBins; b += kBlock) {
    const uint32_t c = h[b];
    if (c) atomicAdd(counts + b, c);
  }
}

// |fl32(x - ay)| of one voxel: k_voxel_huber's residual, missing-data and prior conventions
template <int PASS>
__device__ __forceinline__ void absres_term(uint32_t *h, float xv, float av, float pv, uint32_t prefix) {
  const float a = fabsf(__fsub_rn(xv, av));
  rank_key<PASS>(h, xv != 0.f && a <= FLT_MAX && pv > 0.f, __float_as_uint(a), prefix);
}

// One pass over (x, ay[, prior]): the first n4 groups of 4 voxels by 16-byte loads, the voxels from 4 n4 on one by one
// - the tail of up to 3, or the whole stream where the launcher found a buffer off its boundary and passed n4 = 0.
template <int PASS, bool PRIOR>
__global__ void __launch_bounds__(kBlock) k_median_absres(const float *__restrict__ x, const float *__restrict__ ay,
                                                          const float *__restrict__ prior, size_t n4, size_t n,
                                                          MedianWork *__restrict__ work) {
  __shared__ uint32_t h[kMedianBins];
  const uint32_t prefix = PASS ? work->prefix : 0u;
  if (PASS && work->rank == 0u) return;  // (uniform: nothing eligible)
  hist_clear(h);
  __syncthreads();
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  const auto load = [&](size_t q, float4 &xv, float4 &av, float4 &pv) {
    xv = *reinterpret_cast<const float4 *>(x + 4 * q);
    av = *reinterpret_cast<const float4 *>(ay + 4 * q);
    pv = PRIOR ? *reinterpret_cast<const float4 *>(prior + 4 * q) : make_float4(1.f, 1.f, 1.f, 1.f);
  };
  const auto group = [&](const float4 &xv, const float4 &av, const float4 &pv) {
    absres_term<PASS>(h, xv.x, av.x, pv.x, prefix), absres_term<PASS>(h, xv.y, av.y, pv.y, prefix);
    absres_term<PASS>(h, xv.z, av.z, pv.z, prefix), absres_term<PASS>(h, xv.w, av.w, pv.w, prefix);
  };
  size_t q = tid;
  for (; q + step < n4; q += 2 * step) {  // two groups' loads in flight per lane (the histogram's atomics do not unroll)
    float4 x0, a0, p0, x1, a1, p1;
    load(q, x0, a0, p0), load(q + step, x1, a1, p1);
    group(x0, a0, p0), group(x1, a1, p1);
  }
  if (q < n4) {
    float4 x0, a0, p0;
    load(q, x0, a0, p0);
    group(x0, a0, p0);
  }
  for (size_t e = 4 * n4 + tid; e < n; e += step) absres_term<PASS>(h, x[e], ay[e], PRIOR ? prior[e] : 1.f, prefix);
  __syncthreads();
  hist_flush(h, work->counts[PASS]);
}

// a voxel the noise estimate reads: noise.hip's selection, with 0 excluded on both sides
__device__ __forceinline__ bool hh_voxel(float v, int ct) { return fabsf(v) <= FLT_MAX && v != 0.f && (ct || v > 0.f); }

// One pass over the 2 x 2 cells: a thread per cell, cells in the volume's order (z fastest), so a wave's four loads are
// four runs of consecutive floats; c: the cell counts per axis, sp / sq: the element strides of the cell's two axes.
template <int PASS, bool W>
__global__ void __launch_bounds__(kBlock) k_median_hh(const float *__restrict__ x, const float *__restrict__ w, Dim3i c,
                                                      Dim3i d, size_t sp, size_t sq, int ct, size_t ncell,
                                                      MedianWork *__restrict__ work) {
  __shared__ uint32_t h[kMedianBins];
  const uint32_t prefix = PASS ? work->prefix : 0u;
  if (PASS && work->rank == 0u) return;  // (uniform: no complete cell)
  hist_clear(h);
  __syncthreads();
  const size_t step = (size_t)gridDim.x * kBlock;
  for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < ncell; e += step) {
    const unsigned e32 = (unsigned)e, r = e32 / (unsigned)c.z;  // (ncell <= UINT32_MAX)
    const unsigned k = e32 - r * (unsigned)c.z, i = r / (unsigned)c.y, j = r - i * (unsigned)c.y;
    const size_t o = ((size_t)i * d.y + j) * d.z + k;
    const float va = x[o], vb = x[o + sp], vc = x[o + sq], vd = x[o + sp + sq];
    bool ok = hh_voxel(va, ct) && hh_voxel(vb, ct) && hh_voxel(vc, ct) && hh_voxel(vd, ct);
    if (W) ok = ok && w[o] > 0.f && w[o + sp] > 0.f && w[o + sq] > 0.f && w[o + sp + sq] > 0.f;
    const float t = __fadd_rn(__fsub_rn(__fsub_rn(va, vb), vc), vd);
    rank_key<PASS>(h, ok, key_of(t), prefix);
  }
  __syncthreads();
  hist_flush(h, work->counts[PASS]);
}

// The scan of pass PASS: thread t owns bins [8 t, 8 t + 8); an inclusive scan of the threads' sums through LDS; the one
// thread whose bins hold the rank walks them.  Writes work->prefix / rank (/ n) for the next pass, or out after the last.
template <int PASS>
__global__ void __launch_bounds__(kBlock) k_median_scan(MedianWork *__restrict__ work, double *__restrict__ out) {
  constexpr int kPer = kMedianBins / kBlock;
  __shared__ uint32_t s[kBlock];
  const int t = threadIdx.x;
  const uint32_t prefix = PASS ? work->prefix : 0u, rank_in = PASS ? work->rank : 0u;  // (read before anything is written)
  uint32_t cnt[kPer], local = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) local += cnt[j] = work->counts[PASS][t * kPer + j];
  s[t] = local;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const uint32_t v = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  const uint32_t incl = s[t], excl = incl - local, total = s[kBlock - 1];
  const uint32_t rank = PASS ? rank_in : total / 2u + (total & 1u);  // the lower median: the ceil(N / 2)-th smallest
  if (rank == 0u) {  // (uniform) nothing eligible
    if (t == 0) {
      if (PASS == 0) work->prefix = 0u, work->rank = 0u, work->n = 0u;
      if (PASS == kMedianPasses - 1) out[0] = 0.0, out[1] = 0.0;
    }
    return;
  }
  if (excl < rank && rank <= incl) {
    uint32_t r = rank - excl;
    int bin = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (!found) {
        if (r <= cnt[j])
          found = true, bin = j;
        else
          r -= cnt[j];
      }
    }
    const uint32_t digit = (uint32_t)(t * kPer + bin);
    if (PASS == 0) {
      work->prefix = digit, work->rank = r, work->n = total;
    } else if (PASS == 1) {
      work->prefix = (prefix << kBits1) | digit, work->rank = r;
    } else {
      out[0] = (double)__uint_as_float((prefix << kBits2) | digit);
      out[1] = (double)work->n;
    }
  }
}

// blocks of a pass over `units` loop steps per grid (16-byte groups or single voxels): >= 4 steps per thread
inline unsigned median_blocks(size_t units) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>((units + 4 * kBlock - 1) / (4 * kBlock), 2048));
}

template <int PASS>
void absres_pass(const float *x, const float *ay, const float *prior, size_t n, MedianWork *work, double *out_dev,
                 hipStream_t st) {
  const bool aligned = (((uintptr_t)x | (uintptr_t)ay | (uintptr_t)prior) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  if (n) {
    const dim3 grid(median_blocks(aligned ? n4 + 3 : n));
    if (prior)
      hipLaunchKernelGGL((k_median_absres<PASS, true>), grid, dim3(kBlock), 0, st, x, ay, prior, n4, n, work);
    else
      hipLaunchKernelGGL((k_median_absres<PASS, false>), grid, dim3(kBlock), 0, st, x, ay, prior, n4, n, work);
  }
  hipLaunchKernelGGL(k_median_scan<PASS>, dim3(1), dim3(kBlock), 0, st, work, out_dev);
}

template <int PASS>
void hh_pass(const float *x, Dim3i d, int axis, int ct, const float *w, MedianWork *work, double *out_dev,
             hipStream_t st) {
  const size_t ncell = (size_t)median_hh_cells(d, axis);
  if (ncell) {
    const Dim3i c{d.x - (axis != 0), d.y - (axis != 1), d.z - (axis != 2)};
    const size_t s[3] = {(size_t)d.y * d.z, (size_t)d.z, 1};
    const size_t sp = s[axis == 0 ? 1 : 0], sq = s[axis == 2 ? 1 : 2];
    const dim3 grid(median_blocks(ncell));
    if (w)
      hipLaunchKernelGGL((k_median_hh<PASS, true>), grid, dim3(kBlock), 0, st, x, w, c, d, sp, sq, ct, ncell, work);
    else
      hipLaunchKernelGGL((k_median_hh<PASS, false>), grid, dim3(kBlock), 0, st, x, w, c, d, sp, sq, ct, ncell, work);
  }
  hipLaunchKernelGGL(k_median_scan<PASS>, dim3(1), dim3(kBlock), 0, st, work, out_dev);
}

}  // namespace

void launch_median_absres(const float *x, const float *ay, const float *prior, size_t n, MedianWork *work,
                          double *out_dev, hipStream_t st) {
  absres_pass<0>(x, ay, prior, n, work, out_dev, st);
  absres_pass<1>(x, ay, prior, n, work, out_dev, st);
  absres_pass<2>(x, ay, prior, n, work, out_dev, st);
}

void launch_median_hh(const float *x, Dim3i d, int axis, int ct, const float *w, MedianWork *work, double *out_dev,
                      hipStream_t st) {
  hh_pass<0>(x, d, axis, ct, w, work, out_dev, st);
  hh_pass<1>(x, d, axis, ct, w, work, out_dev, st);
  hh_pass<2>(x, d, axis, ct, w, work, out_dev, st);
}

}  // namespace unires

using namespace unires;

extern "C" int unires_median_absres(const float *x, const float *ay, const float *prior, int64_t n, void *work,
                                    double *out_dev, void *stream) {
  if (!x || !ay || !work || !out_dev) return fail(UNIRES_ERR_ARG, "null x, ay, work or out_dev");
  if (n < 0 || n > (int64_t)UINT32_MAX) return fail(UNIRES_ERR_ARG, "n must be in [0, 2^32 - 1]");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(MedianWork), st));
  launch_median_absres(x, ay, prior, (size_t)n, static_cast<MedianWork *>(work), out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_median_hh(const float *x, const int32_t dim[3], int32_t axis, int32_t ct, const float *w,
                                void *work, double *out_dev, void *stream) {
  if (!x || !dim || !work || !out_dev) return fail(UNIRES_ERR_ARG, "null x, dim, work or out_dev");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "axis: 0, 1 or 2");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (median_hh_cells(mk(dim), axis) > (unsigned long long)UINT32_MAX)
    return fail(UNIRES_ERR_ARG, "more than 2^32 - 1 cells");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(work, 0, sizeof(MedianWork), st));
  launch_median_hh(x, mk(dim), axis, ct != 0, w, static_cast<MedianWork *>(work), out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_voxel_huber_dev(const float *x, const float *ay, const float *prior, const double *scale_dev,
                                      float mult, int64_t n, float *g_out, void *stream) {
  if (!x || !ay || !scale_dev || !g_out) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 0) return fail(UNIRES_ERR_DIM, "bad length");
  if (!(mult > 0.f)) return fail(UNIRES_ERR_ARG, "the multiplier of the scale must be positive");
  launch_voxel_huber_dev(x, ay, prior, scale_dev, mult, (size_t)n, g_out, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}
