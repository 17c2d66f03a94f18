// noise.hip - noise / intensity hyper-parameters of the observations (the reference's
// _estimate_hyperpar, unires/_core.py:96-142; DESIGN 8.1 states the estimator).
//
//   k_noise_range  masked min / max of every observation of a call: grid-stride loop, wave and
//                  workgroup reductions, one (min, max) partial per workgroup.
//   k_noise_hist   the same workgroups again: each reduces its observation's partials to the range,
//                  bins the selected voxels into a private 1024 x uint32 LDS histogram and merges its
//                  non-zero bins with integer atomics (counts do not depend on order).
//   k_noise_fit    one workgroup per observation: a float64 EM fit of a two-class Rice (all values
//                  >= 0) or Gaussian (CT) mixture to the histogram, 4 bins per lane in registers, one
//                  block reduction of 7 sums per iteration, the convergence test in the kernel.
//   k_noise_range_g / k_noise_hist_g
//                  the first two under per-voxel weight maps: a voxel whose weight is not > 0 is not
//                  read into either.
//
// Selected voxels: finite, non-zero, and >= 0 unless the observation is CT.
#include <float.h>
#include <math.h>

#include "noise.hpp"

// No contraction: the fit restates float64 NumPy arithmetic (tests/noise_restated.py), operation by
// operation, so that the two agree to rounding and their stop rules flip together.
#pragma clang fp contract(off)

namespace unires {

namespace {

constexpr int kHistWaves = kNoiseHistBlock / kWave;
constexpr int kFitWaves = kNoiseFitBlock / kWave;
constexpr int kBinsPerLane = kNoiseBins / kNoiseFitBlock;
constexpr int kSeriesTerms = 64;

struct NoiseBatch {  // one chained group of observations, by value in the kernel arguments
  const float *p[kNoiseMaxObs];
  int64_t n[kNoiseMaxObs];
  int32_t ct[kNoiseMaxObs];
  int32_t blk0[kNoiseMaxObs + 1];  // first workgroup of each observation; blk0[nobs] = grid size
  int32_t nobs;
};

__device__ __forceinline__ bool selected(float v, int ct) {
  return fabsf(v) <= FLT_MAX && v != 0.f && (ct || v >= 0.f);
}

// observation of workgroup `b` (uniform; nobs <= kNoiseMaxObs)
__device__ __forceinline__ int obs_of(const NoiseBatch &B, int b) {
  int o = 0;
  while (o + 1 < B.nobs && b >= B.blk0[o + 1]) ++o;
  return o;
}

// f(v) for every element tid, tid + nthr, ... of p[0, n): 16-byte loads, two in flight per lane,
// when p is 16-byte aligned.
template <class F>
__device__ __forceinline__ void for_each_elem(const float *__restrict__ p, int64_t n, int64_t tid, int64_t nthr, F f) {
  int64_t done = 0;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
    const int64_t n4 = n >> 2;
    int64_t i = tid;
    for (; i + nthr < n4; i += 2 * nthr) {
      const float4 a = p4[i];
      const float4 b = p4[i + nthr];
      f(a.x); f(a.y); f(a.z); f(a.w);
      f(b.x); f(b.y); f(b.z); f(b.w);
    }
    if (i < n4) {
      const float4 a = p4[i];
      f(a.x); f(a.y); f(a.z); f(a.w);
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nthr) f(p[i]);
}

__device__ __forceinline__ void wave_minmax(float &lo, float &hi) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, kWave));
    hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
  }
}

// (lo, hi) of the workgroup, in every thread
__device__ __forceinline__ void block_minmax(float &lo, float &hi, float *s_lo, float *s_hi) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  wave_minmax(lo, hi);
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  lo = s_lo[0];
  hi = s_hi[0];
#pragma unroll
  for (int w = 1; w < kHistWaves; ++w) {
    lo = fminf(lo, s_lo[w]);
    hi = fmaxf(hi, s_hi[w]);
  }
}

__global__ void __launch_bounds__(kNoiseHistBlock) k_noise_range(NoiseBatch B, float *__restrict__ part) {
  __shared__ float s_lo[kHistWaves], s_hi[kHistWaves];
  const int o = obs_of(B, blockIdx.x);
  const int blk = blockIdx.x - B.blk0[o], nb = B.blk0[o + 1] - B.blk0[o];
  const int ct = B.ct[o];
  float lo = INFINITY, hi = -INFINITY;
  for_each_elem(B.p[o], B.n[o], (int64_t)blk * kNoiseHistBlock + threadIdx.x, (int64_t)nb * kNoiseHistBlock,
                [&](float v) {
                  if (selected(v, ct)) {
                    lo = fminf(lo, v);
                    hi = fmaxf(hi, v);
                  }
                });
  block_minmax(lo, hi, s_lo, s_hi);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = lo;
    part[2 * blockIdx.x + 1] = hi;
  }
}

// (one count into the LDS histogram: hist_add, common.hpp)
template <int kAgg>
__global__ void __launch_bounds__(kNoiseHistBlock)
    k_noise_hist(NoiseBatch B, const float *__restrict__ part, uint32_t *__restrict__ counts, float *__restrict__ range) {
  __shared__ uint32_t h[kNoiseBins];
  __shared__ float s_lo[kHistWaves], s_hi[kHistWaves];
  static_assert(kNoiseBins == kNoiseHistBlock, "one bin per thread");
  const int o = obs_of(B, blockIdx.x);
  const int b0 = B.blk0[o], blk = blockIdx.x - b0, nb = B.blk0[o + 1] - b0;
  const int ct = B.ct[o];
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += kNoiseHistBlock) {
    lo = fminf(lo, part[2 * (b0 + i)]);
    hi = fmaxf(hi, part[2 * (b0 + i) + 1]);
  }
  block_minmax(lo, hi, s_lo, s_hi);
  h[threadIdx.x] = 0;
  if (blk == 0 && threadIdx.x == 0) {
    range[2 * o] = lo;
    range[2 * o + 1] = hi;
  }
  if (!(hi > lo)) return;  // nothing selected, or one value: the fit reports it
  __syncthreads();
  const double mn = lo, width = (double)hi - (double)lo;
  // torch.histc's binning: floor((v - mn) * B / (mx - mn)) in float64, one true division; v == mx -> last bin
  for_each_elem(B.p[o], B.n[o], (int64_t)blk * kNoiseHistBlock + threadIdx.x, (int64_t)nb * kNoiseHistBlock,
                [&](float v) {
                  const bool ok = selected(v, ct);
                  int bin = 0;
                  if (ok) bin = min((int)((((double)v - mn) * (double)kNoiseBins) / width), kNoiseBins - 1);
                  hist_add<kAgg>(h, ok, bin);
                });
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(counts + (size_t)o * kNoiseBins + threadIdx.x, c);
}

// ---- the same two passes under per-voxel weight maps ---------------------------------
// A voxel is taken when selected(v, ct) and its weight g(v) > 0: the support of the map, not its size
// (counts stay integers).  An observation without a map (g[o] == nullptr) walks as above.
struct NoiseBatchG {
  NoiseBatch B;
  const float *g[kNoiseMaxObs];
};

// f(v, w) for every element tid, tid + nthr, ... of (p, g)[0, n): 16-byte loads of both, two pairs
// in flight per lane, when p AND g are 16-byte aligned; voxel by voxel otherwise.
template <class F>
__device__ __forceinline__ void for_each_pair(const float *__restrict__ p, const float *__restrict__ g, int64_t n,
                                              int64_t tid, int64_t nthr, F f) {
  int64_t done = 0;
  if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g)) & 15) == 0) {
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    const int64_t n4 = n >> 2;
    int64_t i = tid;
    for (; i + nthr < n4; i += 2 * nthr) {
      const float4 a = p4[i], wa = g4[i];
      const float4 b = p4[i + nthr], wb = g4[i + nthr];
      f(a.x, wa.x); f(a.y, wa.y); f(a.z, wa.z); f(a.w, wa.w);
      f(b.x, wb.x); f(b.y, wb.y); f(b.z, wb.z); f(b.w, wb.w);
    }
    if (i < n4) {
      const float4 a = p4[i], wa = g4[i];
      f(a.x, wa.x); f(a.y, wa.y); f(a.z, wa.z); f(a.w, wa.w);
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nthr) f(p[i], g[i]);
}

// f(v, w) over observation o of the batch; w = 1 where the observation has no map
template <class F>
__device__ __forceinline__ void for_each_weighted(const NoiseBatchG &G, int o, int64_t tid, int64_t nthr, F f) {
  if (G.g[o])
    for_each_pair(G.B.p[o], G.g[o], G.B.n[o], tid, nthr, f);
  else
    for_each_elem(G.B.p[o], G.B.n[o], tid, nthr, [&](float v) { f(v, 1.f); });
}

__global__ void __launch_bounds__(kNoiseHistBlock) k_noise_range_g(NoiseBatchG G, float *__restrict__ part) {
  __shared__ float s_lo[kHistWaves], s_hi[kHistWaves];
  const NoiseBatch &B = G.B;
  const int o = obs_of(B, blockIdx.x);
  const int blk = blockIdx.x - B.blk0[o], nb = B.blk0[o + 1] - B.blk0[o];
  const int ct = B.ct[o];
  float lo = INFINITY, hi = -INFINITY;
  for_each_weighted(G, o, (int64_t)blk * kNoiseHistBlock + threadIdx.x, (int64_t)nb * kNoiseHistBlock,
                    [&](float v, float w) {
                      if (selected(v, ct) && w > 0.f) {
                        lo = fminf(lo, v);
                        hi = fmaxf(hi, v);
                      }
                    });
  block_minmax(lo, hi, s_lo, s_hi);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = lo;
    part[2 * blockIdx.x + 1] = hi;
  }
}

template <int kAgg>
__global__ void __launch_bounds__(kNoiseHistBlock)
    k_noise_hist_g(NoiseBatchG G, const float *__restrict__ part, uint32_t *__restrict__ counts, float *__restrict__ range) {
  __shared__ uint32_t h[kNoiseBins];
  __shared__ float s_lo[kHistWaves], s_hi[kHistWaves];
  const NoiseBatch &B = G.B;
  const int o = obs_of(B, blockIdx.x);
  const int b0 = B.blk0[o], blk = blockIdx.x - b0, nb = B.blk0[o + 1] - b0;
  const int ct = B.ct[o];
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += kNoiseHistBlock) {
    lo = fminf(lo, part[2 * (b0 + i)]);
    hi = fmaxf(hi, part[2 * (b0 + i) + 1]);
  }
  block_minmax(lo, hi, s_lo, s_hi);
  h[threadIdx.x] = 0;
  if (blk == 0 && threadIdx.x == 0) {
    range[2 * o] = lo;
    range[2 * o + 1] = hi;
  }
  if (!(hi > lo)) return;  // nothing usable, or one value: the fit reports it
  __syncthreads();
  const double mn = lo, width = (double)hi - (double)lo;
  for_each_weighted(G, o, (int64_t)blk * kNoiseHistBlock + threadIdx.x, (int64_t)nb * kNoiseHistBlock,
                    [&](float v, float w) {
                      const bool ok = selected(v, ct) && w > 0.f;
                      int bin = 0;
                      if (ok) bin = min((int)((((double)v - mn) * (double)kNoiseBins) / width), kNoiseBins - 1);
                      hist_add<kAgg>(h, ok, bin);
                    });
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(counts + (size_t)o * kNoiseBins + threadIdx.x, c);
}

// ---- float64 special functions --------------------------------------------------------------------
struct SeriesRecip {  // 1 / (k (k + order)), k >= 1
  double r[2][kSeriesTerms + 1];
  constexpr SeriesRecip() : r() {
    for (int k = 1; k <= kSeriesTerms; ++k) {
      r[0][k] = 1.0 / ((double)k * k);
      r[1][k] = 1.0 / ((double)k * (k + 1));
    }
  }
};
__constant__ SeriesRecip kRecip{};

// exp(-x) I_order(x), x >= 0, order 0 or 1: the power series up to x = 25 (positive terms), the
// asymptotic expansion beyond (stopped at its smallest term, ~exp(-2x)).
template <int kOrder>
__device__ double bessel_ie(double x) {
  if (x <= 25.0) {
    const double q = 0.25 * x * x;
    double t = kOrder ? 0.5 * x : 1.0, s = t;
    for (int k = 1; k <= kSeriesTerms; ++k) {
      t = t * q * kRecip.r[kOrder][k];
      s += t;
      if (t < 1e-17 * s) break;
    }
    return s * exp(-x);
  }
  const double mu = 4.0 * kOrder * kOrder, z8 = 8.0 * x;
  double t = 1.0, s = 1.0;
  for (int k = 1; k <= 60; ++k) {
    const double a = 2.0 * k - 1.0;
    const double tn = -t * (mu - a * a) / (k * z8);
    if (fabs(tn) >= fabs(t)) break;
    t = tn;
    s += t;
    if (fabs(t) < 1e-17 * fabs(s)) break;
  }
  return s / sqrt(2.0 * M_PI * x);
}

// Koay & Basser's correction factor xi(theta) of the Rice distribution
__device__ double koay_xi(double th) {
  const double t2 = th * th, z = 0.25 * t2;
  const double b = (2.0 + t2) * bessel_ie<0>(z) + t2 * bessel_ie<1>(z);
  return 2.0 + t2 - (M_PI / 8.0) * b * b;
}

// Rice (nu, sigma) with the given mean and variance (Koay-Basser fixed point, started at theta = r)
__device__ void koay_basser(double mean, double var, double &nu, double &sig) {
  const double r = mean / sqrt(var);
  if (!(r > sqrt(M_PI / (4.0 - M_PI)))) {
    nu = 0.0;
    sig = sqrt((mean * mean + var) / 2.0);
    return;
  }
  double th = r;
  for (int k = 0; k < 256; ++k) {
    const double tn = sqrt(fmax(koay_xi(th) * (1.0 + r * r) - 2.0, 0.0));
    const double d = fabs(tn - th);
    th = tn;
    if (d < 1e-6) break;
  }
  const double xi = koay_xi(th);
  sig = sqrt(var / xi);
  nu = sqrt(fmax(mean * mean + (xi - 2.0) * sig * sig, 0.0));
}

__device__ double rice_mean(double nu, double sig) {
  const double a = nu * nu / (2.0 * sig * sig);
  if (a >= 20.0) return nu;
  const double z = 0.5 * a;
  return sqrt(M_PI * sig * sig / 2.0) * ((1.0 + 2.0 * z) * bessel_ie<0>(z) + 2.0 * z * bessel_ie<1>(z));
}

__device__ __forceinline__ double class_pdf(bool gmm, double x, double loc, double sig) {
  const double s2 = sig * sig, d = x - loc;
  if (gmm) return exp(-(d * d) / (2.0 * s2)) / sqrt(2.0 * M_PI * s2);
  return x / s2 * exp(-(d * d) / (2.0 * s2)) * bessel_ie<0>(x * loc / s2);
}

// sums of kFitWaves waves' partials, in wave order, in every thread; buf alternates between calls
__device__ __forceinline__ void fit_reduce(double v[7], double (*buf)[8], double tot[7]) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, kWave);
    if (lane == 0) buf[wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    double s = buf[0][k];
#pragma unroll
    for (int w = 1; w < kFitWaves; ++w) s += buf[w][k];
    tot[k] = s;
  }
}

__global__ void __launch_bounds__(kNoiseFitBlock)
    k_noise_fit(const uint32_t *__restrict__ counts, const float *__restrict__ range, int max_iter, double *__restrict__ out) {
  __shared__ double s_red[2][kFitWaves][8];
  const int o = blockIdx.x;
  double *res = out + (size_t)o * kNoiseOut;
  const float mnf = range[2 * o], mxf = range[2 * o + 1];
  if (!(mxf > mnf)) {
    if (threadIdx.x < kNoiseOut) res[threadIdx.x] = threadIdx.x == kNoModel ? -1.0 : threadIdx.x == kNoMn ? (double)mnf : threadIdx.x == kNoMx ? (double)mxf : NAN;
    return;
  }
  const bool gmm = mnf < 0.f;
  const double mn = mnf, mx = mxf, step = (mx - mn) / (double)(kNoiseBins - 1);
  double x[kBinsPerLane], h[kBinsPerLane];
#pragma unroll
  for (int j = 0; j < kBinsPerLane; ++j) {
    const int i = threadIdx.x + j * kNoiseFitBlock;
    x[j] = i == kNoiseBins - 1 ? mx : (double)i * step + mn;  // numpy.linspace(mn, mx, B)
    h[j] = (double)counts[(size_t)o * kNoiseBins + i];
  }
  double mg[2] = {0.5, 0.5}, loc[2], sig[2];
  if (gmm) {
    loc[0] = mn + 1.0 * (mx - mn) / 3.0;
    loc[1] = mn + 2.0 * (mx - mn) / 3.0;
    sig[0] = sig[1] = (mx - mn) / 20.0;
  } else {
    loc[0] = 0.0;
    loc[1] = mx / 3.0;
    sig[0] = sig[1] = mx / 20.0;
  }
  double v[7], tot[7];
  v[0] = h[0];
  for (int j = 1; j < kBinsPerLane; ++j) v[0] += h[j];
  for (int k = 1; k < 7; ++k) v[k] = 0.0;
  fit_reduce(v, s_red[1], tot);
  const double sumh = tot[0], tol = 1e-8 * sumh;
  double ll = 0.0, ll_prev = -INFINITY;
  int it = 0;
  while (it < max_iter) {
    // E-step: responsibilities, their moments and the log-likelihood
    for (int k = 0; k < 7; ++k) v[k] = 0.0;
#pragma unroll
    for (int j = 0; j < kBinsPerLane; ++j) {
      if (h[j] > 0.0) {
        const double p0 = mg[0] * class_pdf(gmm, x[j], loc[0], sig[0]) + DBL_EPSILON;
        const double p1 = mg[1] * class_pdf(gmm, x[j], loc[1], sig[1]) + DBL_EPSILON;
        const double s = p0 + p1;
        const double r0 = h[j] * (p0 / s), r1 = h[j] * (p1 / s);
        v[0] += r0;
        v[1] += r0 * x[j];
        v[2] += r0 * x[j] * x[j];
        v[3] += r1;
        v[4] += r1 * x[j];
        v[5] += r1 * x[j] * x[j];
        v[6] += h[j] * log(s);
      }
    }
    fit_reduce(v, s_red[it & 1], tot);
    ll = tot[6];
    if (ll - ll_prev < tol) break;
    // M-step, in every lane from the same sums (no broadcast)
    const double m0s = tot[0] + tot[3];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double m0 = tot[3 * k], m1 = tot[3 * k + 1], m2 = tot[3 * k + 2];
      mg[k] = m0 / m0s;
      const double mean = m1 / m0;
      const double var = (m2 - m1 * m1 / m0 + 1e-6) / (m0 + 1e-6);
      if (gmm) {
        loc[k] = mean;
        sig[k] = sqrt(var);
      } else {
        koay_basser(mean, var, loc[k], sig[k]);
      }
    }
    ll_prev = ll;
    ++it;
  }
  if (threadIdx.x == 0) {
    const double mean[2] = {gmm ? loc[0] : rice_mean(loc[0], sig[0]), gmm ? loc[1] : rice_mean(loc[1], sig[1])};
    const bool bg1 = mean[1] < mean[0];  // the noise class: the smaller mean (class 0 on a tie)
    res[kNoMg0] = mg[0];
    res[kNoMg1] = mg[1];
    res[kNoLoc0] = loc[0];
    res[kNoLoc1] = loc[1];
    res[kNoSig0] = sig[0];
    res[kNoSig1] = sig[1];
    res[kNoMean0] = mean[0];
    res[kNoMean1] = mean[1];
    res[kNoLL] = ll;
    res[kNoIters] = (double)it;
    res[kNoSd] = bg1 ? sig[1] : sig[0];
    res[kNoMu] = bg1 ? fabs(mean[0] - mean[1]) : fabs(mean[1] - mean[0]);
    res[kNoModel] = gmm ? 1.0 : 0.0;
    res[kNoSumH] = sumh;
    res[kNoMn] = mn;
    res[kNoMx] = mx;
  }
}

}  // namespace

int noise_hist_blocks(int64_t n) {
  const int64_t per = (int64_t)kNoiseHistBlock * 32;  // >= 32 voxels per thread
  return (int)std::min<int64_t>(std::max<int64_t>((n + per - 1) / per, 1), 512);
}

void launch_noise_hist(int n, const float *const *ptrs, const int64_t *sizes, const int32_t *ct,
                       float *part, uint32_t *counts, float *range, int hist_form, hipStream_t st) {
  NoiseBatch B{};
  B.nobs = n;
  int nb = 0;
  for (int o = 0; o < n; ++o) {
    B.p[o] = ptrs[o];
    B.n[o] = sizes[o];
    B.ct[o] = ct ? ct[o] : 0;
    B.blk0[o] = nb;
    nb += noise_hist_blocks(sizes[o]);
  }
  B.blk0[n] = nb;
  hipLaunchKernelGGL(k_noise_range, dim3(nb), dim3(kNoiseHistBlock), 0, st, B, part);
  if (hist_form)
    hipLaunchKernelGGL(k_noise_hist<1>, dim3(nb), dim3(kNoiseHistBlock), 0, st, B, (const float *)part, counts, range);
  else
    hipLaunchKernelGGL(k_noise_hist<0>, dim3(nb), dim3(kNoiseHistBlock), 0, st, B, (const float *)part, counts, range);
}

void launch_noise_hist_g(int n, const float *const *ptrs, const int64_t *sizes, const int32_t *ct,
                         const float *const *gptrs, float *part, uint32_t *counts, float *range, int hist_form,
                         hipStream_t st) {
  NoiseBatchG G{};
  NoiseBatch &B = G.B;
  B.nobs = n;
  int nb = 0;
  for (int o = 0; o < n; ++o) {
    B.p[o] = ptrs[o];
    G.g[o] = gptrs ? gptrs[o] : nullptr;
    B.n[o] = sizes[o];
    B.ct[o] = ct ? ct[o] : 0;
    B.blk0[o] = nb;
    nb += noise_hist_blocks(sizes[o]);
  }
  B.blk0[n] = nb;
  hipLaunchKernelGGL(k_noise_range_g, dim3(nb), dim3(kNoiseHistBlock), 0, st, G, part);
  if (hist_form)
    hipLaunchKernelGGL(k_noise_hist_g<1>, dim3(nb), dim3(kNoiseHistBlock), 0, st, G, (const float *)part, counts, range);
  else
    hipLaunchKernelGGL(k_noise_hist_g<0>, dim3(nb), dim3(kNoiseHistBlock), 0, st, G, (const float *)part, counts, range);
}

void launch_noise_fit(int n, const uint32_t *counts, const float *range, int max_iter, double *out,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_noise_fit, dim3(n), dim3(kNoiseFitBlock), 0, st, counts, range, max_iter, out);
}

}  // namespace unires
