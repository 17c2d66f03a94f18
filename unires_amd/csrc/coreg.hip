// coreg.hip - rigid coregistration of observations by normalised mutual information (the reference's
// _init_reg -> nitorch affine_align, unires/_core.py:310-368; DESIGN 8.2 states the estimator).
//
//   k_coreg_qinit / k_coreg_qrange / k_coreg_qhist / k_coreg_qparam / k_coreg_quant
//                  uint8 quantisation of a batch of observations: range of the finite voxels, a
//                  1024-bin histogram, the robust maximum (99.99 % of the finite voxels), the
//                  conversion.  Each pass is one launch for every observation of the batch.
//   k_coreg_hist   partial-volume joint histograms of a batch of (fixed G, moving F, voxel map M)
//                  jobs.  A workgroup owns one half of the G-intensity axis (128 x 256 uint32 = 128
//                  KiB of LDS) and at most kCoregChunk sample points, so no Q16 counter can overflow
//                  before its single flush (integer atomics into uint64 counts: order-free).  Both
//                  halves interpolate G; only the owner of g gathers F, and a point outside F counts
//                  as f = 0 (every point inside G is counted).  The background bin pair
//                  (g = 0, f in {0, 1}) is counted in per-lane registers.
//   k_coreg_qrange_m / k_coreg_qhist_m / k_coreg_cellmask / k_coreg_hist_m
//                  the same under supports: range, histogram and robust maximum over the
//                  usable voxels; a joint histogram that drops every sample point whose interpolation
//                  cell in G, or in F when its image is inside F, holds an unusable voxel - one byte
//                  per image per point, from cell supports built once per level.
//   k_coreg_cost   one workgroup per histogram: float64 smoothing, normalisation, marginals and
//                  entropies with a fixed reduction order, one cost per histogram.
#include <float.h>
#include <math.h>

#include "coreg.hpp"

// No contraction: the histograms are restated operation by operation in float32 NumPy
// (tests/coreg_restated.py) and must agree bit for bit.
#pragma clang fp contract(off)

namespace unires {

namespace {

constexpr int kWaves = kCoregBlock / kWave;
constexpr int kHalf = kCoregBins / 2;  // G-intensity rows a histogram workgroup owns

struct JitterTable {  // T[k] = frac((k + 1) * 0.6180339887498949) in float64, rounded to float32
  float t[kCoregJitter];
  constexpr JitterTable() : t() {
    for (int k = 0; k < kCoregJitter; ++k) {
      const double x = (double)(k + 1) * 0.6180339887498949;
      t[k] = (float)(x - (double)(long long)x);
    }
  }
};
__constant__ JitterTable kJitter{};

// ---- quantisation ------------------------------------------------------------------------------
struct QBatch {  // one chained group of observations, by value in the kernel arguments
  const float *p[kCoregMaxObs];
  uint8_t *u[kCoregMaxObs];
  int64_t n[kCoregMaxObs];
  int32_t blk0[kCoregMaxObs + 1];  // first workgroup of each observation; blk0[nobs] = grid size
  int32_t nobs;
};

__device__ __forceinline__ int qobs_of(const QBatch &B, int b) {
  int o = 0;
  while (o + 1 < B.nobs && b >= B.blk0[o + 1]) ++o;
  return o;
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= FLT_MAX; }

// float -> uint32 with the same order (finite values)
__device__ __forceinline__ uint32_t fkey(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ uint32_t *qkeys(float *params, int o) {
  return reinterpret_cast<uint32_t *>(params + (size_t)o * kCoregQOut + kCqKeyLo);
}

__global__ void __launch_bounds__(kCoregQBlock) k_coreg_qinit(uint32_t *__restrict__ counts, float *__restrict__ params) {
  const int o = blockIdx.x;
  counts[(size_t)o * kCoregQBins + threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    uint32_t *k = qkeys(params, o);
    k[0] = 0xffffffffu;  // min key
    k[1] = 0u;           // max key
  }
}

__global__ void __launch_bounds__(kCoregQBlock) k_coreg_qrange(QBatch B, float *__restrict__ params) {
  __shared__ float s_lo[kCoregQBlock / kWave], s_hi[kCoregQBlock / kWave];
  const int o = qobs_of(B, blockIdx.x);
  const int blk = blockIdx.x - B.blk0[o], nb = B.blk0[o + 1] - B.blk0[o];
  float lo = INFINITY, hi = -INFINITY;
  const float *p = B.p[o];
  for (int64_t i = (int64_t)blk * kCoregQBlock + threadIdx.x; i < B.n[o]; i += (int64_t)nb * kCoregQBlock) {
    const float v = p[i];
    if (finite(v)) {
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, kWave));
    hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kCoregQBlock / kWave; ++w) {
      lo = fminf(lo, s_lo[w]);
      hi = fmaxf(hi, s_hi[w]);
    }
    if (lo <= hi) {  // this workgroup saw a finite voxel
      uint32_t *k = qkeys(params, o);
      atomicMin(k, fkey(lo));
      atomicMax(k + 1, fkey(hi));
    }
  }
}

__global__ void __launch_bounds__(kCoregQBlock)
    k_coreg_qhist(QBatch B, const float *__restrict__ params, uint32_t *__restrict__ counts) {
  __shared__ uint32_t h[kCoregQBins];
  static_assert(kCoregQBins == kCoregQBlock, "one bin per thread");
  const int o = qobs_of(B, blockIdx.x);
  const int blk = blockIdx.x - B.blk0[o], nb = B.blk0[o + 1] - B.blk0[o];
  const uint32_t *k = reinterpret_cast<const uint32_t *>(params + (size_t)o * kCoregQOut + kCqKeyLo);
  const uint32_t klo = k[0], khi = k[1];
  if (klo == 0xffffffffu) return;  // no finite voxel
  const float lo = funkey(klo), hi = funkey(khi);
  if (!(hi > lo)) return;
  h[threadIdx.x] = 0;
  __syncthreads();
  const double mn = lo, width = (double)hi - (double)lo;
  const float *p = B.p[o];
  for (int64_t i = (int64_t)blk * kCoregQBlock + threadIdx.x; i < B.n[o]; i += (int64_t)nb * kCoregQBlock) {
    const float v = p[i];
    const bool ok = finite(v);
    int bin = 0;
    if (ok) bin = min((int)((((double)v - mn) * (double)kCoregQBins) / width), kCoregQBins - 1);
    if (ok) {  // lanes that share the first active lane's bin add once (background pile-ups)
      const int b0 = __builtin_amdgcn_readfirstlane(bin);
      const uint64_t same = __ballot(bin == b0);
      if (bin == b0) {
        if ((int)__lane_id() == __ffsll((unsigned long long)same) - 1) atomicAdd(h + b0, (uint32_t)__popcll(same));
      } else {
        atomicAdd(h + bin, 1u);
      }
    }
  }
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(counts + (size_t)o * kCoregQBins + threadIdx.x, c);
}

// one workgroup per observation: inclusive scan of the 1024 counts, the first bin whose cumulative
// count reaches 99.99 % of the finite voxels, its upper edge as the robust maximum
__global__ void __launch_bounds__(kCoregQBins)
    k_coreg_qparam(const uint32_t *__restrict__ counts, float *__restrict__ params) {
  __shared__ uint64_t s_cum[kCoregQBins];
  const int o = blockIdx.x, t = threadIdx.x;
  float *prm = params + (size_t)o * kCoregQOut;
  const uint32_t *k = reinterpret_cast<const uint32_t *>(prm + kCqKeyLo);
  const uint32_t klo = k[0], khi = k[1];
  const float lo = funkey(klo), hi = funkey(khi);
  const bool none = klo == 0xffffffffu, flat = !none && !(hi > lo);
  __syncthreads();  // every lane has read the keys before lane 0 overwrites their neighbours
  if (t == 0) {
    prm[kCqMn] = none ? NAN : lo;
    prm[kCqMax] = none ? NAN : hi;
    if (none || flat) {
      prm[kCqMx] = none ? NAN : hi;
      prm[kCqScale] = 0.f;
      prm[kCqStatus] = none ? 1.f : 2.f;
    }
  }
  if (none || flat) return;
  s_cum[t] = counts[(size_t)o * kCoregQBins + t];
  __syncthreads();
  for (int off = 1; off < kCoregQBins; off <<= 1) {
    const uint64_t add = t >= off ? s_cum[t - off] : 0;
    __syncthreads();
    s_cum[t] += add;
    __syncthreads();
  }
  const uint64_t need = s_cum[kCoregQBins - 1] * 9999u;
  const bool reach = s_cum[t] * 10000u >= need;
  const bool before = t > 0 && s_cum[t - 1] * 10000u >= need;
  if (reach && !before) {
    const float mx = (float)((double)lo + ((double)hi - (double)lo) * (double)(t + 1) / (double)kCoregQBins);
    prm[kCqMx] = mx;
    if (mx > lo) {
      prm[kCqScale] = 255.f / (mx - lo);
      prm[kCqStatus] = 0.f;
    } else {
      prm[kCqScale] = 0.f;
      prm[kCqStatus] = 2.f;
    }
  }
}

__global__ void __launch_bounds__(kCoregQBlock) k_coreg_quant(QBatch B, const float *__restrict__ params) {
  const int o = qobs_of(B, blockIdx.x);
  const int blk = blockIdx.x - B.blk0[o], nb = B.blk0[o + 1] - B.blk0[o];
  const float *prm = params + (size_t)o * kCoregQOut;
  const bool ok = prm[kCqStatus] == 0.f;
  const float mn = prm[kCqMn], scale = prm[kCqScale];
  const float *p = B.p[o];
  uint8_t *u = B.u[o];
  for (int64_t i = (int64_t)blk * kCoregQBlock + threadIdx.x; i < B.n[o]; i += (int64_t)nb * kCoregQBlock) {
    const float v = p[i];
    float q = 0.f;
    if (ok && finite(v)) q = fminf(fmaxf(rintf((v - mn) * scale), 0.f), 255.f);
    u[i] = (uint8_t)q;
  }
}

// ---- quantisation under supports ---------------------------------------------------
// The range and the robust-maximum histogram read the finite voxels whose support byte is non-zero;
// k_coreg_qinit, k_coreg_qparam and k_coreg_quant run as above (every finite voxel is converted).
struct QBatchM {
  QBatch B;
  const uint8_t *m[kCoregMaxObs];  // null: every voxel is usable
};

__global__ void __launch_bounds__(kCoregQBlock) k_coreg_qrange_m(QBatchM Q, float *__restrict__ params) {
  __shared__ float s_lo[kCoregQBlock / kWave], s_hi[kCoregQBlock / kWave];
  const QBatch &B = Q.B;
  const int o = qobs_of(B, blockIdx.x);
  const int blk = blockIdx.x - B.blk0[o], nb = B.blk0[o + 1] - B.blk0[o];
  float lo = INFINITY, hi = -INFINITY;
  const float *p = B.p[o];
  const uint8_t *m = Q.m[o];
  for (int64_t i = (int64_t)blk * kCoregQBlock + threadIdx.x; i < B.n[o]; i += (int64_t)nb * kCoregQBlock) {
    const float v = p[i];
    if (finite(v) && (!m || m[i])) {
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, kWave));
    hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kCoregQBlock / kWave; ++w) {
      lo = fminf(lo, s_lo[w]);
      hi = fmaxf(hi, s_hi[w]);
    }
    if (lo <= hi) {  // this workgroup saw a finite usable voxel
      uint32_t *k = qkeys(params, o);
      atomicMin(k, fkey(lo));
      atomicMax(k + 1, fkey(hi));
    }
  }
}

__global__ void __launch_bounds__(kCoregQBlock)
    k_coreg_qhist_m(QBatchM Q, const float *__restrict__ params, uint32_t *__restrict__ counts) {
  __shared__ uint32_t h[kCoregQBins];
  const QBatch &B = Q.B;
  const int o = qobs_of(B, blockIdx.x);
  const int blk = blockIdx.x - B.blk0[o], nb = B.blk0[o + 1] - B.blk0[o];
  const uint32_t *k = reinterpret_cast<const uint32_t *>(params + (size_t)o * kCoregQOut + kCqKeyLo);
  const uint32_t klo = k[0], khi = k[1];
  if (klo == 0xffffffffu) return;  // no finite usable voxel
  const float lo = funkey(klo), hi = funkey(khi);
  if (!(hi > lo)) return;
  h[threadIdx.x] = 0;
  __syncthreads();
  const double mn = lo, width = (double)hi - (double)lo;
  const float *p = B.p[o];
  const uint8_t *m = Q.m[o];
  for (int64_t i = (int64_t)blk * kCoregQBlock + threadIdx.x; i < B.n[o]; i += (int64_t)nb * kCoregQBlock) {
    const float v = p[i];
    const bool ok = finite(v) && (!m || m[i]);
    int bin = 0;
    if (ok) bin = min((int)((((double)v - mn) * (double)kCoregQBins) / width), kCoregQBins - 1);
    if (ok) {  // lanes that share the first active lane's bin add once (background pile-ups)
      const int b0 = __builtin_amdgcn_readfirstlane(bin);
      const uint64_t same = __ballot(bin == b0);
      if (bin == b0) {
        if ((int)__lane_id() == __ffsll((unsigned long long)same) - 1) atomicAdd(h + b0, (uint32_t)__popcll(same));
      } else {
        atomicAdd(h + bin, 1u);
      }
    }
  }
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(counts + (size_t)o * kCoregQBins + threadIdx.x, c);
}

// cell[i0, i1, i2] = 1 iff the eight voxels (i0..i0+1, i1..i1+1, i2..i2+1) of mask are all non-zero, for
// i_d <= dim_d - 2; the last plane of every axis has no cell and is written 0.  One thread per voxel.
__global__ void __launch_bounds__(256)
    k_coreg_cellmask(const uint8_t *__restrict__ mask, int32_t d0, int32_t d1, int32_t d2, uint8_t *__restrict__ cell) {
  const size_t n = (size_t)d0 * d1 * d2;
  const size_t s1 = (size_t)d2, s0 = (size_t)d1 * d2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int32_t i2 = (int32_t)(i % s1), i1 = (int32_t)((i / s1) % (size_t)d1), i0 = (int32_t)(i / s0);
    uint8_t c = 0;
    if (i0 + 1 < d0 && i1 + 1 < d1 && i2 + 1 < d2) {
      const uint8_t *p = mask + i;
      c = (p[0] && p[1] && p[s1] && p[s1 + 1] && p[s0] && p[s0 + 1] && p[s0 + s1] && p[s0 + s1 + 1]) ? 1 : 0;
    }
    cell[i] = c;
  }
}

// ---- joint histograms --------------------------------------------------------------------------
struct HJob {
  const uint8_t *G;
  const uint8_t *F;
  int32_t dg[3], df[3], ng[3];
  float M[12];
  float s[3];
  int32_t npts;
};

struct HBatch {
  HJob j[kCoregMaxJobs];
  int32_t blk0[kCoregMaxJobs + 1];  // first workgroup of each job (two per chunk); blk0[njobs] = grid size
  int32_t njobs;
};

// Trilinear interpolation of a uint8 volume at x (0 <= x_d <= dim_d - 1, dim_d >= 2): corners from
// i_d = min(floor(x_d), dim_d - 2), weights f_d = x_d - i_d and 1 - f_d, then lerps along axis 0,
// axis 1, axis 2 in that order, each as a * (1 - f) + b * f.
__device__ __forceinline__ float tri_u8(const uint8_t *__restrict__ v, const int32_t *d, float x0, float x1, float x2) {
  const int i0 = min((int)floorf(x0), d[0] - 2), i1 = min((int)floorf(x1), d[1] - 2), i2 = min((int)floorf(x2), d[2] - 2);
  const float f0 = x0 - (float)i0, f1 = x1 - (float)i1, f2 = x2 - (float)i2;
  const float a0 = 1.f - f0, a1 = 1.f - f1, a2 = 1.f - f2;
  const int64_t s1 = d[2], s0 = (int64_t)d[1] * d[2];
  const uint8_t *p = v + (int64_t)i0 * s0 + (int64_t)i1 * s1 + i2;
  const float v000 = p[0], v001 = p[1], v010 = p[s1], v011 = p[s1 + 1];
  const float v100 = p[s0], v101 = p[s0 + 1], v110 = p[s0 + s1], v111 = p[s0 + s1 + 1];
  const float c00 = v000 * a0 + v100 * f0, c01 = v001 * a0 + v101 * f0;
  const float c10 = v010 * a0 + v110 * f0, c11 = v011 * a0 + v111 * f0;
  const float e0 = c00 * a1 + c10 * f1, e1 = c01 * a1 + c11 * f1;
  return e0 * a2 + e1 * f2;
}

__device__ __forceinline__ bool inside(float x, int32_t dim) { return x >= 0.f && x <= (float)(dim - 1); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__global__ void __launch_bounds__(kCoregBlock) k_coreg_hist(HBatch B, uint64_t *__restrict__ hist) {
  __shared__ uint32_t h[kHalf * kCoregBins];
  __shared__ float s_jit[kCoregJitter];
  int o = 0;
  while (o + 1 < B.njobs && (int)blockIdx.x >= B.blk0[o + 1]) ++o;
  const HJob &J = B.j[o];
  const int local = blockIdx.x - B.blk0[o], half = local & 1, chunk = local >> 1;
  const int g_lo = half * kHalf;
  for (int i = threadIdx.x; i < kHalf * kCoregBins; i += kCoregBlock) h[i] = 0;
  if (threadIdx.x < kCoregJitter) s_jit[threadIdx.x] = kJitter.t[threadIdx.x];
  __syncthreads();
  const int p0 = chunk * kCoregChunk, p1 = min(J.npts, p0 + kCoregChunk);
  const uint32_t ng1 = J.ng[1], ng2 = J.ng[2];
  uint32_t r00 = 0, r01 = 0;  // background pair (g = 0, f = 0 | 1), half 0 only
  for (int64_t p = p0 + (int64_t)threadIdx.x; p < p1; p += kCoregBlock) {
    const uint32_t up = (uint32_t)p;
    const uint32_t i2 = up % ng2, t = up / ng2, i1 = t % ng1, i0 = t / ng1;
    const int k0 = (int)((3u * (up % (uint32_t)kCoregJitter)) % (uint32_t)kCoregJitter);
    const int k1 = k0 + 1 == kCoregJitter ? 0 : k0 + 1, k2 = k1 + 1 == kCoregJitter ? 0 : k1 + 1;
    const float x0 = ((float)i0 + s_jit[k0]) * J.s[0];
    const float x1 = ((float)i1 + s_jit[k1]) * J.s[1];
    const float x2 = ((float)i2 + s_jit[k2]) * J.s[2];
    if (!(inside(x0, J.dg[0]) && inside(x1, J.dg[1]) && inside(x2, J.dg[2]))) continue;
    const float y0 = ((J.M[0] * x0 + J.M[1] * x1) + J.M[2] * x2) + J.M[3];
    const float y1 = ((J.M[4] * x0 + J.M[5] * x1) + J.M[6] * x2) + J.M[7];
    const float y2 = ((J.M[8] * x0 + J.M[9] * x1) + J.M[10] * x2) + J.M[11];
    const bool in_f = inside(y0, J.df[0]) && inside(y1, J.df[1]) && inside(y2, J.df[2]);
    const int g = min((int)rintf(tri_u8(J.G, J.dg, x0, x1, x2)), kCoregBins - 1);
    if (g < g_lo || g >= g_lo + kHalf) continue;
    const float f = in_f ? fminf(tri_u8(J.F, J.df, y0, y1, y2), 255.f) : 0.f;
    const int fl = (int)floorf(f);
    const uint32_t whi = (uint32_t)rintf((f - (float)fl) * 65536.f), wlo = 65536u - whi;
    if (g == 0 && fl == 0) {
      r00 += wlo;
      r01 += whi;
      continue;
    }
    uint32_t *row = h + (g - g_lo) * kCoregBins;
    if (wlo) atomicAdd(row + fl, wlo);
    if (fl < kCoregBins - 1 && whi) atomicAdd(row + fl + 1, whi);
  }
  if (half == 0) {  // at most kCoregChunk points x 65536 < 2^32 per workgroup
    r00 = wave_sum_u32(r00);
    r01 = wave_sum_u32(r01);
    if ((threadIdx.x & (kWave - 1)) == 0) {
      if (r00) atomicAdd(h, r00);
      if (r01) atomicAdd(h + 1, r01);
    }
  }
  __syncthreads();
  unsigned long long *out = reinterpret_cast<unsigned long long *>(hist) + (size_t)o * kCoregBins * kCoregBins +
                            (size_t)g_lo * kCoregBins;
  for (int i = threadIdx.x; i < kHalf * kCoregBins; i += kCoregBlock) {
    const uint32_t c = h[i];
    if (c) atomicAdd(out + i, (unsigned long long)c);
  }
}

// ---- joint histograms under cell supports -------------------------------------------
struct HJobM {
  HJob j;
  const uint8_t *mG;  // cell supports (k_coreg_cellmask) of G's / F's shape; null: every cell is usable
  const uint8_t *mF;
};

struct HBatchM {
  HJobM j[kCoregMaxJobs];
  int32_t blk0[kCoregMaxJobs + 1];
  int32_t njobs;
};

// the support byte of the cell tri_u8 reads at x: i_d = min(floor(x_d), dim_d - 2)
__device__ __forceinline__ bool cell_ok(const uint8_t *__restrict__ m, const int32_t *d, float x0, float x1, float x2) {
  const int i0 = min((int)floorf(x0), d[0] - 2), i1 = min((int)floorf(x1), d[1] - 2), i2 = min((int)floorf(x2), d[2] - 2);
  return m[((int64_t)i0 * d[1] + i1) * d[2] + i2] != 0;
}

// k_coreg_hist with the drop rule: a sample point whose G cell is not supported adds nothing (decided
// before the ownership test, so both halves drop the same points); neither does a point whose image
// lies inside F in an unsupported F cell.  A point whose image is outside F counts with f = 0.
__global__ void __launch_bounds__(kCoregBlock) k_coreg_hist_m(HBatchM B, uint64_t *__restrict__ hist) {
  __shared__ uint32_t h[kHalf * kCoregBins];
  __shared__ float s_jit[kCoregJitter];
  int o = 0;
  while (o + 1 < B.njobs && (int)blockIdx.x >= B.blk0[o + 1]) ++o;
  const HJob &J = B.j[o].j;
  const uint8_t *mG = B.j[o].mG, *mF = B.j[o].mF;
  const int local = blockIdx.x - B.blk0[o], half = local & 1, chunk = local >> 1;
  const int g_lo = half * kHalf;
  for (int i = threadIdx.x; i < kHalf * kCoregBins; i += kCoregBlock) h[i] = 0;
  if (threadIdx.x < kCoregJitter) s_jit[threadIdx.x] = kJitter.t[threadIdx.x];
  __syncthreads();
  const int p0 = chunk * kCoregChunk, p1 = min(J.npts, p0 + kCoregChunk);
  const uint32_t ng1 = J.ng[1], ng2 = J.ng[2];
  uint32_t r00 = 0, r01 = 0;  // background pair (g = 0, f = 0 | 1), half 0 only
  for (int64_t p = p0 + (int64_t)threadIdx.x; p < p1; p += kCoregBlock) {
    const uint32_t up = (uint32_t)p;
    const uint32_t i2 = up % ng2, t = up / ng2, i1 = t % ng1, i0 = t / ng1;
    const int k0 = (int)((3u * (up % (uint32_t)kCoregJitter)) % (uint32_t)kCoregJitter);
    const int k1 = k0 + 1 == kCoregJitter ? 0 : k0 + 1, k2 = k1 + 1 == kCoregJitter ? 0 : k1 + 1;
    const float x0 = ((float)i0 + s_jit[k0]) * J.s[0];
    const float x1 = ((float)i1 + s_jit[k1]) * J.s[1];
    const float x2 = ((float)i2 + s_jit[k2]) * J.s[2];
    if (!(inside(x0, J.dg[0]) && inside(x1, J.dg[1]) && inside(x2, J.dg[2]))) continue;
    if (mG && !cell_ok(mG, J.dg, x0, x1, x2)) continue;
    const float y0 = ((J.M[0] * x0 + J.M[1] * x1) + J.M[2] * x2) + J.M[3];
    const float y1 = ((J.M[4] * x0 + J.M[5] * x1) + J.M[6] * x2) + J.M[7];
    const float y2 = ((J.M[8] * x0 + J.M[9] * x1) + J.M[10] * x2) + J.M[11];
    const bool in_f = inside(y0, J.df[0]) && inside(y1, J.df[1]) && inside(y2, J.df[2]);
    const int g = min((int)rintf(tri_u8(J.G, J.dg, x0, x1, x2)), kCoregBins - 1);
    if (g < g_lo || g >= g_lo + kHalf) continue;
    if (in_f && mF && !cell_ok(mF, J.df, y0, y1, y2)) continue;
    const float f = in_f ? fminf(tri_u8(J.F, J.df, y0, y1, y2), 255.f) : 0.f;
    const int fl = (int)floorf(f);
    const uint32_t whi = (uint32_t)rintf((f - (float)fl) * 65536.f), wlo = 65536u - whi;
    if (g == 0 && fl == 0) {
      r00 += wlo;
      r01 += whi;
      continue;
    }
    uint32_t *row = h + (g - g_lo) * kCoregBins;
    if (wlo) atomicAdd(row + fl, wlo);
    if (fl < kCoregBins - 1 && whi) atomicAdd(row + fl + 1, whi);
  }
  if (half == 0) {  // at most kCoregChunk points x 65536 < 2^32 per workgroup
    r00 = wave_sum_u32(r00);
    r01 = wave_sum_u32(r01);
    if ((threadIdx.x & (kWave - 1)) == 0) {
      if (r00) atomicAdd(h, r00);
      if (r01) atomicAdd(h + 1, r01);
    }
  }
  __syncthreads();
  unsigned long long *out = reinterpret_cast<unsigned long long *>(hist) + (size_t)o * kCoregBins * kCoregBins +
                            (size_t)g_lo * kCoregBins;
  for (int i = threadIdx.x; i < kHalf * kCoregBins; i += kCoregBlock) {
    const uint32_t c = h[i];
    if (c) atomicAdd(out + i, (unsigned long long)c);
  }
}

// ---- costs -------------------------------------------------------------------------------------
struct CostArgs {
  double taps[2 * kCoregMaxTapRadius + 1];
  int32_t radius;
  int32_t cost_fun;  // 0 nmi, 1 mi, 2 ecc
};

// sum of one value per thread, pairwise in a fixed tree, in every thread
__device__ double block_sum(double v, double *buf) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  for (int s = kCoregBlock / 2; s > 0; s >>= 1) {
    if (t < s) buf[t] += buf[t + s];
    __syncthreads();
  }
  return buf[0];
}

__global__ void __launch_bounds__(kCoregBlock)
    k_coreg_cost(const uint64_t *__restrict__ hist, CostArgs A, double *__restrict__ work, double *__restrict__ cost) {
  constexpr int kRows = kCoregBlock / kCoregBins;  // 4 rows per pass of the first smoothing
  constexpr int kSpan = kCoregBins / kRows;        // rows per thread in the second
  __shared__ double s_row[kRows][kCoregBins];
  __shared__ double s_buf[kCoregBlock];
  __shared__ double s_s1[kCoregBins], s_s2[kCoregBins];
  const int o = blockIdx.x, t = threadIdx.x, r = t / kCoregBins, c = t % kCoregBins;
  const int R = A.radius;
  const uint64_t *H = hist + (size_t)o * kCoregBins * kCoregBins;
  double *W1 = work + (size_t)o * 2 * kCoregBins * kCoregBins, *W2 = W1 + kCoregBins * kCoregBins;
  // 1: smooth along f (the moving image's axis), zero padding, 'same' size
  for (int g0 = 0; g0 < kCoregBins; g0 += kRows) {
    s_row[r][c] = (double)H[(g0 + r) * kCoregBins + c] * (1.0 / 65536.0);
    __syncthreads();
    double acc = 0.0;
    for (int k = -R; k <= R; ++k) {
      const int j = c + k;
      if (j >= 0 && j < kCoregBins) acc += A.taps[k + R] * s_row[r][j];
    }
    W1[(g0 + r) * kCoregBins + c] = acc;
    __syncthreads();
  }
  // 2: smooth along g (the fixed image's axis), add DBL_EPSILON; column sums
  double col = 0.0;
  for (int g = r * kSpan; g < (r + 1) * kSpan; ++g) {
    double acc = 0.0;
    for (int k = -R; k <= R; ++k) {
      const int j = g + k;
      if (j >= 0 && j < kCoregBins) acc += A.taps[k + R] * W1[j * kCoregBins + c];
    }
    acc += DBL_EPSILON;
    W2[g * kCoregBins + c] = acc;
    col += acc;
  }
  s_buf[t] = col;
  __syncthreads();
  double s1raw = 0.0;
  if (t < kCoregBins) {
    s1raw = s_buf[t];
    for (int q = 1; q < kRows; ++q) s1raw += s_buf[q * kCoregBins + t];
  }
  const double sh = block_sum(s1raw, s_buf);
  // row sums: wave w takes rows w, w + kWaves, ...; lanes in a fixed order, then a fixed shuffle tree
  const int lane = t & (kWave - 1), wave = t / kWave;
  for (int g = wave; g < kCoregBins; g += kWaves) {
    double v = W2[g * kCoregBins + lane];
    for (int q = 1; q < kCoregBins / kWave; ++q) v += W2[g * kCoregBins + lane + q * kWave];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if (lane == 0) s_s2[g] = v / sh;
  }
  if (t < kCoregBins) s_s1[t] = s1raw / sh;
  __syncthreads();
  double hlh = 0.0, mi = 0.0;
  const double s1c = s_s1[c];
  for (int g = r * kSpan; g < (r + 1) * kSpan; ++g) {
    const double p = W2[g * kCoregBins + c] / sh;
    hlh += p * log2(p);
    mi += p * log2(p / (s_s2[g] * s1c));
  }
  double e1 = 0.0, e2 = 0.0;
  if (t < kCoregBins) {
    e1 = s_s1[t] * log2(s_s1[t]);
    e2 = s_s2[t] * log2(s_s2[t]);
  }
  const double Hj = block_sum(hlh, s_buf);
  const double MI = block_sum(mi, s_buf);
  const double E1 = block_sum(e1, s_buf);
  const double E2 = block_sum(e2, s_buf);
  if (t == 0) {
    double v;
    if (A.cost_fun == 0)
      v = -(E1 + E2) / Hj;
    else if (A.cost_fun == 1)
      v = -MI;
    else
      v = 2.0 * MI / (E1 + E2);
    cost[o] = v;
  }
}

}  // namespace

int coreg_quant_blocks(int64_t n) {
  const int64_t per = (int64_t)kCoregQBlock * 32;  // >= 32 voxels per thread
  return (int)std::min<int64_t>(std::max<int64_t>((n + per - 1) / per, 1), 512);
}

int64_t coreg_grid(const CoregJobHost &j, int32_t ng[3]) {
  int64_t n = 1;
  for (int d = 0; d < 3; ++d) {
    const double v = floor((double)(j.dim_g[d] - 1) / (double)j.step[d]) + 1.0;
    ng[d] = v > 2147483647.0 ? 2147483647 : (int32_t)v;
    n *= ng[d];
  }
  return n;
}

void launch_coreg_quantise(int n, const float *const *ptrs, const int64_t *sizes, uint8_t *const *outs,
                           uint32_t *counts, float *params, hipStream_t st) {
  QBatch B{};
  B.nobs = n;
  int nb = 0;
  for (int o = 0; o < n; ++o) {
    B.p[o] = ptrs[o];
    B.u[o] = outs[o];
    B.n[o] = sizes[o];
    B.blk0[o] = nb;
    nb += coreg_quant_blocks(sizes[o]);
  }
  B.blk0[n] = nb;
  hipLaunchKernelGGL(k_coreg_qinit, dim3(n), dim3(kCoregQBlock), 0, st, counts, params);
  hipLaunchKernelGGL(k_coreg_qrange, dim3(nb), dim3(kCoregQBlock), 0, st, B, params);
  hipLaunchKernelGGL(k_coreg_qhist, dim3(nb), dim3(kCoregQBlock), 0, st, B, (const float *)params, counts);
  hipLaunchKernelGGL(k_coreg_qparam, dim3(n), dim3(kCoregQBins), 0, st, (const uint32_t *)counts, params);
  hipLaunchKernelGGL(k_coreg_quant, dim3(nb), dim3(kCoregQBlock), 0, st, B, (const float *)params);
}

void launch_coreg_hist(int n, const CoregJobHost *jobs, uint64_t *hist, hipStream_t st) {
  HBatch B{};
  B.njobs = n;
  int nb = 0;
  for (int o = 0; o < n; ++o) {
    const CoregJobHost &s = jobs[o];
    HJob &j = B.j[o];
    j.G = s.G;
    j.F = s.F;
    for (int d = 0; d < 3; ++d) {
      j.dg[d] = s.dim_g[d];
      j.df[d] = s.dim_f[d];
      j.s[d] = s.step[d];
    }
    for (int e = 0; e < 12; ++e) j.M[e] = s.M[e];
    j.npts = (int32_t)coreg_grid(s, j.ng);  // <= INT32_MAX: checked by the caller
    B.blk0[o] = nb;
    nb += 2 * (int)((j.npts + kCoregChunk - 1) / kCoregChunk);
  }
  B.blk0[n] = nb;
  hipLaunchKernelGGL(k_coreg_hist, dim3(nb), dim3(kCoregBlock), 0, st, B, hist);
}

void launch_coreg_quantise_m(int n, const float *const *ptrs, const int64_t *sizes, const uint8_t *const *masks,
                             uint8_t *const *outs, uint32_t *counts, float *params, hipStream_t st) {
  QBatchM Q{};
  QBatch &B = Q.B;
  B.nobs = n;
  int nb = 0;
  for (int o = 0; o < n; ++o) {
    B.p[o] = ptrs[o];
    B.u[o] = outs[o];
    Q.m[o] = masks ? masks[o] : nullptr;
    B.n[o] = sizes[o];
    B.blk0[o] = nb;
    nb += coreg_quant_blocks(sizes[o]);
  }
  B.blk0[n] = nb;
  hipLaunchKernelGGL(k_coreg_qinit, dim3(n), dim3(kCoregQBlock), 0, st, counts, params);
  hipLaunchKernelGGL(k_coreg_qrange_m, dim3(nb), dim3(kCoregQBlock), 0, st, Q, params);
  hipLaunchKernelGGL(k_coreg_qhist_m, dim3(nb), dim3(kCoregQBlock), 0, st, Q, (const float *)params, counts);
  hipLaunchKernelGGL(k_coreg_qparam, dim3(n), dim3(kCoregQBins), 0, st, (const uint32_t *)counts, params);
  hipLaunchKernelGGL(k_coreg_quant, dim3(nb), dim3(kCoregQBlock), 0, st, B, (const float *)params);
}

void launch_coreg_cellmask(const uint8_t *mask, const int32_t dim[3], uint8_t *cell, hipStream_t st) {
  const size_t n = (size_t)dim[0] * dim[1] * dim[2];
  const int nb = (int)std::min<size_t>((n + 255) / 256, 65536);
  hipLaunchKernelGGL(k_coreg_cellmask, dim3(nb), dim3(256), 0, st, mask, dim[0], dim[1], dim[2], cell);
}

void launch_coreg_hist_m(int n, const CoregJobMHost *jobs, uint64_t *hist, hipStream_t st) {
  HBatchM B{};
  B.njobs = n;
  int nb = 0;
  for (int o = 0; o < n; ++o) {
    const CoregJobHost &s = jobs[o].job;
    HJob &j = B.j[o].j;
    j.G = s.G;
    j.F = s.F;
    for (int d = 0; d < 3; ++d) {
      j.dg[d] = s.dim_g[d];
      j.df[d] = s.dim_f[d];
      j.s[d] = s.step[d];
    }
    for (int e = 0; e < 12; ++e) j.M[e] = s.M[e];
    j.npts = (int32_t)coreg_grid(s, j.ng);  // <= INT32_MAX: checked by the caller
    B.j[o].mG = jobs[o].mG;
    B.j[o].mF = jobs[o].mF;
    B.blk0[o] = nb;
    nb += 2 * (int)((j.npts + kCoregChunk - 1) / kCoregChunk);
  }
  B.blk0[n] = nb;
  hipLaunchKernelGGL(k_coreg_hist_m, dim3(nb), dim3(kCoregBlock), 0, st, B, hist);
}

void launch_coreg_cost(int n, const uint64_t *hist, int cost_fun, const double *taps, int radius, double *work,
                       double *cost, hipStream_t st) {
  CostArgs A{};
  for (int k = 0; k <= 2 * radius; ++k) A.taps[k] = taps[k];
  A.radius = radius;
  A.cost_fun = cost_fun;
  hipLaunchKernelGGL(k_coreg_cost, dim3(n), dim3(kCoregBlock), 0, st, hist, A, work, cost);
}

}  // namespace unires
