// voxel.hip - per-voxel weights of an observation (_input.weight, sett.voxel_robust): the data term of repeat n
// becomes 1/2 tau_n sum_v g_n(v) u_n[s(v)] [x_n(v) != 0] (x_n(v) - (A_n y)(v))^2, a noise precision per voxel.
//   k_voxel_apply: buf[v] *= g[v] on the x-space intermediate between the forward half of A^T A and its push
//     (A^T diag(g . u . m) A), with the slice weights of slice.hip and the validity mask of mask.hip in the same pass;
//     out of place it makes g . u . x for the right-hand side.
//   k_voxel_permute: g from the caller's layout into the plan's canonical one (orient.hip), once per set.
//   k_voxel_sums_rows / k_voxel_sums_z + k_voxel_finish: sum g (x - A y)^2 and sum g of every slice, the one statement
//     of a voxel-weighted repeat's data term.  Not on any solve's path.
//   k_voxel_huber: g = prior . h, h the Huber weight of the residual.  One streaming pass, no reduction.
//   k_voxel_huber_dev: the same with the threshold a multiple of a scale the device holds (median.hip).
//   k_rigid_resid_g: g [u[s(v)]] (A y - x), masked - the residual of the rigid Gauss-Newton step on the same data term
//     (the five sums of the scaling step on it are k_scaling_sums_g, admm.hip).
#include <algorithm>

#include "slice.hpp"
#include "voxel.hpp"

namespace unires {

namespace {

// dst = g [u[s(v)]] src (0 where the mask byte is 0): k_slice_apply's shape.  The first n4 groups of 4 voxels are one
// 16-byte load / store each, their 4 weights g one 16-byte load beside them (their 4 mask bytes one 32-bit load),
// whatever the row length.  With SLICE a thread keeps (i, j, k) of its group's first voxel by carry arithmetic
// (k_scaling_sums' idiom: the position of a thread's first group is decoded once, in 32-bit arithmetic where the volume
// allows, and the stride's (si, sj, sk) comes from the launcher) and steps through the group's four voxels, which may
// cross into the next row; the factor is then g u, exact in float64, and g u src is rounded to float32 once.  Without
// SLICE no position is kept and the product is __fmul_rn(g, src) - the same single rounding.  In place, a group whose
// four factors are 1 is not stored back.  The voxels from 4 n4 on go one by one: the tail of up to 3 - or the whole
// volume, where the launcher found a buffer off its boundary and passed n4 = 0 (the plan's own buffers never are).
template <bool MASK, bool SLICE>
__global__ void __launch_bounds__(kBlock) k_voxel_apply(const float *src, float *dst, const float *__restrict__ g,
                                                        const uint8_t *__restrict__ mask, const float *__restrict__ u,
                                                        Dim3i d, int axis, int flip, int si, int sj, int sk, size_t n4,
                                                        size_t n, const int *__restrict__ done) {
  if (done && *done) return;
  const int S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  const bool inplace = src == dst;
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  const size_t plane = (size_t)d.y * d.z;
  const auto weight = [&](int i, int j, int k) {
    const int c = axis == 0 ? i : (axis == 1 ? j : k);
    return u[flip ? S - 1 - c : c];
  };
  const auto times = [](float gv, float uv, float v) {
    return SLICE ? (float)(((double)gv * (double)uv) * (double)v) : __fmul_rn(gv, v);
  };
  if (tid < n4) {
    int i = 0, j = 0, k = 0;
    if (SLICE) {
      const size_t e0 = 4 * tid;
      if (n <= 0xffffffffull) {  // (uniform: the usual case, without 64-bit divisions)
        const unsigned e = (unsigned)e0, pl = (unsigned)plane, r = e / (unsigned)d.z;
        i = (int)(e / pl), j = (int)(r - (unsigned)i * (unsigned)d.y), k = (int)(e - r * (unsigned)d.z);
      } else {
        i = (int)(e0 / plane), j = (int)((e0 % plane) / d.z), k = (int)(e0 % d.z);
      }
    }
    for (size_t q = tid; q < n4; q += step) {
      float w[4] = {1.f, 1.f, 1.f, 1.f};
      if (SLICE) {
        if (axis != 2 && k + 3 < d.z) {  // (axes 0 and 1: the weight is uniform over a z-row, and the group stays in its row)
          w[0] = w[1] = w[2] = w[3] = weight(i, j, k);
        } else {
          int ie = i, je = j, ke = k;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            w[e] = weight(ie, je, ke);
            if (++ke == d.z) {
              ke = 0;
              if (++je == d.y) je = 0, ++ie;
            }
          }
        }
      }
      const float4 gv = *reinterpret_cast<const float4 *>(g + 4 * q);
      const unsigned m = MASK ? *reinterpret_cast<const unsigned *>(mask + 4 * q) : 0x01010101u;
      const bool k0 = m & 0xffu, k1 = m & 0xff00u, k2 = m & 0xff0000u, k3 = m & 0xff000000u;
      const bool same = k0 && k1 && k2 && k3 && w[0] == 1.f && w[1] == 1.f && w[2] == 1.f && w[3] == 1.f &&
                        gv.x == 1.f && gv.y == 1.f && gv.z == 1.f && gv.w == 1.f;
      if (!(inplace && same)) {
        float4 v = *reinterpret_cast<const float4 *>(src + 4 * q);
        v.x = k0 ? times(gv.x, w[0], v.x) : 0.f, v.y = k1 ? times(gv.y, w[1], v.y) : 0.f;
        v.z = k2 ? times(gv.z, w[2], v.z) : 0.f, v.w = k3 ? times(gv.w, w[3], v.w) : 0.f;
        *reinterpret_cast<float4 *>(dst + 4 * q) = v;
      }
      if (SLICE) {
        k += sk;
        if (k >= d.z) k -= d.z, ++j;
        j += sj;
        if (j >= d.y) j -= d.y, ++i;  // (j + carry + sj <= 2 dy - 1: once)
        i += si;
      }
    }
  }
  for (size_t e = 4 * n4 + tid; e < n; e += step) {
    const float w = SLICE ? weight((int)(e / plane), (int)((e % plane) / d.z), (int)(e % d.z)) : 1.f;
    dst[e] = (!MASK || mask[e]) ? times(g[e], w, src[e]) : 0.f;
  }
}

struct VoxelPerm {
  int d[3];        // canonical dims (z fastest)
  long long s[3];  // source stride (elements, signed) per canonical axis
  long long off;   // source offset of canonical voxel (0, 0, 0)
};

VoxelPerm voxel_perm(const Orient &O, Dim3i du) {
  const int nu[3] = {du.x, du.y, du.z};
  const long long su[3] = {(long long)du.y * du.z, du.z, 1};
  VoxelPerm P;
  P.off = 0;
  for (int j = 0; j < 3; ++j) {
    const int a = O.perm[j];
    P.d[j] = nu[a];
    P.s[j] = O.flip[j] ? -su[a] : su[a];
    if (O.flip[j]) P.off += (long long)(nu[a] - 1) * su[a];
  }
  return P;
}

// One canonical voxel per thread (grid-stride), k_mask_build's decode.  Not on any solve's path: once per set.
__global__ void __launch_bounds__(kBlock) k_voxel_permute(const float *__restrict__ src, float *__restrict__ dst,
                                                          VoxelPerm P, size_t n) {
  const size_t step = (size_t)gridDim.x * kBlock;
  for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < n; idx += step) {
    const size_t ij = idx / (size_t)P.d[2];
    const long long k = (long long)(idx - ij * (size_t)P.d[2]);
    const long long i = (long long)(ij / (size_t)P.d[1]), j = (long long)(ij - (size_t)i * (size_t)P.d[1]);
    dst[idx] = src[P.off + i * P.s[0] + j * P.s[1] + k * P.s[2]];
  }
}

// one term of a slice's weighted sums: float32 residual, square and product with g (slice_term's, times g), float64 sums
__device__ __forceinline__ void voxel_term(const float *__restrict__ x, const float *__restrict__ ay,
                                           const float *__restrict__ g, size_t o, double &acc, double &gs) {
  const float xv = x[o];
  if (xv != 0.f) {
    const float r = __fsub_rn(xv, ay[o]), gv = g[o];
    acc += (double)__fmul_rn(gv, __fmul_rn(r, r));
    gs += (double)gv;
  }
}

// k_slice_sums_rows with g: the same shares, the same order of every thread's terms, of block_sum's tree and of
// k_voxel_finish over the shares - with g = 1 the bits of k_slice_sums_rows.  No atomics.
__global__ void __launch_bounds__(kBlock) k_voxel_sums_rows(const float *__restrict__ x, const float *__restrict__ ay,
                                                            const float *__restrict__ g, Dim3i d, int axis,
                                                            double *__restrict__ part) {
  const size_t s = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  const size_t S = axis == 0 ? d.x : d.y;
  double acc = 0.0, gs = 0.0;
  if (axis == 0) {
    const size_t P = (size_t)d.y * d.z, base = s * P;
    for (size_t e = b * kBlock + threadIdx.x; e < P; e += B * kBlock) voxel_term(x, ay, g, base + e, acc, gs);
  } else {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (size_t i = b * (kBlock / kWave) + wave; i < (size_t)d.x; i += B * (kBlock / kWave)) {
      const size_t base = (i * d.y + s) * d.z;
      for (int k = lane; k < d.z; k += kWave) voxel_term(x, ay, g, base + k, acc, gs);
    }
  }
  const double ts = block_sum(acc), tc = block_sum(gs);
  if (threadIdx.x == 0) part[s * B + b] = ts, part[(S + s) * B + b] = tc;
}

// k_slice_sums_z with g: a lane keeps its z while the workgroup's waves walk the z-rows; the four waves' sums of a z are
// added in wave order through LDS.
__global__ void __launch_bounds__(kBlock) k_voxel_sums_z(const float *__restrict__ x, const float *__restrict__ ay,
                                                         const float *__restrict__ g, Dim3i d,
                                                         double *__restrict__ part) {
  __shared__ double s_acc[kBlock / kWave][kWave];
  __shared__ double s_gs[kBlock / kWave][kWave];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const size_t z = (size_t)blockIdx.x * kWave + lane, b = blockIdx.y, B = gridDim.y;
  const size_t R = (size_t)d.x * d.y, S = d.z;
  double acc = 0.0, gs = 0.0;
  if (z < S)
    for (size_t r = b * (kBlock / kWave) + wave; r < R; r += B * (kBlock / kWave)) voxel_term(x, ay, g, r * S + z, acc, gs);
  s_acc[wave][lane] = acc, s_gs[wave][lane] = gs;
  __syncthreads();
  if (wave == 0 && z < S) {
    double t = s_acc[0][lane], c = s_gs[0][lane];
    for (int w = 1; w < kBlock / kWave; ++w) t += s_acc[w][lane], c += s_gs[w][lane];
    part[z * B + b] = t, part[(S + z) * B + b] = c;
  }
}

// out[c] = sum_b part[c][b]: k_slice_finish's order - a wave per entry, lane l adds the shares l, l + 64, ... in index
// order, wave_sum's fixed tree adds the lanes
__global__ void __launch_bounds__(kBlock) k_voxel_finish(const double *__restrict__ part, int B, size_t ncols,
                                                         double *__restrict__ out) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (size_t c = (size_t)blockIdx.x * (kBlock / kWave) + wave; c < ncols; c += (size_t)gridDim.x * (kBlock / kWave)) {
    double a = 0.0;
    for (int b = lane; b < B; b += kWave) a += part[c * B + b];
    a = wave_sum(a);
    if (lane == 0) out[c] = a;
  }
}

// one voxel of the Huber rule: prior . h, h = 1 where the voxel is missing or |r| <= c, else c / |r|
__device__ __forceinline__ float huber_term(float xv, float av, float pv, float c) {
  const float a = fabsf(__fsub_rn(xv, av));
  const float h = (xv == 0.f || a <= c) ? 1.f : __fdiv_rn(c, a);
  return __fmul_rn(pv, h);
}

// g_out = prior . h (prior == nullptr: h): 16-byte groups, then the tail one by one - or the whole buffer, where the
// launcher found one off its boundary and passed n4 = 0.  g_out may be prior: a thread reads its group before it stores
// it, and no other thread touches the group.
template <bool PRIOR>
__global__ void __launch_bounds__(kBlock) k_voxel_huber(const float *__restrict__ x, const float *__restrict__ ay,
                                                        const float *prior, float c, size_t n4, size_t n, float *g_out) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  for (size_t q = tid; q < n4; q += step) {
    const float4 xv = *reinterpret_cast<const float4 *>(x + 4 * q);
    const float4 av = *reinterpret_cast<const float4 *>(ay + 4 * q);
    const float4 pv = PRIOR ? *reinterpret_cast<const float4 *>(prior + 4 * q) : make_float4(1.f, 1.f, 1.f, 1.f);
    float4 v;
    v.x = huber_term(xv.x, av.x, pv.x, c), v.y = huber_term(xv.y, av.y, pv.y, c);
    v.z = huber_term(xv.z, av.z, pv.z, c), v.w = huber_term(xv.w, av.w, pv.w, c);
    *reinterpret_cast<float4 *>(g_out + 4 * q) = v;
  }
  for (size_t e = 4 * n4 + tid; e < n; e += step) g_out[e] = huber_term(x[e], ay[e], PRIOR ? prior[e] : 1.f, c);
}

// k_voxel_huber with the threshold taken from the device: c = fl32(mult scale[0]), scale a median of median.hip that
// was never read back.  The same walk and the same huber_term, so c > 0 gives k_voxel_huber's bits; a threshold that
// is not > 0 (nothing eligible, a zero median) switches the rule off: g_out = prior.
template <bool PRIOR>
__global__ void __launch_bounds__(kBlock) k_voxel_huber_dev(const float *__restrict__ x, const float *__restrict__ ay,
                                                            const float *prior, const double *__restrict__ scale,
                                                            float mult, size_t n4, size_t n, float *g_out) {
  const float c = __fmul_rn(mult, (float)scale[0]);
  const bool off = !(c > 0.f);
  const auto term = [&](float xv, float av, float pv) { return off ? pv : huber_term(xv, av, pv, c); };
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  for (size_t q = tid; q < n4; q += step) {
    const float4 xv = *reinterpret_cast<const float4 *>(x + 4 * q);
    const float4 av = *reinterpret_cast<const float4 *>(ay + 4 * q);
    const float4 pv = PRIOR ? *reinterpret_cast<const float4 *>(prior + 4 * q) : make_float4(1.f, 1.f, 1.f, 1.f);
    float4 v;
    v.x = term(xv.x, av.x, pv.x), v.y = term(xv.y, av.y, pv.y);
    v.z = term(xv.z, av.z, pv.z), v.w = term(xv.w, av.w, pv.w);
    *reinterpret_cast<float4 *>(g_out + 4 * q) = v;
  }
  for (size_t e = 4 * n4 + tid; e < n; e += step) g_out[e] = term(x[e], ay[e], PRIOR ? prior[e] : 1.f);
}

// one voxel of the rigid step's residual on the voxel-weighted data term: g [u] (ay - x) where both are non-zero
// (_rigid_terms' mask), else +0; the product rounds as k_voxel_apply's: g u exact in float64, times the float32
// difference, one rounding to float32 - or one float32 product where there is no u
template <bool SLICE>
__device__ __forceinline__ float resid_term_g(float xv, float av, float gv, float uv) {
  if (!(xv != 0.f && av != 0.f)) return 0.f;
  const float r = __fsub_rn(av, xv);
  return SLICE ? (float)(((double)gv * (double)uv) * (double)r) : __fmul_rn(gv, r);
}

// out = g [u[s(v)]] (ay - x), masked: k_rigid_resid (slice.hip) with the voxel weights read beside x and ay - 16-byte
// loads of all three and 16-byte stores whatever the row length; with SLICE (i, j, k) of a thread's group of four kept
// by carry arithmetic and a group that crosses a row end stepped through voxel by voxel, without it no position at all;
// the voxels from 4 n4 on one by one (n4 = 0 for a buffer off its boundary).  g = 1 gives k_rigid_resid's bits: g u r
// is then u r, exact in float64 and rounded once, as __fmul_rn(u, r) is.  out may be ay: a thread reads its group
// before it stores it, and no other thread touches the group.  x and g are only read.
template <bool SLICE>
__global__ void __launch_bounds__(kBlock) k_rigid_resid_g(const float *__restrict__ x, const float *ay,
                                                          const float *__restrict__ g, float *out,
                                                          const float *__restrict__ u, Dim3i d, int axis, int si, int sj,
                                                          int sk, size_t n4, size_t n) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  const size_t plane = (size_t)d.y * d.z;
  const auto weight = [&](int i, int j, int k) { return SLICE ? u[axis == 0 ? i : (axis == 1 ? j : k)] : 1.f; };
  if (tid < n4) {
    int i = 0, j = 0, k = 0;
    if (SLICE) {
      const size_t e0 = 4 * tid;
      if (n <= 0xffffffffull) {  // (uniform: the usual case, without 64-bit divisions)
        const unsigned e = (unsigned)e0, pl = (unsigned)plane, r = e / (unsigned)d.z;
        i = (int)(e / pl), j = (int)(r - (unsigned)i * (unsigned)d.y), k = (int)(e - r * (unsigned)d.z);
      } else {
        i = (int)(e0 / plane), j = (int)((e0 % plane) / d.z), k = (int)(e0 % d.z);
      }
    }
    for (size_t q = tid; q < n4; q += step) {
      float w[4] = {1.f, 1.f, 1.f, 1.f};
      if (SLICE) {
        if (axis != 2 && k + 3 < d.z) {  // (axes 0 and 1: the weight is uniform over a z-row, and the group stays in its row)
          w[0] = w[1] = w[2] = w[3] = weight(i, j, k);
        } else {
          int ie = i, je = j, ke = k;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            w[e] = weight(ie, je, ke);
            if (++ke == d.z) {
              ke = 0;
              if (++je == d.y) je = 0, ++ie;
            }
          }
        }
      }
      const float4 xv = *reinterpret_cast<const float4 *>(x + 4 * q);
      const float4 av = *reinterpret_cast<const float4 *>(ay + 4 * q);
      const float4 gv = *reinterpret_cast<const float4 *>(g + 4 * q);
      float4 v;
      v.x = resid_term_g<SLICE>(xv.x, av.x, gv.x, w[0]), v.y = resid_term_g<SLICE>(xv.y, av.y, gv.y, w[1]);
      v.z = resid_term_g<SLICE>(xv.z, av.z, gv.z, w[2]), v.w = resid_term_g<SLICE>(xv.w, av.w, gv.w, w[3]);
      *reinterpret_cast<float4 *>(out + 4 * q) = v;
      if (SLICE) {
        k += sk;
        if (k >= d.z) k -= d.z, ++j;
        j += sj;
        if (j >= d.y) j -= d.y, ++i;  // (j + carry + sj <= 2 dy - 1: once)
        i += si;
      }
    }
  }
  for (size_t e = 4 * n4 + tid; e < n; e += step)
    out[e] = resid_term_g<SLICE>(x[e], ay[e], g[e],
                                 weight((int)(e / plane), (int)((e % plane) / d.z), (int)(e % d.z)));
}

}  // namespace

void launch_rigid_resid_g(const float *x, const float *ay, const float *g, float *out, const float *u, Dim3i d, int axis,
                          hipStream_t st) {
  const size_t n = d.numel();
  if (!n) return;
  const bool aligned = (((uintptr_t)x | (uintptr_t)ay | (uintptr_t)g | (uintptr_t)out) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  // launch_slice_apply's grid and stride decode
  const size_t work = aligned ? n4 + 3 : n;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 2048));
  const size_t se = 4 * blocks * kBlock, plane = (size_t)d.y * d.z;
  const int si = (int)(se / plane), sj = (int)((se % plane) / d.z), sk = (int)(se % d.z);
  if (u)
    hipLaunchKernelGGL(k_rigid_resid_g<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, g, out, u, d, axis, si,
                       sj, sk, n4, n);
  else
    hipLaunchKernelGGL(k_rigid_resid_g<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, g, out, u, d, axis, si,
                       sj, sk, n4, n);
}

void launch_voxel_apply(const float *src, float *dst, const float *g, const uint8_t *mask, const float *u, Dim3i d,
                        int axis, bool flip, const int *done, hipStream_t st) {
  const size_t n = d.numel();
  if (!n) return;
  const bool aligned = (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)g) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  // launch_slice_apply's grid and stride decode: 256 threads x 4 floats per block and loop step, a streaming pass
  const size_t work = aligned ? n4 + 3 : n;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 2048));
  const size_t se = 4 * blocks * kBlock, plane = (size_t)d.y * d.z;
  const int si = (int)(se / plane), sj = (int)((se % plane) / d.z), sk = (int)(se % d.z);
  const int f = flip ? 1 : 0;
#define UNIRES_VOXEL_APPLY(M, S)                                                                                      \
  hipLaunchKernelGGL((k_voxel_apply<M, S>), dim3((unsigned)blocks), dim3(kBlock), 0, st, src, dst, g, mask, u, d, axis, \
                     f, si, sj, sk, n4, n, done)
  if (mask && u)
    UNIRES_VOXEL_APPLY(true, true);
  else if (mask)
    UNIRES_VOXEL_APPLY(true, false);
  else if (u)
    UNIRES_VOXEL_APPLY(false, true);
  else
    UNIRES_VOXEL_APPLY(false, false);
#undef UNIRES_VOXEL_APPLY
}

void launch_voxel_permute(const float *g_u, const Orient &O, Dim3i du, float *g, hipStream_t st) {
  const size_t n = du.numel();
  if (!n) return;
  const size_t blocks = std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
  hipLaunchKernelGGL(k_voxel_permute, dim3((unsigned)blocks), dim3(kBlock), 0, st, g_u, g, voxel_perm(O, du), n);
}

void launch_voxel_sums(const float *x, const float *ay, const float *g, Dim3i d, int axis, double *part, double *out,
                       hipStream_t st) {
  const int B = slice_sums_parts(d, axis);
  const size_t S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  if (axis == 2)
    hipLaunchKernelGGL(k_voxel_sums_z, dim3((unsigned)((S + kWave - 1) / kWave), B), dim3(kBlock), 0, st, x, ay, g, d,
                       part);
  else
    hipLaunchKernelGGL(k_voxel_sums_rows, dim3((unsigned)S, B), dim3(kBlock), 0, st, x, ay, g, d, axis, part);
  const size_t blocks = std::min<size_t>((2 * S + kBlock / kWave - 1) / (kBlock / kWave), 4096);
  hipLaunchKernelGGL(k_voxel_finish, dim3((unsigned)blocks), dim3(kBlock), 0, st, part, B, 2 * S, out);
}

void launch_voxel_huber(const float *x, const float *ay, const float *prior, float c, size_t n, float *g_out,
                        hipStream_t st) {
  if (!n) return;
  const bool aligned = (((uintptr_t)x | (uintptr_t)ay | (uintptr_t)prior | (uintptr_t)g_out) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  const size_t work = aligned ? n4 + 3 : n;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 2048));
  if (prior)
    hipLaunchKernelGGL(k_voxel_huber<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, prior, c, n4, n, g_out);
  else
    hipLaunchKernelGGL(k_voxel_huber<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, prior, c, n4, n, g_out);
}

// launch_voxel_huber's grid and alignment rule
void launch_voxel_huber_dev(const float *x, const float *ay, const float *prior, const double *scale_dev, float mult,
                            size_t n, float *g_out, hipStream_t st) {
  if (!n) return;
  const bool aligned = (((uintptr_t)x | (uintptr_t)ay | (uintptr_t)prior | (uintptr_t)g_out) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  const size_t work = aligned ? n4 + 3 : n;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 2048));
  if (prior)
    hipLaunchKernelGGL(k_voxel_huber_dev<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, prior, scale_dev, mult,
                       n4, n, g_out);
  else
    hipLaunchKernelGGL(k_voxel_huber_dev<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, prior, scale_dev, mult,
                       n4, n, g_out);
}

}  // namespace unires
