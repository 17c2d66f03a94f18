// slice.hip - per-slice weights of an observation (sett.slice_robust, _input.slice_w): the data term of repeat n
// becomes 1/2 tau_n sum_v u_n[s(v)] [x_n(v) != 0] (x_n(v) - (A_n y)(v))^2, a noise precision per slice.
//   k_slice_sums_rows / k_slice_sums_z + k_slice_finish: SSE_s and N_s of every slice, what the weights are estimated
//     from.  Not on any solve's path: once per observation and ADMM iteration.
//   k_slice_apply: buf[v] *= u[s(v)] on the x-space intermediate between the forward half of A^T A and its push
//     (A^T diag(u . m) A), with the validity mask of mask.hip in the same pass; out of place it makes u . x for the
//     right-hand side.
//   k_rigid_resid: u[s(v)] (A y - x), masked - the residual of the rigid Gauss-Newton step on the same data term.
#include <algorithm>

#include "slice.hpp"

namespace unires {

namespace {

// one term of a slice's sums: float32 residual and square (k_masked_sse's, k_scaling_sums'), float64 sum
__device__ __forceinline__ void slice_term(const float *__restrict__ x, const float *__restrict__ ay, size_t o, double &acc,
                                           unsigned &cnt) {
  const float xv = x[o];
  if (xv != 0.f) {
    const float r = __fsub_rn(xv, ay[o]);
    acc += (double)__fmul_rn(r, r);
    ++cnt;
  }
}

// Slices along axis 0 (a slice is a contiguous plane) or axis 1 (a slice is one z-row of every x): workgroup
// (s, b) takes the b-th share of slice s - along axis 0 consecutive threads read consecutive voxels of the plane,
// along axis 1 a wave takes a whole z-row at a time - and writes its two sums to part[s][b], part[S + s][b].  Every
// thread's share, block_sum's tree and k_slice_finish's order over the shares are fixed: no atomics.
__global__ void __launch_bounds__(kBlock) k_slice_sums_rows(const float *__restrict__ x, const float *__restrict__ ay, Dim3i d,
                                                            int axis, double *__restrict__ part) {
  const size_t s = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  const size_t S = axis == 0 ? d.x : d.y;
  double acc = 0.0;
  unsigned cnt = 0;
  if (axis == 0) {
    const size_t P = (size_t)d.y * d.z, base = s * P;
    for (size_t e = b * kBlock + threadIdx.x; e < P; e += B * kBlock) slice_term(x, ay, base + e, acc, cnt);
  } else {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (size_t i = b * (kBlock / kWave) + wave; i < (size_t)d.x; i += B * (kBlock / kWave)) {
      const size_t base = (i * d.y + s) * d.z;
      for (int k = lane; k < d.z; k += kWave) slice_term(x, ay, base + k, acc, cnt);
    }
  }
  const double ts = block_sum(acc), tc = block_sum((double)cnt);
  if (threadIdx.x == 0) part[s * B + b] = ts, part[(S + s) * B + b] = tc;
}

// Slices along axis 2, the fastest: a lane keeps its z - and so its slice - while the workgroup's waves walk the
// z-rows (coalesced: no gathers a row apart).  The four waves' sums of a z are added in wave order through LDS.
__global__ void __launch_bounds__(kBlock) k_slice_sums_z(const float *__restrict__ x, const float *__restrict__ ay, Dim3i d,
                                                         double *__restrict__ part) {
  __shared__ double s_acc[kBlock / kWave][kWave];
  __shared__ unsigned s_cnt[kBlock / kWave][kWave];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const size_t z = (size_t)blockIdx.x * kWave + lane, b = blockIdx.y, B = gridDim.y;
  const size_t R = (size_t)d.x * d.y, S = d.z;
  double acc = 0.0;
  unsigned cnt = 0;
  if (z < S)
    for (size_t r = b * (kBlock / kWave) + wave; r < R; r += B * (kBlock / kWave)) slice_term(x, ay, r * S + z, acc, cnt);
  s_acc[wave][lane] = acc, s_cnt[wave][lane] = cnt;
  __syncthreads();
  if (wave == 0 && z < S) {
    double t = s_acc[0][lane];
    unsigned c = s_cnt[0][lane];
    for (int w = 1; w < kBlock / kWave; ++w) t += s_acc[w][lane], c += s_cnt[w][lane];
    part[z * B + b] = t, part[(S + z) * B + b] = (double)c;
  }
}

// out[c] = sum_b part[c][b]: a wave per entry, lane l adds the shares l, l + 64, ... in index order, wave_sum's fixed tree
// adds the lanes
__global__ void __launch_bounds__(kBlock) k_slice_finish(const double *__restrict__ part, int B, size_t ncols,
                                                         double *__restrict__ out) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (size_t c = (size_t)blockIdx.x * (kBlock / kWave) + wave; c < ncols; c += (size_t)gridDim.x * (kBlock / kWave)) {
    double a = 0.0;
    for (int b = lane; b < B; b += kWave) a += part[c * B + b];
    a = wave_sum(a);
    if (lane == 0) out[c] = a;
  }
}

// dst = u[s(v)] src (0 where the mask byte is 0).  The first n4 groups of 4 voxels are one 16-byte load / store each
// (their 4 mask bytes one 32-bit load), whatever the row length: a thread keeps (i, j, k) of its group's first voxel
// by carry arithmetic (k_scaling_sums' idiom: none per voxel; the position of a thread's first group is decoded once, in
// 32-bit arithmetic where the volume allows, and the stride's (si, sj, sk) comes from the launcher) and steps through the
// group's four voxels, which may cross into the next row.  In place, a group whose four factors are 1 is not stored back.
// The voxels from 4 n4 on go one by one: the tail of up to 3 - or the whole volume, where the launcher found a buffer
// off its boundary and passed n4 = 0 (the plan's own buffers never are).
template <bool MASK>
__global__ void __launch_bounds__(kBlock) k_slice_apply(const float *src, float *dst, const uint8_t *__restrict__ mask,
                                                        const float *__restrict__ u, Dim3i d, int axis, int flip, int si,
                                                        int sj, int sk, size_t n4, size_t n,
                                                        const int *__restrict__ done) {
  if (done && *done) return;
  const int S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  const bool inplace = src == dst;
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  const size_t plane = (size_t)d.y * d.z;
  const auto weight = [&](int i, int j, int k) {
    const int c = axis == 0 ? i : (axis == 1 ? j : k);
    return u[flip ? S - 1 - c : c];
  };
  if (tid < n4) {
    const size_t e0 = 4 * tid;
    int i, j, k;
    if (n <= 0xffffffffull) {  // (uniform: the usual case, without 64-bit divisions)
      const unsigned e = (unsigned)e0, pl = (unsigned)plane, r = e / (unsigned)d.z;
      i = (int)(e / pl), j = (int)(r - (unsigned)i * (unsigned)d.y), k = (int)(e - r * (unsigned)d.z);
    } else {
      i = (int)(e0 / plane), j = (int)((e0 % plane) / d.z), k = (int)(e0 % d.z);
    }
    for (size_t g = tid; g < n4; g += step) {
      float w[4];
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
      const unsigned m = MASK ? *reinterpret_cast<const unsigned *>(mask + 4 * g) : 0x01010101u;
      const bool k0 = m & 0xffu, k1 = m & 0xff00u, k2 = m & 0xff0000u, k3 = m & 0xff000000u;
      const bool same = k0 && k1 && k2 && k3 && w[0] == 1.f && w[1] == 1.f && w[2] == 1.f && w[3] == 1.f;
      if (!(inplace && same)) {
        float4 v = *reinterpret_cast<const float4 *>(src + 4 * g);
        v.x = k0 ? v.x * w[0] : 0.f, v.y = k1 ? v.y * w[1] : 0.f, v.z = k2 ? v.z * w[2] : 0.f, v.w = k3 ? v.w * w[3] : 0.f;
        *reinterpret_cast<float4 *>(dst + 4 * g) = v;
      }
      k += sk;
      if (k >= d.z) k -= d.z, ++j;
      j += sj;
      if (j >= d.y) j -= d.y, ++i;  // (j + carry + sj <= 2 dy - 1: once)
      i += si;
    }
  }
  for (size_t e = 4 * n4 + tid; e < n; e += step) {
    const float w = weight((int)(e / plane), (int)((e % plane) / d.z), (int)(e % d.z));
    dst[e] = (!MASK || mask[e]) ? src[e] * w : 0.f;
  }
}

// one voxel of the rigid step's residual: w (ay - x) where both are non-zero (_rigid_terms' mask), else +0
__device__ __forceinline__ float resid_term(float xv, float av, float w) {
  return (xv != 0.f && av != 0.f) ? __fmul_rn(w, __fsub_rn(av, xv)) : 0.f;
}

// out = u[s(v)] (ay - x), masked: the residual of the rigid Gauss-Newton step in one pass (four volume-sized tensor
// passes before: difference, two comparisons, masked store).  k_slice_apply's shape: 16-byte loads and stores whatever
// the row length, (i, j, k) of a thread's group of four kept by carry arithmetic, a group that crosses a row end
// stepped through voxel by voxel, the voxels from 4 n4 on one by one (n4 = 0 for a buffer off its boundary).  Without
// W the weight is 1 - times 1 is exact - and no position is kept.  out may be ay: a thread reads its group before it
// stores it, and no other thread touches the group.
template <bool W>
__global__ void __launch_bounds__(kBlock) k_rigid_resid(const float *__restrict__ x, const float *ay, float *out,
                                                        const float *__restrict__ u, Dim3i d, int axis, int si, int sj,
                                                        int sk, size_t n4, size_t n) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  const size_t plane = (size_t)d.y * d.z;
  const auto weight = [&](int i, int j, int k) { return W ? u[axis == 0 ? i : (axis == 1 ? j : k)] : 1.f; };
  if (tid < n4) {
    int i = 0, j = 0, k = 0;
    if (W) {
      const size_t e0 = 4 * tid;
      if (n <= 0xffffffffull) {  // (uniform: the usual case, without 64-bit divisions)
        const unsigned e = (unsigned)e0, pl = (unsigned)plane, r = e / (unsigned)d.z;
        i = (int)(e / pl), j = (int)(r - (unsigned)i * (unsigned)d.y), k = (int)(e - r * (unsigned)d.z);
      } else {
        i = (int)(e0 / plane), j = (int)((e0 % plane) / d.z), k = (int)(e0 % d.z);
      }
    }
    for (size_t g = tid; g < n4; g += step) {
      float w[4] = {1.f, 1.f, 1.f, 1.f};
      if (W) {
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
      const float4 xv = *reinterpret_cast<const float4 *>(x + 4 * g);
      const float4 av = *reinterpret_cast<const float4 *>(ay + 4 * g);
      float4 v;
      v.x = resid_term(xv.x, av.x, w[0]), v.y = resid_term(xv.y, av.y, w[1]);
      v.z = resid_term(xv.z, av.z, w[2]), v.w = resid_term(xv.w, av.w, w[3]);
      *reinterpret_cast<float4 *>(out + 4 * g) = v;
      if (W) {
        k += sk;
        if (k >= d.z) k -= d.z, ++j;
        j += sj;
        if (j >= d.y) j -= d.y, ++i;  // (j + carry + sj <= 2 dy - 1: once)
        i += si;
      }
    }
  }
  for (size_t e = 4 * n4 + tid; e < n; e += step)
    out[e] = resid_term(x[e], ay[e], weight((int)(e / plane), (int)((e % plane) / d.z), (int)(e % d.z)));
}

}  // namespace

int slice_sums_parts(Dim3i d, int axis) {
  // about 2048 workgroups in all, no more shares than a slice has work for
  size_t units, groups;
  if (axis == 2) {
    groups = ((size_t)d.z + kWave - 1) / kWave;
    units = ((size_t)d.x * d.y + 15) / 16;  // 4 z-rows per wave at least
  } else if (axis == 1) {
    groups = d.y;
    units = ((size_t)d.x + 3) / 4;  // a z-row per wave
  } else {
    groups = d.x;
    units = ((size_t)d.y * d.z + 4 * kBlock - 1) / (4 * kBlock);  // 4 voxels per thread at least
  }
  const size_t B = std::min<size_t>(std::min<size_t>(units, std::max<size_t>(1, 2048 / groups)), 1024);
  return (int)std::max<size_t>(1, B);
}

void launch_slice_sums(const float *x, const float *ay, Dim3i d, int axis, double *part, double *out, hipStream_t st) {
  const int B = slice_sums_parts(d, axis);
  const size_t S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  if (axis == 2)
    hipLaunchKernelGGL(k_slice_sums_z, dim3((unsigned)((S + kWave - 1) / kWave), B), dim3(kBlock), 0, st, x, ay, d, part);
  else
    hipLaunchKernelGGL(k_slice_sums_rows, dim3((unsigned)S, B), dim3(kBlock), 0, st, x, ay, d, axis, part);
  const size_t blocks = std::min<size_t>((2 * S + kBlock / kWave - 1) / (kBlock / kWave), 4096);
  hipLaunchKernelGGL(k_slice_finish, dim3((unsigned)blocks), dim3(kBlock), 0, st, part, B, 2 * S, out);
}

void launch_slice_apply(const float *src, float *dst, const uint8_t *mask, const float *u, Dim3i d, int axis, bool flip,
                        const int *done, hipStream_t st) {
  const size_t n = d.numel();
  if (!n) return;
  const bool aligned = ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)mask & 3) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  // 256 threads x 4 floats per block and loop step, as k_mask_apply: a streaming pass
  const size_t work = aligned ? n4 + 3 : n;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 2048));
  // the loop's stride of 4 * blocks * kBlock voxels as (planes, rows, voxels)
  const size_t se = 4 * blocks * kBlock, plane = (size_t)d.y * d.z;
  const int si = (int)(se / plane), sj = (int)((se % plane) / d.z), sk = (int)(se % d.z);
  if (mask)
    hipLaunchKernelGGL(k_slice_apply<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, src, dst, mask, u, d, axis,
                       flip ? 1 : 0, si, sj, sk, n4, n, done);
  else
    hipLaunchKernelGGL(k_slice_apply<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, src, dst, mask, u, d, axis,
                       flip ? 1 : 0, si, sj, sk, n4, n, done);
}

void launch_rigid_resid(const float *x, const float *ay, float *out, const float *u, Dim3i d, int axis,
                        hipStream_t st) {
  const size_t n = d.numel();
  if (!n) return;
  const bool aligned = (((uintptr_t)x | (uintptr_t)ay | (uintptr_t)out) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  // launch_slice_apply's grid and stride decode
  const size_t work = aligned ? n4 + 3 : n;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 2048));
  const size_t se = 4 * blocks * kBlock, plane = (size_t)d.y * d.z;
  const int si = (int)(se / plane), sj = (int)((se % plane) / d.z), sk = (int)(se % d.z);
  if (u)
    hipLaunchKernelGGL(k_rigid_resid<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, out, u, d, axis, si, sj,
                       sk, n4, n);
  else
    hipLaunchKernelGGL(k_rigid_resid<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, x, ay, out, u, d, axis, si, sj,
                       sk, n4, n);
}

}  // namespace unires
