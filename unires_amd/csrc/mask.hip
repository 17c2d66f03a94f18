// mask.hip - sett.mask_zeros: the validity mask m_n(v) = [x_n(v) != 0] of an observation and its use inside
// A_n^T diag(m_n) A_n.  k_mask_build writes the mask once per observation (and again when its values change);
// k_mask_apply runs between the forward half of A^T A and its push, on the x-space intermediate the plan owns.
//
// One BYTE per voxel.  The mask is stored in the plan's canonical layout while the observation arrives in the
// caller's, so neighbouring mask entries come from source voxels a whole stride apart: with a byte each thread stores
// its own entry, with a bit 8 (or, by ballot, 64) entries along the canonical z axis would have to be gathered into one
// store and rows whose length is no multiple of 8 would share a byte.  The apply pass reads 4 mask bytes beside each
// 16-byte access to the volume: 1/8 on top of the volume's own read + write, against 1/64 for bits - of a pass that is
// itself a small part of the operator.
#include <algorithm>

#include "mask.hpp"

namespace unires {

namespace {

struct MaskPerm {
  int d[3];        // canonical dims (z fastest)
  long long s[3];  // source stride (elements, signed) per canonical axis
  long long off;   // source offset of canonical voxel (0, 0, 0)
};

MaskPerm mask_perm(const Orient &O, Dim3i du) {
  const int nu[3] = {du.x, du.y, du.z};
  const long long su[3] = {(long long)du.y * du.z, du.z, 1};
  MaskPerm P;
  P.off = 0;
  for (int j = 0; j < 3; ++j) {
    const int a = O.perm[j];
    P.d[j] = nu[a];
    P.s[j] = O.flip[j] ? -su[a] : su[a];
    if (O.flip[j]) P.off += (long long)(nu[a] - 1) * su[a];
  }
  return P;
}

// One canonical voxel per thread (grid-stride).  Not on any solve's path: run once per observation.
template <class T>
__global__ void __launch_bounds__(kBlock) k_mask_build(const T *__restrict__ src, uint8_t *__restrict__ mask, MaskPerm P,
                                                       size_t n) {
  const size_t step = (size_t)gridDim.x * kBlock;
  for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < n; idx += step) {
    const size_t ij = idx / (size_t)P.d[2];
    const long long k = (long long)(idx - ij * (size_t)P.d[2]);
    const long long i = (long long)(ij / (size_t)P.d[1]), j = (long long)(ij - (size_t)i * (size_t)P.d[1]);
    mask[idx] = src[P.off + i * P.s[0] + j * P.s[1] + k * P.s[2]] != (T)0 ? 1 : 0;
  }
}

template <class T>
void launch_build(const T *src, const Orient &O, Dim3i du, uint8_t *mask, hipStream_t st) {
  const size_t n = du.numel();
  const size_t blocks = std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
  hipLaunchKernelGGL(k_mask_build<T>, dim3((unsigned)blocks), dim3(kBlock), 0, st, src, mask, mask_perm(O, du), n);
}

// buf[i] = mask[i] ? buf[i] : 0.  The first n4 groups of 4 voxels are one 16-byte load / store each, their 4 mask bytes
// one 32-bit load (a group with no zero entry is not stored back); the voxels from 4 n4 on go one by one, in the same
// grid-stride loop form: the tail of up to 3 - or the whole buffer, where the launcher found buf off a 16-byte or mask
// off a 4-byte boundary and passed n4 = 0 (the plan's own buffers never are).
__global__ void __launch_bounds__(kBlock) k_mask_apply(float *__restrict__ buf, const uint8_t *__restrict__ mask, size_t n4,
                                                       size_t n, const int *__restrict__ done) {
  if (done && *done) return;
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  for (size_t g = tid; g < n4; g += step) {
    const size_t i = 4 * g;
    const unsigned m = *reinterpret_cast<const unsigned *>(mask + i);
    const bool k0 = m & 0xffu, k1 = m & 0xff00u, k2 = m & 0xff0000u, k3 = m & 0xff000000u;
    if (k0 && k1 && k2 && k3) continue;
    float4 *p = reinterpret_cast<float4 *>(buf + i);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k0 || k1 || k2 || k3) {
      v = *p;
      v.x = k0 ? v.x : 0.f, v.y = k1 ? v.y : 0.f, v.z = k2 ? v.z : 0.f, v.w = k3 ? v.w : 0.f;
    }
    *p = v;
  }
  for (size_t i = 4 * n4 + tid; i < n; i += step)
    if (!mask[i]) buf[i] = 0.f;
}

}  // namespace

void launch_mask_build(const float *x, const Orient &O, Dim3i du, uint8_t *mask, hipStream_t st) {
  launch_build(x, O, du, mask, st);
}

void launch_mask_permute(const uint8_t *mask_u, const Orient &O, Dim3i du, uint8_t *mask, hipStream_t st) {
  launch_build(mask_u, O, du, mask, st);
}

void launch_mask_apply(float *buf, const uint8_t *mask, size_t n, const int *done, hipStream_t st) {
  if (!n) return;
  const bool aligned = ((uintptr_t)buf & 15) == 0 && ((uintptr_t)mask & 3) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  // 256 threads x 4 floats per block and loop step; at most 8 blocks per CU's worth (a streaming pass: the loads of
  // several waves per SIMD cover the memory latency)
  const size_t work = aligned ? n4 + 3 : n;
  const size_t blocks = std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 2048));
  hipLaunchKernelGGL(k_mask_apply, dim3((unsigned)blocks), dim3(kBlock), 0, st, buf, mask, n4, n, done);
}

}  // namespace unires
