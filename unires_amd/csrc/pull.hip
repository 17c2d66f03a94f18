// pull.hip - the affine pulls: trilinear (k_pull), label vote (k_warp_label), nearest neighbour (k_pull_nearest) and
// the spatial gradient of the trilinear sample (k_pull_grad), and the support of the trilinear pull under a weight
// map (k_pull_support).
//
// Layout: float32 volumes, (X,Y,Z) C-contiguous, Z fastest.  Every kernel puts
// the 64 lanes of a wave along Z so that HBM/L2 requests are coalesced.
// Launch shape: block (64,4,1) -> grid (ceil(Z/64), ceil(Y/4), X).
#include "pull.hpp"

namespace unires {

// --------------------------------------------------------------------------
// pull: dst[g] = mask(g) * sum_8 w_c * src[corner_c(M g)]
// (nitorch grid_pull linear / zero / extrapolate=False)
// --------------------------------------------------------------------------
constexpr int kPullChunksMax = 4;  // z chunks of 64 per thread: up to 16 eight-byte loads in flight

// block = 4 waves = 4 consecutive grid rows j (same i); each lane takes kPullChunks grid-z
// positions 64 apart.  Blocks whose whole footprint is inside the volume (all but a thin
// shell) take the interior path.
// kPullChunks = chunks per thread, chosen so that the last one is not mostly idle lanes
// (a 181-long row takes 3 chunks, not 4)
template <int kPullChunks>
__global__ void __launch_bounds__(kBlock) k_pull(const float *__restrict__ src, Dim3i sd, Affine A,
                                                 float *__restrict__ dst, Dim3i gd, float tol,
                                                 const int *__restrict__ done) {
  if (done && *done) return;
  const int lane = threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  const int i = blockIdx.z;
  const int kbase = blockIdx.x * (kWave * kPullChunks);
  if (j >= gd.y) return;
  const RowBase rb = affine_row(A, (float)i, (float)j);
  float *row = dst + ((size_t)i * gd.y + j) * gd.z;
  const unsigned ny = sd.y, nz = sd.z, nynz = ny * nz;
  const float bx = (float)(sd.x - 1), by = (float)(sd.y - 1), bz = (float)(sd.z - 1);
  float g[kPullChunks][3];
  bool inside = sd.z >= 2 && fits_fast_index(sd);
#pragma unroll
  for (int u = 0; u < kPullChunks; ++u) {
    const int k = min(kbase + u * kWave + lane, gd.z - 1);
    affine_along(A, rb, (float)k, g[u][0], g[u][1], g[u][2]);
    inside = inside && g[u][0] >= 0.f && g[u][0] < bx && g[u][1] >= 0.f && g[u][1] < by &&
             g[u][2] >= 0.f && g[u][2] < bz;
  }
  if (__all(inside)) {  // every corner of every sample of this wave is inside the volume
#pragma unroll
    for (int u = 0; u < kPullChunks; ++u) {
      const int k = kbase + u * kWave + lane;
      const float v = pull_interior(src, ny, nz, nynz, g[u][0], g[u][1], g[u][2]);
      if (k < gd.z) row[k] = v;
    }
    return;
  }
  PullLoads L[kPullChunks];
#pragma unroll
  for (int u = 0; u < kPullChunks; ++u) pull_issue(src, sd, g[u][0], g[u][1], g[u][2], tol, L[u]);
#pragma unroll
  for (int u = 0; u < kPullChunks; ++u) {
    const int k = kbase + u * kWave + lane;
    if (k < gd.z) row[k] = pull_finish(L[u]);
  }
}

// --------------------------------------------------------------------------
// label vote: dst[g] = argmax_u p_u(g), p_u = linear pull of the indicator (label == u)
// (the reference's _warp_label, unires/_core.py:419-436: one pull + one select pass per
// distinct value, ascending, strict '>' against a running best that starts at 0).
// Each output voxel sees at most 8 distinct values among its 8 corners, so one gather decides
// it.  p_u is the float32 sum, in corner order, of the products wx*wy*wz of the corners that
// carry u (every other term of the reference's sum is an exact +0): the same bits as the
// product form of pull_finish / the oracle's loop, so exact ties resolve as the reference
// resolves them - the smallest value among the best wins, and a best of 0 gives 0.
// __fmul_rn / __fadd_rn keep the compiler from contracting the sums into FMAs.
// --------------------------------------------------------------------------
__device__ __forceinline__ float label_vote(const PullLoads &L) {
  const float wxy[4] = {__fmul_rn(L.wx0, L.wy0), __fmul_rn(L.wx0, L.wy1), __fmul_rn(L.wx1, L.wy0),
                        __fmul_rn(L.wx1, L.wy1)};
  const float2 vp[4] = {L.v00, L.v01, L.v10, L.v11};
  float v[8], w[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    v[2 * r] = vp[r].x, w[2 * r] = __fmul_rn(wxy[r], L.wz0);
    v[2 * r + 1] = vp[r].y, w[2 * r + 1] = __fmul_rn(wxy[r], L.wz1);
  }
  bool same = true;
#pragma unroll
  for (int c = 1; c < 8; ++c) same = same && v[c] == v[0];
  if (same) {  // one value at all 8 corners (inside a region): it wins iff any weight is > 0
    bool any = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) any = any || w[c] > 0.f;
    return any ? v[0] : 0.f;
  }
  // slot of corner c = the first corner carrying v[c]; p[d] collects, in corner order, the
  // weights of corners c >= d with v[c] == v[d] (meaningful where d is a first occurrence)
  float p[8];
  bool first[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    p[c] = w[c];
    first[c] = true;
#pragma unroll
    for (int d = 0; d < c; ++d) {
      const bool eq = v[c] == v[d];
      first[c] = first[c] && !eq;
      p[d] = __fadd_rn(p[d], eq ? w[c] : 0.f);
    }
  }
  float bv = 0.f, bp = 0.f;
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const bool win = first[d] && (p[d] > bp || (p[d] == bp && p[d] > 0.f && v[d] < bv));
    bv = win ? v[d] : bv;
    bp = win ? p[d] : bp;
  }
  return bv;
}

// Launch shape and coordinates as k_pull; no interior path (its lerp form rounds differently).
template <int kChunks>
__global__ void __launch_bounds__(kBlock) k_warp_label(const float *__restrict__ label, Dim3i sd,
                                                       Affine A, float *__restrict__ dst, Dim3i gd,
                                                       float tol) {
  const int lane = threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  const int i = blockIdx.z;
  const int kbase = blockIdx.x * (kWave * kChunks);
  if (j >= gd.y) return;
  const RowBase rb = affine_row(A, (float)i, (float)j);
  float *row = dst + ((size_t)i * gd.y + j) * gd.z;
  PullLoads L[kChunks];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int k = min(kbase + u * kWave + lane, gd.z - 1);
    float gx, gy, gz;
    affine_along(A, rb, (float)k, gx, gy, gz);
    pull_issue(label, sd, gx, gy, gz, tol, L[u]);
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int k = kbase + u * kWave + lane;
    if (k < gd.z) row[k] = label_vote(L[u]);
  }
}

// --------------------------------------------------------------------------
// nearest-neighbour pull (grid_pull order 0, zero bound, extrapolate=False):
// dst[g] = src[rint(M g)] if that index is inside the volume and M g is inside the FOV, else 0.
// rintf rounds half-way cases to even, like the oracle's torch.round.
// --------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
    k_pull_nearest(const float *__restrict__ src, Dim3i sd, Affine A, float *__restrict__ dst,
                   Dim3i gd, float tol) {
  const int k = blockIdx.x * kWave + threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  const int i = blockIdx.z;
  if (k >= gd.z || j >= gd.y) return;
  float gx, gy, gz;
  affine_along(A, affine_row(A, (float)i, (float)j), (float)k, gx, gy, gz);
  const float rx = rintf(gx), ry = rintf(gy), rz = rintf(gz);
  // range test on the float index: no int conversion of an out-of-range value
  const bool ok = in_fov(gx, gy, gz, sd, tol) && rx >= 0.f && rx < (float)sd.x && ry >= 0.f &&
                  ry < (float)sd.y && rz >= 0.f && rz < (float)sd.z;
  float v = 0.f;
  if (ok) v = src[((size_t)(int)rx * sd.y + (int)ry) * sd.z + (int)rz];
  dst[((size_t)i * gd.y + j) * gd.z + k] = v;
}

// dst[(i,j,k), 0..2] = gradient of the trilinear sample at A (i,j,k)  (nitorch grid_grad layout)
__global__ void __launch_bounds__(kBlock) k_pull_grad(const float *__restrict__ src, Dim3i sd,
                                                      Affine A, float *__restrict__ dst, Dim3i gd,
                                                      float tol) {
  const int k = blockIdx.x * kWave + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, i = blockIdx.z;
  if (k >= gd.z || j >= gd.y) return;
  float gx, gy, gz, dx, dy, dz;
  affine_point(A, (float)i, (float)j, (float)k, gx, gy, gz);
  pull_grad_sample(src, sd, gx, gy, gz, tol, dx, dy, dz);
  float *o = dst + (((size_t)i * gd.y + j) * gd.z + k) * 3;
  o[0] = dx, o[1] = dy, o[2] = dz;
}

// --------------------------------------------------------------------------
// support of a pull under a weight map g: dst[v] = 1 iff k_pull's sample at v is inside
// the FOV and every corner (floor(c_d), floor(c_d) + 1) of it that lies inside the volume has g > 0.
// A corner outside the volume adds 0 to a zero-bound pull and does not decide; a corner inside it
// decides even at weight 0 (0 x NaN is not 0).  Coordinates and loads are k_pull's own (affine_row /
// affine_along, pull_issue on the map): the floors below are of the same floats.
// --------------------------------------------------------------------------
__device__ __forceinline__ bool support_of(const PullLoads &L, const Dim3i &sd, float gx, float gy, float gz,
                                           float tol) {
  if (!in_fov(gx, gy, gz, sd, tol)) return false;
  const int ix = (int)floorf(gx), iy = (int)floorf(gy), iz = (int)floorf(gz);
  const bool x0 = ix >= 0 && ix < sd.x, x1 = ix + 1 >= 0 && ix + 1 < sd.x;
  const bool y0 = iy >= 0 && iy < sd.y, y1 = iy + 1 >= 0 && iy + 1 < sd.y;
  const bool z0 = iz >= 0 && iz < sd.z, z1 = iz + 1 >= 0 && iz + 1 < sd.z;
  // pull_issue's z pair (b, b + 1): which of its two loads hold the corners iz and iz + 1
  const int b = min(max(iz, 0), max(sd.z - 2, 0));
  const bool px = iz == b ? z0 : (iz == b - 1 ? z1 : false);  // pair.x is a corner inside the volume
  const bool py = iz == b ? z1 : (iz == b + 1 ? z0 : false);  // pair.y likewise
  bool ok = true;
  ok = ok && (!(x0 && y0 && px) || L.v00.x > 0.f) && (!(x0 && y0 && py) || L.v00.y > 0.f);
  ok = ok && (!(x0 && y1 && px) || L.v01.x > 0.f) && (!(x0 && y1 && py) || L.v01.y > 0.f);
  ok = ok && (!(x1 && y0 && px) || L.v10.x > 0.f) && (!(x1 && y0 && py) || L.v10.y > 0.f);
  ok = ok && (!(x1 && y1 && px) || L.v11.x > 0.f) && (!(x1 && y1 && py) || L.v11.y > 0.f);
  return ok;
}

// Launch shape and coordinates as k_pull.
template <int kChunks>
__global__ void __launch_bounds__(kBlock) k_pull_support(const float *__restrict__ g, Dim3i sd, Affine A,
                                                         uint8_t *__restrict__ dst, Dim3i gd, float tol) {
  const int lane = threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  const int i = blockIdx.z;
  const int kbase = blockIdx.x * (kWave * kChunks);
  if (j >= gd.y) return;
  const RowBase rb = affine_row(A, (float)i, (float)j);
  uint8_t *row = dst + ((size_t)i * gd.y + j) * gd.z;
  PullLoads L[kChunks];
  float c[kChunks][3];
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int k = min(kbase + u * kWave + lane, gd.z - 1);
    affine_along(A, rb, (float)k, c[u][0], c[u][1], c[u][2]);
    pull_issue(g, sd, c[u][0], c[u][1], c[u][2], tol, L[u]);
  }
#pragma unroll
  for (int u = 0; u < kChunks; ++u) {
    const int k = kbase + u * kWave + lane;
    if (k < gd.z) row[k] = support_of(L[u], sd, c[u][0], c[u][1], c[u][2], tol) ? 1 : 0;
  }
}

// --------------------------------------------------------------------------
// host launchers
// --------------------------------------------------------------------------
// fewest idle lanes: chunks per thread = the count (<= 4) that wastes least of the row's tail
static int pull_chunks(int nz) {
  int best = kPullChunksMax, waste = 1 << 30;
  for (int c = kPullChunksMax; c >= 1; --c) {
    const int span = kWave * c, w = (nz + span - 1) / span * span - nz;
    if (w < waste) waste = w, best = c;
  }
  return best;
}

void launch_pull(const float *src, Dim3i sd, const Affine &A, float *dst, Dim3i gd, float tol,
                 const int *done, hipStream_t st) {
  const int best = pull_chunks(gd.z);
  const int zspan = kWave * best;
  const dim3 grid((gd.z + zspan - 1) / zspan, (gd.y + 3) / 4, gd.x);
  if (best == 4)
    hipLaunchKernelGGL(k_pull<4>, grid, vol_block(), 0, st, src, sd, A, dst, gd, tol, done);
  else if (best == 3)
    hipLaunchKernelGGL(k_pull<3>, grid, vol_block(), 0, st, src, sd, A, dst, gd, tol, done);
  else if (best == 2)
    hipLaunchKernelGGL(k_pull<2>, grid, vol_block(), 0, st, src, sd, A, dst, gd, tol, done);
  else
    hipLaunchKernelGGL(k_pull<1>, grid, vol_block(), 0, st, src, sd, A, dst, gd, tol, done);
}

void launch_warp_label(const float *label, Dim3i sd, const Affine &A, float *dst, Dim3i gd,
                       float tol, hipStream_t st) {
  const int best = pull_chunks(gd.z);
  const int zspan = kWave * best;
  const dim3 grid((gd.z + zspan - 1) / zspan, (gd.y + 3) / 4, gd.x);
  if (best == 4)
    hipLaunchKernelGGL(k_warp_label<4>, grid, vol_block(), 0, st, label, sd, A, dst, gd, tol);
  else if (best == 3)
    hipLaunchKernelGGL(k_warp_label<3>, grid, vol_block(), 0, st, label, sd, A, dst, gd, tol);
  else if (best == 2)
    hipLaunchKernelGGL(k_warp_label<2>, grid, vol_block(), 0, st, label, sd, A, dst, gd, tol);
  else
    hipLaunchKernelGGL(k_warp_label<1>, grid, vol_block(), 0, st, label, sd, A, dst, gd, tol);
}

void launch_pull_support(const float *g, Dim3i sd, const Affine &A, uint8_t *dst, Dim3i gd, float tol,
                         hipStream_t st) {
  const int best = pull_chunks(gd.z);
  const int zspan = kWave * best;
  const dim3 grid((gd.z + zspan - 1) / zspan, (gd.y + 3) / 4, gd.x);
  if (best == 4)
    hipLaunchKernelGGL(k_pull_support<4>, grid, vol_block(), 0, st, g, sd, A, dst, gd, tol);
  else if (best == 3)
    hipLaunchKernelGGL(k_pull_support<3>, grid, vol_block(), 0, st, g, sd, A, dst, gd, tol);
  else if (best == 2)
    hipLaunchKernelGGL(k_pull_support<2>, grid, vol_block(), 0, st, g, sd, A, dst, gd, tol);
  else
    hipLaunchKernelGGL(k_pull_support<1>, grid, vol_block(), 0, st, g, sd, A, dst, gd, tol);
}

void launch_pull_nearest(const float *src, Dim3i sd, const Affine &A, float *dst, Dim3i gd,
                         float tol, hipStream_t st) {
  hipLaunchKernelGGL(k_pull_nearest, vol_grid(gd), vol_block(), 0, st, src, sd, A, dst, gd, tol);
}

void launch_pull_grad(const float *src, Dim3i sd, const Affine &A, float *dst, Dim3i gd, float tol,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_pull_grad, vol_grid(gd), vol_block(), 0, st, src, sd, A, dst, gd, tol);
}

}  // namespace unires
