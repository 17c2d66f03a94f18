// gain.hip - per-slice intensity gains of an observation (sett.slice_gain, _input.slice_gain): the data term of repeat
// n becomes 1/2 tau_n sum_v W(v) (x_n(v) - e_n[s(v)] (A_n y)(v))^2 + 1/2 kappa_n sum_s (e_s - 1)^2, W = g . u . [x != 0].
//   k_gain_sums_rows / k_gain_sums_z + k_gain_finish: P_s = sum W x a, Q_s = sum W a^2 and the effective count sum W of
//     every slice, a = A y without gains - what the gains are estimated from (e_s = (tau P_s + kappa) / (tau Q_s + kappa),
//     _update.gain_rule).  Not on any solve's path: once per observation and ADMM iteration.
//   k_gain_compose: the two per-slice tables of a gained repeat, u e^2 for the pass between the halves of A^T A and u e
//     for the right-hand side; the passes themselves are slice.hip's and voxel.hip's, which take either table where they
//     took u.
//   k_rigid_terms_e_rows / k_rigid_terms_e_z + k_gain_finish: the rigid Gauss-Newton step of a gained repeat in one pass
//     (sett.gain_gn) - the slice sums of x - e . A y and the residual t[s] (e . A y - x), e . A y never stored.
#include <algorithm>

#include "gain.hpp"
#include "slice.hpp"

namespace unires {

namespace {

// one term of a slice's three sums: float32 products (k_scaling_sums' terms), W = g uw and the summands W t in float64,
// each one multiplication rounded on its own - no fused multiply-add, whose sum would round differently
template <bool G>
__device__ __forceinline__ void gain_term(const float *__restrict__ x, const float *__restrict__ ay,
                                          const float *__restrict__ g, size_t o, double uw, double &p, double &q,
                                          double &c) {
#pragma clang fp contract(off)
  const float xv = x[o];
  if (xv != 0.f) {
    const float av = ay[o];
    const double W = G ? __dmul_rn((double)g[o], uw) : uw;
    const double tp = __dmul_rn(W, (double)__fmul_rn(xv, av)), tq = __dmul_rn(W, (double)__fmul_rn(av, av));
    p += tp, q += tq, c += W;
  }
}

// Slices along axis 0 (a slice is a contiguous plane) or axis 1 (a slice is one z-row of every x), k_slice_sums_rows'
// walk: workgroup (., b) takes the b-th share of slice s - along axis 0 consecutive threads read consecutive voxels
// of the plane, along axis 1 a wave takes a whole z-row at a time - and writes its three sums to part[s][b],
// part[S + s][b], part[2 S + s][b].  The grid's x holds at most kGainGroups slices at a time: a workgroup goes on to
// slice s + gridDim.x.  Every thread's share, block_sum's tree and k_gain_finish's order over the shares are fixed: no
// atomics.
constexpr size_t kGainGroups = 2048;

template <bool G>
__global__ void __launch_bounds__(kBlock) k_gain_sums_rows(const float *__restrict__ x, const float *__restrict__ ay,
                                                           const float *__restrict__ g, const float *__restrict__ u,
                                                           Dim3i d, int axis, double *__restrict__ part) {
  const size_t b = blockIdx.y, B = gridDim.y;
  const size_t S = axis == 0 ? d.x : d.y;
  for (size_t s = blockIdx.x; s < S; s += gridDim.x) {  // (uniform over the workgroup: block_sum's barriers are met by all)
    const double uw = u ? (double)u[s] : 1.0;
    double p = 0.0, q = 0.0, c = 0.0;
    if (axis == 0) {
      const size_t P = (size_t)d.y * d.z, base = s * P;
      for (size_t e = b * kBlock + threadIdx.x; e < P; e += B * kBlock) gain_term<G>(x, ay, g, base + e, uw, p, q, c);
    } else {
      const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
      for (size_t i = b * (kBlock / kWave) + wave; i < (size_t)d.x; i += B * (kBlock / kWave)) {
        const size_t base = (i * d.y + s) * d.z;
        for (int k = lane; k < d.z; k += kWave) gain_term<G>(x, ay, g, base + k, uw, p, q, c);
      }
    }
    const double tp = block_sum(p), tq = block_sum(q), tc = block_sum(c);
    if (threadIdx.x == 0) part[s * B + b] = tp, part[(S + s) * B + b] = tq, part[(2 * S + s) * B + b] = tc;
  }
}

// Slices along axis 2, the fastest, k_slice_sums_z's walk: a lane keeps its z - and so its slice and its u - while the
// workgroup's waves walk the z-rows (coalesced: no gathers a row apart).  The four waves' sums of a z are added in wave
// order through LDS (a lane's own column of doubles: no bank is shared inside a half-wave).
template <bool G>
__global__ void __launch_bounds__(kBlock) k_gain_sums_z(const float *__restrict__ x, const float *__restrict__ ay,
                                                        const float *__restrict__ g, const float *__restrict__ u,
                                                        Dim3i d, double *__restrict__ part) {
  __shared__ double s_p[kBlock / kWave][kWave];
  __shared__ double s_q[kBlock / kWave][kWave];
  __shared__ double s_c[kBlock / kWave][kWave];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const size_t b = blockIdx.y, B = gridDim.y;
  const size_t R = (size_t)d.x * d.y, S = d.z, groups = (S + kWave - 1) / kWave;
  for (size_t zb = blockIdx.x; zb < groups; zb += gridDim.x) {  // (uniform over the workgroup)
    const size_t z = zb * kWave + lane;
    double p = 0.0, q = 0.0, c = 0.0;
    if (z < S) {
      const double uw = u ? (double)u[z] : 1.0;
      for (size_t r = b * (kBlock / kWave) + wave; r < R; r += B * (kBlock / kWave))
        gain_term<G>(x, ay, g, r * S + z, uw, p, q, c);
    }
    s_p[wave][lane] = p, s_q[wave][lane] = q, s_c[wave][lane] = c;
    __syncthreads();
    if (wave == 0 && z < S) {
      double tp = s_p[0][lane], tq = s_q[0][lane], tc = s_c[0][lane];
      for (int w = 1; w < kBlock / kWave; ++w) tp += s_p[w][lane], tq += s_q[w][lane], tc += s_c[w][lane];
      part[z * B + b] = tp, part[(S + z) * B + b] = tq, part[(2 * S + z) * B + b] = tc;
    }
    __syncthreads();  // (the next group's sums overwrite the LDS wave 0 has just read)
  }
}

// out[c] = sum_b part[c][b]: k_slice_finish's order - a wave per entry, lane l adds the shares l, l + 64, ... in index
// order, wave_sum's fixed tree adds the lanes
__global__ void __launch_bounds__(kBlock) k_gain_finish(const double *__restrict__ part, int B, size_t ncols,
                                                        double *__restrict__ out) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (size_t c = (size_t)blockIdx.x * (kBlock / kWave) + wave; c < ncols; c += (size_t)gridDim.x * (kBlock / kWave)) {
    double a = 0.0;
    for (int b = lane; b < B; b += kWave) a += part[c * B + b];
    a = wave_sum(a);
    if (lane == 0) out[c] = a;
  }
}

// One workgroup: a few hundred slices at the most.  Plain stores; u e in float64 is exact (24 + 24 significant bits).
__global__ void __launch_bounds__(kBlock) k_gain_compose(const float *__restrict__ u, const float *__restrict__ e, int S,
                                                         float *__restrict__ w_mat, float *__restrict__ w_rhs) {
#pragma clang fp contract(off)
  for (int s = threadIdx.x; s < S; s += kBlock) {
    const double ev = (double)e[s], ue = __dmul_rn(u ? (double)u[s] : 1.0, ev);
    w_rhs[s] = (float)ue;
    w_mat[s] = (float)__dmul_rn(ue, ev);
  }
}

// One voxel of the rigid Gauss-Newton step of a gained repeat: p = fl32(e ay) (k_slice_apply's product) stays in a
// register.  Its term of the slice's sums is slice_term's on p - voxel_term's with G, and the count as a double, which
// holds the integers slice_term counts exactly - and, with OUT, its residual is resid_term's / resid_term_g<true>'s on p
// with the slice's factor tv = fl32(u e) for u.  The two differences are taken separately: x - p and p - x differ in
// the sign of a zero.  The store goes to the offset just read: out may be ay.
template <bool G, bool OUT>
__device__ __forceinline__ void terms_e_term(const float *__restrict__ x, const float *ay, const float *__restrict__ g,
                                             float *out, size_t o, float ev, float tv, double &acc, double &cnt) {
#pragma clang fp contract(off)
  // (the product and the differences it feeds are written out under the pragma: __fmul_rn and __fsub_rn are plain
  // operators in a header compiled with contraction on, and a product that feeds a difference would fuse through them)
  const float xv = x[o], p = ay[o] * ev;
  const float gv = G ? g[o] : 1.f;
  if (xv != 0.f) {
    const float r = xv - p, rr = __fmul_rn(r, r);
    acc += (double)(G ? __fmul_rn(gv, rr) : rr);
    cnt += G ? (double)gv : 1.0;
  }
  if (OUT) {
    float v = 0.f;
    if (xv != 0.f && p != 0.f) {
      const float d = p - xv;
      v = G ? (float)__dmul_rn(__dmul_rn((double)gv, (double)tv), (double)d) : __fmul_rn(tv, d);
    }
    out[o] = v;
  }
}

// t[s] = fl32(fl64(u[s]) fl64(e[s])), exact in float64 and rounded once: k_gain_compose's w_rhs[s]
__device__ __forceinline__ float terms_e_factor(const float *__restrict__ u, float ev, size_t s) {
#pragma clang fp contract(off)
  return u ? (float)__dmul_rn((double)u[s], (double)ev) : ev;
}

// k_slice_sums_rows' / k_voxel_sums_rows' walk, grid and shares (axes 0 and 1), with the gain and the residual in the
// same pass: e[s] and t[s] are uniform over the workgroup.  Every voxel is visited by exactly one thread, once.
template <bool G, bool OUT>
__global__ void __launch_bounds__(kBlock) k_rigid_terms_e_rows(const float *__restrict__ x, const float *ay,
                                                               const float *__restrict__ g, const float *__restrict__ u,
                                                               const float *__restrict__ e, float *out, Dim3i d, int axis,
                                                               double *__restrict__ part) {
  const size_t s = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  const size_t S = axis == 0 ? d.x : d.y;
  const float ev = e[s], tv = terms_e_factor(u, ev, s);
  double acc = 0.0, cnt = 0.0;
  if (axis == 0) {
    const size_t P = (size_t)d.y * d.z, base = s * P;
    for (size_t i = b * kBlock + threadIdx.x; i < P; i += B * kBlock)
      terms_e_term<G, OUT>(x, ay, g, out, base + i, ev, tv, acc, cnt);
  } else {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (size_t i = b * (kBlock / kWave) + wave; i < (size_t)d.x; i += B * (kBlock / kWave)) {
      const size_t base = (i * d.y + s) * d.z;
      for (int k = lane; k < d.z; k += kWave) terms_e_term<G, OUT>(x, ay, g, out, base + k, ev, tv, acc, cnt);
    }
  }
  const double ts = block_sum(acc), tc = block_sum(cnt);
  if (threadIdx.x == 0) part[s * B + b] = ts, part[(S + s) * B + b] = tc;
}

// k_slice_sums_z's / k_voxel_sums_z's walk, grid and shares (axis 2): a lane keeps its z, and so its e and t.
template <bool G, bool OUT>
__global__ void __launch_bounds__(kBlock) k_rigid_terms_e_z(const float *__restrict__ x, const float *ay,
                                                            const float *__restrict__ g, const float *__restrict__ u,
                                                            const float *__restrict__ e, float *out, Dim3i d,
                                                            double *__restrict__ part) {
  __shared__ double s_acc[kBlock / kWave][kWave];
  __shared__ double s_cnt[kBlock / kWave][kWave];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const size_t z = (size_t)blockIdx.x * kWave + lane, b = blockIdx.y, B = gridDim.y;
  const size_t R = (size_t)d.x * d.y, S = d.z;
  double acc = 0.0, cnt = 0.0;
  if (z < S) {
    const float ev = e[z], tv = terms_e_factor(u, ev, z);
    for (size_t r = b * (kBlock / kWave) + wave; r < R; r += B * (kBlock / kWave))
      terms_e_term<G, OUT>(x, ay, g, out, r * S + z, ev, tv, acc, cnt);
  }
  s_acc[wave][lane] = acc, s_cnt[wave][lane] = cnt;
  __syncthreads();
  if (wave == 0 && z < S) {
    double t = s_acc[0][lane], c = s_cnt[0][lane];
    for (int w = 1; w < kBlock / kWave; ++w) t += s_acc[w][lane], c += s_cnt[w][lane];
    part[z * B + b] = t, part[(S + z) * B + b] = c;
  }
}

}  // namespace

void launch_gain_finish(const double *part, int B, size_t ncols, double *out, hipStream_t st) {
  const size_t blocks = std::min<size_t>((ncols + kBlock / kWave - 1) / (kBlock / kWave), 4096);
  hipLaunchKernelGGL(k_gain_finish, dim3((unsigned)blocks), dim3(kBlock), 0, st, part, B, ncols, out);
}

void launch_rigid_terms_e(const float *x, const float *ay, const float *g, const float *u, const float *e, Dim3i d,
                          int axis, double *part, double *sums, float *out, hipStream_t st) {
  const int B = slice_sums_parts(d, axis);
  const size_t S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  const dim3 grid(axis == 2 ? (unsigned)((S + kWave - 1) / kWave) : (unsigned)S, B);
#define UNIRES_TERMS_E(G, OUT)                                                                                         \
  do {                                                                                                                 \
    if (axis == 2)                                                                                                     \
      hipLaunchKernelGGL((k_rigid_terms_e_z<G, OUT>), grid, dim3(kBlock), 0, st, x, ay, g, u, e, out, d, part);        \
    else                                                                                                               \
      hipLaunchKernelGGL((k_rigid_terms_e_rows<G, OUT>), grid, dim3(kBlock), 0, st, x, ay, g, u, e, out, d, axis,      \
                         part);                                                                                        \
  } while (0)
  if (g && out)
    UNIRES_TERMS_E(true, true);
  else if (g)
    UNIRES_TERMS_E(true, false);
  else if (out)
    UNIRES_TERMS_E(false, true);
  else
    UNIRES_TERMS_E(false, false);
#undef UNIRES_TERMS_E
  launch_gain_finish(part, B, 2 * S, sums, st);
}

void launch_gain_sums(const float *x, const float *ay, const float *g, const float *u, Dim3i d, int axis, double *part,
                      double *out, hipStream_t st) {
  const int B = slice_sums_parts(d, axis);  // (with more than kGainGroups groups: 1)
  const size_t S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  if (axis == 2) {
    const dim3 grid((unsigned)std::min<size_t>((S + kWave - 1) / kWave, kGainGroups), B);
    if (g)
      hipLaunchKernelGGL(k_gain_sums_z<true>, grid, dim3(kBlock), 0, st, x, ay, g, u, d, part);
    else
      hipLaunchKernelGGL(k_gain_sums_z<false>, grid, dim3(kBlock), 0, st, x, ay, g, u, d, part);
  } else {
    const dim3 grid((unsigned)std::min<size_t>(S, kGainGroups), B);
    if (g)
      hipLaunchKernelGGL(k_gain_sums_rows<true>, grid, dim3(kBlock), 0, st, x, ay, g, u, d, axis, part);
    else
      hipLaunchKernelGGL(k_gain_sums_rows<false>, grid, dim3(kBlock), 0, st, x, ay, g, u, d, axis, part);
  }
  launch_gain_finish(part, B, 3 * S, out, st);
}

void launch_gain_compose(const float *u, const float *e, int S, float *w_mat, float *w_rhs, hipStream_t st) {
  hipLaunchKernelGGL(k_gain_compose, dim3(1), dim3(kBlock), 0, st, u, e, S, w_mat, w_rhs);
}

}  // namespace unires
