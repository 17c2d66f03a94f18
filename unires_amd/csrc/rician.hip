// rician.hip - the Rician data term of a magnitude observation (sett.noise_model = 'rician').  With
// mu = e . (A y), z = tau x mu, the negative log-likelihood of a voxel is 1/2 tau (x - mu)^2 + c(z) - log(tau x),
// c(z) = (z - |z|) - log i0e(|z|).  log I0 is convex: its tangent at the current z majorises the voxel's term by
// 1/2 tau (mu - x R(z))^2 + const, R = I1 / I0 - the y-update as it stands on the effective observation x R(z).
//   k_rician_rows / k_rician_z (+ gain.hip's finish): one pass over x and A y that writes the effective observation
//     and / or the per-slice sums of g c(z) the objective adds to the Gaussian term.  k_rigid_terms_e_rows' /
//     k_rigid_terms_e_z's walk, grids and shares: every voxel is visited by one thread, once; no atomics.
//   k_rigid_terms_r_rows / k_rigid_terms_r_z (+ gain.hip's finish): the rigid Gauss-Newton step of a Rician repeat in
//     one pass (sett.rician_gn) - the slice sums of x - e . A y, the sums of g c(z), and the residual
//     t[s] (e . A y - x R(z)); neither e . A y nor x R(z) is stored.
#include "rician.hpp"

#include "gain.hpp"
#include "slice.hpp"

// No contraction: tests/rician64.py restates the float32 arithmetic below operation by operation.
#pragma clang fp contract(off)

namespace unires {

namespace {

// I0 and I1 by the handbook polynomials (Abramowitz & Stegun 9.8.1 - 9.8.4), t = z / 3.75:
//   |z| <= 3.75:  I0 = P0(t^2), I1 = z P1(t^2);   beyond:  sqrt(z) e^-z I0 = Q0(1 / t), sqrt(z) e^-z I1 = Q1(1 / t).
// In R = I1 / I0 the exponentials cancel, and i0e = e^-z I0 needs none: -log i0e = z - log P0, or -log(Q0 / sqrt(z)).
constexpr float kRicianBranch = 3.75f;

__device__ __forceinline__ float rician_p0(float s) {
  float p = 0.0045813f;
  p = p * s + 0.0360768f;
  p = p * s + 0.2659732f;
  p = p * s + 1.2067492f;
  p = p * s + 3.0899424f;
  p = p * s + 3.5156229f;
  return p * s + 1.0f;
}

__device__ __forceinline__ float rician_p1(float s) {
  float p = 0.00032411f;
  p = p * s + 0.00301532f;
  p = p * s + 0.02658733f;
  p = p * s + 0.15084934f;
  p = p * s + 0.51498869f;
  p = p * s + 0.87890594f;
  return p * s + 0.5f;
}

__device__ __forceinline__ float rician_q0(float u) {
  float p = 0.00392377f;
  p = p * u - 0.01647633f;
  p = p * u + 0.02635537f;
  p = p * u - 0.02057706f;
  p = p * u + 0.00916281f;
  p = p * u - 0.00157565f;
  p = p * u + 0.00225319f;
  p = p * u + 0.01328592f;
  return p * u + 0.39894228f;
}

__device__ __forceinline__ float rician_q1(float u) {
  float p = -0.00420059f;
  p = p * u + 0.01787654f;
  p = p * u - 0.02895312f;
  p = p * u + 0.02282967f;
  p = p * u - 0.01031555f;
  p = p * u + 0.00163801f;
  p = p * u - 0.00362018f;
  p = p * u - 0.03988024f;
  return p * u + 0.39894228f;
}

// R(|z|) in [0, 1] and, with C, c(z) of one z.  Both forms are evaluated and one select picks: the form not picked
// may hold inf or NaN (P0 of a huge z, Q0 of 1 / 0), which the select drops.  a = inf: Q1(0) / Q0(0) = 1 exactly, and
// c = z (+-inf, not inf - inf).
template <bool C>
__device__ __forceinline__ float rician_ratio(float z, float &c) {
  const float a = fabsf(z);
  const bool small = a <= kRicianBranch;
  const float t = a / kRicianBranch, s = t * t;
  const float u = kRicianBranch / a;
  const float p0 = rician_p0(s), q0 = rician_q0(u);
  const float rs = (a * rician_p1(s)) / p0, rl = rician_q1(u) / q0;
  if (C) {
    // -log i0e(a): a - log P0(s), or -log(Q0 / sqrt(a)); then (z - a), 0 or 2 z, exact
    const float l = logf(small ? p0 : q0 / sqrtf(a));
    const float c0 = (small ? a : 0.f) - l;
    c = a == INFINITY ? z : c0 + (z - a);
  }
  return fminf(small ? rs : rl, 1.f);
}

// One voxel: p = fl32(e ay) (k_slice_apply's product; ev = 1 without gains: ay itself), z = fl32(fl32(tau x) p).
template <bool G, bool OUT, bool SUMS>
__device__ __forceinline__ void rician_term(const float *__restrict__ x, const float *ay, const float *__restrict__ g,
                                            float *xt, size_t o, float ev, float tau, double &acc) {
  const float xv = x[o], p = ay[o] * ev;
  const float z = (tau * xv) * p;
  float c = 0.f;
  const float r = rician_ratio<SUMS>(z, c);
  if (SUMS) acc += G ? __dmul_rn((double)g[o], (double)c) : (double)c;
  if (OUT) xt[o] = xv == 0.f ? 0.f : xv * copysignf(r, z);
}

template <bool G, bool OUT, bool SUMS>
__global__ void __launch_bounds__(kBlock) k_rician_rows(const float *__restrict__ x, const float *ay,
                                                        const float *__restrict__ g, const float *__restrict__ e,
                                                        float *xt, Dim3i d, int axis, float tau,
                                                        double *__restrict__ part) {
  const size_t s = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  const float ev = e ? e[s] : 1.f;
  double acc = 0.0;
  if (axis == 0) {
    const size_t P = (size_t)d.y * d.z, base = s * P;
    for (size_t i = b * kBlock + threadIdx.x; i < P; i += B * kBlock)
      rician_term<G, OUT, SUMS>(x, ay, g, xt, base + i, ev, tau, acc);
  } else {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (size_t i = b * (kBlock / kWave) + wave; i < (size_t)d.x; i += B * (kBlock / kWave)) {
      const size_t base = (i * d.y + s) * d.z;
      for (int k = lane; k < d.z; k += kWave) rician_term<G, OUT, SUMS>(x, ay, g, xt, base + k, ev, tau, acc);
    }
  }
  if (SUMS) {
    const double t = block_sum(acc);
    if (threadIdx.x == 0) part[s * B + b] = t;
  }
}

template <bool G, bool OUT, bool SUMS>
__global__ void __launch_bounds__(kBlock) k_rician_z(const float *__restrict__ x, const float *ay,
                                                     const float *__restrict__ g, const float *__restrict__ e, float *xt,
                                                     Dim3i d, float tau, double *__restrict__ part) {
  __shared__ double s_acc[kBlock / kWave][kWave];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const size_t z = (size_t)blockIdx.x * kWave + lane, b = blockIdx.y, B = gridDim.y;
  const size_t R = (size_t)d.x * d.y, S = d.z;
  double acc = 0.0;
  if (z < S) {
    const float ev = e ? e[z] : 1.f;
    for (size_t r = b * (kBlock / kWave) + wave; r < R; r += B * (kBlock / kWave))
      rician_term<G, OUT, SUMS>(x, ay, g, xt, r * S + z, ev, tau, acc);
  }
  if (SUMS) {
    s_acc[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && z < S) {
      double t = s_acc[0][lane];
      for (int w = 1; w < kBlock / kWave; ++w) t += s_acc[w][lane];
      part[z * B + b] = t;
    }
  }
}

// One voxel of the rigid Gauss-Newton step of a Rician repeat (sett.rician_gn): rician_term's p, z, R and c, with
// gain.hip's terms_e_term around them.  Its terms of the slice's SSE and count are slice_term's / voxel_term's on p (E:
// terms_e_term's), its term of L_s is rician_term's, and with OUT its residual is resid_term's / resid_term_g's on
// (x~, p), x~ = fl32(x R(z)) rician_term's effective observation, with the slice's factor tv for u - tab: the repeat
// has u or e; without either the factor 1 is not multiplied in, as those two do not.  The mask reads the true x: x~
// may underflow to 0 where x is not.  The derivative of the voxel's term W [1/2 tau (x - p)^2 + c(tau x p)] in A y
// is tau times this residual.  The store goes to the offset just read: out may be ay.
template <bool G, bool E, bool OUT>
__device__ __forceinline__ void terms_r_term(const float *__restrict__ x, const float *ay, const float *__restrict__ g,
                                             float *out, size_t o, float ev, float tv, bool tab, float tau, double &acc,
                                             double &cnt, double &lik) {
  const float xv = x[o], av = ay[o], p = E ? av * ev : av;
  const float gv = G ? g[o] : 1.f;
  const float z = (tau * xv) * p;
  float c = 0.f;
  const float r = rician_ratio<true>(z, c);
  lik += G ? __dmul_rn((double)gv, (double)c) : (double)c;
  if (xv != 0.f) {
    const float d = xv - p, dd = d * d;
    acc += (double)(G ? gv * dd : dd);
    cnt += G ? (double)gv : 1.0;
  }
  if (OUT) {
    float v = 0.f;
    if (xv != 0.f && p != 0.f) {
      const float xt = xv * copysignf(r, z);
      const float d = p - xt;
      if (tab)
        v = G ? (float)(((double)gv * (double)tv) * (double)d) : tv * d;
      else
        v = G ? gv * d : d;
    }
    out[o] = v;
  }
}

// t[s] = fl32(fl64(u[s]) fl64(e[s])), 1 where a table is missing: gain.hip's terms_e_factor with either table optional
__device__ __forceinline__ float terms_r_factor(const float *__restrict__ u, const float *__restrict__ e, size_t s) {
  if (u && e) return (float)((double)u[s] * (double)e[s]);
  return u ? u[s] : (e ? e[s] : 1.f);
}

// k_rigid_terms_e_rows' walk, grid and shares (axes 0 and 1) - k_slice_sums_rows', k_voxel_sums_rows' and k_rician_rows'
// too - with the Rician terms in the same pass: e[s] and t[s] are uniform over the workgroup.  Every voxel is visited
// by exactly one thread, once; three block sums in place of two, each its own tree.
template <bool G, bool E, bool OUT>
__global__ void __launch_bounds__(kBlock) k_rigid_terms_r_rows(const float *__restrict__ x, const float *ay,
                                                               const float *__restrict__ g, const float *__restrict__ u,
                                                               const float *__restrict__ e, float *out, Dim3i d, int axis,
                                                               float tau, double *__restrict__ part) {
  const size_t s = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  const size_t S = axis == 0 ? d.x : d.y;
  const float ev = E ? e[s] : 1.f, tv = terms_r_factor(u, E ? e : nullptr, s);
  const bool tab = E || u;
  double acc = 0.0, cnt = 0.0, lik = 0.0;
  if (axis == 0) {
    const size_t P = (size_t)d.y * d.z, base = s * P;
    for (size_t i = b * kBlock + threadIdx.x; i < P; i += B * kBlock)
      terms_r_term<G, E, OUT>(x, ay, g, out, base + i, ev, tv, tab, tau, acc, cnt, lik);
  } else {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (size_t i = b * (kBlock / kWave) + wave; i < (size_t)d.x; i += B * (kBlock / kWave)) {
      const size_t base = (i * d.y + s) * d.z;
      for (int k = lane; k < d.z; k += kWave)
        terms_r_term<G, E, OUT>(x, ay, g, out, base + k, ev, tv, tab, tau, acc, cnt, lik);
    }
  }
  const double ts = block_sum(acc), tc = block_sum(cnt), tl = block_sum(lik);
  if (threadIdx.x == 0) part[s * B + b] = ts, part[(S + s) * B + b] = tc, part[(2 * S + s) * B + b] = tl;
}

// k_rigid_terms_e_z's walk, grid and shares (axis 2): a lane keeps its z, and so its e and t.  The four waves' sums
// of a z are added in wave order through LDS (a lane's own column of doubles: 6 KiB in all).
template <bool G, bool E, bool OUT>
__global__ void __launch_bounds__(kBlock) k_rigid_terms_r_z(const float *__restrict__ x, const float *ay,
                                                            const float *__restrict__ g, const float *__restrict__ u,
                                                            const float *__restrict__ e, float *out, Dim3i d, float tau,
                                                            double *__restrict__ part) {
  __shared__ double s_acc[kBlock / kWave][kWave];
  __shared__ double s_cnt[kBlock / kWave][kWave];
  __shared__ double s_lik[kBlock / kWave][kWave];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const size_t z = (size_t)blockIdx.x * kWave + lane, b = blockIdx.y, B = gridDim.y;
  const size_t R = (size_t)d.x * d.y, S = d.z;
  const bool tab = E || u;
  double acc = 0.0, cnt = 0.0, lik = 0.0;
  if (z < S) {
    const float ev = E ? e[z] : 1.f, tv = terms_r_factor(u, E ? e : nullptr, z);
    for (size_t r = b * (kBlock / kWave) + wave; r < R; r += B * (kBlock / kWave))
      terms_r_term<G, E, OUT>(x, ay, g, out, r * S + z, ev, tv, tab, tau, acc, cnt, lik);
  }
  s_acc[wave][lane] = acc, s_cnt[wave][lane] = cnt, s_lik[wave][lane] = lik;
  __syncthreads();
  if (wave == 0 && z < S) {
    double t = s_acc[0][lane], c = s_cnt[0][lane], l = s_lik[0][lane];
    for (int w = 1; w < kBlock / kWave; ++w) t += s_acc[w][lane], c += s_cnt[w][lane], l += s_lik[w][lane];
    part[z * B + b] = t, part[(S + z) * B + b] = c, part[(2 * S + z) * B + b] = l;
  }
}

}  // namespace

void launch_rigid_terms_r(const float *x, const float *ay, const float *g, const float *u, const float *e, Dim3i d,
                          int axis, float tau, double *part, double *sums, float *out, hipStream_t st) {
  const int B = slice_sums_parts(d, axis);
  const size_t S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  const dim3 grid(axis == 2 ? (unsigned)((S + kWave - 1) / kWave) : (unsigned)S, B);
#define UNIRES_TERMS_R(G, E, OUT)                                                                                      \
  do {                                                                                                                 \
    if (axis == 2)                                                                                                     \
      hipLaunchKernelGGL((k_rigid_terms_r_z<G, E, OUT>), grid, dim3(kBlock), 0, st, x, ay, g, u, e, out, d, tau,       \
                         part);                                                                                        \
    else                                                                                                               \
      hipLaunchKernelGGL((k_rigid_terms_r_rows<G, E, OUT>), grid, dim3(kBlock), 0, st, x, ay, g, u, e, out, d, axis,   \
                         tau, part);                                                                                   \
  } while (0)
#define UNIRES_TERMS_R_GE(G, E)                                                                                        \
  do {                                                                                                                 \
    if (out)                                                                                                           \
      UNIRES_TERMS_R(G, E, true);                                                                                      \
    else                                                                                                               \
      UNIRES_TERMS_R(G, E, false);                                                                                     \
  } while (0)
  if (g && e)
    UNIRES_TERMS_R_GE(true, true);
  else if (g)
    UNIRES_TERMS_R_GE(true, false);
  else if (e)
    UNIRES_TERMS_R_GE(false, true);
  else
    UNIRES_TERMS_R_GE(false, false);
#undef UNIRES_TERMS_R_GE
#undef UNIRES_TERMS_R
  launch_gain_finish(part, B, 3 * S, sums, st);
}

void launch_rician_terms(const float *x, const float *ay, const float *g, const float *e, Dim3i d, int axis, float tau,
                         float *xt, double *part, double *sums, hipStream_t st) {
  const int B = slice_sums_parts(d, axis);
  const size_t S = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
  const dim3 grid(axis == 2 ? (unsigned)((S + kWave - 1) / kWave) : (unsigned)S, B);
#define UNIRES_RICIAN(G, OUT, SUMS)                                                                                    \
  do {                                                                                                                 \
    if (axis == 2)                                                                                                     \
      hipLaunchKernelGGL((k_rician_z<G, OUT, SUMS>), grid, dim3(kBlock), 0, st, x, ay, g, e, xt, d, tau, part);        \
    else                                                                                                               \
      hipLaunchKernelGGL((k_rician_rows<G, OUT, SUMS>), grid, dim3(kBlock), 0, st, x, ay, g, e, xt, d, axis, tau,      \
                         part);                                                                                        \
  } while (0)
  if (!sums)  // (g weights the sums only)
    UNIRES_RICIAN(false, true, false);
  else if (g && xt)
    UNIRES_RICIAN(true, true, true);
  else if (g)
    UNIRES_RICIAN(true, false, true);
  else if (xt)
    UNIRES_RICIAN(false, true, true);
  else
    UNIRES_RICIAN(false, false, true);
#undef UNIRES_RICIAN
  if (sums) launch_gain_finish(part, B, S, sums, st);
}

}  // namespace unires
