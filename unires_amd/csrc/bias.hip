// bias.hip - a smooth multiplicative bias field per observation (sett.bias, _input.bias_coef): the data term
// of repeat n becomes 1/2 tau_n sum_v W(v) (x_n(v) - b(v) mu(v))^2 + 1/2 c^T Lambda c, mu = e . A_n y, W = g . u . [x != 0],
// b = exp(beta), beta = sum_abc c_abc phi_a(i) phi_b(j) phi_c(z) on the observation's grid, phi_m(i) = cos(pi m (2 i + 1) / 2 n).
//   k_bias_field: b from the coefficients, and the two volumes the plan reads for a repeat with a field - its voxel map
//     g b^2 and its effective observation x / b (W b^2 in the matrix, W b x = (W b^2)(x / b) on the right; no hot kernel
//     changes).  The coefficients are folded over the two outer axes once per plane and row: k_z multiply-adds and one exp
//     per voxel.
//   k_bias_proj + k_bias_finish: what the field's Gauss-Newton step is assembled from (_update.bias_step) - the
//     objective sum W r^2, the projection of W m r onto the orders < k and the projection of W m^2 onto the orders
//     < 2 k - 1 (phi_m phi_m' = (phi_|m - m'| + phi_(m + m')) / 2: every entry of the Hessian is 1/8 of eight of its
//     entries), m = b mu, r = m - x.  Not on any solve's path: once per observation and ADMM iteration, and once per
//     line-search candidate for the objective alone.
#include <algorithm>

#include "bias.hpp"

namespace unires {

namespace {

constexpr int kBiasRowsPerGroup = 256;  // rows j of a plane one workgroup of k_bias_field folds and walks

// Workgroup (i, jb): plane i, rows jb * 256 ... of it.  s_e[b][c] = sum_a coef[a][b][c] phi_a(i); s_d[j][c] = sum_b
// s_e[b][c] phi_b(j); a wave takes a row at a time, a lane keeps its z and with it the k.z values phi_c(z).
__global__ void __launch_bounds__(kBlock) k_bias_field(const double *__restrict__ coef, const double *__restrict__ tx,
                                                       const double *__restrict__ ty, const double *__restrict__ tz,
                                                       Dim3i k, Dim3i d, double beta_max, const float *__restrict__ g,
                                                       const float *__restrict__ x, float *__restrict__ b,
                                                       float *__restrict__ gb2, float *__restrict__ xb) {
#pragma clang fp contract(off)
  __shared__ double s_e[kBiasMaxOrder * kBiasMaxOrder];
  __shared__ double s_d[kBiasRowsPerGroup][kBiasMaxOrder];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int i = blockIdx.x, j0 = blockIdx.y * kBiasRowsPerGroup, nj = min(kBiasRowsPerGroup, d.y - j0);
  if ((int)threadIdx.x < k.y * k.z) {
    const int bb = threadIdx.x / k.z, c = threadIdx.x % k.z;
    double acc = 0.0;
    for (int a = 0; a < k.x; ++a) acc += coef[((size_t)a * k.y + bb) * k.z + c] * tx[(size_t)a * d.x + i];
    s_e[bb * k.z + c] = acc;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nj * k.z; t += kBlock) {
    const int jj = t / k.z, c = t % k.z;
    double acc = 0.0;
    for (int bb = 0; bb < k.y; ++bb) acc += s_e[bb * k.z + c] * ty[(size_t)bb * d.y + j0 + jj];
    s_d[jj][c] = acc;
  }
  __syncthreads();
  for (int z = lane; z < d.z; z += kWave) {
    double pz[kBiasMaxOrder];
#pragma unroll
    for (int c = 0; c < kBiasMaxOrder; ++c) pz[c] = c < k.z ? tz[(size_t)c * d.z + z] : 0.0;
    for (int jj = wave; jj < nj; jj += kBlock / kWave) {
      double beta = 0.0;
#pragma unroll
      for (int c = 0; c < kBiasMaxOrder; ++c)
        if (c < k.z) beta += s_d[jj][c] * pz[c];
      beta = beta > beta_max ? beta_max : (beta < -beta_max ? -beta_max : beta);
      const float bv = (float)exp(beta);
      const size_t o = ((size_t)i * d.y + j0 + jj) * d.z + z;
      b[o] = bv;
      if (gb2) gb2[o] = (float)__dmul_rn(__dmul_rn(g ? (double)g[o] : 1.0, (double)bv), (double)bv);
      if (xb) {
        const float xv = x[o];
        xb[o] = xv == 0.f ? 0.f : __fdiv_rn(xv, bv);
      }
    }
  }
}

// Rows of a workgroup's LDS table: the objective, the orders of W m r along y, the orders of W m^2 along y.
constexpr int kRowG = 1, kRowH = 1 + kBiasMaxOrder, kRows = 1 + kBiasMaxOrder + kBiasMaxProj;

// Workgroup (i, zg): plane i, the 64 z of group zg.  Wave w takes the rows j = w, w + 4, ...; a lane keeps its z.  FULL:
// the projections beside the objective (8 + 15 accumulators a lane; orders beyond k.y / q.y multiply by 0 and are not
// stored).  The table rows are padded to 65 doubles: in the fold over z the threads of a wave read different rows at
// one z.
template <bool FULL>
__global__ void __launch_bounds__(kBlock) k_bias_proj(const float *__restrict__ x, const float *__restrict__ mu,
                                                      const float *__restrict__ b, const float *__restrict__ g,
                                                      const float *__restrict__ u, int axis,
                                                      const double *__restrict__ ty, const double *__restrict__ tz,
                                                      Dim3i k, Dim3i q, Dim3i d, double *__restrict__ part) {
#pragma clang fp contract(off)
  constexpr int R = FULL ? kRows : 1;
  __shared__ double s_t[kBlock / kWave][R][kWave + 1];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int i = blockIdx.x, zg = blockIdx.y, ZG = gridDim.y;
  const int z = zg * kWave + lane;
  double obj = 0.0, ag[kBiasMaxOrder], ah[kBiasMaxProj];
#pragma unroll
  for (int m = 0; m < kBiasMaxOrder; ++m) ag[m] = 0.0;
#pragma unroll
  for (int m = 0; m < kBiasMaxProj; ++m) ah[m] = 0.0;
  if (z < d.z) {
    for (int j = wave; j < d.y; j += kBlock / kWave) {
      const size_t o = ((size_t)i * d.y + j) * d.z + z;
      const float xv = x[o];
      if (xv == 0.f) continue;
      const float m = __fmul_rn(b[o], mu[o]);
      const double md = (double)m, r = md - (double)xv;
      const double uw = u ? (double)u[axis == 0 ? i : (axis == 1 ? j : z)] : 1.0;
      const double W = g ? __dmul_rn((double)g[o], uw) : uw;
      obj += __dmul_rn(__dmul_rn(W, r), r);
      if (FULL) {
        const double wm = __dmul_rn(W, md), fg = __dmul_rn(wm, r), fh = __dmul_rn(wm, md);
#pragma unroll
        for (int bb = 0; bb < kBiasMaxOrder; ++bb) ag[bb] += fg * (bb < k.y ? ty[(size_t)bb * d.y + j] : 0.0);
#pragma unroll
        for (int bb = 0; bb < kBiasMaxProj; ++bb) ah[bb] += fh * (bb < q.y ? ty[(size_t)bb * d.y + j] : 0.0);
      }
    }
  }
  s_t[wave][0][lane] = obj;
  if (FULL) {
#pragma unroll
    for (int bb = 0; bb < kBiasMaxOrder; ++bb) s_t[wave][kRowG + bb][lane] = ag[bb];
#pragma unroll
    for (int bb = 0; bb < kBiasMaxProj; ++bb) s_t[wave][kRowH + bb][lane] = ah[bb];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < R * kWave; e += kBlock) {  // (the waves' sums in wave order; an entry has one thread)
    const int row = e / kWave, l = e % kWave;
    double t = s_t[0][row][l];
    for (int w = 1; w < kBlock / kWave; ++w) t += s_t[w][row][l];
    s_t[0][row][l] = t;
  }
  __syncthreads();
  const int nG = FULL ? k.y * k.z : 0, nH = FULL ? q.y * q.z : 0, E = 1 + nG + nH;
  const int nl = min(kWave, d.z - zg * kWave);
  double *out = part + ((size_t)i * ZG + zg) * E;
  for (int e = threadIdx.x; e < E; e += kBlock) {  // (the fold over the group's z in index order)
    double t = 0.0;
    if (e == 0) {
      for (int l = 0; l < nl; ++l) t += s_t[0][0][l];
    } else {
      const bool isg = e - 1 < nG;
      const int f = isg ? e - 1 : e - 1 - nG, nz = isg ? k.z : q.z;
      const int row = (isg ? kRowG : kRowH) + f / nz, c = f % nz;
      const double *pz = tz + (size_t)c * d.z + (size_t)zg * kWave;
      for (int l = 0; l < nl; ++l) t += s_t[0][row][l] * pz[l];
    }
    out[e] = t;
  }
}

// out[e], a thread per entry: the z-groups of a plane added in index order, the planes folded with phi_a(i) in index
// order.  E: the entries of a (plane, z-group) share of part.
__global__ void __launch_bounds__(kBlock) k_bias_finish(const double *__restrict__ part, int ZG, int E,
                                                        const double *__restrict__ tx, Dim3i k, Dim3i q, Dim3i d,
                                                        double *__restrict__ out) {
#pragma clang fp contract(off)
  const int nG = k.y * k.z, nH = q.y * q.z;
  const int total = 1 + k.x * nG + q.x * nH;
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= total) return;
  int a = 0, pe = 0;
  if (e > 0) {
    if (e - 1 < k.x * nG)
      a = (e - 1) / nG, pe = 1 + (e - 1) % nG;
    else
      a = (e - 1 - k.x * nG) / nH, pe = 1 + nG + (e - 1 - k.x * nG) % nH;
  }
  double acc = 0.0;
  for (int i = 0; i < d.x; ++i) {
    double s = 0.0;
    for (int zg = 0; zg < ZG; ++zg) s += part[((size_t)i * ZG + zg) * E + pe];
    acc += e == 0 ? s : s * tx[(size_t)a * d.x + i];
  }
  out[e] = acc;
}

}  // namespace

void launch_bias_field(const double *coef, const double *tx, const double *ty, const double *tz, Dim3i k, Dim3i d,
                       double beta_max, const float *g, const float *x, float *b, float *gb2, float *xb,
                       hipStream_t st) {
  const dim3 grid((unsigned)d.x, (unsigned)((d.y + kBiasRowsPerGroup - 1) / kBiasRowsPerGroup));
  hipLaunchKernelGGL(k_bias_field, grid, dim3(kBlock), 0, st, coef, tx, ty, tz, k, d, beta_max, g, x, b, gb2, xb);
}

int bias_terms_groups(Dim3i d) { return (d.z + kWave - 1) / kWave; }

size_t bias_terms_scratch(Dim3i d, Dim3i k) {
  const Dim3i q{std::max(2 * k.x - 1, 0), std::max(2 * k.y - 1, 0), std::max(2 * k.z - 1, 0)};
  const size_t E = 1 + (size_t)k.y * k.z + (size_t)q.y * q.z;
  return (size_t)d.x * bias_terms_groups(d) * E;
}

void launch_bias_terms(const float *x, const float *mu, const float *b, const float *g, const float *u, int axis,
                       const double *tx, const double *ty, const double *tz, Dim3i k, Dim3i d, double *part,
                       double *out, hipStream_t st) {
  const bool full = k.x > 0;
  const Dim3i q{full ? 2 * k.x - 1 : 0, full ? 2 * k.y - 1 : 0, full ? 2 * k.z - 1 : 0};
  const int ZG = bias_terms_groups(d), E = 1 + k.y * k.z + q.y * q.z;
  const dim3 grid((unsigned)d.x, (unsigned)ZG);
  if (full)
    hipLaunchKernelGGL(k_bias_proj<true>, grid, dim3(kBlock), 0, st, x, mu, b, g, u, axis, ty, tz, k, q, d, part);
  else
    hipLaunchKernelGGL(k_bias_proj<false>, grid, dim3(kBlock), 0, st, x, mu, b, g, u, axis, ty, tz, k, q, d, part);
  const int total = 1 + k.x * k.y * k.z + q.x * q.y * q.z;
  hipLaunchKernelGGL(k_bias_finish, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part, ZG, E,
                     tx, k, q, d, out);
}

}  // namespace unires
