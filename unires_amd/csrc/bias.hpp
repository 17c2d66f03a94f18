// bias.hpp - a smooth multiplicative bias field per observation (bias.hip; sett.bias, _input.bias_coef): the synthesis
// of b = exp(beta) from the coefficients of a separable cosine basis, with the two volumes the plan reads for a repeat
// with a field, and the projections the field's Gauss-Newton step is assembled from.
#pragma once
#include "common.hpp"

namespace unires {

constexpr int kBiasMaxOrder = 8;                      // orders per axis of the field: 1 .. 8
constexpr int kBiasMaxProj = 2 * kBiasMaxOrder - 1;   // orders per axis of the projection of W m^2: 2 k - 1

// beta(i, j, z) = sum_{a < k.x, b < k.y, c < k.z} coef[(a k.y + b) k.z + c] tx[a d.x + i] ty[b d.y + j] tz[c d.z + z] in
// float64, folded over a, then b, then c, each in index order (one product and one addition per term, no fused
// multiply-add); clamped to +- beta_max;
//   b   = fl32(exp(beta))
//   gb2 (nullptr: not written) = fl32(fl64(fl64(g b) b)), g = 1 where nullptr: g b is exact in float64
//   xb  (nullptr: not written) = fl32(x / b), +0 where x == 0
// coef and the tables on the device, float64; the tables hold at least k rows of d entries.  All volumes z-fastest.
void launch_bias_field(const double *coef, const double *tx, const double *ty, const double *tz, Dim3i k, Dim3i d,
                       double beta_max, const float *g, const float *x, float *b, float *gb2, float *xb,
                       hipStream_t st);

// workgroups along z and doubles of scratch launch_bias_terms needs for (d, k)
int bias_terms_groups(Dim3i d);
size_t bias_terms_scratch(Dim3i d, Dim3i k);

// With m = fl32(b mu), r = fl64(m) - fl64(x), W = g u[s(v)] [x != 0] (either factor 1 where nullptr; u counted along
// `axis`), everything after m in float64, each product rounded on its own:
//   out[0]                    = sum_v W r^2
//   out[1 + (a k.y + b) k.z + c]                  = sum_v W m r  tx[a][i] ty[b][j] tz[c][z]   a < k.x, b < k.y, c < k.z
//   out[1 + k.x k.y k.z + (a q.y + b) q.z + c]    = sum_v W m^2  tx[a][i] ty[b][j] tz[c][z]   a < q.x ..., q = 2 k - 1
// k = (0, 0, 0): out[0] alone (the tables are not read).  The tables hold at least q rows.  A workgroup owns a plane i
// and 64 consecutive z: its four waves share the rows j, a lane keeps its z and sums over j for every order along y in
// registers; the waves' sums are added in wave order and folded over z through LDS; k_bias_finish folds the z-groups and
// the planes in index order.  No atomics: the same bits every run.  part: bias_terms_scratch(d, k) doubles.
void launch_bias_terms(const float *x, const float *mu, const float *b, const float *g, const float *u, int axis,
                       const double *tx, const double *ty, const double *tz, Dim3i k, Dim3i d, double *part,
                       double *out, hipStream_t st);

}  // namespace unires
