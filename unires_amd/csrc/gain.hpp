// gain.hpp - per-slice intensity gains of an observation (gain.hip): the sums per slice the gains are estimated from,
// and the two per-slice tables a gained repeat's passes read (slice.hip's and voxel.hip's apply passes, unchanged).
#pragma once
#include "common.hpp"

namespace unires {

// With W(v) = g(v) u[s(v)] (either factor 1 where its pointer is nullptr), over the voxels of slice s with x(v) != 0:
//   out[s] = sum W fl32(x ay), out[S + s] = sum W fl32(ay ay), out[2 S + s] = sum W;  S = d[axis].
// x, ay, g z-fastest with dims d, u S floats.  float32 terms, W and the summand W t in float64 (g u is exact there, W t
// exact with one factor and rounded once with both: k_scaling_sums_g's conventions), float64 sums in a fixed order:
// the same bits every run.  part: 3 * S * slice_sums_parts(d, axis) doubles of scratch (slice.hpp).
void launch_gain_sums(const float *x, const float *ay, const float *g, const float *u, Dim3i d, int axis, double *part,
                      double *out, hipStream_t st);

// w_rhs[s] = fl32(fl64(u[s] e[s])), w_mat[s] = fl32(fl64(fl64(u[s] e[s]) e[s])) for s < S; u == nullptr: u = 1.  One
// workgroup.  u e is exact in float64; u e e is rounded there once, then once more to float32.
void launch_gain_compose(const float *u, const float *e, int S, float *w_mat, float *w_rhs, hipStream_t st);

// The terms of the rigid Gauss-Newton step of a gained repeat in one pass, on p = fl32(e[s(v)] ay(v)) held in registers
// (launch_slice_apply's product, never stored); g a volume or nullptr (1), u S floats or nullptr (1), e S floats.
//   sums[s], sums[S + s]: launch_slice_sums' bits on (x, p) - launch_voxel_sums' with g - by their walk, grid, shares
//     and finish order;  part: 2 * S * slice_sums_parts(d, axis) doubles of scratch.
//   out (nullptr: not written): launch_rigid_resid's bits on (x, p) with t[s] = fl32(fl64(u[s]) fl64(e[s])) (u nullptr:
//     e[s]) for u - launch_rigid_resid_g's with g.  out may be ay: a voxel is read and stored by one thread, once.
void launch_rigid_terms_e(const float *x, const float *ay, const float *g, const float *u, const float *e, Dim3i d,
                          int axis, double *part, double *sums, float *out, hipStream_t st);

// out[c] = sum_b part[c * B + b] for c < ncols: the finish of every per-slice sum above (and of rician.hip's) - a wave
// per entry, lane l adds the shares l, l + 64, ... in index order, a fixed tree adds the lanes.  Plain stores.
void launch_gain_finish(const double *part, int B, size_t ncols, double *out, hipStream_t st);

}  // namespace unires
