// slice.hpp - per-slice weights of an observation (slice.hip): the residual sums per slice the weights are estimated
// from, and the pass that multiplies an x-space volume by the weight of each voxel's slice (with the validity mask of
// mask.hip in the same pass where the repeat has one).
#pragma once
#include "common.hpp"

namespace unires {

// Shares per slice of launch_slice_sums: part holds 2 * S * slice_sums_parts(d, axis) doubles of scratch, S = d[axis].
int slice_sums_parts(Dim3i d, int axis);
// out[s] = sum_{v in slice s, x(v) != 0} (x(v) - ay(v))^2, out[S + s] = #{v in slice s : x(v) != 0}; x, ay z-fastest
// with dims d, slices counted along `axis`.  float32 terms, float64 sums in a fixed order: the same bits every run.
void launch_slice_sums(const float *x, const float *ay, Dim3i d, int axis, double *part, double *out, hipStream_t st);

// dst[v] = u[s(v)] * src[v] (and 0 where mask[v] == 0, mask != nullptr) over a z-fastest volume of dims d;
// s(v) = v's index along `axis`, counted from the far end where `flip`.  dst == src: in place (a group of voxels the
// pass leaves as it is is then not stored back).  Returns at entry where *done is set.
void launch_slice_apply(const float *src, float *dst, const uint8_t *mask, const float *u, Dim3i d, int axis,
                        bool flip, const int *done, hipStream_t st);

// The x-space residual of the rigid Gauss-Newton step (_rigid.py): out[v] = u[s(v)] * (ay[v] - x[v]) where x[v] != 0
// and ay[v] != 0, else +0; float32, one rounding each for the difference and the product.  u == nullptr: weight 1,
// the bits of the unweighted residual.  out == ay is allowed; x is only read.
void launch_rigid_resid(const float *x, const float *ay, float *out, const float *u, Dim3i d, int axis,
                        hipStream_t st);

}  // namespace unires
