// voxel.hpp - per-voxel weights of an observation (voxel.hip): the pass that multiplies an x-space volume by a weight
// map (with the slice weights of slice.hip and the validity mask of mask.hip in the same pass where the repeat has
// them), the map's copy into the plan's canonical layout, the weighted residual sums per slice, and the Huber rule.
#pragma once
#include "common.hpp"
#include "orient.hpp"

namespace unires {

// dst[v] = g[v] * src[v] [* u[s(v)]] (and 0 where mask[v] == 0, mask != nullptr) over a z-fastest volume of dims d; g
// has the volume's layout.  u != nullptr: one weight per slice along `axis`, counted from the far end where `flip`;
// g u src is then rounded to float32 once (the product g u is exact in float64).  dst == src: in place (a group of
// voxels the pass leaves as it is is then not stored back).  Returns at entry where *done is set.
void launch_voxel_apply(const float *src, float *dst, const float *g, const uint8_t *mask, const float *u, Dim3i d,
                        int axis, bool flip, const int *done, hipStream_t st);

// g (canonical layout) <- g_u (caller's layout, dims du): launch_mask_permute's float counterpart
void launch_voxel_permute(const float *g_u, const Orient &O, Dim3i du, float *g, hipStream_t st);

// out[s] = sum_{v in slice s, x(v) != 0} g(v) (x(v) - ay(v))^2, out[S + s] = sum_{v in slice s, x(v) != 0} g(v); x, ay, g
// z-fastest with dims d, slices counted along `axis`.  float32 terms, float64 sums in launch_slice_sums' fixed order
// (part: 2 * S * slice_sums_parts(d, axis) doubles of scratch): the same bits every run.
void launch_voxel_sums(const float *x, const float *ay, const float *g, Dim3i d, int axis, double *part, double *out,
                       hipStream_t st);

// The x-space residual of the rigid Gauss-Newton step on the voxel-weighted data term: out[v] = g[v] [u[s(v)]] *
// (ay[v] - x[v]) where x[v] != 0 and ay[v] != 0, else +0; launch_voxel_apply's rounding.  u == nullptr: no slice weights.
// g = 1 gives launch_rigid_resid's bits (slice.hpp).  out == ay is allowed; x and g are only read.
void launch_rigid_resid_g(const float *x, const float *ay, const float *g, float *out, const float *u, Dim3i d, int axis,
                          hipStream_t st);

// g_out[v] = (prior ? prior[v] : 1) * h(v); h = 1 where x == 0 or |x - ay| <= c, else c / |x - ay|.  g_out may be prior.
void launch_voxel_huber(const float *x, const float *ay, const float *prior, float c, size_t n, float *g_out,
                        hipStream_t st);
// The same with c = fl32(mult * (float)scale_dev[0]) read on the device; c not > 0: g_out = prior (ones without one).
void launch_voxel_huber_dev(const float *x, const float *ay, const float *prior, const double *scale_dev, float mult,
                            size_t n, float *g_out, hipStream_t st);

}  // namespace unires
