// mask.hpp - validity mask of an observation (mask.hip): one byte per x-space voxel, 1 where the observation is
// non-zero, in the plan's canonical layout; and the pass that zeroes the x-space intermediate of A^T A where it is 0.
#pragma once
#include "common.hpp"
#include "orient.hpp"

namespace unires {

// mask (canonical layout of O) <- x != 0 (float32, the caller's layout, dims du)
void launch_mask_build(const float *x, const Orient &O, Dim3i du, uint8_t *mask, hipStream_t st);
// mask (canonical layout of O) <- a mask in the caller's layout (a new orientation of the same observation)
void launch_mask_permute(const uint8_t *mask_u, const Orient &O, Dim3i du, uint8_t *mask, hipStream_t st);
// buf[i] = mask[i] ? buf[i] : 0 for i < n, in place; returns at entry where *done is set
void launch_mask_apply(float *buf, const uint8_t *mask, size_t n, const int *done, hipStream_t st);

}  // namespace unires
