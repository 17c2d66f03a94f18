// pull.hpp - host launchers of the affine pulls (pull.hip).
#pragma once
#include "common.hpp"

namespace unires {

void launch_pull(const float *src, Dim3i sd, const Affine &A, float *dst, Dim3i gd, float tol,
                 const int *done, hipStream_t st);
// dst = the label value whose indicator has the highest trilinear pull (ties: smallest value;
// a best of 0 gives 0) - one gather for what the reference does with one pull per value
void launch_warp_label(const float *label, Dim3i sd, const Affine &A, float *dst, Dim3i gd,
                       float tol, hipStream_t st);
// dst = 1 where launch_pull's sample is inside the FOV and every corner of it inside the volume has g > 0
void launch_pull_support(const float *g, Dim3i sd, const Affine &A, uint8_t *dst, Dim3i gd, float tol,
                         hipStream_t st);
// nearest-neighbour pull (order 0, zero bound, in-FOV mask)
void launch_pull_nearest(const float *src, Dim3i sd, const Affine &A, float *dst, Dim3i gd,
                         float tol, hipStream_t st);
void launch_pull_grad(const float *src, Dim3i sd, const Affine &A, float *dst, Dim3i gd, float tol,
                      hipStream_t st);

}  // namespace unires
