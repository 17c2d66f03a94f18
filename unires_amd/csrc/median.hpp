// median.hpp - launchers of the exact masked median of a stream of float32 magnitudes (median.hip): a three-pass radix
// select on the bit patterns of |t|, entirely on the device.
#pragma once
#include "common.hpp"

namespace unires {

constexpr int kMedianBins = 2048;  // bins of a pass: 11 + 11 + 10 key bits (the last pass fills 1024 of them)
constexpr int kMedianPasses = 3;

// The scratch of one median (UNIRES_MEDIAN_WORK_BYTES of the C ABI): a histogram per pass, then what a pass's scan
// leaves for the next pass to filter on.  The launchers take it zeroed (the entry points clear it, on the stream).
struct MedianWork {
  uint32_t counts[kMedianPasses][kMedianBins];
  uint32_t prefix;  // the key bits chosen so far (the high 11, then the high 21)
  uint32_t rank;    // the rank still looked for among the keys that share them, from 1; 0: nothing eligible
  uint32_t n;       // eligible voxels
  uint32_t pad;
};
static_assert(sizeof(MedianWork) == UNIRES_MEDIAN_WORK_BYTES, "UNIRES_MEDIAN_WORK_BYTES is the size of MedianWork");

// Lower median of |fl32(x - ay)| over the voxels with x != 0, a finite difference and (prior == nullptr or prior > 0)
// -> out_dev[0] (0 where there is none), their number -> out_dev[1].  n <= UINT32_MAX.
void launch_median_absres(const float *x, const float *ay, const float *prior, size_t n, MedianWork *work,
                          double *out_dev, hipStream_t st);

// Lower median of |((a - b) - c) + d| over the 2 x 2 cells of the planes orthogonal to `axis` (a = x[p, q],
// b = x[p + 1, q], c = x[p, q + 1], d = x[p + 1, q + 1]; p, q the two other axes in ascending order) whose four voxels
// are finite, != 0 (ct == 0: > 0) and (w == nullptr or) of weight > 0.  The cell count is <= UINT32_MAX.
void launch_median_hh(const float *x, Dim3i d, int axis, int ct, const float *w, MedianWork *work, double *out_dev,
                      hipStream_t st);

// the number of 2 x 2 cells launch_median_hh ranks
inline unsigned long long median_hh_cells(Dim3i d, int axis) {
  const unsigned long long c[3] = {(unsigned long long)d.x - (axis != 0), (unsigned long long)d.y - (axis != 1),
                                   (unsigned long long)d.z - (axis != 2)};
  return c[0] * c[1] * c[2];
}

}  // namespace unires
