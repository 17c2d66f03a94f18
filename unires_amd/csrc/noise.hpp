// noise.hpp - launchers of the noise / intensity hyper-parameter estimator (noise.hip): the masked
// range and 1024-bin histogram of a batch of observations, then a two-class mixture fit of every
// histogram in one launch.
#pragma once
#include "common.hpp"

namespace unires {

constexpr int kNoiseBins = 1024;     // histogram bins
constexpr int kNoiseMaxObs = 32;     // observations per histogram launch (more: chained launches)
constexpr int kNoiseHistBlock = 1024;  // threads of a range / histogram workgroup
constexpr int kNoiseFitBlock = 256;  // threads of a fit workgroup (4 bins per lane)
constexpr int kNoiseOut = 16;        // doubles per observation written by the fit

// fit output, per observation (kNoiseOut doubles)
enum NoiseOut {
  kNoMg0 = 0, kNoMg1 = 1,      // mixing proportions
  kNoLoc0 = 2, kNoLoc1 = 3,    // Rice nu | Gaussian mean
  kNoSig0 = 4, kNoSig1 = 5,    // Rice / Gaussian sigma
  kNoMean0 = 6, kNoMean1 = 7,  // class means
  kNoLL = 8,                   // log-likelihood of the last E-step
  kNoIters = 9,                // M-steps taken
  kNoSd = 10, kNoMu = 11,      // sigma of the noise class, |mean_fg - mean_bg|
  kNoModel = 12,               // 0 Rice, 1 Gaussian, -1 no usable voxels / mn == mx (nothing else written)
  kNoSumH = 13, kNoMn = 14, kNoMx = 15
};

// Blocks one observation of n voxels gets in the range and histogram launches.
int noise_hist_blocks(int64_t n);

// One chained group of at most kNoiseMaxObs observations.  part: 2 * sum_o noise_hist_blocks(n_o) floats
// of scratch; counts (n x kNoiseBins, zeroed by the caller) and range (n x 2) are this group's slices.
// hist_form: 0 plain LDS atomics, 1 wave pre-aggregation of lanes that share the first lane's bin.
void launch_noise_hist(int n, const float *const *ptrs, const int64_t *sizes, const int32_t *ct,
                       float *part, uint32_t *counts, float *range, int hist_form, hipStream_t st);
// The same under per-voxel weight maps: gptrs[o] (or gptrs itself) may be null; a voxel of an
// observation with a map is taken only where its weight is > 0.
void launch_noise_hist_g(int n, const float *const *ptrs, const int64_t *sizes, const int32_t *ct,
                         const float *const *gptrs, float *part, uint32_t *counts, float *range, int hist_form,
                         hipStream_t st);
void launch_noise_fit(int n, const uint32_t *counts, const float *range, int max_iter, double *out,
                      hipStream_t st);

}  // namespace unires
