// coreg.hpp - launchers of the rigid coregistration estimator (coreg.hip): uint8
// quantisation of a batch of observations, the partial-volume joint histograms of a batch of
// (fixed, moving, voxel map) jobs, and the histogram costs (nmi / mi / ecc) of a batch.
#pragma once
#include "common.hpp"

namespace unires {

constexpr int kCoregBins = 256;         // joint histogram side (uint8 intensities)
constexpr int kCoregQBins = 1024;       // bins of the robust-maximum histogram
constexpr int kCoregQOut = 8;           // floats per observation written by the quantisation
constexpr int kCoregMaxObs = 32;        // observations per quantisation launch (more: chained launches)
constexpr int kCoregMaxJobs = 16;       // jobs per histogram launch (more: chained launches)
constexpr int kCoregBlock = 1024;       // threads of a histogram / cost workgroup
constexpr int kCoregPtsPerThread = 63;  // points a histogram lane visits between flushes
constexpr int kCoregChunk = kCoregBlock * kCoregPtsPerThread;  // points per workgroup (< 65536)
constexpr int kCoregJitter = 97;        // entries of the sampling jitter table
constexpr int kCoregMaxTapRadius = 32;  // histogram smoothing: at most 65 taps
constexpr int kCoregQBlock = 1024;      // threads of a quantisation workgroup

// quantisation output, per observation (kCoregQOut floats)
enum CoregQOut {
  kCqMn = 0,      // minimum of the finite voxels
  kCqMax = 1,     // maximum of the finite voxels
  kCqMx = 2,      // robust maximum (upper edge of the 99.99 % bin)
  kCqScale = 3,   // 255 / (mx - mn), float32
  kCqStatus = 4,  // 0 ok, 1 no finite voxel, 2 all finite voxels equal (or mx == mn)
  kCqKeyLo = 6, kCqKeyHi = 7  // scratch: ordered-integer keys of the min / max
};

struct CoregJobHost {  // mirrors unires_coreg_job_t
  const uint8_t *G;
  const uint8_t *F;
  int32_t dim_g[3];
  int32_t dim_f[3];
  float M[12];
  float step[3];
};

struct CoregJobMHost {  // mirrors unires_coreg_job_m_t
  CoregJobHost job;
  const uint8_t *mG;  // cell supports of G's / F's shape, or null
  const uint8_t *mF;
};

// Blocks one observation of n voxels gets in the quantisation launches.
int coreg_quant_blocks(int64_t n);
// Sample-grid size of a job along each axis: floor((dim_g - 1) / step) + 1 (float64), and points.
int64_t coreg_grid(const CoregJobHost &j, int32_t ng[3]);

// One chained group of at most kCoregMaxObs observations; counts (n x kCoregQBins uint32) and
// params (n x kCoregQOut float) are this group's slices, both initialised here.
void launch_coreg_quantise(int n, const float *const *ptrs, const int64_t *sizes, uint8_t *const *outs,
                           uint32_t *counts, float *params, hipStream_t st);
// One chained group of at most kCoregMaxJobs jobs; hist (n x 256 x 256 uint64) zeroed by the caller.
void launch_coreg_hist(int n, const CoregJobHost *jobs, uint64_t *hist, hipStream_t st);
// The two above under supports.  masks[o] (or masks itself) may be null: uint8, non-zero = usable;
// range, histogram and robust maximum read the finite usable voxels, every finite voxel is converted.
void launch_coreg_quantise_m(int n, const float *const *ptrs, const int64_t *sizes, const uint8_t *const *masks,
                             uint8_t *const *outs, uint32_t *counts, float *params, hipStream_t st);
// cell[i] = 1 iff the eight voxels of the cell at i are all usable (0 in the last plane of every axis)
void launch_coreg_cellmask(const uint8_t *mask, const int32_t dim[3], uint8_t *cell, hipStream_t st);
// a sample point in an unsupported G cell, or imaged into an unsupported F cell, adds nothing
void launch_coreg_hist_m(int n, const CoregJobMHost *jobs, uint64_t *hist, hipStream_t st);
// n histograms -> n float64 costs; work: n x 256 x 256 doubles of scratch.
void launch_coreg_cost(int n, const uint64_t *hist, int cost_fun, const double *taps, int radius, double *work,
                       double *cost, hipStream_t st);

}  // namespace unires
