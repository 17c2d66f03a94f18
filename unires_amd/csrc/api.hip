// api.hip - the C ABI of libunires_hip.so (include/unires_hip.h), first part: error plumbing and argument
// checking, the op-level entry points, the ADMM sums and the stream marks.  The plan object is api_plan.hip, the
// sequencing of kernels for _proj_apply / _proj('AtA') / the y-update RHS api_operator.hip, nitorch-style cg()
// api_cg.hip; api_internal.hpp is what the four share.
// Nothing here touches torch; the caller hands over raw device pointers and a
// hipStream_t.
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <map>
#include <mutex>
#include <new>

#include "admm.hpp"
#include "api_internal.hpp"
#include "bias.hpp"
#include "conv.hpp"
#include "coreg.hpp"
#include "noise.hpp"
#include "pull.hpp"
#include "rician.hpp"
#include "stencil.hpp"

using namespace unires;

// --------------------------------------------------------------------------
// error plumbing, argument checking
// --------------------------------------------------------------------------
thread_local std::string unires::g_err;

int unires::make_taps(const float *const taps[3], const int32_t ntaps[3], const int32_t stride[3], Taps &T) {
  memset(&T, 0, sizeof(T));
  for (int d = 0; d < 3; ++d) {
    if (ntaps[d] < 1 || ntaps[d] > UNIRES_MAX_TAPS)
      return fail(UNIRES_ERR_UNSUPPORTED, "ntaps must be in [1, UNIRES_MAX_TAPS]");
    if (stride[d] < 1) return fail(UNIRES_ERR_ARG, "stride must be >= 1");
    if (!taps[d]) return fail(UNIRES_ERR_NULL, "null taps pointer");
    T.n[d] = ntaps[d];
    T.s[d] = stride[d];
    for (int i = 0; i < ntaps[d]; ++i) T.t[d][i] = taps[d][i];
  }
  return UNIRES_OK;
}

// inverse of a row-major 3x4 float32 affine, computed in double
bool unires::invert_affine(const Affine &A, Affine &out) {
  const double a = A.m[0], b = A.m[1], c = A.m[2], d = A.m[4], e = A.m[5], f = A.m[6],
               g = A.m[8], h = A.m[9], i = A.m[10];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  if (!(fabs(det) > 1e-12)) return false;
  const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                         (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                         (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
  const double t[3] = {A.m[3], A.m[7], A.m[11]};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) out.m[4 * r + k] = (float)inv[3 * r + k];
    out.m[4 * r + 3] = (float)-(inv[3 * r] * t[0] + inv[3 * r + 1] * t[1] + inv[3 * r + 2] * t[2]);
  }
  return true;
}

int unires::check_conv_dims(const Dim3i &hi, const Dim3i &lo, const Taps &T) {
  const int h[3] = {hi.x, hi.y, hi.z}, l[3] = {lo.x, lo.y, lo.z};
  for (int d = 0; d < 3; ++d)
    if (h[d] != (l[d] - 1) * T.s[d] + T.n[d])
      return fail(UNIRES_ERR_DIM, "conv dims: need hi = (lo-1)*stride + ntaps");
  return UNIRES_OK;
}

extern "C" const char *unires_last_error(void) { return g_err.c_str(); }
extern "C" int unires_abi_version(void) { return UNIRES_HIP_ABI_VERSION; }

// scratch of the float64 reductions (per-workgroup sums, added in index order by a second launch): one buffer per
// (device, stream), grown on demand, used in stream order by the launches that share it
static int reduce_scratch(hipStream_t st, size_t ndoubles, double **out) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, std::pair<double *, size_t>> scratch;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto &slot = scratch[std::make_pair(dev, st)];
  if (slot.second < ndoubles) {
    if (slot.first) {
      HIP_TRY(hipDeviceSynchronize());
      (void)hipFree(slot.first);
      slot = {nullptr, 0};
    }
    const size_t n = std::max<size_t>(ndoubles, 16384);
    HIP_TRY(hipMalloc((void **)&slot.first, n * sizeof(double)));
    slot.second = n;
  }
  *out = slot.first;
  return UNIRES_OK;
}

// --------------------------------------------------------------------------
// op level
// --------------------------------------------------------------------------
extern "C" int unires_pull3d_affine(const float *src, const int32_t sdim[3], const float M[12],
                                    float *dst, const int32_t gdim[3], float fov_tol,
                                    void *stream) {
  if (!src || !dst || !sdim || !gdim || !M) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(sdim) || !dims_ok(gdim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  launch_pull(src, mk(sdim), A, dst, mk(gdim), fov_tol, nullptr, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_warp_label(const float *label, const int32_t ldim[3], const float M[12],
                                 float *dst, const int32_t gdim[3], float fov_tol, void *stream) {
  if (!label || !dst || !ldim || !gdim || !M) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(ldim) || !dims_ok(gdim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  launch_warp_label(label, mk(ldim), A, dst, mk(gdim), fov_tol, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_pull3d_nearest(const float *src, const int32_t sdim[3], const float M[12],
                                     float *dst, const int32_t gdim[3], float fov_tol,
                                     void *stream) {
  if (!src || !dst || !sdim || !gdim || !M) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(sdim) || !dims_ok(gdim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  launch_pull_nearest(src, mk(sdim), A, dst, mk(gdim), fov_tol, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

// UNIRES_NOISE_HIST_FORM: 0 plain LDS atomics, 1 wave pre-aggregation (default; profiles/noise_time.json),
// read at every call (tools/noise_time.py measures both in one process)
static int noise_hist_form() {
  const char *e = getenv("UNIRES_NOISE_HIST_FORM");
  return e && *e ? (atoi(e) ? 1 : 0) : 1;
}

extern "C" int unires_noise_hist(int32_t n_obs, const float *const *ptrs, const int64_t *sizes,
                                 const int32_t *ct, uint32_t *counts, float *range, void *stream) {
  if (!ptrs || !sizes || !ct || !counts || !range) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_obs < 1) return fail(UNIRES_ERR_ARG, "n_obs must be >= 1");
  size_t blocks = 0;
  for (int32_t o = 0; o < n_obs; ++o) {
    if (!ptrs[o]) return fail(UNIRES_ERR_NULL, "null observation pointer");
    if (sizes[o] < 1 || sizes[o] > (int64_t)UINT32_MAX) return fail(UNIRES_ERR_DIM, "observation size out of range");
    blocks += (size_t)noise_hist_blocks(sizes[o]);
  }
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;  // one (min, max) float pair per workgroup
  if (int rc = reduce_scratch(st, blocks, &part)) return rc;
  HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_obs * kNoiseBins * sizeof(uint32_t), st));
  for (int32_t o = 0; o < n_obs; o += kNoiseMaxObs) {
    const int n = std::min<int32_t>(kNoiseMaxObs, n_obs - o);
    size_t off = 0;  // a group's partials after the previous group's (one scratch, stream-ordered anyway)
    for (int32_t q = 0; q < o; ++q) off += (size_t)noise_hist_blocks(sizes[q]);
    launch_noise_hist(n, ptrs + o, sizes + o, ct + o, reinterpret_cast<float *>(part + off),
                      counts + (size_t)o * kNoiseBins, range + 2 * (size_t)o, noise_hist_form(), st);
    CHECK_LAUNCH();
  }
  return UNIRES_OK;
}

extern "C" int unires_pull3d_support(const float *g, const int32_t sdim[3], const float M[12], uint8_t *dst,
                                     const int32_t gdim[3], float fov_tol, void *stream) {
  if (!g || !dst || !sdim || !gdim || !M) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(sdim) || !dims_ok(gdim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  launch_pull_support(g, mk(sdim), A, dst, mk(gdim), fov_tol, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_noise_hist_g(int32_t n_obs, const float *const *ptrs, const int64_t *sizes, const int32_t *ct,
                                   const float *const *gptrs, uint32_t *counts, float *range, void *stream) {
  if (!ptrs || !sizes || !ct || !counts || !range) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_obs < 1) return fail(UNIRES_ERR_ARG, "n_obs must be >= 1");
  size_t blocks = 0;
  for (int32_t o = 0; o < n_obs; ++o) {
    if (!ptrs[o]) return fail(UNIRES_ERR_NULL, "null observation pointer");
    if (sizes[o] < 1 || sizes[o] > (int64_t)UINT32_MAX) return fail(UNIRES_ERR_DIM, "observation size out of range");
    blocks += (size_t)noise_hist_blocks(sizes[o]);
  }
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;  // one (min, max) float pair per workgroup
  if (int rc = reduce_scratch(st, blocks, &part)) return rc;
  HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_obs * kNoiseBins * sizeof(uint32_t), st));
  for (int32_t o = 0; o < n_obs; o += kNoiseMaxObs) {
    const int n = std::min<int32_t>(kNoiseMaxObs, n_obs - o);
    size_t off = 0;
    for (int32_t q = 0; q < o; ++q) off += (size_t)noise_hist_blocks(sizes[q]);
    launch_noise_hist_g(n, ptrs + o, sizes + o, ct + o, gptrs ? gptrs + o : nullptr, reinterpret_cast<float *>(part + off),
                        counts + (size_t)o * kNoiseBins, range + 2 * (size_t)o, noise_hist_form(), st);
    CHECK_LAUNCH();
  }
  return UNIRES_OK;
}

extern "C" int unires_noise_fit(int32_t n_obs, const uint32_t *counts, const float *range,
                                int32_t max_iter, double *out, void *stream) {
  if (!counts || !range || !out) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_obs < 1) return fail(UNIRES_ERR_ARG, "n_obs must be >= 1");
  if (max_iter < 0) return fail(UNIRES_ERR_ARG, "max_iter must be >= 0");
  launch_noise_fit(n_obs, counts, range, max_iter, out, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_coreg_quantise(int32_t n_obs, const float *const *ptrs, const int64_t *sizes,
                                     uint8_t *const *outs, uint32_t *counts, float *params, void *stream) {
  if (!ptrs || !sizes || !outs || !counts || !params) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_obs < 1) return fail(UNIRES_ERR_ARG, "n_obs must be >= 1");
  for (int32_t o = 0; o < n_obs; ++o) {
    if (!ptrs[o] || !outs[o]) return fail(UNIRES_ERR_NULL, "null observation pointer");
    if (sizes[o] < 1 || sizes[o] > (int64_t)UINT32_MAX) return fail(UNIRES_ERR_DIM, "observation size out of range");
  }
  hipStream_t st = (hipStream_t)stream;
  for (int32_t o = 0; o < n_obs; o += kCoregMaxObs) {
    const int n = std::min<int32_t>(kCoregMaxObs, n_obs - o);
    launch_coreg_quantise(n, ptrs + o, sizes + o, outs + o, counts + (size_t)o * kCoregQBins,
                          params + (size_t)o * kCoregQOut, st);
    CHECK_LAUNCH();
  }
  return UNIRES_OK;
}

extern "C" int unires_coreg_hist(int32_t n_jobs, const unires_coreg_job_t *jobs, uint64_t *hist, void *stream) {
  static_assert(sizeof(unires_coreg_job_t) == sizeof(CoregJobHost), "job layout");
  if (!jobs || !hist) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_jobs < 1) return fail(UNIRES_ERR_ARG, "n_jobs must be >= 1");
  const CoregJobHost *J = reinterpret_cast<const CoregJobHost *>(jobs);
  for (int32_t o = 0; o < n_jobs; ++o) {
    if (!J[o].G || !J[o].F) return fail(UNIRES_ERR_NULL, "null volume pointer");
    for (int d = 0; d < 3; ++d) {
      if (J[o].dim_g[d] < 2 || J[o].dim_f[d] < 2) return fail(UNIRES_ERR_DIM, "every dimension must be >= 2");
      if (!(J[o].step[d] > 0.f) || !(J[o].step[d] <= 3.0e38f)) return fail(UNIRES_ERR_ARG, "step must be finite and > 0");
    }
    if (!dims_ok(J[o].dim_g) || !dims_ok(J[o].dim_f)) return fail(UNIRES_ERR_DIM, "bad dimensions");
    int32_t ng[3];
    if (coreg_grid(J[o], ng) > (int64_t)INT32_MAX) return fail(UNIRES_ERR_DIM, "more than 2^31 - 1 sample points");
  }
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(hist, 0, (size_t)n_jobs * kCoregBins * kCoregBins * sizeof(uint64_t), st));
  for (int32_t o = 0; o < n_jobs; o += kCoregMaxJobs) {
    const int n = std::min<int32_t>(kCoregMaxJobs, n_jobs - o);
    launch_coreg_hist(n, J + o, hist + (size_t)o * kCoregBins * kCoregBins, st);
    CHECK_LAUNCH();
  }
  return UNIRES_OK;
}

extern "C" int unires_coreg_quantise_m(int32_t n_obs, const float *const *ptrs, const int64_t *sizes,
                                       const uint8_t *const *masks, uint8_t *const *outs, uint32_t *counts,
                                       float *params, void *stream) {
  if (!ptrs || !sizes || !outs || !counts || !params) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_obs < 1) return fail(UNIRES_ERR_ARG, "n_obs must be >= 1");
  for (int32_t o = 0; o < n_obs; ++o) {
    if (!ptrs[o] || !outs[o]) return fail(UNIRES_ERR_NULL, "null observation pointer");
    if (sizes[o] < 1 || sizes[o] > (int64_t)UINT32_MAX) return fail(UNIRES_ERR_DIM, "observation size out of range");
  }
  hipStream_t st = (hipStream_t)stream;
  for (int32_t o = 0; o < n_obs; o += kCoregMaxObs) {
    const int n = std::min<int32_t>(kCoregMaxObs, n_obs - o);
    launch_coreg_quantise_m(n, ptrs + o, sizes + o, masks ? masks + o : nullptr, outs + o,
                            counts + (size_t)o * kCoregQBins, params + (size_t)o * kCoregQOut, st);
    CHECK_LAUNCH();
  }
  return UNIRES_OK;
}

extern "C" int unires_coreg_cellmask(const uint8_t *mask, const int32_t dim[3], uint8_t *cell, void *stream) {
  if (!mask || !dim || !cell) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (mask == cell) return fail(UNIRES_ERR_ARG, "cellmask cannot run in place");
  launch_coreg_cellmask(mask, dim, cell, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_coreg_hist_m(int32_t n_jobs, const unires_coreg_job_m_t *jobs, uint64_t *hist, void *stream) {
  static_assert(sizeof(unires_coreg_job_m_t) == sizeof(CoregJobMHost), "job layout");
  static_assert(offsetof(unires_coreg_job_m_t, mG) == offsetof(CoregJobMHost, mG), "job layout");
  if (!jobs || !hist) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_jobs < 1) return fail(UNIRES_ERR_ARG, "n_jobs must be >= 1");
  const CoregJobMHost *J = reinterpret_cast<const CoregJobMHost *>(jobs);
  for (int32_t o = 0; o < n_jobs; ++o) {
    const CoregJobHost &j = J[o].job;
    if (!j.G || !j.F) return fail(UNIRES_ERR_NULL, "null volume pointer");
    for (int d = 0; d < 3; ++d) {
      if (j.dim_g[d] < 2 || j.dim_f[d] < 2) return fail(UNIRES_ERR_DIM, "every dimension must be >= 2");
      if (!(j.step[d] > 0.f) || !(j.step[d] <= 3.0e38f)) return fail(UNIRES_ERR_ARG, "step must be finite and > 0");
    }
    if (!dims_ok(j.dim_g) || !dims_ok(j.dim_f)) return fail(UNIRES_ERR_DIM, "bad dimensions");
    int32_t ng[3];
    if (coreg_grid(j, ng) > (int64_t)INT32_MAX) return fail(UNIRES_ERR_DIM, "more than 2^31 - 1 sample points");
  }
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(hist, 0, (size_t)n_jobs * kCoregBins * kCoregBins * sizeof(uint64_t), st));
  for (int32_t o = 0; o < n_jobs; o += kCoregMaxJobs) {
    const int n = std::min<int32_t>(kCoregMaxJobs, n_jobs - o);
    launch_coreg_hist_m(n, J + o, hist + (size_t)o * kCoregBins * kCoregBins, st);
    CHECK_LAUNCH();
  }
  return UNIRES_OK;
}

extern "C" int unires_coreg_cost(int32_t n, const uint64_t *hist, int32_t cost_fun, double fwhm, double *work,
                                 double *cost, void *stream) {
  if (!hist || !work || !cost) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 1) return fail(UNIRES_ERR_ARG, "n must be >= 1");
  if (cost_fun < 0 || cost_fun > 2) return fail(UNIRES_ERR_ARG, "cost_fun must be 0 (nmi), 1 (mi) or 2 (ecc)");
  if (!(fwhm >= 0.0 && fwhm <= 16.0)) return fail(UNIRES_ERR_ARG, "fwhm must be in [0, 16]");
  // SPM's histogram kernel (spm_coreg's smoothing_kernel): a Gaussian of the given FWHM convolved
  // with the unit box, over -round(2 fwhm) .. round(2 fwhm), normalised to sum 1
  const int R = (int)lround(2.0 * fwhm);
  double taps[2 * kCoregMaxTapRadius + 1];
  const double s = pow(fwhm / sqrt(8.0 * log(2.0)), 2) + DBL_EPSILON, w1 = 1.0 / sqrt(2.0 * s);
  double sum = 0.0;
  for (int k = -R; k <= R; ++k) {
    const double v = 0.5 * (erf(w1 * (k + 0.5)) - erf(w1 * (k - 0.5)));
    taps[k + R] = v > 0.0 ? v : 0.0;
    sum += taps[k + R];
  }
  for (int k = 0; k <= 2 * R; ++k) taps[k] /= sum;
  launch_coreg_cost(n, hist, cost_fun, taps, R, work, cost, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_pull_grad3d_affine(const float *src, const int32_t sdim[3], const float M[12],
                                         float *dst3, const int32_t gdim[3], float fov_tol,
                                         void *stream) {
  if (!src || !dst3 || !sdim || !gdim || !M) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(sdim) || !dims_ok(gdim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  launch_pull_grad(src, mk(sdim), A, dst3, mk(gdim), fov_tol, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_push3d_affine(const float *src, const int32_t gdim[3], const float M[12],
                                    float *dst, const int32_t ddim[3], float alpha, float fov_tol,
                                    int accumulate, void *stream) {
  if (!src || !dst || !ddim || !gdim || !M) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(ddim) || !dims_ok(gdim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  Affine Ainv;
  if (!invert_affine(A, Ainv)) return fail(UNIRES_ERR_ARG, "singular affine");
  PushSrc ps;
  memset(&ps, 0, sizeof(ps));
  ps.data = src;
  ps.gd = mk(gdim);
  ps.S = kNoScaling;
  PushEpilogue ep;
  ep.accumulate = accumulate ? 1 : 0;
  SplatSafety safe;
  splat_safety(A, safe.row_sep, safe.use_atomics);
  if (push_mode() == PushMode::kTile ||
      launch_splat(ps, A, Ainv, safe, alpha, fov_tol, ep, dst, mk(ddim), nullptr, (hipStream_t)stream))
    (void)launch_push_tile(ps, A, Ainv, safe, alpha, fov_tol, ep, dst, mk(ddim), nullptr,
                           (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_conv_down3d(const float *src, const int32_t sdim[3],
                                  const float *const taps[3], const int32_t ntaps[3],
                                  const int32_t stride[3], float *dst, const int32_t ddim[3],
                                  float scl, int32_t scl_dim, void *stream) {
  if (!src || !dst || !sdim || !ddim || !taps || !ntaps || !stride)
    return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(sdim) || !dims_ok(ddim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (scl != 0.f && (scl_dim < 0 || scl_dim > 2)) return fail(UNIRES_ERR_ARG, "bad scl_dim");
  Taps T;
  int rc = make_taps(taps, ntaps, stride, T);
  if (rc) return rc;
  if ((rc = check_conv_dims(mk(sdim), mk(ddim), T))) return rc;
  launch_conv_down(src, mk(sdim), T, make_scaling(scl, scl_dim), dst, mk(ddim), nullptr,
                   (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_conv_up3d(const float *src, const int32_t sdim[3],
                                const float *const taps[3], const int32_t ntaps[3],
                                const int32_t stride[3], float *dst, const int32_t ddim[3],
                                float scl, int32_t scl_dim, void *stream) {
  if (!src || !dst || !sdim || !ddim || !taps || !ntaps || !stride)
    return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(sdim) || !dims_ok(ddim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (scl != 0.f && (scl_dim < 0 || scl_dim > 2)) return fail(UNIRES_ERR_ARG, "bad scl_dim");
  Taps T;
  int rc = make_taps(taps, ntaps, stride, T);
  if (rc) return rc;
  if ((rc = check_conv_dims(mk(ddim), mk(sdim), T))) return rc;
  launch_conv_up(src, mk(sdim), T, make_scaling(scl, scl_dim), dst, mk(ddim), (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

// (each forward-only name is its _which sibling with UNIRES_DIFF_FORWARD)
extern "C" int unires_grad_which(const float *src, const int32_t dim[3], const float vx[3], int32_t which,
                                 float *dst3, void *stream) {
  if (!src || !dst3 || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (!vx_ok(vx)) return fail(UNIRES_ERR_ARG, "voxel size must be positive");
  if (!diff_ok(which)) return fail(UNIRES_ERR_ARG, "which: forward (0), backward (1) or central (2)");
  launch_grad(src, mk(dim), vx, dst3, (hipStream_t)stream, which);
  CHECK_LAUNCH();
  return UNIRES_OK;
}
extern "C" int unires_grad_fwd_zero(const float *src, const int32_t dim[3], const float vx[3],
                                    float *dst3, void *stream) {
  return unires_grad_which(src, dim, vx, UNIRES_DIFF_FORWARD, dst3, stream);
}

extern "C" int unires_div_which(const float *src3, const int32_t dim[3], const float vx[3], int32_t which,
                                float *dst, void *stream) {
  if (!src3 || !dst || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (!vx_ok(vx)) return fail(UNIRES_ERR_ARG, "voxel size must be positive");
  if (!diff_ok(which)) return fail(UNIRES_ERR_ARG, "which: forward (0), backward (1) or central (2)");
  launch_div(src3, nullptr, 1.f, 0.f, mk(dim), vx, 1.f, nullptr, dst, (hipStream_t)stream, which);
  CHECK_LAUNCH();
  return UNIRES_OK;
}
extern "C" int unires_div_fwd_zero(const float *src3, const int32_t dim[3], const float vx[3],
                                   float *dst, void *stream) {
  return unires_div_which(src3, dim, vx, UNIRES_DIFF_FORWARD, dst, stream);
}

extern "C" int unires_dtd_which(const float *src, const int32_t dim[3], const float vx[3], int32_t which,
                                float a, float c, float *dst, void *stream) {
  if (!src || !dst || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (!vx_ok(vx)) return fail(UNIRES_ERR_ARG, "voxel size must be positive");
  if (!diff_ok(which)) return fail(UNIRES_ERR_ARG, "which: forward (0), backward (1) or central (2)");
  if (src == dst) return fail(UNIRES_ERR_ARG, "dtd cannot run in place");
  launch_dtd(src, mk(dim), vx, a, c, dst, nullptr, nullptr, nullptr, (hipStream_t)stream, which);
  CHECK_LAUNCH();
  return UNIRES_OK;
}
extern "C" int unires_dtd(const float *src, const int32_t dim[3], const float vx[3], float a,
                          float c, float *dst, void *stream) {
  return unires_dtd_which(src, dim, vx, UNIRES_DIFF_FORWARD, a, c, dst, stream);
}

// --------------------------------------------------------------------------
// z / w updates and objective sums  (unires/_update.py:154-195, 396-427)
// --------------------------------------------------------------------------
static int check_channels(const float *const *y_ptrs, const float *lam, int32_t n) {
  if (!y_ptrs || !lam) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 1 || n > 4096) return fail(UNIRES_ERR_ARG, "channel count out of range");
  for (int c = 0; c < n; ++c)
    if (!y_ptrs[c]) return fail(UNIRES_ERR_NULL, "null channel pointer");
  return UNIRES_OK;
}

extern "C" int unires_zw_update_which(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                                      const int32_t dim[3], const float vx[3], int32_t which, float rho,
                                      float alpha, float *z, float *w, float *jtv, void *stream) {
  int rc = check_channels(y_ptrs, lam, n_channels);
  if (rc) return rc;
  if (!diff_ok(which)) return fail(UNIRES_ERR_ARG, "which: forward (0), backward (1) or central (2)");
  if (!z || !w || !jtv || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (!vx_ok(vx)) return fail(UNIRES_ERR_ARG, "voxel size must be positive");
  if (!(rho > 0.f)) return fail(UNIRES_ERR_ARG, "rho must be positive");
  hipStream_t st = (hipStream_t)stream;
  const Dim3i d = mk(dim);
  launch_jtv_scale(y_ptrs, lam, n_channels, w, z, d, vx, rho, alpha, jtv, nullptr, nullptr, 0, st, which);
  const size_t n = d.numel();
  for (int c = 0; c < n_channels; ++c)
    launch_zw_update(y_ptrs[c], lam[c], jtv, z + (size_t)c * 3 * n, w + (size_t)c * 3 * n, d, vx,
                     rho, alpha, st, which);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_zw_update(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                                const int32_t dim[3], const float vx[3], float rho, float alpha,
                                float *z, float *w, float *jtv, void *stream) {
  return unires_zw_update_which(y_ptrs, lam, n_channels, dim, vx, UNIRES_DIFF_FORWARD, rho, alpha, z, w, jtv, stream);
}

extern "C" int unires_nll_prior_which(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                                      const int32_t dim[3], const float vx[3], int32_t which, double *out_dev,
                                      void *stream) {
  int rc = check_channels(y_ptrs, lam, n_channels);
  if (rc) return rc;
  if (!diff_ok(which)) return fail(UNIRES_ERR_ARG, "which: forward (0), backward (1) or central (2)");
  if (!out_dev || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dimensions");
  if (!vx_ok(vx)) return fail(UNIRES_ERR_ARG, "voxel size must be positive");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(double), st));
  // more than 8 channels: the running sum of squares needs a volume of scratch.  It is kept (one per
  // device, grown on demand, used in stream order by the chained launches) instead of allocated and freed
  // per call: no allocation inside a stream capture, nothing to leak on an error path
  float *acc = nullptr;
  if (n_channels > 8) {
    static std::mutex mu;
    static std::map<int, std::pair<float *, size_t>> scratch;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const size_t need = mk(dim).numel() * sizeof(float);
    std::lock_guard<std::mutex> lock(mu);
    auto &slot = scratch[dev];
    if (slot.second < need) {
      if (slot.first) {
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(slot.first);
        slot = {nullptr, 0};
      }
      HIP_TRY(hipMalloc((void **)&slot.first, need));
      slot.second = need;
    }
    acc = slot.first;
  }
  double *part = nullptr;
  if ((rc = reduce_scratch(st, (size_t)jtv_scale_blocks(mk(dim)), &part))) return rc;
  launch_jtv_scale(y_ptrs, lam, n_channels, nullptr, nullptr, mk(dim), vx, 1.f, 1.f, acc, part, out_dev, 1, st, which);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_nll_prior(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                                const int32_t dim[3], const float vx[3], double *out_dev,
                                void *stream) {
  return unires_nll_prior_which(y_ptrs, lam, n_channels, dim, vx, UNIRES_DIFF_FORWARD, out_dev, stream);
}

extern "C" int unires_scaling_sums(const float *x, const float *ay, const int32_t dim[3],
                                   int32_t dim_thick, double *out_dev, void *stream) {
  if (!x || !ay || !dim || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (dim_thick < 0 || dim_thick > 2) return fail(UNIRES_ERR_ARG, "bad dim_thick");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  if (int rc = reduce_scratch(st, 5 * (size_t)scaling_sums_blocks(mk(dim)), &part)) return rc;
  launch_scaling_sums(x, ay, mk(dim), dim_thick, nullptr, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_scaling_sums_w(const float *x, const float *ay, const int32_t dim[3], int32_t dim_thick,
                                     const float *u_dev, double *out_dev, void *stream) {
  if (!x || !ay || !dim || !u_dev || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (dim_thick < 0 || dim_thick > 2) return fail(UNIRES_ERR_ARG, "bad dim_thick");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  if (int rc = reduce_scratch(st, 5 * (size_t)scaling_sums_blocks(mk(dim)), &part)) return rc;
  launch_scaling_sums(x, ay, mk(dim), dim_thick, u_dev, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_scaling_sums_g(const float *x, const float *ay, const int32_t dim[3], int32_t dim_thick,
                                     const float *g_dev, const float *u_dev, double *out_dev, void *stream) {
  if (!x || !ay || !dim || !g_dev || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (dim_thick < 0 || dim_thick > 2) return fail(UNIRES_ERR_ARG, "bad dim_thick");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  if (int rc = reduce_scratch(st, 5 * (size_t)scaling_sums_blocks(mk(dim)), &part)) return rc;
  launch_scaling_sums_g(x, ay, g_dev, mk(dim), dim_thick, u_dev, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rigid_sums(const float *gr3, const float *diff, const float *ctc,
                                 const int32_t dim[3], const float d_rigid[72], double *out_dev,
                                 void *stream) {
  if (!gr3 || !diff || !dim || !d_rigid || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  hipStream_t st = (hipStream_t)stream;
  float D[6][12];
  memcpy(D, d_rigid, sizeof(D));
  double *part = nullptr;
  if (int rc = reduce_scratch(st, 27 * (size_t)rigid_sums_blocks(mk(dim)), &part)) return rc;
  launch_rigid_sums(gr3, diff, ctc, mk(dim), D, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_clean_fov(float *y, const int32_t dim_y[3], const float M[12],
                                const int32_t dim_x[3], void *stream) {
  if (!y || !dim_y || !M || !dim_x) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim_y) || !dims_ok(dim_x)) return fail(UNIRES_ERR_DIM, "bad dims");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  launch_clean_fov(y, mk(dim_y), A, mk(dim_x), (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_masked_sse(const float *x, const float *ay, int64_t n, double *out_dev,
                                 void *stream) {
  if (!x || !ay || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 1) return fail(UNIRES_ERR_DIM, "bad length");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  if (int rc = reduce_scratch(st, (size_t)masked_sse_blocks((size_t)n), &part)) return rc;
  launch_masked_sse(x, ay, (size_t)n, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_slice_sums(const float *x, const float *ay, const int32_t dim[3], int32_t dim_thick,
                                 double *out_dev, void *stream) {
  if (!x || !ay || !dim || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (dim_thick < 0 || dim_thick > 2) return fail(UNIRES_ERR_ARG, "bad dim_thick");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  const size_t cols = 2 * (size_t)dim[dim_thick];
  if (int rc = reduce_scratch(st, cols * (size_t)slice_sums_parts(mk(dim), dim_thick), &part)) return rc;
  launch_slice_sums(x, ay, mk(dim), dim_thick, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_voxel_sums(const float *x, const float *ay, const float *g, const int32_t dim[3],
                                 int32_t dim_thick, double *out_dev, void *stream) {
  if (!x || !ay || !g || !dim || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (dim_thick < 0 || dim_thick > 2) return fail(UNIRES_ERR_ARG, "bad dim_thick");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  const size_t cols = 2 * (size_t)dim[dim_thick];
  if (int rc = reduce_scratch(st, cols * (size_t)slice_sums_parts(mk(dim), dim_thick), &part)) return rc;
  launch_voxel_sums(x, ay, g, mk(dim), dim_thick, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_gain_sums(const float *x, const float *ay, const float *g, const float *u, const int32_t dim[3],
                                int32_t dim_thick, double *out_dev, void *stream) {
  if (!x || !ay || !dim || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (dim_thick < 0 || dim_thick > 2) return fail(UNIRES_ERR_ARG, "bad dim_thick");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  const size_t cols = 3 * (size_t)dim[dim_thick];
  if (int rc = reduce_scratch(st, cols * (size_t)slice_sums_parts(mk(dim), dim_thick), &part)) return rc;
  launch_gain_sums(x, ay, g, u, mk(dim), dim_thick, part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rigid_terms_e(const float *x, const float *ay, const float *g, const float *u, const float *e,
                                    const int32_t dim[3], int32_t axis, double *sums_dev, float *out, void *stream) {
  if (!x || !ay || !e || !dim || !sums_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "bad axis");
  if (out && (out == x || out == g)) return fail(UNIRES_ERR_ARG, "out must not be x or g: they are only read");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  const size_t cols = 2 * (size_t)dim[axis];
  if (int rc = reduce_scratch(st, cols * (size_t)slice_sums_parts(mk(dim), axis), &part)) return rc;
  launch_rigid_terms_e(x, ay, g, u, e, mk(dim), axis, part, sums_dev, out, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rician_terms(const float *x, const float *ay, const float *g, const float *e, const int32_t dim[3],
                                   int32_t axis, float tau, float *xt, double *sums_dev, void *stream) {
  if (!x || !ay || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "bad axis");
  if (!xt && !sums_dev) return fail(UNIRES_ERR_ARG, "nothing to write: xt and sums are both null");
  if (xt && (xt == x || xt == g)) return fail(UNIRES_ERR_ARG, "xt must not be x or g: they are only read");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  if (sums_dev)
    if (int rc = reduce_scratch(st, (size_t)dim[axis] * (size_t)slice_sums_parts(mk(dim), axis), &part)) return rc;
  launch_rician_terms(x, ay, g, e, mk(dim), axis, tau, xt, part, sums_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rigid_terms_r(const float *x, const float *ay, const float *g, const float *u, const float *e,
                                    const int32_t dim[3], int32_t axis, float tau, double *sums_dev, float *out,
                                    void *stream) {
  if (!x || !ay || !dim || !sums_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "bad axis");
  if (out && (out == x || out == g)) return fail(UNIRES_ERR_ARG, "out must not be x or g: they are only read");
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  const size_t cols = 3 * (size_t)dim[axis];
  if (int rc = reduce_scratch(st, cols * (size_t)slice_sums_parts(mk(dim), axis), &part)) return rc;
  launch_rigid_terms_r(x, ay, g, u, e, mk(dim), axis, tau, part, sums_dev, out, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_bias_field(const double *coef, const double *tx, const double *ty, const double *tz,
                                 const int32_t order[3], const int32_t dim[3], double beta_max, const float *g,
                                 const float *x, float *b, float *gb2, float *xb, void *stream) {
  if (!coef || !tx || !ty || !tz || !order || !dim || !b) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  for (int a = 0; a < 3; ++a)
    if (order[a] < 1 || order[a] > kBiasMaxOrder) return fail(UNIRES_ERR_ARG, "bias orders: 1 .. 8 along every axis");
  if (!(beta_max > 0.0)) return fail(UNIRES_ERR_ARG, "the bound on log b must be positive");
  if (xb && !x) return fail(UNIRES_ERR_NULL, "x / b needs x");
  if (b == x || b == g || (gb2 && (gb2 == x || gb2 == g || gb2 == b)) || (xb && (xb == x || xb == g || xb == b || xb == gb2)))
    return fail(UNIRES_ERR_ARG, "b, gb2 and xb must be buffers of their own: x and g are only read");
  launch_bias_field(coef, tx, ty, tz, mk(order), mk(dim), beta_max, g, x, b, gb2, xb, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_bias_terms(const float *x, const float *mu, const float *b, const float *g, const float *u,
                                 int32_t axis, const double *tx, const double *ty, const double *tz,
                                 const int32_t order[3], const int32_t dim[3], double *out_dev, void *stream) {
  if (!x || !mu || !b || !order || !dim || !out_dev) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "bad axis");
  const bool none = order[0] == 0 && order[1] == 0 && order[2] == 0;
  if (!none) {
    for (int a = 0; a < 3; ++a)
      if (order[a] < 1 || order[a] > kBiasMaxOrder)
        return fail(UNIRES_ERR_ARG, "bias orders: 1 .. 8 along every axis, or all 0 for the objective alone");
    if (!tx || !ty || !tz) return fail(UNIRES_ERR_NULL, "null argument");
  }
  hipStream_t st = (hipStream_t)stream;
  double *part = nullptr;
  if (int rc = reduce_scratch(st, bias_terms_scratch(mk(dim), mk(order)), &part)) return rc;
  launch_bias_terms(x, mu, b, g, u, axis, tx, ty, tz, mk(order), mk(dim), part, out_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_slice_apply(const float *src, float *dst, const float *u, const int32_t dim[3], int32_t axis,
                                  void *stream) {
  if (!src || !dst || !u || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "slice axis: 0, 1 or 2");
  launch_slice_apply(src, dst, nullptr, u, mk(dim), axis, false, nullptr, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_voxel_apply(const float *src, float *dst, const float *g, const uint8_t *mask, const float *u,
                                  const int32_t dim[3], int32_t axis, int32_t flip, const int32_t *done, void *stream) {
  if (!src || !dst || !g || !dim) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "slice axis: 0, 1 or 2");
  launch_voxel_apply(src, dst, g, mask, u, mk(dim), axis, flip != 0, done, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_voxel_huber(const float *x, const float *ay, const float *prior, float c, int64_t n,
                                  float *g_out, void *stream) {
  if (!x || !ay || !g_out) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 0) return fail(UNIRES_ERR_DIM, "bad length");
  if (!(c > 0.f)) return fail(UNIRES_ERR_ARG, "the Huber threshold must be positive");
  launch_voxel_huber(x, ay, prior, c, (size_t)n, g_out, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rigid_resid(const float *x, const float *ay, const int32_t dim[3], int32_t axis,
                                  const float *u_dev, float *out, void *stream) {
  if (!x || !ay || !dim || !out) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "bad axis");
  launch_rigid_resid(x, ay, out, u_dev, mk(dim), axis, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rigid_resid_g(const float *x, const float *ay, const float *g, const int32_t dim[3], int32_t axis,
                                    const float *u_dev, float *out, void *stream) {
  if (!x || !ay || !g || !dim || !out) return fail(UNIRES_ERR_NULL, "null argument");
  if (!dims_ok(dim)) return fail(UNIRES_ERR_DIM, "bad dims");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "bad axis");
  if (out == g) return fail(UNIRES_ERR_ARG, "out must not be g: the weights are only read");
  launch_rigid_resid_g(x, ay, g, out, u_dev, mk(dim), axis, (hipStream_t)stream);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

// --------------------------------------------------------------------------
// Stream marks (round 5): how a host thread follows its GPU WITHOUT runtime calls.
// Every hipEventQuery / hipStreamQuery on work that is still running makes the runtime submit a marker
// packet whose completion wakes its signal thread, which then polls for a while before it sleeps again:
// measured on the MI355X box (tools/host_profile.py, profiles/r05_host_profile.txt) that helper thread
// cost 4.3 ms of CPU per 13.6 ms ADMM iteration under a 0.5 ms event poll.  A mark is a word of mapped host
// memory that a one-thread kernel sets when the stream gets there: the host reads memory, nothing else.
// --------------------------------------------------------------------------
struct unires_mark {
  unsigned long long *host = nullptr;
  unsigned long long *dev = nullptr;
};

__global__ void k_mark(unsigned long long *w, unsigned long long v) {
  __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" int unires_mark_create(unires_mark_t **out) {
  if (!out) return fail(UNIRES_ERR_NULL, "null argument");
  *out = nullptr;
  unires_mark *m = new (std::nothrow) unires_mark;
  if (!m) return fail(UNIRES_ERR_ALLOC, "out of host memory");
  // (portable: a process that drives several devices may signal the mark from any of them)
  if (hipHostMalloc((void **)&m->host, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    delete m;
    return fail(UNIRES_ERR_ALLOC, "hipHostMalloc failed");
  }
  *m->host = 0ull;
  if (hipHostGetDevicePointer((void **)&m->dev, (void *)m->host, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipHostFree(m->host);
    delete m;
    return fail(UNIRES_ERR_HIP, "hipHostGetDevicePointer failed");
  }
  *out = m;
  return UNIRES_OK;
}

extern "C" int unires_mark_destroy(unires_mark_t *m) {
  if (!m) return UNIRES_OK;
  if (m->host) (void)hipHostFree(m->host);  // (waits for the device: no kernel writes it afterwards)
  delete m;
  return UNIRES_OK;
}

extern "C" int unires_mark_signal(unires_mark_t *m, uint64_t value, void *stream) {
  if (!m) return fail(UNIRES_ERR_NULL, "null argument");
  hipLaunchKernelGGL(k_mark, dim3(1), dim3(1), 0, (hipStream_t)stream, m->dev, (unsigned long long)value);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_mark_read(const unires_mark_t *m, uint64_t *value) {
  if (!m || !value) return fail(UNIRES_ERR_NULL, "null argument");
  *value = (uint64_t)__atomic_load_n(m->host, __ATOMIC_ACQUIRE);
  return UNIRES_OK;
}
