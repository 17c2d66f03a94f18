/*
 * unires_hip.h - C ABI of libunires_hip.so: the MI355X (gfx950) implementation of
 * the UniRes ADMM y-update hot path.
 *
 * All volumes are float32, C-contiguous (X,Y,Z) with Z fastest, resident in
 * device memory; all `dim`/`M`/`taps`/descriptor arguments are HOST pointers
 * read during the call (never retained).  Every entry point returns an int
 * status (0 = OK) and never throws; unires_last_error() gives the message of
 * the calling thread's last failure.  Kernels are launched on the caller's
 * stream (`stream` is a hipStream_t passed as void*; NULL = default stream).
 * No entry point synchronises a stream, except unires_cg_solve when the caller asks for
 * the realised iteration count / objective trace on the host.  (A solve that can stop
 * early - tol > 0 - keeps the calling thread until its last chunk of iterations is
 * enqueued; it watches a host-mapped progress word, not the stream.)
 *
 * The reference (brudfors/UniRes) has no FFI layer: its seam is Python calls
 * into nitorch + torch.  Each entry point below cites the
 * reference call it replaces (paths relative to the reference tree).
 */
#ifndef UNIRES_HIP_H
#define UNIRES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNIRES_HIP_ABI_VERSION 1
#define UNIRES_MAX_TAPS 32 /* per axis */

enum unires_status {
  UNIRES_OK = 0,
  UNIRES_ERR_NULL = 1,        /* null pointer argument                         */
  UNIRES_ERR_DIM = 2,         /* inconsistent / non-positive dimensions        */
  UNIRES_ERR_ARG = 3,         /* bad enum / value ("Undefined operator" ...)   */
  UNIRES_ERR_HIP = 4,         /* HIP runtime error (message has hipGetErrorString) */
  UNIRES_ERR_ALLOC = 5,       /* device allocation failed                      */
  UNIRES_ERR_UNSUPPORTED = 6  /* valid request this build cannot serve         */
};

/* unires/_project.py:122-126: 'A' | 'At' | 'AtA' ('none' is regime 0) */
enum unires_operator { UNIRES_OP_A = 0, UNIRES_OP_AT = 1, UNIRES_OP_ATA = 2 };

/* unires/_core.py:209-260 selects one of three operator regimes */
enum unires_regime {
  UNIRES_REGIME_IDENTITY = 0, /* sett.do_proj == False: A = I   (_project.py:76-77,91-92) */
  UNIRES_REGIME_DENOISE = 1,  /* method 'denoising': A = pull   (_project.py:180-188)     */
  UNIRES_REGIME_SUPERRES = 2  /* method 'super-resolution': A = S conv_down pull (:161-179) */
};

/* nitorch cg(stop=...) objective branch */
enum unires_cg_stop {
  UNIRES_STOP_RESIDUAL = 0,       /* 'e': obj = sqrt(r.z)                                  */
  UNIRES_STOP_MAXGAIN = 1,        /* anything else, e.g. 'max_gain' as UniRes passes
                                     (_update.py:145): obj = 0.5*sum(x*(A(x)-2b)),
                                     one extra A(x) per iteration (reference-faithful)     */
  UNIRES_STOP_MAXGAIN_RECURRED = 2, /* same objective from the recurred residual,
                                     obj = -0.5*sum(x*(b+r)): no extra A(x) (build-side)   */
  UNIRES_STOP_MAXGAIN_GUARDED = 3  /* the recurred objective while its gain is >= 4 tol, the fresh one
                                     (mode 1's) from there on: mode 1's decisions - both values of a close
                                     gain are fresh ones - at about mode 2's cost                          */
};

enum unires_precond {
  UNIRES_PRECOND_IDENTITY = 0, /* the reference's only live mode (_update.py:136-137) */
  UNIRES_PRECOND_JACOBI = 1,   /* _precond (_update.py:80-102), commented out at :136:
                                  z = r / (tau AtA(1) + 2 rho lam^2 sum_d 1/vx_d^2)         */
  UNIRES_PRECOND_FFT = 2       /* build-side extension (not in the reference): exact inverse of
                                  the circulant operator a I + rho lam^2 sum_d L_d / vx_d^2 with
                                  periodic second differences L_d, a = mean diagonal of
                                  sum_n tau_n AtA_n; two rocFFT real 3-D transforms per call  */
};

const char *unires_last_error(void);
int unires_abi_version(void);

/* ------------------------------------------------------------------------
 * Op level - one call per nitorch / torch function on the path
 * ---------------------------------------------------------------------- */

/* nitorch grid_pull(src, affine_grid(M, gdim), 'linear', bound='zero',
 * extrapolate=False)  (_project.py:159,164,174,183,187).  M is the row-major
 * 3x4 float32 affine mapping a grid voxel (i,j,k) to src voxel coordinates.
 * dst[gdim] is overwritten. fov_tol = nitorch's in-FOV tolerance (5e-2). */
int unires_pull3d_affine(const float *src, const int32_t sdim[3], const float M[12], float *dst,
                         const int32_t gdim[3], float fov_tol, void *stream);

/* The reference's _warp_label(label, affine_grid(M, gdim)) (unires/_core.py:419-436): for every
 * distinct value u of label, ascending, p_u = the pull above of the indicator (label == u), and
 * dst = u wherever p_u > the best so far (which starts at 0).  One gather per output voxel:
 * ties go to the smallest value, a best of 0 gives 0, p_u has the bits of the pull's product
 * form.  label holds any float32 values (the caller checks there are at most 255). */
int unires_warp_label(const float *label, const int32_t ldim[3], const float M[12], float *dst,
                      const int32_t gdim[3], float fov_tol, void *stream);

/* nitorch grid_pull(src, affine_grid(M, gdim), 0, bound='zero', extrapolate=False)
 * (unires/_core.py:484): src at the voxel rint(M g) (half-way cases to even) when that voxel is
 * inside the volume and M g inside the FOV, else 0. */
int unires_pull3d_nearest(const float *src, const int32_t sdim[3], const float M[12], float *dst,
                          const int32_t gdim[3], float fov_tol, void *stream);

/* Noise / intensity hyper-parameters (the reference's _estimate_hyperpar -> nitorch estimate_noise,
 * unires/_core.py:96-142; DESIGN 8.1 states the estimator).  Step 1: the masked range and 1024-bin
 * histogram of n_obs observations in one pass.  ptrs / sizes / ct: HOST arrays of n_obs device
 * pointers to float32 voxels, their counts (1 .. 2^32 - 1) and CT flags.  Voxels taken: finite,
 * non-zero, and >= 0 unless ct[o].  counts: (n_obs, 1024) uint32 device, overwritten;
 * range: (n_obs, 2) float32 device = (min, max) of the voxels taken (+inf, -inf when none).
 * Bin of v: floor((v - min) * 1024 / (max - min)) in float64, clamped to 1023. */
int unires_noise_hist(int32_t n_obs, const float *const *ptrs, const int64_t *sizes, const int32_t *ct,
                      uint32_t *counts, float *range, void *stream);

/* Step 2: a two-class float64 EM fit of every histogram in one launch - Rice when range min >= 0,
 * Gaussian otherwise - stopped when the log-likelihood gains less than 1e-8 x the voxel count, or
 * after max_iter M-steps.  out: (n_obs, 16) float64 device: mg0 mg1, nu|mu 0 1, sigma 0 1, class
 * mean 0 1, final ll, M-steps, sd (sigma of the class with the smaller mean), |mean_fg - mean_bg|,
 * model (0 Rice, 1 Gaussian, -1 = no voxels or min == max: only [12..15] are meaningful), sum of
 * counts, min, max. */
int unires_noise_fit(int32_t n_obs, const uint32_t *counts, const float *range, int32_t max_iter,
                     double *out, void *stream);

/* Rigid coregistration by (normalised) mutual information (the reference's _init_reg -> nitorch
 * affine_align, unires/_core.py:310-368; DESIGN 8.2 states the estimator).  Step 1: uint8
 * quantisation of n_obs observations.  ptrs / sizes / outs: HOST arrays of n_obs device pointers to
 * float32 voxels, their counts (1 .. 2^32 - 1) and uint8 outputs of the same size.
 * counts: (n_obs, 1024) uint32 device, overwritten: histogram of the finite voxels over [min, max].
 * params: (n_obs, 8) float32 device, overwritten: min, max, robust maximum mx, 255 / (mx - min),
 * status (0 ok, 1 no finite voxel, 2 all finite voxels equal: the output is all 0), 3 scratch. */
int unires_coreg_quantise(int32_t n_obs, const float *const *ptrs, const int64_t *sizes,
                          uint8_t *const *outs, uint32_t *counts, float *params, void *stream);

/* One joint-histogram job: the fixed image G and the moving image F (uint8, C-contiguous,
 * every dimension >= 2), M (float32 row-major 3x4) maps a G voxel to an F voxel, step: the
 * sampling step in G voxels per axis (> 0). */
typedef struct {
  const uint8_t *G;
  const uint8_t *F;
  int32_t dim_g[3];
  int32_t dim_f[3];
  float M[12];
  float step[3];
} unires_coreg_job_t;

/* Step 2: the partial-volume joint histograms of n_jobs jobs (HOST array) in one launch.
 * hist: (n_jobs, 256, 256) uint64 device, overwritten: hist[j][g][f] in Q16 units (every sample
 * point inside G adds 65536; a point whose image falls outside F counts as f = 0).  At most 2^31 - 1 sample points per job. */
int unires_coreg_hist(int32_t n_jobs, const unires_coreg_job_t *jobs, uint64_t *hist, void *stream);

/* Voxel weight maps in the initialisation: the support of a map - g(v) > 0 - decides
 * which voxels the noise estimator, the coregistration and the first guess read.
 *
 * unires_noise_hist under weight maps.  gptrs: a HOST array of n_obs device pointers to float32 maps
 * of the same sizes; an entry, or the array, may be NULL (that observation is read as by
 * unires_noise_hist).  Voxels taken: those unires_noise_hist takes whose weight is > 0.  The 16-byte
 * loads are used where an observation AND its map are 16-byte aligned. */
int unires_noise_hist_g(int32_t n_obs, const float *const *ptrs, const int64_t *sizes, const int32_t *ct,
                        const float *const *gptrs, uint32_t *counts, float *range, void *stream);

/* unires_coreg_quantise under supports.  masks: a HOST array of n_obs device pointers to uint8
 * supports of the same sizes (non-zero usable, 0 not); an entry, or the array, may be NULL.  min, max,
 * the 1024-bin histogram and the robust maximum are those of the finite USABLE voxels; every finite
 * voxel, usable or not, is converted with them (clamped to 0 .. 255).  Status 1: no finite usable
 * voxel; 2: all of them equal. */
int unires_coreg_quantise_m(int32_t n_obs, const float *const *ptrs, const int64_t *sizes,
                            const uint8_t *const *masks, uint8_t *const *outs, uint32_t *counts,
                            float *params, void *stream);

/* Cell support of a uint8 support: cell[i0, i1, i2] = 1 iff the eight voxels (i0..i0+1, i1..i1+1,
 * i2..i2+1) of mask are non-zero, for i_d <= dim_d - 2; the last plane of every axis (no cell
 * starts there; unires_coreg_hist_m never reads it) is written 0.  cell has mask's shape and is
 * not mask. */
int unires_coreg_cellmask(const uint8_t *mask, const int32_t dim[3], uint8_t *cell, void *stream);

/* unires_coreg_job_t, then the cell supports (unires_coreg_cellmask) of G and of F; either may be
 * NULL. */
typedef struct {
  const uint8_t *G;
  const uint8_t *F;
  int32_t dim_g[3];
  int32_t dim_f[3];
  float M[12];
  float step[3];
  const uint8_t *mG;
  const uint8_t *mF;
} unires_coreg_job_m_t;

/* unires_coreg_hist under cell supports.  The cell of a point is the one its interpolation reads,
 * i_d = min(floor(x_d), dim_d - 2).  A sample point inside G whose G cell has mG == 0 adds nothing;
 * neither does one whose image lies inside F in a cell with mF == 0.  A point whose image falls
 * outside F counts as f = 0 whatever mF holds.  No voxel outside a support is interpolated into a
 * counted sample. */
int unires_coreg_hist_m(int32_t n_jobs, const unires_coreg_job_m_t *jobs, uint64_t *hist, void *stream);

/* Support of unires_pull3d_affine(., sdim, M, ., gdim, fov_tol) under the weight map g (sdim,
 * float32): dst[gdim] (uint8) = 1 iff the coordinate c = M (i,j,k) is inside the FOV by the pull's
 * rule and every corner (floor(c_d) | floor(c_d) + 1 per axis) that lies inside the volume has
 * g > 0; else 0.  Corners outside the volume add 0 to the pull and do not decide.  The coordinate is
 * computed by the pull's own device code. */
int unires_pull3d_support(const float *g, const int32_t sdim[3], const float M[12], uint8_t *dst,
                          const int32_t gdim[3], float fov_tol, void *stream);

/* Step 3: the cost of n histograms in one launch.  cost_fun: 0 'nmi', 1 'mi', 2 'ecc'; fwhm: the
 * histogram smoothing in bins (0 <= fwhm <= 16).  work: n x 2 x 256 x 256 float64 device scratch;
 * cost: (n,) float64 device. */
int unires_coreg_cost(int32_t n, const uint64_t *hist, int32_t cost_fun, double fwhm, double *work,
                      double *cost, void *stream);

/* nitorch grid_grad(src, affine_grid(M, gdim), 'linear', bound='zero', extrapolate=False)
 * (_update.py:508, the rigid Gauss-Newton's spatial derivatives): gradient of the trilinear
 * sample w.r.t. the voxel coordinate; dst3 is (gdim, 3), component fastest. */
int unires_pull_grad3d_affine(const float *src, const int32_t sdim[3], const float M[12],
                              float *dst3, const int32_t gdim[3], float fov_tol, void *stream);

/* nitorch grid_push(src, affine_grid(M, gdim), shape=ddim, ...)
 * (_project.py:172,179,185,188): dst (+)= alpha * push(src).
 * accumulate == 0 overwrites dst. */
int unires_push3d_affine(const float *src, const int32_t gdim[3], const float M[12], float *dst,
                         const int32_t ddim[3], float alpha, float fov_tol, int accumulate,
                         void *stream);

/* F.conv3d(src, smo_ker, stride)  (_project.py:153) with a separable kernel
 * smo_ker = taps[0] (x) taps[1] (x) taps[2] (cross-correlation, no padding), followed
 * by the optional even/odd slice scaling of _apply_scaling (_project.py:9-24):
 * slices with even index along scl_dim are multiplied by exp(scl), odd by
 * exp(-scl); scl == 0 skips it.  Requires sdim = (ddim-1)*stride + ntaps. */
int unires_conv_down3d(const float *src, const int32_t sdim[3], const float *const taps[3],
                       const int32_t ntaps[3], const int32_t stride[3], float *dst,
                       const int32_t ddim[3], float scl, int32_t scl_dim, void *stream);

/* F.conv_transpose3d(S(scl) src, smo_ker, stride)  (_project.py:154,168-171): exact
 * adjoint of unires_conv_down3d, scaling applied to the INPUT.  src has sdim
 * (low-res), dst has ddim = (sdim-1)*stride + ntaps and is overwritten. */
int unires_conv_up3d(const float *src, const int32_t sdim[3], const float *const taps[3],
                     const int32_t ntaps[3], const int32_t stride[3], float *dst,
                     const int32_t ddim[3], float scl, int32_t scl_dim, void *stream);

/* nitorch im_gradient(src, vx, bound='zero', which='forward')
 * (_project.py:314; _update.py:168,176,188,419): dst is (3,X,Y,Z). */
int unires_grad_fwd_zero(const float *src, const int32_t dim[3], const float vx[3], float *dst3,
                         void *stream);

/* nitorch im_divergence(src3, vx, bound='zero', which='forward') - the POSITIVE
 * adjoint of the gradient (_project.py:315; _update.py:132). */
int unires_div_fwd_zero(const float *src3, const int32_t dim[3], const float vx[3], float *dst,
                        void *stream);

/* dst = a*src + c*DtD(src): _DtD (_project.py:300-317) fused with the scalar
 * multiply-add of _proj (_project.py:87). */
int unires_dtd(const float *src, const int32_t dim[3], const float vx[3], float a, float c,
               float *dst, void *stream);

/* The difference the regulariser's D takes (nitorch diff1d / div1d `which`, the reference's sett.diff; zero bound:
 * samples outside the volume read as 0).  Restated from nitorch's published definitions  [recalled]:
 *   forward : (D y)[i] = (y[i+1] - y[i]) / vx         (Dt g)[i] = (g[i-1] - g[i]) / vx
 *   backward: (D y)[i] = (y[i] - y[i-1]) / vx         (Dt g)[i] = (g[i] - g[i+1]) / vx
 *   central : (D y)[i] = (y[i+1] - y[i-1]) / (2 vx)   (Dt g)[i] = (g[i-1] - g[i+1]) / (2 vx)
 * Any other value is UNIRES_ERR_ARG.  UNIRES_DIFF_FORWARD gives the bits of the entry points without `which`. */
#define UNIRES_DIFF_FORWARD 0
#define UNIRES_DIFF_BACKWARD 1
#define UNIRES_DIFF_CENTRAL 2

/* unires_grad_fwd_zero / unires_div_fwd_zero / unires_dtd with the difference chosen. */
int unires_grad_which(const float *src, const int32_t dim[3], const float vx[3], int32_t which,
                      float *dst3, void *stream);
int unires_div_which(const float *src3, const int32_t dim[3], const float vx[3], int32_t which,
                     float *dst, void *stream);
int unires_dtd_which(const float *src, const int32_t dim[3], const float vx[3], int32_t which, float a,
                     float c, float *dst, void *stream);

/* ------------------------------------------------------------------------
 * Fused level - plan + matvec + RHS + CG  (unires/_update.py:118-152)
 * ---------------------------------------------------------------------- */

/* One observation ("repeat") of a channel: the fields of _proj_op
 * (struct.py:36-54) that the operators read, flattened. */
typedef struct unires_repeat {
  int32_t dim_x[3];  /* observed image dims                                             */
  int32_t dim_g[3];  /* grid dims: dim_yx (super-resolution) or dim_x (denoising)       */
  float M[12];       /* float32(mat_y \ (rigid*mat_yx|mat_x)), row-major 3x4 (:147,150,159) */
  int32_t ratio[3];  /* conv stride (:153)                                              */
  int32_t ntaps[3];  /* separable factors of smo_ker (:277)                             */
  const float *taps[3]; /* HOST pointers, ntaps[d] floats each                          */
  float scl;         /* even/odd slice scaling parameter po.scl (:287-290); 0 = off     */
  int32_t dim_thick; /* axis the scaling runs along (:241)                              */
  float tau;         /* noise precision x[c][n].tau (_core.py:134-136)                  */
} unires_repeat_t;

typedef struct unires_plan unires_plan_t;

/* Builds the per-channel operator  sum_n tau_n A_n^T A_n + rho lam^2 D^T D  and
 * allocates every workspace it will ever need (r, p, Ap, one grid-space and one
 * x-space intermediate, reduction partials).  Nothing is allocated afterwards. */
int unires_plan_create(unires_plan_t **plan, const int32_t dim_y[3], const float vx_y[3],
                       int32_t regime, int32_t n_repeats, const unires_repeat_t *repeats,
                       float fov_tol);
int unires_plan_destroy(unires_plan_t *plan);
/* Replace repeat n's descriptor (after a rigid / scaling update; _update.py:576). */
int unires_plan_set_repeat(unires_plan_t *plan, int32_t n, const unires_repeat_t *repeat);
/* Hint: the caller keeps `n_concurrent` solves (this plan's and other plans') in flight on the device at once - the
 * channels of one y-update, which do not couple (unires/_update.py:122-150), each on a stream of its own.  The
 * plan then sizes the persistent kernels of its matvec so that other channels' kernels find room on the CUs (see
 * api_plan.hip; results are unchanged, reductions are summed in another - still fixed - order).  1 = the default. */
int unires_plan_set_concurrency(unires_plan_t *plan, int32_t n_concurrent);
/* The difference of the plan's regulariser (UNIRES_DIFF_*; a new plan has UNIRES_DIFF_FORWARD): the D of the matvec,
 * of the right-hand side and of the FFT preconditioner's symbol.  A non-forward plan applies every AtA on the
 * kernels a forward plan uses, without their stencil epilogue, and closes the matvec with one streaming stencil
 * pass (stencil.hip: k_dtd_flat_w).  Changing it drops the captured CG graphs and the built preconditioner. */
int unires_plan_set_diff(unires_plan_t *plan, int32_t which);
/* Missing data (no counterpart in the reference, whose y-update treats a zero-filled voxel as an observed 0):
 * x = repeat n's observation, dim_x float32 in the caller's voxel layout, on the device.  The plan builds the mask
 * m(v) = [x(v) != 0] on `stream` (one byte per voxel, owned by the plan, stored in its canonical layout) and from then
 * on applies A_n^T diag(m) A_n wherever it applied A_n^T A_n: in the matvec of unires_ata_matvec and of the CG solves,
 * in unires_proj_apply's UNIRES_OP_ATA, in the Jacobi diagonal and in the mean diagonal of the FFT preconditioner's
 * symbol (the symbol's form is unchanged).  A, A^T and the right-hand side are unchanged: A_n^T x_n carries the
 * zeros already.  A masked repeat runs forward -> mask -> push: the one-kernel matvecs, the single-pass AtA kernel and
 * the hybrid forms are not taken (unires_plan_repeat_info shows it); unmasked repeats of the plan keep their forms.
 * x == NULL clears the mask.  Call again when the observation's values change; unires_plan_set_repeat keeps the mask
 * (the new descriptor must have the same dim_x).  Setting, changing or clearing a mask drops the captured CG graphs
 * and the built preconditioner.  The mask is written by kernels on `stream` and not waited for: work that uses the
 * plan on ANOTHER stream must be ordered after this call by the caller (an event recorded on `stream` afterwards).
 * A one-repeat plan whose observation is all zero has an empty data term: its system is still positive definite
 * (the zero-bound D^T D is), CG and the Jacobi diagonal work, but UNIRES_PRECOND_FFT returns UNIRES_ERR_ARG ("data
 * term has an empty diagonal") as it does for any operator with a zero mean diagonal - the symbol's constant would
 * be 0.  UNIRES_REGIME_IDENTITY has no x-space intermediate: UNIRES_ERR_UNSUPPORTED (build
 * the plan as UNIRES_REGIME_DENOISE with the identity affine instead). */
int unires_plan_set_missing(unires_plan_t *plan, int32_t n, const float *x, void *stream);
/* Per-slice weights of repeat n's data term (no counterpart in the reference): u_dev = dim_x[axis] float32 ON THE
 * DEVICE, one per slice along the caller's voxel axis `axis` (0, 1 or 2; the thick-slice axis dim_thick in
 * practice), in the caller's slice order.  The data term becomes 1/2 tau_n sum_v u[s(v)] m(v) (x - A y)^2(v), a noise
 * precision tau_n u_s per slice, and the plan applies A_n^T diag(u . m) A_n wherever it applied A_n^T diag(m) A_n
 * (m: the mask of unires_plan_set_missing, or 1): the matvec of unires_ata_matvec and of the CG solves, the Jacobi
 * diagonal tau A^T (u . m . A 1) + 2 rho lam^2 sum 1 / vx^2, the mean diagonal of the FFT preconditioner's symbol.
 * Unlike a mask the weights change the right-hand side: unires_rhs_assemble and unires_atx_assemble accumulate
 * tau_n A_n^T (u . x_n), made in the plan's scratch (the observation is not written).  unires_proj_apply keeps the
 * unweighted A, A^T and A^T A (a mask still applies to its A^T A).  The values are not checked: u >= 0 is the caller's
 * contract and keeps the system symmetric positive definite.
 * The plan copies the weights into a buffer it owns whose address does not change while the repeat is weighted; the
 * copy is enqueued on `stream` and not waited for - work that uses the plan on ANOTHER stream is ordered after it by
 * the caller, as for unires_plan_set_missing.  A weighted repeat runs forward -> weights (and mask, same pass) ->
 * push: it declines what a masked repeat declines.  A first set, a clear (u_dev == NULL) or a new axis therefore
 * rebuilds the repeat's tables where its kernel family changes, waits for the plan's earlier launches, and drops the
 * captured CG graphs and the built preconditioner.  New VALUES on the same axis rebuild nothing and wait for nothing:
 * a captured solve is kept and reads the new values from the same buffer when it is replayed; only the built
 * preconditioner is dropped.  unires_plan_set_repeat keeps the weights (the new descriptor must have the same dim_x;
 * the canonical axis behind `axis` and its direction follow the new orientation).  Errors: a bad n or axis
 * UNIRES_ERR_ARG; UNIRES_REGIME_IDENTITY UNIRES_ERR_UNSUPPORTED, as for the mask. */
int unires_plan_set_slice_weights(unires_plan_t *plan, int32_t n, int32_t axis, const float *u_dev, void *stream);
/* Per-slice intensity gains of repeat n's data term (no counterpart in the reference, whose even / odd scaling is one
 * special case): e_dev = dim_x[axis] float32 ON THE DEVICE, one per slice along the caller's voxel axis `axis`, in the
 * caller's slice order.  The data term becomes 1/2 tau_n sum_v W(v) (x(v) - e[s(v)] (A y)(v))^2 with W = g . u . m (the
 * voxel weights, the slice weights and the mask, each 1 where the repeat has none): diag(e) sits in observation space
 * after S(scl), beside diag(u) and diag(m), and commutes with them.  The plan applies A_n^T diag(W . e^2) A_n wherever
 * it applied A_n^T diag(W) A_n - the matvec of unires_ata_matvec and of the CG solves, the Jacobi diagonal, the mean
 * diagonal of the FFT preconditioner's symbol - and unires_rhs_assemble / unires_atx_assemble accumulate
 * tau_n A_n^T (W . e . x_n).  unires_proj_apply keeps the reference's A, A^T and A^T A, without gains.
 * The plan keeps the gains and two composed per-slice tables at fixed addresses,
 *   w_mat[s] = fl32(fl64(fl64(u e) e)),  w_rhs[s] = fl32(fl64(u e))      (u = 1 without slice weights; u e is exact in
 * float64), written by a one-workgroup kernel on `stream` whenever gains OR slice weights are set on a gained repeat; the
 * passes of a weighted repeat take w_mat or w_rhs where they took u, so e = 1 gives the bits of the plan without gains.
 * A gained repeat runs forward -> pass -> push and declines what a weighted repeat declines.  Call semantics as for
 * unires_plan_set_slice_weights: a first set, a clear (e_dev == NULL) or a new axis rebuilds the repeat's tables where
 * its kernel family changes, waits for the plan's earlier launches and drops the captured CG graphs; new VALUES rebuild
 * nothing, wait for nothing and keep a captured solve, which reads the new tables when it is replayed.  Every set drops
 * the built preconditioner.  unires_plan_set_repeat keeps the gains (the new descriptor must have the same dim_x).
 * The values are not checked: e > 0 is the caller's contract.  Errors: a bad n or axis, or an axis that differs from
 * the one the repeat's slice weights run along (and likewise slice weights set along another axis than the gains'),
 * UNIRES_ERR_ARG; UNIRES_REGIME_IDENTITY UNIRES_ERR_UNSUPPORTED, as for the mask. */
int unires_plan_set_slice_gains(unires_plan_t *plan, int32_t n, int32_t axis, const float *e_dev, void *stream);
/* Per-voxel weights of repeat n's data term (no counterpart in the reference): g_dev = dim_x float32 ON THE DEVICE, one
 * per x-space voxel in the caller's layout (the observation's).  The data term becomes
 * 1/2 tau_n sum_v g(v) u[s(v)] m(v) (x - A y)^2(v) and the plan applies A_n^T diag(g . u . m) A_n wherever it applied
 * A_n^T diag(u . m) A_n (u: the weights of unires_plan_set_slice_weights, m: the mask of unires_plan_set_missing, or 1;
 * all three in one pass): the matvec of unires_ata_matvec and of the CG solves, the Jacobi diagonal, the mean diagonal
 * of the FFT preconditioner's symbol.  unires_rhs_assemble and unires_atx_assemble accumulate tau_n A_n^T (g . u . x_n),
 * made in the plan's scratch (the observation is not written).  unires_proj_apply keeps the unweighted A, A^T and
 * A^T A.  The values are not checked: g >= 0 is the caller's contract and keeps the system symmetric positive definite.
 * The plan copies the weights into a buffer it owns - and, where it relabels the observation, into a second one in its
 * canonical layout - whose addresses do not change while the repeat is weighted; copy and permute are enqueued on
 * `stream` and not waited for.  A first set or a clear (g_dev == NULL) rebuilds the repeat's tables where its kernel
 * family changes, waits for the plan's earlier launches and drops the captured CG graphs.  New VALUES rebuild nothing
 * and wait for nothing: a captured solve is kept and reads the new values when it is replayed.  Every set drops the
 * built preconditioner.  unires_plan_set_repeat keeps the weights (the new descriptor must have the same dim_x) and
 * re-permutes them.  Errors: a bad n UNIRES_ERR_ARG; UNIRES_REGIME_IDENTITY UNIRES_ERR_UNSUPPORTED, as for the mask. */
int unires_plan_set_voxel_weights(unires_plan_t *plan, int32_t n, const float *g_dev, void *stream);
/* Bytes of device workspace the plan owns. */
int64_t unires_plan_workspace_bytes(const unires_plan_t *plan);
/* Which kernels repeat n's operator runs on (no counterpart in the reference, whose _proj_apply
 * takes any mat_x through a dense grid, _project.py:147-159; here the plan relabels the observation's
 * voxel axes so that sagittal / coronal / reflected storage takes the same kernels as axial).
 * info[0..2] = caller's voxel axis behind canonical axis 0..2, info[3] = bit j set where canonical axis
 * j is reversed, info[4] = 1 if the LDS-window pull serves it, info[5] = 0 if the schedule-driven
 * splat does not serve it, else 2 + its conv_up axis (1: grid-space source, 2..4: along x / y / z, 5: all), info[6] bit 0 = the translation-only one-kernel
 * matvec serves it, bit 1 = the single-pass AtA kernel of the denoising regime does (ata1.hip), bit 2 = the repeat is masked (unires_plan_set_missing:
 * bits 0 and 1 are then clear), bit 3 = the repeat is weighted (unires_plan_set_slice_weights: bits 0 and 1 are then clear), bit 4 = the repeat is voxel-weighted (unires_plan_set_voxel_weights: bits 0 and 1 are then clear), bit 5 = the repeat has slice gains (unires_plan_set_slice_gains: bits 0 and 1 are then clear), info[7] = 1 if the convolutions run as separable passes. */
int unires_plan_repeat_info(const unires_plan_t *plan, int32_t n, int32_t info[8]);
/* The relabelling a plan applies to an operator with grid -> output affine M (host arithmetic only, no device
 * call): perm[j] = caller's voxel axis behind canonical axis j, flip[j] = 1 where it is reversed, chosen so that
 * the permuted, sign-flipped linear part of M is as close to a positive diagonal as a signed permutation gets
 * (identity for every axis-aligned, right-handed geometry: the descriptor is then used as it is). */
int unires_orient_of(const float M[12], int32_t perm[3], int32_t flip[3]);
/* Measurement aid (no counterpart in the reference; bench.py's roofline leg).  While on,
 * unires_cg_solve launches its kernels one by one (no hipGraph replay) and brackets every operator
 * application A(p) of the solve with HIP events on the caller's stream.  Meaningful with tol == 0
 * only: launches enqueued after a solve has converged return at entry and are still counted.
 * on == 2: no events; instead every A(p) of a solve is enqueued TWICE (it is idempotent: same result), the solve
 * stays what it is in production - one hipGraph replayed.  The difference between a solve timed this way and a
 * plain one, divided by its iterations, is what an operator application costs INSIDE the replayed graph
 * (kernel + its dependent boundary, no host launch latency): bench.py's `us_per_launch_in_graph`. */
int unires_plan_time_matvecs(unires_plan_t *plan, int32_t on);
/* Waits for the recorded events; returns how many applications were recorded since the last call and
 * the sum of their durations (microseconds), and forgets them. */
int unires_plan_matvec_time(unires_plan_t *plan, int32_t *launches, double *total_us);
/* Deferred iterate update of tol == 0 solves (no FFT preconditioner): x += alpha_k p_k is applied for K iterations
 * at once, in iteration order, with the same roundings (the same bits); the last K directions are kept in a ring of
 * plan buffers.  k > 0 asks for K = min(k, 8) for this plan's next solves (1: the iterate updated every iteration;
 * default: UNIRES_CG_RING, else 8); the ring is allocated at the plan's first such solve and never grown, so K is
 * capped by what was allocated then.  k == 0 changes nothing.  *last (nullable) gets the K the plan's last solve ran
 * with (1 for solves outside the scope and for a plan that has not solved yet). */
int unires_plan_cg_ring(unires_plan_t *plan, int32_t k, int32_t *last);
/* How the plan's last solve was enqueued at its two ends (see unires_cg_solve): *trimmed (nullable) = 1 if its last
 * iteration updated x alone, *start_fused (nullable) = 1 if the operator's last kernel wrote the start's residual. */
int unires_plan_cg_ends(unires_plan_t *plan, int32_t *trimmed, int32_t *start_fused);
/* 1 if the plan's last solve ran inside the two-lane schedule of unires_cg_solve_many (see there), else 0. */
int unires_plan_cg_lockstep(unires_plan_t *plan);

/* _proj_apply(operator, ., po_n)  (_project.py:99-190) for repeat n, WITHOUT tau.
 * in/out sizes follow the operator (A: dim_y -> dim_x; At: dim_x -> dim_y; AtA: dim_y -> dim_y). */
int unires_proj_apply(unires_plan_t *plan, int32_t n, int32_t op, const float *in, float *out,
                      void *stream);

/* q = sum_n tau_n AtA_n p + rho*lam^2 DtD p   (_proj('AtA'), _project.py:73-87).
 * If dot_dev != NULL the float64 sum(p*q) is written there (device pointer). */
int unires_ata_matvec(unires_plan_t *plan, float rho, float lam, const float *p, float *q,
                      double *dot_dev, void *stream);

/* b = sum_n tau_n At_n x_n - lam * Dt(w_c - rho z_c)   (_update.py:124-133).
 * x_ptrs: HOST array of n_repeats device pointers; w_c,z_c: (3,X,Y,Z) device. */
int unires_rhs_assemble(unires_plan_t *plan, const float *const *x_ptrs, const float *w_c,
                        const float *z_c, float rho, float lam, float *b, void *stream);

/* The data term of the RHS alone, atx = sum_n tau_n At_n x_n  (_update.py:125-128).  It only
 * changes when an observation, its rigid or its scaling changes, so a caller may keep it
 * across ADMM iterations (the reference recomputes it every time). */
int unires_atx_assemble(unires_plan_t *plan, const float *const *x_ptrs, float *atx,
                        void *stream);

/* b = atx - lam * Dt(w_c - rho z_c)   (_update.py:131-133) from a kept atx. */
int unires_rhs_from_atx(unires_plan_t *plan, const float *atx, const float *w_c,
                        const float *z_c, float rho, float lam, float *b, void *stream);

/* Builds the diagonal of _precond (_update.py:80-102) for (rho, lam) into plan-owned memory
 * (allocated on the first call): M = tau AtA(1) + 2 rho lam^2 sum_d 1/vx_d^2.  Like the
 * reference it supports one repeat per channel only.  If m_out != NULL the diagonal is also
 * copied there (device, dim_y floats).  Needed before unires_cg_solve(precond_mode = JACOBI)
 * with the same rho and lam. */
int unires_precond_build(unires_plan_t *plan, int32_t precond_mode, float rho, float lam,
                         float *m_out, void *stream);

/* out = precond(in) for the preconditioner last built on this plan (identity: copy). */
int unires_precond_apply(unires_plan_t *plan, const float *in, float *out, void *stream);

/* nitorch cg(A=lhs, b, x, precond, max_iter, tolerance, stop,
 * inplace=True, sum_dtype=float64)  (_update.py:142-148): x is updated in place.
 * tol == 0 runs exactly max_iter iterations with no objective evaluation.  Such a solve (no FFT preconditioner)
 * does only the work x needs at its two ends: its last iteration is A(p), alpha and x += the pending alpha p
 * terms - no residual, r.z, beta or next direction, which nothing would read - so the plan's internal r, r.z and
 * beta are afterwards those of iteration max_iter - 1 (no entry point hands them out, and the next solve on the
 * plan starts by writing all of them); and where the operator's last kernel is the schedule-driven push of a
 * forward-difference plan whose last repeat has no mask, that kernel writes r = b - A(x), the first direction and
 * the partials of r.z (and of obj[0], for a solve with a tolerance) itself and A(x) is never stored.  The trimmed
 * last iteration leaves x the same bits.  The fused start sums the same float32 terms of r.z and obj[0] in float64
 * in another grouping: the two agree with the separate kernel's to the rounding of such a sum, and x changes only
 * if that moves alpha_1 or beta_1 across a float32 rounding boundary (not seen; the bench's outputs are the same
 * bytes).  UNIRES_CG_TRIM=0 / UNIRES_CG_START_FUSED=0 (read once per process) enqueue the last iteration in
 * full / keep the separate start kernel everywhere.
 * If iters_out != NULL the call synchronises the stream and returns the realised
 * iteration count; obj_trace (HOST, max_iter+1 doubles, may be NULL) then
 * receives the objective values obj[0..iters].
 * tol > 0 (the reference's default, struct.py:65-67): the solve is enqueued in chunks of
 * UNIRES_CG_CHUNK iterations (default 2), one chunk ahead of the device; the kernel that ends an
 * iteration publishes (done, iterations) to host-mapped memory and the next chunk is enqueued only
 * while the stopping test has not fired - same kernels, same order, same iterate and trace as
 * enqueuing all max_iter iterations, without their no-op tail.  max_iter may then exceed 4096
 * (nitorch's default is 10 numel); obj_trace receives at most 4097 values (a ring beyond that). */
int unires_cg_solve(unires_plan_t *plan, float rho, float lam, const float *b, float *x,
                    int32_t max_iter, double tol, int32_t stop_mode, int32_t precond_mode,
                    int32_t *iters_out, double *obj_trace, void *stream);

/* The channels' solves of one y-update together (_update.py:122-150 loops over the channels; they do
 * not couple inside the y-update): n plans, each with its own b, x, rho, lam and stream (all HOST
 * arrays of n entries).  One host loop feeds the chunks of all of them, so channels on separate
 * streams keep overlapping on the device.  iters_out: n ints or NULL (non-NULL synchronises every
 * stream); obj_trace: n x (min(max_iter, 4096) + 1) doubles or NULL.
 * With UNIRES_CG_LOCKSTEP=1 (read once per process; off by default: measured slower, experiments/E20), fixed-iteration
 * solves (tol == 0, max_iter > 0, identity or Jacobi preconditioner) of n >= 2 plans, none in timing mode, no stream
 * under capture, at least two different streams among `streams`, are enqueued as ONE
 * two-lane schedule - the operator applications of all channels in rotation on streams[0], their scalar and vector
 * kernels in the same rotation on the first other stream, so that a channel's vector phase runs under the next
 * channel's operator - captured once into one hipGraph (two parallel branches) and replayed while every channel's
 * arguments and plan stay what they were.  streams[0] waits for every channel stream before the graph and every
 * channel stream for the graph's end, so the caller orders its work as for free-running solves.  Per channel the
 * kernels, arguments and order are unires_cg_solve's: x is the same bits as that plan's solve alone with the same
 * grids (the mode has its own cap on k_splat2's grid, UNIRES_LOCKSTEP_S2, in unires_plan_set_concurrency's unit).
 * The switch also takes the flush of the deferred iterate update in two halves of four directions (fewer registers,
 * the same bits).  GPU_MAX_HW_QUEUES below 4 (read once: the runtime is not trusted with branched graphs on fewer
 * hardware queues) and a refused capture keep the free-running solves.  unires_plan_cg_lockstep tells which way a
 * plan's last solve went. */
int unires_cg_solve_many(int32_t n, unires_plan_t *const *plans, const float *rho, const float *lam,
                         const float *const *b, float *const *x, int32_t max_iter, double tol,
                         int32_t stop_mode, int32_t precond_mode, int32_t *iters_out,
                         double *obj_trace, void *const *streams);

/* ------------------------------------------------------------------------
 * Next rows of the path: the updates and sums that follow the
 * y-update inside every ADMM iteration  (unires/_update.py:154-195, 396-427)
 * ---------------------------------------------------------------------- */

/* UPDATE z and w  (_update.py:160-193), all channels:
 *   u_c = w_c/rho + lam_c D y_c ;  s = max(|u| - 1/rho, 0) / (|u| + 1e-7), |u| joint over c,d
 *   z_c = s u_c ;  w_c += rho (lam_c D y_c - z_c)
 * y_ptrs / lam: HOST arrays of n_channels device pointers / scalars (any n_channels >= 1; more than 8 run as chained launches);
 * z, w: (C,3,X,Y,Z) device, updated in place; jtv: (X,Y,Z) device, receives s (the
 * reference returns it as `tmp`, _update.py:195).  alpha is the over-relaxation
 * parameter (1 = none). */
int unires_zw_update(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                     const int32_t dim[3], const float vx[3], float rho, float alpha, float *z,
                     float *w, float *jtv, void *stream);

/* -ln p(y) = sum_v sqrt(sum_c |lam_c D y_c|^2)  (_update.py:419-425) -> *out_dev (float64). */
int unires_nll_prior(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                     const int32_t dim[3], const float vx[3], double *out_dev, void *stream);

/* unires_zw_update / unires_nll_prior with the difference of D chosen (UNIRES_DIFF_*). */
int unires_zw_update_which(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                           const int32_t dim[3], const float vx[3], int32_t which, float rho, float alpha,
                           float *z, float *w, float *jtv, void *stream);
int unires_nll_prior_which(const float *const *y_ptrs, const float *lam, int32_t n_channels,
                           const int32_t dim[3], const float vx[3], int32_t which, double *out_dev,
                           void *stream);

/* sum_{x != 0} (x - ay)^2 in float64  (_update.py:414-417; the caller multiplies by tau/2). */
int unires_masked_sse(const float *x, const float *ay, int64_t n, double *out_dev, void *stream);

/* The same sum per slice (no counterpart in the reference; what per-slice weights are estimated from): x, ay x-space
 * volumes `dim`, slices counted along dim_thick, S = dim[dim_thick].
 *   out_dev[s]     = sum_{v in slice s, x != 0} (x - ay)^2
 *   out_dev[S + s] = #{v in slice s : x != 0}
 * float32 terms, float64 sums added in a fixed order (no atomics: the same bits every run); every one of the 2 S
 * entries is written.  out_dev: 2 S doubles on the device. */
int unires_slice_sums(const float *x, const float *ay, const int32_t dim[3], int32_t dim_thick, double *out_dev,
                      void *stream);

/* The slice sums weighted per voxel (no counterpart in the reference): g an x-space volume `dim` of weights >= 0.
 *   out_dev[s]     = sum_{v in slice s, x != 0} g(v) (x - ay)^2     terms fl(g fl(r r)), r = fl(x - ay), float32
 *   out_dev[S + s] = sum_{v in slice s, x != 0} g(v)                the slice's effective count
 * float64 sums in unires_slice_sums' fixed order (no atomics: the same bits every run; with g = 1 its bits).  The one
 * statement of a voxel-weighted repeat's data term: 1/2 tau sum_s u_s out_dev[s].  out_dev: 2 S doubles on the device. */
int unires_voxel_sums(const float *x, const float *ay, const float *g, const int32_t dim[3], int32_t dim_thick,
                      double *out_dev, void *stream);

/* The sums per slice that per-slice intensity gains are estimated from (no counterpart in the reference): with
 * W(v) = g(v) u[s(v)] - g an x-space volume `dim` of weights or NULL (1), u dim[dim_thick] slice weights or NULL (1),
 * all on the device - over the voxels of slice s with x != 0, S = dim[dim_thick]:
 *   out_dev[s]       = sum W fl32(x ay)      (tau times this is P_s of the rule e_s = (P_s + kappa) / (Q_s + kappa))
 *   out_dev[S + s]   = sum W fl32(ay ay)     (Q_s / tau)
 *   out_dev[2 S + s] = sum W                 the slice's effective count
 * ay is A y WITHOUT gains.  float32 terms; W is formed in float64, where g u is exact; the summand fl64(W t) is exact
 * with one factor and rounded once with both (unires_scaling_sums_g's conventions); float64 sums added in a fixed order
 * (no atomics: the same bits every run); every one of the 3 S entries is written.  out_dev: 3 S doubles on the device.
 * tau is the caller's.  Errors as for unires_slice_sums. */
int unires_gain_sums(const float *x, const float *ay, const float *g, const float *u, const int32_t dim[3],
                     int32_t dim_thick, double *out_dev, void *stream);

/* Terms of the rigid Gauss-Newton step of a repeat with per-slice gains e (S = dim[axis] floats, > 0), g a volume or
 * NULL (1), u S floats or NULL (1), all on the device (no counterpart in the reference).  p = fl32(e[s] ay) is formed in
 * registers and never stored.
 *   sums_dev[s]     = sum_{v in s, x != 0} [g] (x - p)^2    unires_slice_sums' terms (g NULL) / unires_voxel_sums' (g)
 *   sums_dev[S + s] = the count / effective count, as those two write it
 *   out (NULL: not written) = t[s] (p - x), masked where x == 0 or p == 0 (+0 there), t[s] = fl32(fl64(u[s]) fl64(e[s]))
 *                  (u NULL: t = e): unires_rigid_resid's / unires_rigid_resid_g's roundings with u := t, ay := p
 * Bit for bit what unires_slice_apply(ay, e) -> P, unires_slice_sums(x, P) / unires_voxel_sums(x, P, g) and
 * unires_rigid_resid(x, P, u := t) / unires_rigid_resid_g(x, P, g, u := t) give, in one pass over x, ay [and g]; no
 * atomics: the same bits every run.  out == NULL is a line-search evaluation (nothing but 2 S doubles is written).
 * out == ay is allowed; x, g, u, e are only read (out == x or out == g: UNIRES_ERR_ARG).  Errors as for
 * unires_slice_sums.  sums_dev: 2 S doubles on the device. */
int unires_rigid_terms_e(const float *x, const float *ay, const float *g, const float *u, const float *e,
                         const int32_t dim[3], int32_t axis, double *sums_dev, float *out, void *stream);

/* Terms of the Rician data term of a magnitude observation (no counterpart in the reference; sett.noise_model =
 * 'rician'): x, ay x-space volumes `dim`, g a volume of weights or NULL (1), e S = dim[axis] per-slice gains or NULL
 * (1), all on the device; tau the observation's precision 1 / sigma^2.  Per voxel, in registers,
 * p = fl32(e[s] ay) (unires_slice_apply's product; ay itself without e) and z = fl32(fl32(tau x) p).
 *   xt (NULL: not written) = fl32(x R(z)), R = I1 / I0: the effective observation of the quadratic majoriser - the
 *                  y-update's right-hand side takes it where it took x.  R odd, |R| <= 1, R(+-inf) = +-1; +0 where
 *                  x == 0.  xt == ay is allowed; x, g, e are only read (xt == x or xt == g: UNIRES_ERR_ARG).
 *   sums_dev[s] (NULL: not written) = sum_{v in slice s} g(v) c(z(v)),  c(z) = (z - |z|) - log i0e(|z|): what the
 *                  voxel's negative log-likelihood holds beside 1/2 tau (x - p)^2 (the term -log(tau x), which does
 *                  not depend on y, is dropped).  float32 terms, widened; fl64(g c) rounded on its own; float64 sums in
 *                  unires_rigid_terms_e's fixed order (no atomics: the same bits every run); every one of the S
 *                  entries is written.  Slice weights are the caller's: sum_s u_s sums_dev[s].
 * R and c are float32 evaluations of fixed-degree forms (Abramowitz & Stegun 9.8.1 - 9.8.4 as ratios: |z| <= 3.75
 * polynomials in z^2, beyond polynomials in 1 / |z|; one select, no loops, no exp, no overflow): R to 2e-6 relative,
 * c to 1e-6 (1 + |c|).  One pass over x, ay [and g].  Errors as for unires_slice_sums; xt and sums_dev both NULL:
 * UNIRES_ERR_ARG.  sums_dev: S doubles on the device. */
int unires_rician_terms(const float *x, const float *ay, const float *g, const float *e, const int32_t dim[3],
                        int32_t axis, float tau, float *xt, double *sums_dev, void *stream);

/* Terms of the rigid Gauss-Newton step of a repeat with the Rician data term (no counterpart in the reference;
 * sett.rician_gn): x, ay x-space volumes `dim`, g a volume of weights or NULL (1), u S = dim[axis] slice weights or
 * NULL (1), e S per-slice gains or NULL (1), all on the device; tau the observation's precision.  One pass over x, ay
 * [and g]; per voxel, in registers, p = fl32(e[s] ay) (ay itself with e NULL) and z = fl32(fl32(tau x) p).
 *   sums_dev[s], sums_dev[S + s]  = the SSE and the count of slice s: exactly unires_rigid_terms_e's - with e NULL
 *                  unires_slice_sums' (g NULL) or unires_voxel_sums' (g) on ay
 *   sums_dev[2 S + s] = sum_{v in s} g c(z): exactly unires_rician_terms' sums_dev
 *   out (NULL: not written; a line-search evaluation) = t[s] [g] (p - x~), x~ = fl32(x R(z)) unires_rician_terms'
 *                  effective observation, never stored; +0 where x == 0 or p == 0 - the mask reads the true x, not
 *                  x~, which can underflow to 0 where x is not; t[s] = fl32(fl64(u[s]) fl64(e[s])), 1 where a table
 *                  is NULL; unires_rigid_resid's / unires_rigid_resid_g's roundings with u := t, ay := p, x := x~
 *                  (both tables NULL: theirs with u NULL).  tau times out is the exact derivative of the repeat's
 *                  Rician term W [1/2 tau (x - p)^2 + c(z)] in A y.
 * No atomics: the same bits every run; every one of the 3 S entries is written with a plain store.  out == ay is
 * allowed; x, g, u, e are only read (out == x or out == g: UNIRES_ERR_ARG).  Errors as for unires_slice_sums; nothing
 * is launched on a bad argument.  sums_dev: 3 S doubles on the device. */
int unires_rigid_terms_r(const float *x, const float *ay, const float *g, const float *u, const float *e,
                         const int32_t dim[3], int32_t axis, float tau, double *sums_dev, float *out, void *stream);

/* A smooth multiplicative bias field b = exp(beta) of an observation (no counterpart in the reference; sett.bias,
 * _input.bias_coef): beta(i, j, z) = sum_{a < k0, b < k1, c < k2} coef[(a k1 + b) k2 + c] tx[a n0 + i] ty[b n1 + j]
 * tz[c n2 + z], k = order (1 .. 8 along every axis), n = dim.  coef and the three tables are float64 on the device; a
 * table holds at least k rows of n entries, row m the caller's phi_m (the unnormalised DCT-II function
 * cos(pi m (2 i + 1) / (2 n)), phi_0 = 1).  beta is evaluated in float64 - folded over a, then b, then c, each in index
 * order, one product and one addition per term - and clamped to +- beta_max (> 0).
 *   b                     = fl32(exp(beta))
 *   gb2 (NULL: not written) = fl32(fl64(fl64(g b) b)), g an x-space volume of weights or NULL (1): g b is exact in
 *                  float64, the chain is rounded there once and once more to float32 - the voxel map the plan takes for
 *                  a repeat with a field (unires_plan_set_voxel_weights)
 *   xb  (NULL: not written) = fl32(x / b), +0 where x == 0: the effective observation the right-hand side reads
 * One streaming pass: the coefficients are folded over the two outer axes once per plane and row; a voxel costs k2
 * multiply-adds and one exp.  b, gb2, xb are buffers of their own (UNIRES_ERR_ARG); x and g are only read. */
int unires_bias_field(const double *coef, const double *tx, const double *ty, const double *tz, const int32_t order[3],
                      const int32_t dim[3], double beta_max, const float *g, const float *x, float *b, float *gb2,
                      float *xb, void *stream);

/* What the Gauss-Newton step of a bias field is assembled from, in one pass over x, mu, b [and g] (no counterpart in the
 * reference): mu the prediction e . A y without the field, g a volume of weights or NULL (1), u dim[axis] slice weights
 * or NULL (1), all on the device.  Per voxel m = fl32(b mu), r = fl64(m) - fl64(x), W = g u [x != 0]; everything after m
 * in float64, each product rounded on its own.  With k = order, q = 2 k - 1 and the tables of unires_bias_field (at
 * least q rows each):
 *   out_dev[0]                                   = sum_v W r^2
 *   out_dev[1 + (a k1 + b) k2 + c]               = sum_v W m r  phi_a(i) phi_b(j) phi_c(z),   a < k0, b < k1, c < k2
 *   out_dev[1 + k0 k1 k2 + (a q1 + b) q2 + c]    = sum_v W m^2 phi_a(i) phi_b(j) phi_c(z),   a < q0, b < q1, c < q2
 * order = (0, 0, 0): out_dev[0] alone, and the tables are not read - a line-search evaluation.  float64 sums in a fixed
 * order (no atomics: the same bits every run); every entry is written with a plain store.  Errors as for
 * unires_slice_sums; orders outside 1 .. 8 (and not all 0): UNIRES_ERR_ARG. */
int unires_bias_terms(const float *x, const float *mu, const float *b, const float *g, const float *u, int32_t axis,
                      const double *tx, const double *ty, const double *tz, const int32_t order[3], const int32_t dim[3],
                      double *out_dev, void *stream);

/* dst[v] = fl32(u[s(v)] src[v]) over a z-fastest volume `dim`, s(v) = v's index along `axis`, u dim[axis] floats on the
 * device: the pass of a slice-weighted repeat on its own, without mask and without a `done` word (no counterpart in the
 * reference).  dst == src: in place; dst != src: src is only read.  With the gains of a repeat as u it makes e . (A y),
 * the prediction every residual sum and rule of a gained repeat is taken on.  Buffers off a 16-byte boundary are served
 * voxel by voxel. */
int unires_slice_apply(const float *src, float *dst, const float *u, const int32_t dim[3], int32_t axis, void *stream);

/* The pass a voxel-weighted repeat runs between the forward half of A^T A and its push, on its own (no counterpart in
 * the reference): over a z-fastest volume `dim`
 *   dst[v] = g[v] src[v]                      (u == NULL; one float32 product)
 *   dst[v] = fl32(fl64(g[v] u[s(v)]) src[v])  (u: one weight per slice along `axis`, counted from the far end where
 *                                              flip != 0; g u is exact in float64, one rounding to float32 at the end)
 * and +0 where mask[v] == 0 (mask: one byte per voxel, or NULL).  dst == src: in place; dst != src: src is only read.
 * done: a device word, or NULL - the pass returns at entry where *done != 0, as inside a CG solve.  All device
 * pointers; buffers off a 16-byte boundary (mask: 4-byte) are served voxel by voxel. */
int unires_voxel_apply(const float *src, float *dst, const float *g, const uint8_t *mask, const float *u,
                       const int32_t dim[3], int32_t axis, int32_t flip, const int32_t *done, void *stream);

/* The Huber weights of a residual (no counterpart in the reference): over n voxels
 *   g_out[v] = prior[v] h(v)   (prior == NULL: h(v)),   h = 1 where x == 0 or |r| <= c, else fl(c / |r|),  r = fl(x - ay)
 * in float32, c > 0.  One streaming pass; g_out may be prior. */
int unires_voxel_huber(const float *x, const float *ay, const float *prior, float c, int64_t n, float *g_out,
                       void *stream);

/* ------------------------------------------------------------------------
 * Exact medians on the device (no counterpart in the reference): a radix select on the bit patterns of |t(v)|, three
 * histogram passes of 11 + 11 + 10 bits with a one-workgroup scan after each.
 *
 * Both entry points give the LOWER median (the ceil(N/2)-th smallest of N, torch.median's convention) of |t(v)| over
 * the eligible voxels.  out_dev: 2 float64 on the device:
 *   [0] the median (a float32 value that occurs in the stream, widened; 0 when N = 0)
 *   [1] N.
 * work: UNIRES_MEDIAN_WORK_BYTES of device scratch, 4-byte aligned; the caller need not clear it, and may reuse it for
 * the next call on the same stream.  No read-back, no host synchronisation, the same bits every run (integer counts).
 * Status of the two median entry points: n < 0, n or a cell count above 2^32 - 1, an axis outside 0..2 and a null x, ay,
 * dim, work or out_dev are UNIRES_ERR_ARG; a `dim` with an entry < 1 (or beyond what every volume entry point takes) is
 * UNIRES_ERR_DIM.
 * ------------------------------------------------------------------------ */
#define UNIRES_MEDIAN_WORK_BYTES 24592

/* t = fl32(x - ay) over n voxels;
 * eligible: x != 0, t finite, and (prior == NULL or prior > 0): the missing-data and prior conventions of the Huber
 * rule above.  16-byte loads where x, ay and prior are on a 16-byte boundary, voxel by voxel otherwise. */
int unires_median_absres(const float *x, const float *ay, const float *prior, int64_t n, void *work, double *out_dev,
                         void *stream);

/* Haar diagonal detail in the plane orthogonal to `axis`, at every 2x2 in-plane cell (undecimated) of the volume `dim`:
 *   t = ((a - b) - c) + d,  in float32, in this order,
 *   where a = x[p,q], b = x[p+1,q], c = x[p,q+1], d = x[p+1,q+1];
 *   p, q run along the two other axes in ascending axis order.
 * Eligible: all four voxels finite, != 0 (ct == 0: > 0), and (w == NULL or all four w > 0); w: a volume `dim`.
 * Of i.i.d. noise of variance s^2, t has variance 4 s^2. */
int unires_median_hh(const float *x, const int32_t dim[3], int32_t axis, int32_t ct, const float *w, void *work,
                     double *out_dev, void *stream);

/* The Huber weights above with the threshold taken from the device:
 *   c = fl32(mult * (float)scale_dev[0]),  mult > 0.
 * c > 0: the bits the Huber entry point gives for that c.
 * c == 0 (nothing eligible, or a zero median): g_out = prior (ones where prior == NULL).
 * g_out may be prior.  Status, as the Huber entry point above: a null x, ay, scale_dev or g_out is UNIRES_ERR_NULL,
 * n < 0 UNIRES_ERR_DIM, a mult that is not > 0 UNIRES_ERR_ARG. */
int unires_voxel_huber_dev(const float *x, const float *ay, const float *prior, const double *scale_dev, float mult,
                           int64_t n, float *g_out, void *stream);

/* Gradient and Hessian sums of one rigid Gauss-Newton step (_update_rigid_channel,
 * _update.py:622-650) in one pass over the grid: gr3 (dim,3) = grid_grad of the pulled image,
 * diff (dim) = residual (conv_transposed, _update.py:524), ctc (dim) = conv_transpose(conv(1))
 * or NULL, d_rigid = the six 3x4 matrices mat_y^-1 dR/dq_i mat (row-major, float32).
 * out_dev (27 float64, device): [0..5] gradient, [6..26] upper triangle of the 6x6 Hessian,
 * row by row. */
int unires_rigid_sums(const float *gr3, const float *diff, const float *ctc, const int32_t dim[3],
                      const float d_rigid[72], double *out_dev, void *stream);

/* fit()'s clean_fov post-processing (run.py:150-164): y[v] = 0 where the voxel M v of the
 * low-resolution image lies outside [0, dim_x) on any axis; M (12 floats, row-major 3x4) =
 * float32 of inv(mat_y^-1 rigid mat_x).  Call once per observation. */
int unires_clean_fov(float *y, const int32_t dim_y[3], const float M[12], const int32_t dim_x[3],
                     void *stream);

/* The masked sums of one Gauss-Newton step on the even/odd slice scaling
 * (_update_scaling, _update.py:310-336); x, ay: x-space volumes `dim`, ay = A y with the
 * current scaling; slices alternate along dim_thick ('odd' = [::2], 'even' = [1::2], :430-445).
 *   out_dev[0] = sum_{x!=0} (x-ay)^2          (ll = 0.5 tau out[0])
 *   out_dev[1] = sum_even ay (x-ay)   out_dev[2] = sum_odd ay (x-ay)   (gr  = tau (out[1]-out[2]))
 *   out_dev[3] = sum_even ay^2        out_dev[4] = sum_odd ay^2        (Hes = tau (out[3]+out[4]))
 * float32 terms, float64 sums; out_dev: 5 doubles on the device. */
int unires_scaling_sums(const float *x, const float *ay, const int32_t dim[3], int32_t dim_thick,
                        double *out_dev, void *stream);

/* The same five sums of the weighted data term 1/2 tau sum_v u[s(v)] [x != 0] (x - ay)^2 (per-slice weights; no
 * counterpart in the reference): every term above times the weight of its voxel's slice along dim_thick.  u_dev: a
 * DEVICE pointer to dim[dim_thick] floats, NULL is UNIRES_ERR_NULL.  A term is the float32 term of
 * unires_scaling_sums times the float32 weight, the product taken in float64 (exact); float64 sums in a fixed order,
 * no atomics: the same bits every run, and with u = 1 the bits of unires_scaling_sums. */
int unires_scaling_sums_w(const float *x, const float *ay, const int32_t dim[3], int32_t dim_thick,
                          const float *u_dev, double *out_dev, void *stream);

/* The same five sums of the data term with per-voxel weights, 1/2 tau sum_v g(v) u[s(v)] [x != 0] (x - ay)^2 (no
 * counterpart in the reference): every term of unires_scaling_sums times W(v) = g(v), or g(v) u[s(v)] where u_dev is
 * given.  g_dev: a DEVICE volume `dim` in the caller's layout, NULL is UNIRES_ERR_NULL; u_dev: a DEVICE pointer to
 * dim[dim_thick] floats, or NULL.  The float32 term is unires_scaling_sums'; W is formed in float64, where g u is exact;
 * the summand fl64(W t) is exact without u and rounded once with it.  float64 sums in unires_scaling_sums' fixed order,
 * no atomics: the same bits every run; with g = 1 the bits of unires_scaling_sums_w (u_dev given) or of
 * unires_scaling_sums (u_dev NULL), with g constant on every slice and u_dev NULL those of unires_scaling_sums_w with
 * these constants as u. */
int unires_scaling_sums_g(const float *x, const float *ay, const int32_t dim[3], int32_t dim_thick, const float *g_dev,
                          const float *u_dev, double *out_dev, void *stream);

/* The x-space residual of one rigid Gauss-Newton step (_rigid_match, _update.py:515-519) in one pass:
 *   out[v] = u[s(v)] * (ay[v] - x[v])  where x[v] != 0 and ay[v] != 0, else +0
 * x, ay, out: volumes `dim`; s(v) = v's index along `axis`; u_dev: a DEVICE pointer to dim[axis] floats, or NULL
 * (weight 1: the unweighted residual, bit for bit).  float32: the difference and the product round once each.
 * out == ay is allowed; x is only read. */
int unires_rigid_resid(const float *x, const float *ay, const int32_t dim[3], int32_t axis, const float *u_dev,
                       float *out, void *stream);

/* The same residual on the data term with per-voxel weights (no counterpart in the reference):
 *   out[v] = fl32(W(v) r(v)),  r = fl32(ay[v] - x[v]),  where x[v] != 0 and ay[v] != 0, else +0
 * with W = g (u_dev == NULL: one float32 product) or W = g[v] u[s(v)] (exact in float64, times r, rounded to float32
 * once) - unires_voxel_apply's rounding.  g: a DEVICE volume `dim` of weights; u_dev: dim[axis] floats on the device,
 * or NULL.  g = 1 gives the bits of unires_rigid_resid with the same u_dev.  out == ay is allowed; x and g are only
 * read, and out == g is UNIRES_ERR_ARG.  Buffers off a 16-byte boundary are served voxel by voxel. */
int unires_rigid_resid_g(const float *x, const float *ay, const float *g, const int32_t dim[3], int32_t axis,
                         const float *u_dev, float *out, void *stream);

/* ------------------------------------------------------------------------
 * Stream marks: following a stream from the host by reading memory.
 * Not part of the reference (single process, unires/run.py); it serves the one-process-per-GPU batch
 * mode, where eight ranks share one host: every hipEventQuery / hipStreamQuery on running
 * work costs the runtime's signal thread CPU time (profiles/r05_host_profile.txt).  A mark is a 64-bit
 * word in mapped host memory; unires_mark_signal enqueues a one-thread kernel that stores `value` into it
 * once everything enqueued on `stream` before it has finished; unires_mark_read is a plain load (never
 * blocks, no runtime call).  Seeing the value orders NOTHING else for the host: results are still read
 * through a stream synchronisation / a blocking copy - the mark only tells when that will not wait.
 * ---------------------------------------------------------------------- */
typedef struct unires_mark unires_mark_t;
int unires_mark_create(unires_mark_t **out);
int unires_mark_destroy(unires_mark_t *mark);
int unires_mark_signal(unires_mark_t *mark, uint64_t value, void *stream);
int unires_mark_read(const unires_mark_t *mark, uint64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* UNIRES_HIP_H */
