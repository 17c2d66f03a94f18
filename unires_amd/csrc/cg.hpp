// cg.hpp - device-resident CG state + launchers of the vector / scalar kernels (cg.hip).
#pragma once
#include "common.hpp"

namespace unires {

constexpr int kMaxCgIter = 4096;
constexpr int kMaxRing = 8;  // most direction buffers a deferred-iterate solve keeps (api_cg.hip: cg_ring_prepare)

struct CgState {  // lives in device memory, owned by the plan
  double rz, pAp, alpha, beta, obj_max, obj_min;
  int done, iters;
  unsigned gen, pad_;  // solves started on this plan (k_sc_init counts); tags the published progress word
  double rzpp[2];  // r.z of iterations k (slot k & 1) and k - 1, kept by the scalar kernels
  double obj[kMaxCgIter + 1];  // objective trace; iteration k at slot k % (kMaxCgIter + 1)
  // UNIRES_STOP_MAXGAIN_GUARDED (k_sc_beta_guarded / k_sc_obj_guarded)
  int skip_fresh;        // 1: this iteration's fresh objective (a second A(x)) is not needed - its kernels return at entry
  int fresh_prev_ok;     // fresh_prev holds the FRESH objective of the previous iteration
  double rec_prev, fresh_prev, gain_rec;  // recurred objective of the previous iteration; this iteration's recurred gain
  // deferred iterate update (launch_update_p_ring / _flush): alpha of the iteration whose direction is in ring slot j,
  // and whether that iteration's "x += alpha p" was committed (its p update ran, i.e. the solve was not done)
  double ahist[kMaxRing];
  int committed[kMaxRing];
};
struct RingPtrs {  // the ring's direction buffers, slot j = the j-th iteration since the last flush (by value: kernarg)
  const float *p[kMaxRing];
};

// Progress word of a solve, published by its scalar kernels to host-mapped memory (chunked solves,
// api_cg.hip): generation << 32 | done << 31 | iterations completed.
__host__ __device__ inline unsigned long long cg_progress_word(unsigned gen, int done, int iters) {
  return ((unsigned long long)gen << 32) | (done ? 0x80000000ull : 0ull) | (unsigned)(iters & 0x7fffffff);
}

// UNIRES_CG_LOCKSTEP, read once per process with the other switches of the CG driver (api_cg.hip: CgSwitches, which
// defines cg_lockstep_env): 1 takes the two-lane schedule of several channels' fixed-iteration solves and what makes
// room for it - the flush applied in two halves.  Off unless asked for: measured, every kernel takes about twice as long
// under the other lane's and the job is 4 - 12 % slower (experiments/E20).
constexpr bool kLockstepDefault = false;
bool cg_lockstep_env();
int vec_num_blocks(size_t n);  // grid (= number of partials) of the vector kernels
void launch_residual_init(const float *b, const float *ax, const float *x, float *r, float *p,
                          size_t n, double *part_rr, double *part_obj, const float *M,
                          hipStream_t st);
void launch_dot(const float *a, const float *b, size_t n, double *part, const int *done,
                hipStream_t st);
void launch_update_xr(const CgState *s, const float *p, const float *ap, float *x, float *r,
                      const float *b, size_t n, double *part_rr, double *part_obj, const float *M,
                      hipStream_t st);
// x == nullptr in launch_update_xr defers "x += alpha p" to launch_update_p(..., x): one volume
// pass less per iteration (only valid when nothing stops the solve between the two launches)
void launch_update_p(const CgState *s, const float *r, float *p, size_t n, const float *M, float *x,
                     hipStream_t st);
// Deferred iterate update (tol = 0 solves, api_cg.hip): the directions of up to kMaxRing iterations stay in a ring and
// x takes their alpha p terms at once, in iteration order, with the same roundings.
// ring: p_out = beta p_in + z for the iteration whose direction is ring slot `slot`; records its alpha and whether it
// was committed (the state not done).
void launch_update_p_ring(CgState *s, const float *r, const float *p_in, float *p_out, int slot, size_t n,
                          const float *M, hipStream_t st);
// flush: the same p update for slot m - 1 (p_out may be slot 0: see k_update_p_flush), then
// x = fl(x + fl(alpha_j p_j)) for the committed slots j = 0 .. m - 1 in ascending order
void launch_update_p_flush(CgState *s, const float *r, const RingPtrs &ring, int m, float *p_out, size_t n,
                           const float *M, float *x, hipStream_t st);
// The iterate alone, for the last iteration of a solve that runs all of its iterations (nothing reads the r, beta and
// p that would follow it): the flush without its p update and without reading r, and x = fl(x + fl(alpha p)) for K = 1
void launch_update_x_flush(CgState *s, const RingPtrs &ring, int m, size_t n, float *x, hipStream_t st);
void launch_update_x(const CgState *s, const float *p, size_t n, float *x, hipStream_t st);
// M = nullptr: identity preconditioner; else z = r / M (Jacobi)
void launch_scale_shift(float a, float c, float *y, size_t n, hipStream_t st);
void launch_fill(float v, float *y, size_t n, hipStream_t st);
void launch_div(const float *a, const float *m, float *y, size_t n, hipStream_t st);  // y = a / m
void launch_axpy(float a, const float *x, float *y, size_t n, hipStream_t st);
// hostw (nullable): host-mapped progress word, written (system scope) when an iteration's last scalar
// kernel has run.  k < 0 in sc_beta / sc_obj: the iteration index is the state's own counter (iters + 1 /
// iters), so that a captured chunk of iterations can be replayed for any part of a solve.
void launch_sc_init(CgState *s, const double *part_rr, const double *part_obj, int g, int mode,
                    int check, unsigned long long *hostw, hipStream_t st);
// iters_end > 0: sc_alpha also sets the state's iteration count to it (the last iteration of a solve enqueued without
// that iteration's sc_beta)
void launch_sc_alpha(CgState *s, const double *part, int g, hipStream_t st, int iters_end = 0);
void launch_sc_beta(CgState *s, const double *part_rr, const double *part_obj, int g, int k,
                    int obj_kind, double tol, unsigned long long *hostw, hipStream_t st);
void launch_sc_obj(CgState *s, const double *part, int g, int k, double tol, unsigned long long *hostw,
                   hipStream_t st);
// guarded 'max_gain' (api_cg.hip: cg_enqueue_iters): sc_beta with the recurred objective decides whether the fresh one is
// needed; sc_obj, if it runs, decides with it
void launch_sc_beta_guarded(CgState *s, const double *part_rr, const double *part_obj, int g, int k, double tol,
                            unsigned long long *hostw, hipStream_t st);
void launch_sc_obj_guarded(CgState *s, const double *part, int g, int k, double tol, unsigned long long *hostw,
                           hipStream_t st);
void launch_sum_to(const double *part, int g, double *out, hipStream_t st);

}  // namespace unires
