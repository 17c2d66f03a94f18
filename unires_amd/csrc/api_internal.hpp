// api_internal.hpp - what the translation units behind the C ABI (include/unires_hip.h) share: error plumbing,
// the description of an operator and the device tables built for it, the plan object, the description of a CG
// solve, and the few functions that cross files.  api.hip: op-level entry points, ADMM sums, marks; api_plan.hip:
// the plan and its table builds; api_operator.hip: which kernels apply A, A^T, A^T A and the matvec; api_cg.hip:
// the CG driver.  Host-only.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/unires_hip.h"
#include "ata1.hpp"
#include "cg.hpp"
#include "fftpre.hpp"
#include "fused.hpp"
#include "gain.hpp"
#include "mask.hpp"
#include "orient.hpp"
#include "pull2.hpp"
#include "shift.hpp"
#include "slice.hpp"
#include "splat2.hpp"
#include "voxel.hpp"

namespace unires {

// --------------------------------------------------------------------------
// error plumbing (the string unires_last_error returns; defined in api.hip)
// --------------------------------------------------------------------------
extern thread_local std::string g_err;

inline int fail(int code, const char *msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                               \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      unires::g_err = std::string(#expr) + ": " + hipGetErrorString(e_);            \
      return UNIRES_ERR_HIP;                                                        \
    }                                                                               \
  } while (0)

#define CHECK_LAUNCH()                                                              \
  do {                                                                              \
    hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) {                                                         \
      unires::g_err = std::string("kernel launch: ") + hipGetErrorString(e_);       \
      return UNIRES_ERR_HIP;                                                        \
    }                                                                               \
  } while (0)

inline bool dims_ok(const int32_t d[3]) {
  return d[0] > 0 && d[1] > 0 && d[2] > 0 && d[0] <= 65535 &&
         (long long)d[0] * d[1] * d[2] < (1ll << 40);
}
inline bool vx_ok(const float vx[3]) { return vx && vx[0] > 0 && vx[1] > 0 && vx[2] > 0; }
inline Dim3i mk(const int32_t d[3]) { return Dim3i{d[0], d[1], d[2]}; }
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// argument checking shared by the op level and the plan (api.hip)
int make_taps(const float *const taps[3], const int32_t ntaps[3], const int32_t stride[3], Taps &T);
int check_conv_dims(const Dim3i &hi, const Dim3i &lo, const Taps &T);  // hi = (lo - 1) * stride + ntaps
bool invert_affine(const Affine &A, Affine &out);  // row-major 3x4 float32, computed in double

// --------------------------------------------------------------------------
// scaling (kNoScaling, is_dirac, set_dirac, fan_in: common.hpp)
// --------------------------------------------------------------------------
inline Scaling make_scaling(float scl, int dim) {
  if (scl == 0.f) return kNoScaling;
  return Scaling{expf(scl), expf(-scl), dim};
}

// UNIRES_PUSH, read once per process.  Unset: the schedule-driven splat (k_splat2) and ata_forward's one-kernel
// x / y forms, then the general kernels where an operator is outside their domain.  "tile": the general tile kernel
// only (the tests' cross-check).  Any other value: neither of those - k_splat, then the tile kernel.
enum class PushMode { kDefault, kTile, kNoSchedule };
inline PushMode push_mode() {
  static const PushMode mode = [] {
    const char *e = getenv("UNIRES_PUSH");
    return !e ? PushMode::kDefault : !strcmp(e, "tile") ? PushMode::kTile : PushMode::kNoSchedule;
  }();
  return mode;
}

// --------------------------------------------------------------------------
// one repeat (observation) of a plan: the operator's description, and the device tables built for it
// --------------------------------------------------------------------------
// What fill_repeat derives from a unires_repeat_t.  Trivially copyable; owns nothing.
struct RepeatDesc {
  // Everything below is in the plan's CANONICAL voxel layout of the observation: x-space axis d runs
  // mainly along +d of the output (orient.hpp).  `orient` maps it to the caller's layout, `dim_xu`
  // are the caller's x-space dims; only 'A' outputs and 'At' / RHS inputs are ever re-ordered.
  Orient orient;
  bool oriented = false;
  Dim3i dim_xu;
  Dim3i dim_x, dim_g;
  Affine A;
  Taps T;
  float scl;
  int dim_thick;
  float tau;
  // fused path: zero taps trimmed, grid shifted accordingly, inverse affine
  Dim3i dim_gf;
  Affine Af, Afinv;
  Taps Tf;
  SplatSafety safe;  // of Af (the linear part is the same for A)
  bool sep = false;  // many-tap profile: convolutions run as separable 1-D passes
  bool sep0 = false; // ... as decided from the taps alone (the hybrid form clears `sep`; kept for its fallback)
  // profile along x and / or y AND z with a z fan-in <= 2 (isotropic down-sampling, BASELINE config
  // 4): the x / y part runs as 1-D passes through a (gf.x, gf.y, xd.z) intermediate, the z part
  // stays fused in the pull / splat kernels, which then cost what they cost for a z-only profile
  // (build_repeat_kernels revises hyb / hybf / sep where the kernels turn out to be unavailable)
  bool hyb = false;
  // forward-only hybrid (r3): many-tap profiles (sep) whose z part the window pull can still fuse -
  // any number of z taps - while conv_up keeps its 1-D passes (the splat tabulates a fan-in of 2 only):
  // the default Gaussian in-plane profile of BASELINE config 4
  bool hybf = false;
  Taps Tz, Txy;
  Dim3i dim_h;
};

// What the build_* functions make for a description; keeps its device allocations across unires_plan_set_repeat
// (contents rebuilt), freed by free_tables.
struct RepeatTables {
  // schedule-driven splat (splat2.hip): per-tile segment lists of this operator + conv_up tables
  // along the schedule's axis ([0] no scaling, [1] S(scl)); ctab_n entries, second x-space value
  // ctab_step elements after the first
  SplatSched sched;
  float *ctab_dev[2] = {nullptr, nullptr};
  int ctab_n = 0, ctab_cap = 0;
  unsigned ctab_step = 1, src_stride = 1;
  float *xytab_dev[2] = {nullptr, nullptr};  // axis 3: conv_up tables along x and y (schedule build)
  int xytab_cap[2] = {0, 0};
  PullPlan pplan;   // LDS-window pull: per-workgroup geometry of this operator (pull2.hip)
  ShiftPlan shift;  // translation-only operators: factors of AtA for the one-kernel matvec (shift.hip)
  F1Sched f1;       // denoising regime: schedule of the single-pass AtA kernel (ata1.hip)
};

// sett.mask_zeros (unires_plan_set_missing): the validity mask of the repeat's observation, one byte per x-space voxel
// (mask.hip).  mask_u is in the caller's layout and kept so that a new orientation (unires_plan_set_repeat) can be
// served without the observation; mask_c, only where the plan relabels the observation, is its canonical-layout copy.
// The allocations stay until the plan goes; `masked` says whether they count.
struct RepeatMask {
  bool masked = false;
  uint8_t *mask_u = nullptr, *mask_c = nullptr;
  size_t mask_cap = 0;  // entries of either allocation
};

// Per-slice weights (unires_plan_set_slice_weights): u, one float per slice along the caller's axis w_axis, in the
// caller's slice order.  ONE buffer, whatever the orientation: the pass that applies it (slice.hip) is given the
// canonical axis behind w_axis and whether it is reversed, so unires_plan_set_repeat needs no device work, and the
// buffer's address stays while the repeat is weighted - a captured solve reads the values it holds when it runs.
// Sized for the longest axis of the observation at the first set; freed with the plan.
struct RepeatWeights {
  bool weighted = false;
  float *w_dev = nullptr;
  int w_axis = 0;
  size_t w_cap = 0;  // entries
};

// Per-voxel weights (unires_plan_set_voxel_weights): g, one float per x-space voxel (voxel.hip).  As the mask: g_u is in
// the caller's layout and kept so that a new orientation (unires_plan_set_repeat) can be served without the caller's
// map; g_c, only where the plan relabels the observation, is its canonical-layout copy.  Neither address changes while
// the repeat is weighted - a captured solve reads the values they hold when it runs.  Freed with the plan.
struct RepeatVoxel {
  bool voxw = false;
  float *g_u = nullptr, *g_c = nullptr;
  size_t g_cap = 0;  // entries of either allocation
};

// Per-slice intensity gains (unires_plan_set_slice_gains): e, one float per slice along the caller's axis e_axis, in the
// caller's slice order, and the two tables composed from it and the slice weights u (1 where the repeat has none;
// gain.hip: k_gain_compose): w_mat = u e^2, what the pass between the halves of A^T A multiplies by, and w_rhs = u e,
// what the right-hand side's observation is multiplied by.  ONE allocation of three tables, as for the weights: the
// passes are given the canonical axis and its direction, and no address changes while the repeat is gained - a
// captured solve reads the values the tables hold when it runs.  Freed with the plan.
struct RepeatGains {
  bool gained = false;
  float *e_dev = nullptr, *wm_dev = nullptr, *wr_dev = nullptr;
  int e_axis = 0;
  size_t e_cap = 0;  // entries of each table
};

struct Repeat : RepeatDesc, RepeatTables, RepeatMask, RepeatWeights, RepeatVoxel, RepeatGains {
  // the voxel weights in the layout the x-space intermediate of A^T A has
  const float *vox() const { return oriented ? g_c : g_u; }
  // the mask in the layout the x-space intermediate of A^T A has
  const uint8_t *mask() const { return oriented ? mask_c : mask_u; }
  // a pass runs on the x-space intermediate of A^T A (mask, slice weights, voxel weights, gains or any of them
  // together): the intermediate has to exist, so the one-kernel matvecs, the single-pass AtA kernel and the hybrid
  // forms are declined
  bool mid() const { return masked || weighted || voxw || gained; }
  // the per-slice factor of the pass between the halves of A^T A and of the right-hand side's observation: the slice
  // weights, or a gained repeat's composed tables; nullptr: none
  const float *w_mat() const { return gained ? wm_dev : (weighted ? w_dev : nullptr); }
  const float *w_rhs() const { return gained ? wr_dev : (weighted ? w_dev : nullptr); }
  // the caller's axis the slices of that factor are counted along (weights and gains of one repeat share it)
  int s_axis() const { return gained && !weighted ? e_axis : w_axis; }
  // the canonical axis the slices of s_axis() run along, and whether the plan reversed it
  int w_caxis() const {
    const int a = s_axis();
    for (int j = 0; j < 3; ++j)
      if (orient.perm[j] == a) return j;
    return a;
  }
  bool w_flip() const { return orient.flip[w_caxis()] != 0; }
};

// --------------------------------------------------------------------------
// one CG solve: what the caller asked for, what follows from it, and how it is enqueued.  The parameter of the
// cg_enqueue_* functions, and the key a captured graph is compared against.
// --------------------------------------------------------------------------
struct CgSolve {
  const float *b = nullptr;
  float *x = nullptr;
  float rho = 0.f, lam = 0.f;
  int max_iter = -1, stop = -1, pre = -1;
  double tol = -1.0;
  int ring = 1;   // direction buffers of the deferred iterate update (1: the iterate updated every iteration)
  int chunk = 0;  // iterations per chunk of a chunked solve; 0: the solve is enqueued whole
  // derived (not compared): the Jacobi diagonal, or nullptr; the FFT-diagonal preconditioner
  const float *M = nullptr;
  bool fft = false;
  // a graph captured for `o` serves this solve (a captured solve has every one of these baked in)
  bool same_graph(const CgSolve &o) const {
    return b == o.b && x == o.x && rho == o.rho && lam == o.lam && max_iter == o.max_iter && stop == o.stop &&
           pre == o.pre && ring == o.ring && chunk == o.chunk && tol == o.tol;
  }
};

// How a solve went: what unires_plan_cg_ring, unires_plan_cg_ends and unires_plan_cg_lockstep report of the plan's last
// one.  The enqueue functions (api_cg.hip) say it of what they enqueue, a captured solve keeps it for its replays, and
// the entry point that finishes a solve puts it into the plan.
struct CgHow {
  int ring = 1;      // K of the deferred iterate update (1: the iterate updated every iteration)
  int trim = 0;      // the last iteration was the operator, alpha and the iterate alone
  int fused = 0;     // the start's residual was written by the operator's push
  int lockstep = 0;  // the solve ran inside the channels' two-lane schedule
};

// A captured solve: the executable graph(s), the solve they were captured for, and what a replay of them reports.
// Empty (no graph, a key that no solve has) until a capture succeeds and again after destroy().
struct CgCaptured {
  hipGraphExec_t exec = nullptr;   // the whole solve; of a chunked solve, the start
  hipGraphExec_t chunk = nullptr;  // a chunked solve's `key.chunk` iterations
  CgSolve key;
  CgHow how;
  bool matches(const CgSolve &s) const { return key.same_graph(s); }
  void destroy() {  // (the caller has waited for launches in flight where there may be any)
    if (exec) (void)hipGraphExecDestroy(exec);
    if (chunk) (void)hipGraphExecDestroy(chunk);
    *this = CgCaptured();
  }
};

}  // namespace unires

struct unires_plan {
  unires::Dim3i dy;
  float vx[3];
  int regime;
  float fov_tol;
  int diff = UNIRES_DIFF_FORWARD;  // the difference of the regulariser's D (unires_plan_set_diff)
  std::vector<unires::Repeat> reps;
  // device workspace (one allocation)
  char *ws = nullptr;
  size_t ws_bytes = 0;
  float *r = nullptr, *p = nullptr, *ap = nullptr, *ax = nullptr;  // N_y each
  // measurement aid (unires_plan_time_matvecs): event pairs around the operator applications of a solve
  bool timing = false;
  bool twice = false;  // unires_plan_time_matvecs(plan, 2): every A(p) of a solve is enqueued twice (same result)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;
  float *gbuf = nullptr;                                           // max N_g
  float *gbuf2 = nullptr;  // second grid-space scratch, only for many-tap profiles (separable passes)
  float *xbuf = nullptr;                                           // max N_x
  float *xperm = nullptr;  // max N_x: an x-space volume on its way between the caller's layout and the canonical one
  double *part0 = nullptr, *part1 = nullptr;                       // kMaxPartials each
  unires::CgState *state = nullptr;
  size_t cap_g = 0, cap_x = 0;
  // the whole CG solve as one hipGraph, re-launched while (b, x, rho, lam, options) stay the
  // same - the ADMM loop calls it with identical arguments until the schedule changes
  unires::CgCaptured cg_whole;
  // chunked solves: start + chunk graphs (keyed without max_iter: they serve a solve of any length), the host-mapped
  // progress word and the solve counter
  unires::CgCaptured cg_chunks;
  unires::CgHow last;  // how the plan's last solve went
  unsigned long long *progress = nullptr, *progress_dev = nullptr;
  unsigned cg_gen = 0;
  float *precM = nullptr;  // Jacobi diagonal (own allocation, made by unires_precond_build)
  // deferred iterate update of tol = 0 solves (cg_ring_prepare): ring slot 0 is `p`, slots 1 .. ring_slots live in
  // `ring` (own allocation, made at the first such solve, freed with the plan only: a graph may have it baked in)
  float *ring = nullptr;
  int ring_slots = 0;
  bool ring_tried = false;  // the allocation was decided (made, refused by the budget, or failed)
  int ring_req = 0;         // unires_plan_cg_ring: K asked for (0: UNIRES_CG_RING or the default)
  unires::FftPre fft;      // FFT-diagonal preconditioner (plans + buffers, made on demand)
  float prec_rho = 0.f, prec_lam = 0.f;
  int prec_mode = UNIRES_PRECOND_IDENTITY;
  bool prec_ready = false;
  // the last launch that reads this plan's tables: unires_plan_set_repeat / the graph teardown wait for THIS
  // event instead of the whole device (other channels' streams keep running).  A launch enqueued while its
  // stream was being captured cannot be waited for through an event: `captured_use` sends those to the
  // device-wide wait.
  hipEvent_t last_use = nullptr;
  std::vector<hipStream_t> use_streams;
  bool captured_use = false;
  // unires_plan_set_concurrency: how many solves the caller keeps in flight on the device (channels of a y-update on
  // streams of their own), and the caps on the persistent kernels' grids that follow from it (0: the whole chip)
  int concurrency = 1;
  int cap_s2 = 0, cap_f1 = 0;
  // the two-lane schedule of several channels' solves (api_cg.hip: cg_lockstep_solve).  cap_s2_ls: k_splat2's grid
  // cap in that mode, taken while `lockstep` is up (the schedule is being enqueued); cg_epoch: moved by drop_cg_graph,
  // unique among all plans of the process - a schedule captured at another epoch is stale
  int cap_s2_ls = 0;
  bool lockstep = false;
  unsigned long long cg_epoch = 0;
};

namespace unires {

// api_plan.hip
bool stream_capturing(hipStream_t st);
void mark_use(unires_plan *pl, hipStream_t st);  // note the plan's last use (see unires_plan::last_use) ...
void await_use(unires_plan *pl);                 // ... and wait for it
void drop_cg_chunk_graphs(unires_plan *pl);
void drop_cg_graph(unires_plan *pl);  // every captured solve of the plan, the chunk graphs included
unsigned long long next_cg_epoch();

// api_cg.hip
void cg_lockstep_forget(unires_plan *pl);  // the captured schedules the plan is part of (unires_plan_destroy)

// api_operator.hip
// q = sum_n tau_n AtA_n p + rho lam^2 DtD p ; optional dot partials of sum(p*q).
// With objb (and part): the partials hold sum (q - 2 objb) * p instead and the final q is not
// stored (q is still scratch for the partial sums of a multi-repeat operator).
// Returns the number of partials written (0 if none requested).
// With res (the start of a CG solve; part and objb unset): a route that can (k_splat2 as the last repeat's push of a
// forward-difference plan without masked or weighted repeats) writes r = b - q, z = r or r / M and the partials of sum r z
// instead of storing q, and sets res->served; the return value is then the number of those partials.  Any other
// route ignores it: q is stored as without res, served stays false.
struct StartResidual {
  const float *b;
  float *r, *p;       // r, and z = the first direction
  const float *M;     // Jacobi diagonal or nullptr
  double *partials;
  double *obj_partials;  // nullable: the partials of the start's objective sum (A(x) - 2 b) x
  bool served;
};
int matvec(unires_plan *pl, float rho, float lam, const float *p, float *q, double *part, const int *done,
           hipStream_t st, const float *objb = nullptr, StartResidual *res = nullptr);

}  // namespace unires
