// api_cg.hip - CG (nitorch.core.optim.cg as UniRes calls it): how a solve (CgSolve,
// api_internal.hpp) is enqueued - whole, with the iterate update deferred over a ring of directions, or in chunks
// that follow the device's progress -, the hipGraphs it is captured into, and unires_cg_solve(_many).
#include <time.h>

#include <functional>
#include <mutex>

#include "api_internal.hpp"

using namespace unires;

// The switches of the CG driver, read once per process, at its first solve (the ring's budget apart).
//   UNIRES_CG_START_FUSED  0: k_residual_init at the start of every solve, never the operator's own push
//   UNIRES_CG_TRIM         0: the last iteration of every solve is enqueued in full
//   UNIRES_CG_GRAPH        0: plain launches, no solve is captured into a hipGraph
//                          (these three are off only when set with '0' as the first character)
//   UNIRES_CG_LOCKSTEP     the halved flush (`flush_halved`: cg.hip, through cg_lockstep_env) and the two-lane schedule of
//                          several channels' fixed-iteration solves (`lockstep`): on when set and the first character is
//                          not '0', else kLockstepDefault (cg.hpp).  The schedule's graph has two parallel branches,
//                          which the runtime is known to mishandle with fewer than 4 hardware queues: it is never taken
//                          when GPU_MAX_HW_QUEUES is set below 4
//   UNIRES_CG_RING         K of the deferred iterate update (atoi; default 8; clamped by cg_ring_prepare)
//   UNIRES_CG_RING_MB      the ring's budget in MiB (atof; unset: an eighth of the free device memory) - read by
//                          ring_budget() at each plan's first deferred solve, not with the others
//   UNIRES_CG_CHUNK        iterations per chunk of a solve that can stop early (atoi; default 2; chunk_size() clamps it
//                          to 1 .. 64); 0: no chunked solves
struct CgSwitches {
  bool start_fused = not_off("UNIRES_CG_START_FUSED"), trim = not_off("UNIRES_CG_TRIM");
  bool graphs = not_off("UNIRES_CG_GRAPH");
  bool flush_halved = kLockstepDefault, lockstep = false;
  int ring = 8, chunk = 2;
  CgSwitches() {
    if (const char *e = getenv("UNIRES_CG_LOCKSTEP")) flush_halved = e[0] != '0';
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    lockstep = flush_halved && !(q && atoi(q) < 4);
    if (const char *e = getenv("UNIRES_CG_RING")) ring = atoi(e);
    if (const char *e = getenv("UNIRES_CG_CHUNK")) chunk = atoi(e);
  }
  int chunk_size() const { return std::max(1, std::min(chunk, 64)); }
  static size_t ring_budget() {
    if (const char *e = getenv("UNIRES_CG_RING_MB")) return (size_t)std::max(0.0, atof(e) * 1048576.0);
    size_t free_b = 0, total_b = 0;
    const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    (void)hipGetLastError();
    return known ? free_b / 8 : 0;
  }

 private:
  static bool not_off(const char *name) {
    const char *e = getenv(name);
    return !(e && e[0] == '0');
  }
};
static const CgSwitches &cg_switches() {
  static const CgSwitches sw;
  return sw;
}
bool unires::cg_lockstep_env() { return cg_switches().flush_halved; }

// The solve is enqueued in two parts: the start (r = b - A x, p, r.z, obj[0]) and runs of iterations.
// `dev_k`: the iteration index is the device state's own counter (a captured chunk of iterations then
// serves any part of a solve); `hostw`: the scalar kernel that ends an iteration publishes the state's
// (generation, done, iterations) to this host-mapped word.  Each part says what it did in `how` (CgHow,
// api_internal.hpp); the entry point that finishes the solve puts that into the plan.
static int cg_enqueue_start(unires_plan *pl, const CgSolve &s, unsigned long long *hostw, hipStream_t st, CgHow &how) {
  const size_t ny = pl->dy.numel();
  const bool check = s.tol != 0.0;
  CgState *S = pl->state;
  const int gv = vec_num_blocks(ny);
  // r = b - A(x); p = r; rz = r.r; obj[0]
  HIP_TRY(hipMemsetAsync(&S->done, 0, sizeof(int), st));
  // Where the push that ends the operator can (matvec, api_operator.hip) it writes r, p and the partials of r.z - and
  // of the start's objective, where the stopping rule wants obj[0] - itself, and A(x) is never stored.  The partials
  // are then grouped by the push's waves, not by k_residual_init's blocks: r.z and obj[0] are the float64 sums of the
  // same float32 terms in another order, and agree with the other route's to the rounding of such a sum.
  const bool want_obj0 = check && s.stop != UNIRES_STOP_RESIDUAL;
  StartResidual res = {s.b, pl->r, pl->p, s.M, pl->part0, want_obj0 ? pl->part1 : nullptr, false};
  const bool ask = cg_switches().start_fused && !s.fft;
  int g0 = matvec(pl, s.rho, s.lam, s.x, pl->ap, nullptr, nullptr, st, nullptr, ask ? &res : nullptr);
  how.fused = ask && res.served;
  if (!how.fused) {
    launch_residual_init(s.b, pl->ap, s.x, pl->r, pl->p, ny, pl->part0, want_obj0 ? pl->part1 : nullptr, s.M, st);
    g0 = gv;
  }
  if (s.fft) {  // z = M^-1 r ; p = z ; rz = r.z
    if (fftpre_apply(pl->fft, pl->r, pl->fft.z, st)) return fail(UNIRES_ERR_HIP, "hipFFT execution failed");
    HIP_TRY(hipMemcpyAsync(pl->p, pl->fft.z, ny * sizeof(float), hipMemcpyDeviceToDevice, st));
    launch_dot(pl->r, pl->fft.z, ny, pl->part0, nullptr, st);
  }
  launch_sc_init(S, pl->part0, pl->part1, g0, s.stop, check ? 1 : 0, hostw, st);
  return UNIRES_OK;
}

// slot j of the plan's direction ring (slot 0: the buffer the start writes p into)
static float *ring_slot(unires_plan *pl, int j) {
  return j == 0 ? pl->p : pl->ring + (size_t)(j - 1) * (align_up(pl->dy.numel() * 4) / 4);
}

// Iterations k_first .. k_first + count - 1 of the solve.
// s.ring > 1 (tol = 0 solves enqueued whole, cg_ring_prepare): the iterate update is deferred - iteration k's
// direction is slot (k - k_first) mod ring, and x takes the window's alpha p terms at every ring-th iteration and at
// the last (k_update_p_flush, cg.hip).
// The last iteration of a solve that runs all its iterations and is enqueued whole (tol = 0, !dev_k, no FFT
// preconditioner: the scope of the deferred update) is the operator, alpha and the iterate alone: nothing reads the
// residual, r.z, beta or direction that would follow it.  k_sc_alpha writes the iteration count in k_sc_beta's stead;
// the plan's r, rz and beta stay those of the iteration before.
// An iteration is stated in two parts, each once: its operator application (cg_iter_operator) and everything after
// it (cg_iter_rest).  cg_enqueue_iters puts them on one stream in turn; the two-lane schedule of several channels
// (cg_lockstep_enqueue) puts the first on one stream and the second on another.
struct CgIters {
  int k_first = 1, count = 0;
  bool dev_k = false, trim = false;
  unsigned long long *hostw = nullptr;
  RingPtrs rp = {};
};

static int cg_iters_begin(unires_plan *pl, const CgSolve &s, int k_first, int count, bool dev_k,
                          unsigned long long *hostw, CgIters &it, CgHow &how) {
  const bool check = s.tol != 0.0;
  const int ring = s.ring;
  if (ring > 1 && (check || s.fft || dev_k || ring > kMaxRing || ring - 1 > pl->ring_slots))
    return fail(UNIRES_ERR_ARG, "deferred iterate update outside its scope");  // (cg_ring_prepare decides; never here)
  it.k_first = k_first, it.count = count, it.dev_k = dev_k, it.hostw = hostw;
  // (enqueued whole: this call IS the solve, so its last iteration is the solve's; a chunk - dev_k - never is)
  it.trim = cg_switches().trim && !check && !s.fft && !dev_k && k_first == 1 && count == s.max_iter && count > 0;
  how.ring = ring, how.trim = it.trim;
  it.rp = RingPtrs{};
  for (int j = 0; j < ring && ring > 1; ++j) it.rp.p[j] = ring_slot(pl, j);
  return UNIRES_OK;
}

// this iteration's direction
static float *cg_iter_direction(unires_plan *pl, const CgSolve &s, const CgIters &it, int k) {
  return s.ring > 1 ? ring_slot(pl, (k - it.k_first) % s.ring) : pl->p;
}

// The operator of iteration k: ap = A(p_k) and the partials of p.Ap.  Returns the number of partials.
static int cg_iter_operator(unires_plan *pl, const CgSolve &s, const CgIters &it, int k, hipStream_t st) {
  const int *done = &pl->state->done;
  float *p = cg_iter_direction(pl, s, it, k);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (pl->timing && hipEventCreate(&ev0) == hipSuccess) {
    if (hipEventCreate(&ev1) == hipSuccess) {
      (void)hipEventRecord(ev0, st);
    } else {
      (void)hipEventDestroy(ev0);
      ev0 = nullptr;
    }
  }
  if (pl->twice) (void)matvec(pl, s.rho, s.lam, p, pl->ap, pl->part0, done, st);  // (measurement: see the header)
  const int g = matvec(pl, s.rho, s.lam, p, pl->ap, pl->part0, done, st);
  if (ev0 && ev1) {
    (void)hipEventRecord(ev1, st);
    if (pl->tev.size() >= 65536) {  // a caller that never collects: forget the oldest pair
      (void)hipEventDestroy(pl->tev.front().first), (void)hipEventDestroy(pl->tev.front().second);
      pl->tev.erase(pl->tev.begin());
    }
    pl->tev.emplace_back(ev0, ev1);
  }
  return g;
}

// The rest of iteration k, after its operator wrote `g` partials: alpha, x / r, beta and the next direction - or,
// for the trimmed last iteration, alpha and the iterate alone.
static int cg_iter_rest(unires_plan *pl, const CgSolve &s, const CgIters &it, int k, int g, hipStream_t st) {
  const size_t ny = pl->dy.numel();
  const bool check = s.tol != 0.0;
  const int ring = s.ring;
  CgState *S = pl->state;
  const int *done = &S->done;
  const int gv = vec_num_blocks(ny);
  unsigned long long *hostw = it.hostw;
  const RingPtrs &rp = it.rp;
  const int k_first = it.k_first, count = it.count;
  const int kk = it.dev_k ? -1 : k;
  const int slot = ring > 1 ? (k - k_first) % ring : 0;
  float *p = cg_iter_direction(pl, s, it, k);
  const bool guarded = check && s.stop == UNIRES_STOP_MAXGAIN_GUARDED;
  const bool recur = check && (s.stop == UNIRES_STOP_MAXGAIN_RECURRED || guarded);
  int obj_kind = 0;
  if (check && s.stop == UNIRES_STOP_RESIDUAL) obj_kind = 1;
  if (recur) obj_kind = 2;
  // "x += alpha p" rides with the p update unless sc_beta can stop the solve in between
  const bool lazy_x = obj_kind == 0;
  if (it.trim && k == k_first + count - 1) {
    launch_sc_alpha(S, pl->part0, g, st, k);
    if (ring > 1)
      launch_update_x_flush(S, rp, slot + 1, ny, s.x, st);
    else
      launch_update_x(S, p, ny, s.x, st);
    return UNIRES_OK;
  }
  launch_sc_alpha(S, pl->part0, g, st);
  launch_update_xr(S, p, pl->ap, lazy_x ? nullptr : s.x, pl->r, s.b, ny, pl->part0,
                   recur ? pl->part1 : nullptr, s.M, st);
  if (s.fft) {  // (the transforms also run after convergence: hipFFT has no device-side skip)
    if (fftpre_apply(pl->fft, pl->r, pl->fft.z, st)) return fail(UNIRES_ERR_HIP, "hipFFT execution failed");
    launch_dot(pl->r, pl->fft.z, ny, pl->part0, done, st);
  }
  if (guarded)
    launch_sc_beta_guarded(S, pl->part0, pl->part1, gv, kk, s.tol, hostw, st);
  else
    launch_sc_beta(S, pl->part0, pl->part1, gv, kk, obj_kind, s.tol, obj_kind ? hostw : nullptr, st);
  if (ring > 1 && (slot == ring - 1 || k == k_first + count - 1))
    launch_update_p_flush(S, pl->r, rp, slot + 1, ring_slot(pl, (slot + 1) % ring), ny, s.M, s.x, st);
  else if (ring > 1)
    launch_update_p_ring(S, pl->r, p, ring_slot(pl, slot + 1), slot, ny, s.M, st);
  else
    launch_update_p(S, s.fft ? pl->fft.z : pl->r, pl->p, ny, s.M, lazy_x ? s.x : nullptr, st);
  if (check && s.stop == UNIRES_STOP_MAXGAIN) {
    // objective sum x (Ax - 2b) folded into the matvec epilogue: A(x) is never stored
    const int go = matvec(pl, s.rho, s.lam, s.x, pl->ax, pl->part1, done, st, s.b);
    launch_sc_obj(S, pl->part1, go, kk, s.tol, hostw, st);
  }
  if (guarded) {
    // ... the same, but its kernels return at entry unless k_sc_beta_guarded asked for it (cg.hip)
    const int go = matvec(pl, s.rho, s.lam, s.x, pl->ax, pl->part1, &S->skip_fresh, st, s.b);
    launch_sc_obj_guarded(S, pl->part1, go, kk, s.tol, hostw, st);
  }
  return UNIRES_OK;
}

static int cg_enqueue_iters(unires_plan *pl, const CgSolve &s, int k_first, int count, bool dev_k,
                            unsigned long long *hostw, hipStream_t st, CgHow &how) {
  CgIters it;
  int rc = cg_iters_begin(pl, s, k_first, count, dev_k, hostw, it, how);
  for (int k = k_first; !rc && k < k_first + count; ++k) {
    const int g = cg_iter_operator(pl, s, it, k, st);
    rc = cg_iter_rest(pl, s, it, k, g, st);
  }
  return rc;
}

// Enqueues the whole solve (every kernel of nitorch's cg()) on `st`.
static int cg_enqueue(unires_plan *pl, const CgSolve &s, hipStream_t st, CgHow &how) {
  const int rc = cg_enqueue_start(pl, s, nullptr, st, how);
  if (rc) return rc;
  return cg_enqueue_iters(pl, s, 1, s.max_iter, false, nullptr, st, how);
}

// K of the deferred iterate update for a solve that nothing reads x of before it ends (tol = 0, no FFT
// preconditioner; the caller checks that): unires_plan_cg_ring's request, else
// UNIRES_CG_RING, else 8, clamped to 1 .. kMaxRing.  The K - 1 extra direction buffers are allocated at the plan's
// first such solve, within a budget (UNIRES_CG_RING_MB, default an eighth of the free device memory); the ring is
// never grown or freed after that (a graph - ours or a caller's capture - may have its buffers baked in), so later
// requests get at most what was allocated then.  No room, a failed allocation, or a stream under capture at that
// first solve: K = 1, the iterate updated every iteration.
static int cg_ring_prepare(unires_plan *pl, hipStream_t st) {
  int want = pl->ring_req > 0 ? pl->ring_req : cg_switches().ring;
  want = std::max(1, std::min(want, kMaxRing));
  if (want <= 1) return 1;
  if (!pl->ring_tried) {
    if (stream_capturing(st)) return 1;  // (no allocation inside a capture: decided at the next plain solve)
    pl->ring_tried = true;
    const size_t slot = align_up(pl->dy.numel() * 4);
    const int n = (int)std::min<size_t>((size_t)(want - 1), CgSwitches::ring_budget() / slot);
    if (n < 1) return 1;
    if (hipMalloc((void **)&pl->ring, (size_t)n * slot) != hipSuccess) {
      (void)hipGetLastError();
      pl->ring = nullptr;
      return 1;
    }
    pl->ring_slots = n;
  }
  return std::min(want, pl->ring_slots + 1);
}

// --------------------------------------------------------------------------
// Chunked solves (round 4): a solve that can stop early (tolerance > 0: the reference's default,
// struct.py:65-67 cgs_tol = 1e-3, 'max_gain') is enqueued as the start + chunks of `chunk` iterations,
// one chunk of look-ahead.  The kernel that ends an iteration publishes (generation, done, iterations)
// to a host-mapped word; the host enqueues the next chunk when the older of the two in flight has
// finished and the flag is not up - no stream synchronisation, the device never idles, and at most
// 2 chunk - 1 iterations run as no-op kernels after convergence (enqueuing all max_iter iterations, as
// rounds 1-3 did, ran 45 of config 3's 60 iterations as ~10 no-op kernels each).  The realised
// iteration count, iterate and objective trace are those of the full enqueue: the same kernels in
// the same order, the stopping test on the device.  Start and chunk are hipGraphs, captured once per
// (b, x, rho, lam, options) and replayed.
// --------------------------------------------------------------------------
struct CgRun {
  unires_plan *pl = nullptr;
  CgSolve s;  // (s.chunk: iterations per chunk)
  hipStream_t st = nullptr;
  int enqueued = 0;     // iterations enqueued so far
  unsigned gen = 0;     // generation of this solve
  bool finished = false;
  bool use_graph = false;
  CgHow how;  // what the start and the chunks did, enqueued or replayed
};

// The host counts the solves it starts (cg_gen), k_sc_init counts the ones that run (state->gen); the chunked
// driver matches the two in the progress word.  After an enqueue / capture / launch that FAILED somewhere
// between the two increments they may be out of step for the life of the plan: read the device's back.
static void cg_resync_gen(unires_plan *pl) {
  (void)hipDeviceSynchronize();
  (void)hipGetLastError();
  unsigned g = pl->cg_gen;
  if (pl->state && hipMemcpy(&g, &pl->state->gen, sizeof(g), hipMemcpyDeviceToHost) == hipSuccess) pl->cg_gen = g;
  (void)hipGetLastError();
}

static int capture_graph(hipStream_t st, hipGraphExec_t *exec, const std::function<int()> &body) {
  *exec = nullptr;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return -1;  // capture refused: the caller launches plainly
  }
  const int rc = body();
  hipGraph_t graph = nullptr;
  const hipError_t ce = hipStreamEndCapture(st, &graph);
  if (rc) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (ce != hipSuccess || !graph) return fail(UNIRES_ERR_HIP, "hipStreamEndCapture failed");
  const hipError_t ge = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ge != hipSuccess) {
    *exec = nullptr;
    return fail(UNIRES_ERR_HIP, "hipGraphInstantiate failed");
  }
  return UNIRES_OK;
}

static int cg_run_enqueue_chunk(CgRun &R) {
  unires_plan *pl = R.pl;
  const int n = std::min(R.s.chunk, R.s.max_iter - R.enqueued);
  if (n <= 0) return UNIRES_OK;
  if (R.use_graph && n == R.s.chunk && pl->cg_chunks.chunk) {
    HIP_TRY(hipGraphLaunch(pl->cg_chunks.chunk, R.st));
  } else {
    const int rc = cg_enqueue_iters(pl, R.s, R.enqueued + 1, n, true, pl->progress_dev, R.st, R.how);
    if (rc) return rc;
  }
  R.enqueued += n;
  return UNIRES_OK;
}

static int cg_run_start_impl(CgRun &R) {
  unires_plan *pl = R.pl;
  if (!pl->progress) {
    HIP_TRY(hipHostMalloc((void **)&pl->progress, 64, hipHostMallocMapped));
    *pl->progress = 0ull;
    HIP_TRY(hipHostGetDevicePointer((void **)&pl->progress_dev, (void *)pl->progress, 0));
  }
  R.gen = ++pl->cg_gen;
  R.enqueued = 0;
  R.finished = false;
  // the start and chunk graphs serve a solve of any length, and see the preconditioner as a diagonal or none
  CgSolve key = R.s;
  key.max_iter = 0;
  key.pre = R.s.M ? UNIRES_PRECOND_JACOBI : UNIRES_PRECOND_IDENTITY;
  CgCaptured &G = pl->cg_chunks;
  if (R.use_graph && !G.matches(key)) {
    drop_cg_chunk_graphs(pl);
    CgHow how;
    int rc = capture_graph(R.st, &G.exec, [&] { return cg_enqueue_start(pl, R.s, pl->progress_dev, R.st, how); });
    if (rc > 0) return rc;
    if (rc == 0)
      rc = capture_graph(R.st, &G.chunk, [&] {
        return cg_enqueue_iters(pl, R.s, 1, R.s.chunk, true, pl->progress_dev, R.st, how);
      });
    if (rc > 0) return rc;
    if (rc < 0 || !G.exec || !G.chunk) {
      drop_cg_chunk_graphs(pl);
      R.use_graph = false;
    } else {
      G.key = key, G.how = how;
    }
  }
  if (R.use_graph) {
    R.how = G.how;
    HIP_TRY(hipGraphLaunch(G.exec, R.st));
  } else {
    const int rc = cg_enqueue_start(pl, R.s, pl->progress_dev, R.st, R.how);
    if (rc) return rc;
  }
  // two chunks in flight
  int rc = cg_run_enqueue_chunk(R);
  if (!rc) rc = cg_run_enqueue_chunk(R);
  if (rc) return rc;
  if (R.enqueued >= R.s.max_iter) R.finished = true;
  return UNIRES_OK;
}

static int cg_run_start(CgRun &R) {
  const int rc = cg_run_start_impl(R);
  if (rc) cg_resync_gen(R.pl);
  return rc;
}

// One look at the progress word (never blocks): enqueues the next chunk when the older chunk in flight is
// through and the solve has not converged.
static int cg_run_poll(CgRun &R) {
  if (R.finished) return UNIRES_OK;
  const unsigned long long w = __atomic_load_n(R.pl->progress, __ATOMIC_ACQUIRE);
  if ((unsigned)(w >> 32) != R.gen) return UNIRES_OK;  // this solve's first kernels have not run yet
  if (w & 0x80000000ull) {
    R.finished = true;
    return UNIRES_OK;
  }
  const int iters = (int)(w & 0x7fffffffull);
  while (!R.finished && iters >= R.enqueued - R.s.chunk) {
    const int rc = cg_run_enqueue_chunk(R);
    if (rc) return rc;
    if (R.enqueued >= R.s.max_iter) R.finished = true;
  }
  return UNIRES_OK;
}

// Drive a set of runs (each on its own plan and stream) until every one has everything it needs
// enqueued.  The host spins on the progress words; every so often it asks the streams for errors.
static int cg_runs_drive(std::vector<CgRun> &runs) {
  unsigned spins = 0;
  for (;;) {
    bool all = true;
    for (CgRun &R : runs) {
      if (R.finished) continue;
      const int rc = cg_run_poll(R);
      if (rc) return rc;
      all = all && R.finished;
    }
    if (all) return UNIRES_OK;
    // a chunk is hundreds of microseconds of device work and one more is queued behind it: after a short spin
    // the thread sleeps between looks (eight ranks on one host must not each burn a core on the wait)
    if (++spins > 256) {
      const struct timespec nap = {0, 50000};
      (void)nanosleep(&nap, nullptr);
    }
    // (a watchdog, not the progress signal - the word is: every 512th nap, ~25 ms, catches a faulted stream as
    // well as every 16th did, and a stream query on running work is not free: the runtime submits a marker
    // packet for it and its signal thread handles the completion)
    if ((spins <= 256 && (spins & 0xff) == 0) || (spins > 256 && (spins & 0x1ff) == 0)) {
      for (CgRun &R : runs) {
        if (R.finished) continue;
        const hipError_t q = hipStreamQuery(R.st);
        if (q == hipSuccess) {
          // the stream drained: whatever was enqueued has run and published; a look at the word must
          // either end the run or enqueue more
          const int before = R.enqueued;
          const int rc = cg_run_poll(R);
          if (rc) return rc;
          if (!R.finished && R.enqueued == before)
            return fail(UNIRES_ERR_HIP, "chunked CG: the stream drained without the expected progress");
        } else if (q != hipErrorNotReady) {
          g_err = std::string("chunked CG: ") + hipGetErrorString(q);
          return UNIRES_ERR_HIP;
        }
      }
    }
  }
}

static int cg_check_args(unires_plan *plan, float rho, float lam, const float *b, float *x, int32_t max_iter,
                         double tol, int32_t stop_mode, int32_t precond_mode) {
  if (!plan || !b || !x) return fail(UNIRES_ERR_NULL, "null argument");
  if (b == x) return fail(UNIRES_ERR_ARG, "b and x must not alias");
  if (max_iter < 0) return fail(UNIRES_ERR_ARG, "max_iter out of range");
  if (max_iter > kMaxCgIter && !(tol > 0.0))
    return fail(UNIRES_ERR_ARG, "max_iter beyond 4096 needs a tolerance (the solve is then enqueued in chunks)");
  if (stop_mode < 0 || stop_mode > 3) return fail(UNIRES_ERR_ARG, "bad stop mode");
  if (precond_mode < UNIRES_PRECOND_IDENTITY || precond_mode > UNIRES_PRECOND_FFT)
    return fail(UNIRES_ERR_UNSUPPORTED, "preconditioner modes: identity (0), Jacobi (1), FFT (2)");
  if (precond_mode != UNIRES_PRECOND_IDENTITY &&
      (!plan->prec_ready || plan->prec_mode != precond_mode || plan->prec_rho != rho ||
       plan->prec_lam != lam))
    return fail(UNIRES_ERR_ARG, "call unires_precond_build with this mode, rho and lam first");
  if (!(tol >= 0.0)) return fail(UNIRES_ERR_ARG, "tolerance must be >= 0");
  return UNIRES_OK;
}

// chunked enqueue: solves that can stop early, unless switched off (UNIRES_CG_CHUNK=0: the full enqueue)
static bool cg_chunked(double tol, int max_iter) {
  const bool off = cg_switches().chunk == 0;
  return tol != 0.0 && max_iter > 0 && (!off || max_iter > kMaxCgIter);
}

static CgSolve cg_describe(const unires_plan *pl, float rho, float lam, const float *b, float *x, int max_iter,
                           double tol, int stop_mode, int precond_mode) {
  CgSolve s;
  s.b = b, s.x = x, s.rho = rho, s.lam = lam, s.max_iter = max_iter, s.stop = stop_mode, s.pre = precond_mode;
  s.tol = tol;
  s.M = precond_mode == UNIRES_PRECOND_JACOBI ? pl->precM : nullptr;
  s.fft = precond_mode == UNIRES_PRECOND_FFT;
  return s;
}

static CgRun cg_make_run(unires_plan *pl, CgSolve s, hipStream_t st) {
  CgRun R;
  R.pl = pl, R.s = s, R.st = st;
  R.s.chunk = cg_switches().chunk_size();
  R.use_graph = cg_switches().graphs && !s.fft && !pl->timing;
  return R;
}

static int cg_read_back(unires_plan *pl, int max_iter, double tol, int32_t *iters_out, double *obj_trace,
                        hipStream_t st) {
  CgState *S = pl->state;
  int it = 0;
  HIP_TRY(hipMemcpyAsync(&it, &S->iters, sizeof(int), hipMemcpyDeviceToHost, st));
  if (obj_trace && tol != 0.0)
    HIP_TRY(hipMemcpyAsync(obj_trace, S->obj, sizeof(double) * (size_t)(std::min(max_iter, kMaxCgIter) + 1),
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *iters_out = it;
  return UNIRES_OK;
}

// One solve enqueued whole on `st`.  hipGraph replay (UNIRES_CG_GRAPH=0 disables): the ~8 launches per iteration of a
// solve are captured once and re-launched as one graph while the arguments stay the same.  In order: replay the plan's
// captured solve if it serves this one; else drop it, capture this one, and launch that; capture refused, or the solve
// not one to capture: plain launches.  `how`: what the enqueue did - now, or when the graph was captured.
static int cg_solve_whole(unires_plan *pl, const CgSolve &s, hipStream_t st, CgHow &how) {
  ++pl->cg_gen;  // (k_sc_init counts every solve)
  const bool graphable = cg_switches().graphs && !s.fft && s.max_iter > 0 && !pl->timing;  // (events go with plain launches)
  CgCaptured &G = pl->cg_whole;
  const bool replay = graphable && G.matches(s);
  int rc = -1;
  if (graphable && !replay) {
    if (G.exec) drop_cg_graph(pl);
    rc = capture_graph(st, &G.exec, [&] { return cg_enqueue(pl, s, st, how); });
    if (rc == 0) G.key = s, G.how = how;
  }
  if (replay || rc == 0) {
    how = G.how;
    rc = hipGraphLaunch(G.exec, st) == hipSuccess ? UNIRES_OK : fail(UNIRES_ERR_HIP, "hipGraphLaunch failed");
  } else if (rc < 0) {
    rc = cg_enqueue(pl, s, st, how);
  }
  if (rc) cg_resync_gen(pl);
  return rc;
}

// --------------------------------------------------------------------------
// The two-lane schedule of several channels' fixed-iteration solves.  The operator of an iteration is bound by
// instruction issue and LDS, the scalar and vector kernels after it by the fabric; on free-running streams the
// channels mostly queue behind each other.  Here all of them are enqueued as ONE schedule on two streams:
//   lane M: start(0) .. start(n-1), then matvec(c, k) for k = 1 .. N, c = 0 .. n-1 (c fastest);
//   lane V: in the same (k, c) order, the rest of iteration k of channel c;
//   matvec(c, k) waits for V(c, k-1) (for start(c) when k = 1: same lane), V(c, k) waits for matvec(c, k)
// - channel c's vector phase runs under channel c+1's operator every time.  Per channel the kernels, their arguments
// and their order are those of cg_enqueue, so x is the same bits as that plan's solve alone with the same grids.
// The schedule is captured once, by fork / join capture across the two lanes, into one hipGraphExec_t with two
// parallel branches, kept here and keyed by every channel's CgSolve and the plans' epochs (drop_cg_graph moves a
// plan's epoch: whatever invalidates a plan's own captured solve invalidates this one).
// --------------------------------------------------------------------------
namespace {
struct Lockstep {
  std::vector<unires_plan *> plans;
  CgCaptured graph;            // the one executable graph all channels share (no key of its own)
  std::vector<CgCaptured> ch;  // per channel: the solve it was captured for and what a replay reports (no graph)
  std::vector<unsigned long long> epochs;
  std::vector<hipEvent_t> joins;  // one per channel stream, and the graph's end
};
std::vector<Lockstep> g_lockstep;
std::mutex g_lockstep_mutex;
constexpr size_t kMaxLockstep = 4;  // sets of plans with a captured schedule (a reconstruction has one)

void lockstep_destroy(Lockstep &L, bool wait) {
  if (wait)
    for (unires_plan *pl : L.plans) await_use(pl);  // (a launch of the graph may still be in flight)
  L.graph.destroy();
  for (hipEvent_t e : L.joins) (void)hipEventDestroy(e);
  L.ch.clear(), L.joins.clear();
}
}  // namespace

// unires_plan_destroy: the schedules the plan is part of go with it
void unires::cg_lockstep_forget(unires_plan *pl) {
  std::lock_guard<std::mutex> lock(g_lockstep_mutex);
  for (size_t i = g_lockstep.size(); i-- > 0;)
    if (std::find(g_lockstep[i].plans.begin(), g_lockstep[i].plans.end(), pl) != g_lockstep[i].plans.end()) {
      lockstep_destroy(g_lockstep[i], false);
      g_lockstep.erase(g_lockstep.begin() + (long)i);
    }
}

// The whole schedule on lanes lm (operators) and lv (everything else); called under capture of lm.  `ev`: fresh
// events, one per edge.  how[c]: what channel c's start and iterations did.
static int cg_lockstep_enqueue(int n, unires_plan *const *plans, const std::vector<CgSolve> &s, hipStream_t lm,
                               hipStream_t lv, const std::vector<hipEvent_t> &ev, std::vector<CgHow> &how) {
  size_t ne = 0;
  auto edge = [&](hipStream_t from, hipStream_t to) -> int {
    hipEvent_t e = ev[ne++];
    HIP_TRY(hipEventRecord(e, from));
    HIP_TRY(hipStreamWaitEvent(to, e, 0));
    return UNIRES_OK;
  };
  int rc = edge(lm, lv);  // fork: lane V joins the capture
  std::vector<CgIters> it((size_t)n);
  for (int c = 0; c < n && !rc; ++c) {
    rc = cg_enqueue_start(plans[c], s[c], nullptr, lm, how[c]);
    if (!rc) rc = cg_iters_begin(plans[c], s[c], 1, s[c].max_iter, false, nullptr, it[c], how[c]);
  }
  const int N = s[0].max_iter;
  std::vector<hipEvent_t> vdone((size_t)n, nullptr);
  for (int k = 1; k <= N && !rc; ++k)
    for (int c = 0; c < n && !rc; ++c) {
      if (vdone[c]) HIP_TRY(hipStreamWaitEvent(lm, vdone[c], 0));  // matvec(c, k) after V(c, k - 1)
      const int g = cg_iter_operator(plans[c], s[c], it[c], k, lm);
      if ((rc = edge(lm, lv))) break;  // V(c, k) after matvec(c, k)
      if ((rc = cg_iter_rest(plans[c], s[c], it[c], k, g, lv))) break;
      if (k < N) {
        vdone[c] = ev[ne++];
        HIP_TRY(hipEventRecord(vdone[c], lv));
      }
    }
  if (!rc) rc = edge(lv, lm);  // join
  return rc;
}

// Takes the channels' solves if they are in the schedule's scope and it could be captured (or was): returns 0 with
// *taken set, or an error.  *taken false: nothing was enqueued, the caller goes on as before.
static int cg_lockstep_solve(int n, unires_plan *const *plans, const float *rho, const float *lam,
                             const float *const *b, float *const *x, int max_iter, double tol, int stop_mode,
                             int precond_mode, void *const *streams, bool *taken) {
  *taken = false;
  if (!cg_switches().lockstep || !cg_switches().graphs || n < 2 || tol != 0.0 || max_iter < 1 ||
      precond_mode == UNIRES_PRECOND_FFT)
    return UNIRES_OK;
  hipStream_t lm = (hipStream_t)streams[0], lv = nullptr;
  for (int c = 1; c < n && !lv; ++c)
    if (streams[c] != streams[0]) lv = (hipStream_t)streams[c];
  if (!lm || !lv) return UNIRES_OK;  // (two lanes need two of the caller's streams)
  for (int c = 0; c < n; ++c)
    if (plans[c]->timing || stream_capturing((hipStream_t)streams[c])) return UNIRES_OK;

  std::vector<CgSolve> s;
  for (int c = 0; c < n; ++c) {
    s.push_back(cg_describe(plans[c], rho[c], lam[c], b[c], x[c], max_iter, tol, stop_mode, precond_mode));
    s[c].ring = cg_ring_prepare(plans[c], (hipStream_t)streams[c]);  // (before capture: it may allocate)
  }
  std::lock_guard<std::mutex> lock(g_lockstep_mutex);
  Lockstep *L = nullptr;
  for (Lockstep &e : g_lockstep)
    if (e.plans == std::vector<unires_plan *>(plans, plans + n)) L = &e;
  bool fresh = !L || !L->graph.exec;
  for (int c = 0; L && !fresh && c < n; ++c)
    fresh = !L->ch[c].matches(s[c]) || L->epochs[c] != plans[c]->cg_epoch;
  if (fresh) {
    if (L) {
      lockstep_destroy(*L, true);
    } else {
      if (g_lockstep.size() >= kMaxLockstep) {
        lockstep_destroy(g_lockstep.front(), true);
        g_lockstep.erase(g_lockstep.begin());
      }
      g_lockstep.emplace_back();
      L = &g_lockstep.back();
      L->plans.assign(plans, plans + n);
    }
    std::vector<hipEvent_t> ev((size_t)(2 + 2 * n * max_iter), nullptr);
    bool ok = true;
    for (hipEvent_t &e : ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    L->joins.assign((size_t)n + 1, nullptr);
    for (hipEvent_t &e : L->joins) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    std::vector<CgHow> how((size_t)n);
    int rc = -1;
    if (ok) {
      for (int c = 0; c < n; ++c) plans[c]->lockstep = true;  // (the operators' grids are this mode's: cap_s2_ls)
      rc = capture_graph(lm, &L->graph.exec, [&] { return cg_lockstep_enqueue(n, plans, s, lm, lv, ev, how); });
      for (int c = 0; c < n; ++c) plans[c]->lockstep = false;
    }
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    (void)hipGetLastError();
    if (rc != 0) {  // refused (rc < 0: the caller's path serves the solves) or failed
      lockstep_destroy(*L, false);
      g_lockstep.erase(g_lockstep.begin() + (L - g_lockstep.data()));
      if (rc > 0)
        for (int c = 0; c < n; ++c) cg_resync_gen(plans[c]);
      return rc > 0 ? rc : UNIRES_OK;
    }
    L->ch.assign((size_t)n, CgCaptured()), L->epochs.clear();
    for (int c = 0; c < n; ++c) {
      L->ch[c].key = s[c], L->ch[c].how = how[c], L->ch[c].how.lockstep = 1;
      L->epochs.push_back(plans[c]->cg_epoch);
    }
  }
  // the right-hand sides were enqueued on the channels' streams: the launch stream waits for every one of them, and
  // every one of them for the graph's end (the caller joins its streams as it did)
  for (int c = 0; c < n; ++c)
    if ((hipStream_t)streams[c] != lm) {
      HIP_TRY(hipEventRecord(L->joins[c], (hipStream_t)streams[c]));
      HIP_TRY(hipStreamWaitEvent(lm, L->joins[c], 0));
    }
  for (int c = 0; c < n; ++c) ++plans[c]->cg_gen;  // (k_sc_init counts every solve)
  if (hipGraphLaunch(L->graph.exec, lm) != hipSuccess) {
    for (int c = 0; c < n; ++c) cg_resync_gen(plans[c]);
    return fail(UNIRES_ERR_HIP, "hipGraphLaunch failed");
  }
  HIP_TRY(hipEventRecord(L->joins[n], lm));
  for (int c = 0; c < n; ++c) {
    if ((hipStream_t)streams[c] != lm) HIP_TRY(hipStreamWaitEvent((hipStream_t)streams[c], L->joins[n], 0));
    plans[c]->last = L->ch[c].how;
    mark_use(plans[c], (hipStream_t)streams[c]);
  }
  *taken = true;
  CHECK_LAUNCH();
  return UNIRES_OK;
}

// One or several solves, each on its own plan and stream (unires/_update.py:122-150 loops over the channels; they do
// not couple inside the y-update).  Solves that can stop early are enqueued in chunks, the chunks of all of them fed from
// one host loop, so that the channels still overlap on the device where they run on separate streams; the others whole,
// one after the other, or - fixed-iteration solves of several channels, where switched on - as one two-lane schedule.
static int cg_solve_n(int n, unires_plan *const *plans, const float *rho, const float *lam, const float *const *b,
                      float *const *x, int max_iter, double tol, int stop_mode, int precond_mode, int32_t *iters_out,
                      double *obj_trace, void *const *streams) {
  for (int c = 0; c < n; ++c) {
    const int rc = cg_check_args(plans[c], rho[c], lam[c], b[c], x[c], max_iter, tol, stop_mode, precond_mode);
    if (rc) return rc;
    for (int d = 0; d < c; ++d)
      if (plans[d] == plans[c]) return fail(UNIRES_ERR_ARG, "one plan per solve");
  }
  auto stream = [&](int c) { return (hipStream_t)streams[c]; };
  bool capturing = false;
  for (int c = 0; c < n; ++c) capturing = capturing || stream_capturing(stream(c));
  // (a stream under capture - e.g. the caller's torch.cuda.graph - runs nothing until the graph is launched: the
  // chunk feeder would wait for progress that never comes.  The whole solve then joins the capture, as in r3;
  // kernels after convergence return at entry.)
  if (capturing && tol != 0.0 && max_iter > kMaxCgIter)
    return fail(UNIRES_ERR_ARG, "a solve with a tolerance and more than 4096 iterations cannot join a stream capture "
                                "(it is fed to the device chunk by chunk, following its progress)");
  // (before anything is enqueued: a failed start or drive below is remembered too)
  for (int c = 0; c < n; ++c) mark_use(plans[c], stream(c));
  auto describe = [&](int c) {
    return cg_describe(plans[c], rho[c], lam[c], b[c], x[c], max_iter, tol, stop_mode, precond_mode);
  };
  bool lockstep = false;
  if (!capturing) {
    const int rc = cg_lockstep_solve(n, plans, rho, lam, b, x, max_iter, tol, stop_mode, precond_mode, streams, &lockstep);
    if (rc) return rc;
  }
  if (lockstep) {
    // (enqueued as one schedule across the channels' streams)
  } else if (cg_chunked(tol, max_iter) && !(capturing && max_iter <= kMaxCgIter)) {
    std::vector<CgRun> runs;
    for (int c = 0; c < n; ++c) runs.push_back(cg_make_run(plans[c], describe(c), stream(c)));
    for (CgRun &R : runs) {
      const int rc = cg_run_start(R);
      if (rc) return rc;
    }
    const int rc = cg_runs_drive(runs);
    if (rc) return rc;
    for (int c = 0; c < n; ++c) plans[c]->last = runs[c].how, mark_use(plans[c], stream(c));
    CHECK_LAUNCH();
  } else {  // nothing to steer: each solve is enqueued whole
    for (int c = 0; c < n; ++c) {
      CgSolve s = describe(c);
      // deferred iterate update: only where nothing reads x before the solve ends
      s.ring = tol == 0.0 && !s.fft && max_iter > 0 ? cg_ring_prepare(plans[c], stream(c)) : 1;
      CgHow how;
      const int rc = cg_solve_whole(plans[c], s, stream(c), how);
      if (rc) return rc;
      plans[c]->last = how;
      mark_use(plans[c], stream(c));
      CHECK_LAUNCH();
    }
  }
  if (iters_out)
    for (int c = 0; c < n; ++c) {
      const int rc = cg_read_back(plans[c], max_iter, tol, iters_out + c,
                                  obj_trace ? obj_trace + (size_t)c * (std::min(max_iter, kMaxCgIter) + 1) : nullptr,
                                  stream(c));
      if (rc) return rc;
    }
  return UNIRES_OK;
}

extern "C" int unires_cg_solve(unires_plan_t *plan, float rho, float lam, const float *b, float *x,
                               int32_t max_iter, double tol, int32_t stop_mode,
                               int32_t precond_mode, int32_t *iters_out, double *obj_trace,
                               void *stream) {
  return cg_solve_n(1, &plan, &rho, &lam, &b, &x, max_iter, tol, stop_mode, precond_mode, iters_out, obj_trace, &stream);
}

extern "C" int unires_cg_solve_many(int32_t n, unires_plan_t *const *plans, const float *rho, const float *lam,
                                    const float *const *b, float *const *x, int32_t max_iter, double tol,
                                    int32_t stop_mode, int32_t precond_mode, int32_t *iters_out,
                                    double *obj_trace, void *const *streams) {
  if (n < 1 || !plans || !rho || !lam || !b || !x || !streams) return fail(UNIRES_ERR_NULL, "null argument");
  return cg_solve_n(n, plans, rho, lam, b, x, max_iter, tol, stop_mode, precond_mode, iters_out, obj_trace, streams);
}
