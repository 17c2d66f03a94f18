// api_plan.hip - the plan object of the C ABI (include/unires_hip.h): the description of each repeat's operator
// (fill_repeat: canonical layout, trimmed taps, which family of kernels), the device tables built for it (splat
// schedule, conv_up tables, window-pull plan, shift factors, single-pass schedule), and the plan's life cycle.
#include <stdio.h>
#include <time.h>

#include <atomic>
#include <new>

#include "api_internal.hpp"

using namespace unires;

// --------------------------------------------------------------------------
// who still uses the plan: streams to wait for, captured solves to drop
// --------------------------------------------------------------------------
static void drop_timing(unires_plan *pl) {
  for (auto &e : pl->tev) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
  pl->tev.clear();
}

bool unires::stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return cs != hipStreamCaptureStatusNone;
}

// note / await the plan's last use (see unires_plan::last_use).  Noting is free - the stream is remembered, no
// event is recorded per call (an event per entry point kept a second host thread busy: host_share 1.04 -> 2.0 in
// tools/host_time.py); the event is recorded on the remembered streams when somebody has to wait, and waited for
// between sleeps (hipEventSynchronize polls flat out unless the process set hipDeviceScheduleBlockingSync before
// its context existed, tools/wait_probe.py).
void unires::mark_use(unires_plan *pl, hipStream_t st) {
  if (stream_capturing(st)) {
    pl->captured_use = true;
    return;
  }
  for (hipStream_t s : pl->use_streams)
    if (s == st) return;
  if (pl->use_streams.size() >= 8)
    pl->captured_use = true;  // (more streams than anybody uses: fall back to the device-wide wait)
  else
    pl->use_streams.push_back(st);
}
void unires::await_use(unires_plan *pl) {
  static const bool device_wide = getenv("UNIRES_SET_REPEAT_DEVICE_SYNC") != nullptr;  // (measurement: the r4 behaviour)
  if (pl->captured_use || device_wide) {
    // (sticky: a graph the caller captured may be replayed at any time without an entry point being called - a plan
    // that was ever used under capture is waited for device-wide from then on)
    (void)hipDeviceSynchronize();
    pl->use_streams.clear();
    return;
  }
  if (pl->use_streams.empty()) return;
  if (!pl->last_use && hipEventCreateWithFlags(&pl->last_use, hipEventDisableTiming) != hipSuccess) {
    pl->last_use = nullptr;
    (void)hipDeviceSynchronize();
    pl->use_streams.clear();
    return;
  }
  for (hipStream_t s : pl->use_streams) {
    if (hipEventRecord(pl->last_use, s) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipDeviceSynchronize();
      break;
    }
    unsigned spins = 0;
    for (;;) {
      const hipError_t q = hipEventQuery(pl->last_use);
      if (q != hipErrorNotReady) break;
      if (++spins > 4096) {  // (the usual wait is a kernel or two: spin that long, then sleep)
        const struct timespec nap = {0, 50000};
        (void)nanosleep(&nap, nullptr);
      }
    }
    (void)hipGetLastError();
  }
  pl->use_streams.clear();
}

void unires::drop_cg_chunk_graphs(unires_plan *pl) {
  if (!pl->cg_chunks.exec && !pl->cg_chunks.chunk) return;
  await_use(pl);
  pl->cg_chunks.destroy();
}

unsigned long long unires::next_cg_epoch() {
  static std::atomic<unsigned long long> epoch{0};
  return ++epoch;
}

// Drop the captured CG solves.  A launch of one may still be in flight (the ADMM loop never syncs):
// wait for the plan's last use before destroying the executable graph.
void unires::drop_cg_graph(unires_plan *pl) {
  pl->cg_epoch = next_cg_epoch();  // (the channels' joint schedule, kept in api_cg.hip, is stale from here on)
  drop_cg_chunk_graphs(pl);
  if (!pl->cg_whole.exec) return;
  await_use(pl);
  pl->cg_whole.destroy();
}

// --------------------------------------------------------------------------
// the description of a repeat's operator
// --------------------------------------------------------------------------
// Relabel the observation's voxel axes so that grid axis d runs mainly along +d of the output
// (orient.hpp).  With u[perm[j]] = flip[j] ? n[perm[j]] - 1 - u'[j] : u'[j] on the grid and on x-space
// alike: columns of A permuted and negated, the translation moved to the far end of a reversed axis
// (composed in double from the float32 entries the reference's grid is made of, rounded once); dims,
// strides and taps permuted; the taps of a reversed axis reversed - x[k] = sum_t ker[t] g[r k + t] with
// n_g = (n_x - 1) r + K reads x'[k'] = sum_t ker[K - 1 - t] g'[r k' + t] - and the even / odd slice
// factors swapped where reversal changes the parity of a slice index (n_x even).
static void canonicalise(RepeatDesc &R) {
  static const bool off = getenv("UNIRES_NO_CANON") != nullptr;  // (measurement: the r3 behaviour)
  R.orient = off ? Orient() : orient_of(R.A);
  R.oriented = !R.orient.identity();
  if (!R.oriented) return;
  const Orient &O = R.orient;
  const int nx[3] = {R.dim_x.x, R.dim_x.y, R.dim_x.z}, ng[3] = {R.dim_g.x, R.dim_g.y, R.dim_g.z};
  const Affine A = R.A;
  const Taps T = R.T;
  int cx[3], cg[3];
  double t[3] = {A.m[3], A.m[7], A.m[11]};
  for (int j = 0; j < 3; ++j) {
    const int a = O.perm[j];
    cx[j] = nx[a], cg[j] = ng[a];
    for (int r = 0; r < 3; ++r) {
      R.A.m[4 * r + j] = O.flip[j] ? -A.m[4 * r + a] : A.m[4 * r + a];
      if (O.flip[j]) t[r] += (double)(ng[a] - 1) * (double)A.m[4 * r + a];
    }
    R.T.n[j] = T.n[a], R.T.s[j] = T.s[a];
    for (int i = 0; i < UNIRES_MAX_TAPS; ++i)
      R.T.t[j][i] = i < T.n[a] ? (O.flip[j] ? T.t[a][T.n[a] - 1 - i] : T.t[a][i]) : 0.f;
  }
  for (int r = 0; r < 3; ++r) R.A.m[4 * r + 3] = (float)t[r];
  R.dim_x = Dim3i{cx[0], cx[1], cx[2]};
  R.dim_g = Dim3i{cg[0], cg[1], cg[2]};
  if (R.dim_thick >= 0 && R.dim_thick <= 2) {
    int jt = 0;
    for (int j = 0; j < 3; ++j)
      if (O.perm[j] == R.dim_thick) jt = j;
    if (O.flip[jt] && (nx[R.dim_thick] & 1) == 0) R.scl = -R.scl;
    R.dim_thick = jt;
  }
}

// Drop leading/trailing zero taps (nitorch's rect profile carries one on each
// side): the skipped grid voxels contribute exactly 0, so A is unchanged; the
// grid shrinks and its affine is shifted by the number of leading taps dropped.
static void trim_taps(const Taps &T, const Affine &A, const Dim3i &gd, Taps &Tt, Affine &At,
                      Dim3i &gdt) {
  Tt = T;
  At = A;
  int g[3] = {gd.x, gd.y, gd.z};
  for (int d = 0; d < 3; ++d) {
    // (r6) ... and end taps below two ulps of the accumulated value, |t| < 2^-22 sum |t|: the +-5 taps of the default
    // Gaussian profile at ratio 2 (2.1e-7 of the sum each; the +-4 ones, 4.3e-5, stay) - 11 taps become 9: the operator
    // changes by <= 4.2e-7 relative, 250 x below the 1e-4 parity bar and below the disagreement of the three recollections
    // of nitorch's truncation of that Gaussian (11 / 9 / 7 taps).  UNIRES_TRIM_TINY=0 keeps every non-zero tap.
    static const bool tiny_on = !(getenv("UNIRES_TRIM_TINY") && atoi(getenv("UNIRES_TRIM_TINY")) == 0);
    double sum = 0.0;
    for (int i = 0; i < T.n[d]; ++i) sum += fabs((double)T.t[d][i]);
    const double eps = tiny_on ? sum * 2.384185791015625e-7 : 1e-300;
    int lead = 0, trail = 0;
    while (lead < T.n[d] - 1 && fabs((double)T.t[d][lead]) < eps) ++lead;
    while (trail < T.n[d] - 1 - lead && fabs((double)T.t[d][T.n[d] - 1 - trail]) < eps) ++trail;
    Tt.n[d] = T.n[d] - lead - trail;
    for (int i = 0; i < UNIRES_MAX_TAPS; ++i) Tt.t[d][i] = i < Tt.n[d] ? T.t[d][lead + i] : 0.f;
    g[d] -= lead + trail;
    for (int r = 0; r < 3; ++r)
      At.m[4 * r + 3] = (float)((double)At.m[4 * r + 3] + (double)lead * (double)A.m[4 * r + d]);
  }
  gdt = Dim3i{g[0], g[1], g[2]};
}

// Which family of kernels the trimmed taps select: separable passes, the hybrid forms.  A masked repeat
// (unires_plan_set_missing) takes no hybrid form - what UNIRES_NO_HYBRID selects: its A^T A multiplies a materialised
// x-space intermediate, which the forms that run conv_down and conv_up as one kernel never have.
static void choose_family(const unires_plan *pl, RepeatDesc &out, bool masked) {
  // many taps (e.g. a Gaussian in-plane profile on top of the slice profile): the fused kernels'
  // direct 3-D sum (prod n_d taps per output, fan-in^3 gathers per grid voxel) loses to one
  // 1-D pass per axis through grid-space scratch
  out.sep = (long long)out.Tf.n[0] * out.Tf.n[1] * out.Tf.n[2] > 64;
  for (int d = 0; d < 3; ++d)
    if (fan_in(out.Tf, d) > 2) out.sep = true;
  out.sep0 = out.sep;
  out.hyb = out.hybf = false;
  if (pl->regime == UNIRES_REGIME_SUPERRES) {
    static const bool env_no_hyb = getenv("UNIRES_NO_HYBRID") != nullptr;
    const bool no_hyb = env_no_hyb || masked;
    const bool xy = !is_dirac(out.Tf, 0) || !is_dirac(out.Tf, 1);
    const bool z_ok = fan_in(out.Tf, 2) <= 2 && out.dim_x.z >= 2;
    int nconv = 0;
    for (int d = 0; d < 3; ++d) nconv += !is_dirac(out.Tf, d);
    const bool both = !no_hyb && xy && nconv > 1 && z_ok;
    const bool fwd_only = !no_hyb && !both && out.sep && xy && !is_dirac(out.Tf, 2) && out.dim_x.z >= 2;
    if (both || fwd_only) {
      out.hyb = both, out.hybf = fwd_only;
      if (both) out.sep = false;
      out.Tz = out.Tf, out.Txy = out.Tf;
      set_dirac(out.Tz, 0), set_dirac(out.Tz, 1);
      set_dirac(out.Txy, 2);
      out.dim_h = Dim3i{out.dim_gf.x, out.dim_gf.y, out.dim_x.z};
    }
  }
}

static int fill_repeat(const unires_plan *pl, const unires_repeat_t *in, RepeatDesc &out, bool masked = false) {
  if (!in) return fail(UNIRES_ERR_NULL, "null repeat descriptor");
  if (!(in->tau > 0.f)) return fail(UNIRES_ERR_ARG, "tau must be positive");
  out = RepeatDesc();
  out.tau = in->tau;
  out.scl = in->scl;
  out.dim_thick = in->dim_thick;
  if (pl->regime == UNIRES_REGIME_IDENTITY) {
    out.dim_x = out.dim_xu = pl->dy;
    out.dim_g = pl->dy;
    return UNIRES_OK;
  }
  if (!dims_ok(in->dim_x) || !dims_ok(in->dim_g)) return fail(UNIRES_ERR_DIM, "bad repeat dims");
  out.dim_x = mk(in->dim_x);
  out.dim_g = mk(in->dim_g);
  memcpy(out.A.m, in->M, sizeof(out.A.m));
  for (int i = 0; i < 12; ++i)
    if (!isfinite(out.A.m[i])) return fail(UNIRES_ERR_ARG, "non-finite affine");
  if (pl->regime == UNIRES_REGIME_SUPERRES) {
    int rc = make_taps(in->taps, in->ntaps, in->ratio, out.T);
    if (rc) return rc;
    if ((rc = check_conv_dims(out.dim_g, out.dim_x, out.T))) return rc;
    if (out.scl != 0.f && (out.dim_thick < 0 || out.dim_thick > 2))
      return fail(UNIRES_ERR_ARG, "bad dim_thick");
  } else {
    if (out.dim_g.x != out.dim_x.x || out.dim_g.y != out.dim_x.y || out.dim_g.z != out.dim_x.z)
      return fail(UNIRES_ERR_DIM, "denoising regime needs dim_g == dim_x");
    for (int d = 0; d < 3; ++d) set_dirac(out.T, d);
  }
  out.dim_xu = out.dim_x;
  canonicalise(out);
  trim_taps(out.T, out.A, out.dim_g, out.Tf, out.Af, out.dim_gf);
  choose_family(pl, out, masked);
  if (!invert_affine(out.Af, out.Afinv)) return fail(UNIRES_ERR_ARG, "singular affine");
  splat_safety(out.Af, out.safe.row_sep, out.safe.use_atomics);
  return UNIRES_OK;
}

// --------------------------------------------------------------------------
// the device tables of a repeat
// --------------------------------------------------------------------------
// (re)build the splat schedule of a repeat for its current operator; a non-applicable operator
// simply leaves the schedule invalid (the general push kernels then run)
// tables_only: the operator's geometry is unchanged (a new slice scaling only): the conv_up tables are rewritten,
// the schedule itself - which does not see the scaling - stays
static int build_sched(unires_plan *pl, Repeat &R, bool tables_only = false) {
  const bool was_valid = R.sched.valid;
  R.sched.valid = false;
  if (pl->regime == UNIRES_REGIME_IDENTITY) return UNIRES_OK;
  int axis = -1;
  int rows_y = R.dim_gf.y;
  R.src_stride = (unsigned)R.dim_gf.z;
  R.ctab_step = 1;
  const bool direct = pl->regime == UNIRES_REGIME_DENOISE || R.sep;
  if (!direct) {
    int nconv = 0;
    for (int d = 0; d < 3; ++d) {
      if (is_dirac(R.Tf, d)) continue;
      ++nconv;
      axis = d;
    }
    const int xdv[3] = {R.dim_x.x, R.dim_x.y, R.dim_x.z}, gdv[3] = {R.dim_gf.x, R.dim_gf.y, R.dim_gf.z};
    if (R.dim_x.numel() >= (1ull << 30)) return UNIRES_OK;
    if (R.hyb) {
      axis = 2;
    } else if (nconv > 1) {
      // conv_up along several axes (isotropic down-sampling, BASELINE config 4): x / y parts per
      // segment in the schedule, z part per lane
      for (int d = 0; d < 3; ++d)
        if (fan_in(R.Tf, d) > 2 || xdv[d] < 2) return UNIRES_OK;
      if (R.scl != 0.f && R.dim_thick != 2) return UNIRES_OK;
      axis = 3;
    } else {
      if (axis < 0) axis = 2;  // all dirac: conv_up is the identity, any axis works
      if (fan_in(R.Tf, axis) > 2 || xdv[axis] < 2) return UNIRES_OK;
      if (R.scl != 0.f && R.dim_thick != axis && !R.hyb) return UNIRES_OK;  // (hybrid: x / y scaling rides with the 1-D passes)
    }
    const unsigned xyz = (unsigned)R.dim_x.y * (unsigned)R.dim_x.z, xz = (unsigned)R.dim_x.z;
    const int taxis = axis == 3 ? 2 : axis;  // axis of the run-time (per-lane) table
    if (axis == 2) rows_y = R.hyb ? R.dim_h.y : R.dim_x.y, R.src_stride = xz, R.ctab_step = 1;
    if (axis == 1) R.src_stride = xyz, R.ctab_step = xz;  // source offset ui * xyz + koff(uj) * xz + k
    if (axis == 0) R.src_stride = xz, R.ctab_step = xyz;  // source offset uj * xz + koff(ui) * xyz + k
    if (axis == 3) R.src_stride = xz, R.ctab_step = xyz;  // (x-space row / slab strides)
    const int gn = gdv[taxis];
    if (gn + 128 > 1400) return UNIRES_OK;  // LDS copy of the table
    std::vector<float> host((size_t)gn * 4);
    for (int v = 0; v < 2; ++v) {
      if (!R.ctab_dev[v] || R.ctab_cap < gn) {
        if (R.ctab_dev[v]) (void)hipFree(R.ctab_dev[v]);
        R.ctab_dev[v] = nullptr;
        if (hipMalloc((void **)&R.ctab_dev[v], host.size() * sizeof(float)) != hipSuccess)
          return fail(UNIRES_ERR_ALLOC, "hipMalloc conv table");
      }
      splat2_convtab(R.Tf, v ? make_scaling(R.scl, R.dim_thick) : kNoScaling, taxis, gn, xdv[taxis], host.data());
      if (hipMemcpy(R.ctab_dev[v], host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) !=
          hipSuccess)
        return fail(UNIRES_ERR_HIP, "hipMemcpy conv table");
    }
    R.ctab_n = gn;
    R.ctab_cap = std::max(R.ctab_cap, gn);
    if (axis == 3) {
      for (int d = 0; d < 2; ++d) {
        std::vector<float> hx((size_t)gdv[d] * 4);
        if (!R.xytab_dev[d] || R.xytab_cap[d] < gdv[d]) {
          if (R.xytab_dev[d]) (void)hipFree(R.xytab_dev[d]);
          R.xytab_dev[d] = nullptr;
          if (hipMalloc((void **)&R.xytab_dev[d], hx.size() * sizeof(float)) != hipSuccess)
            return fail(UNIRES_ERR_ALLOC, "hipMalloc conv table");
          R.xytab_cap[d] = gdv[d];
        }
        splat2_convtab(R.Tf, kNoScaling, d, gdv[d], xdv[d], hx.data());
        if (hipMemcpy(R.xytab_dev[d], hx.data(), hx.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
          return fail(UNIRES_ERR_HIP, "hipMemcpy conv table");
      }
    }
  }
  if (tables_only) {
    R.sched.valid = was_valid;
    return UNIRES_OK;
  }
  (void)splat2_build(R.sched, R.Af, R.Afinv, R.dim_gf, pl->dy, pl->fov_tol, R.safe, axis, rows_y,
                     (const float4 *)R.xytab_dev[0], (const float4 *)R.xytab_dev[1], R.dim_x);
  (void)hipGetLastError();
  return UNIRES_OK;
}

// translation-only operator (and a single repeat: the kernel is the whole matvec); carries the slice scaling
static void build_shift(unires_plan *pl, Repeat &R) {
  R.shift.valid = false;
  if (pl->reps.size() == 1 && pl->regime != UNIRES_REGIME_IDENTITY)
    (void)shift_build(R.shift, pl->dy, R.dim_gf, R.dim_x, R.Tf, make_scaling(2.f * R.scl, R.dim_thick), R.Af,
                      pl->fov_tol);
  (void)hipGetLastError();
}

// the pull of the same operator through the LDS-window kernel (denoising: plain pull onto the
// grid; super-resolution: + conv_down); outside its domain the plan stays invalid
static void build_pull(unires_plan *pl, Repeat &R) {
  R.pplan.valid = false;
  if (pl->regime == UNIRES_REGIME_DENOISE)
    (void)pull2_build(R.pplan, pl->dy, R.A, R.T, R.dim_g, R.dim_g, pl->fov_tol);
  else if (pl->regime == UNIRES_REGIME_SUPERRES && (R.hyb || R.hybf))
    (void)pull2_build(R.pplan, pl->dy, R.Af, R.Tz, R.dim_h, R.dim_gf, pl->fov_tol);
  else if (pl->regime == UNIRES_REGIME_SUPERRES && !R.sep)
    (void)pull2_build(R.pplan, pl->dy, R.Af, R.Tf, R.dim_x, R.dim_gf, pl->fov_tol);
  build_shift(pl, R);
}

// schedule + window plan of one repeat.  A hybrid operator (z profile inside the pull / splat kernels,
// x / y profiles as 1-D passes) whose kernels turn out to be unavailable - window plan outside
// pull2's domain, or no axis-2 schedule (atomics needed, table too long for LDS, a tile overflowing
// the segment lists) - is rebuilt as what the taps alone would have chosen: the separable passes for
// a many-tap profile (with the forward half of the hybrid where its window plan exists), not the dense
// 3-D conv kernels the general fall-through ends in.
static int build_repeat_kernels(unires_plan *pl, Repeat &R) {
  int rc = build_sched(pl, R);
  if (rc) return rc;
  build_pull(pl, R);
  R.f1.valid = false;
  if (pl->regime == UNIRES_REGIME_DENOISE) {  // pull and push in one pass where the operator allows it
    (void)ata1_build(R.f1, R.Af, R.Afinv, R.dim_gf, pl->dy, pl->fov_tol, R.safe);
    (void)hipGetLastError();
  }
  if (R.hyb && !(R.pplan.valid && R.sched.valid && R.sched.axis == 2)) {
    R.hyb = false;
    R.sep = R.sep0;
    R.hybf = R.sep0 && R.pplan.valid;  // (the window plan of the forward half is the one just built)
    rc = build_sched(pl, R);
    if (rc) return rc;
    if (!R.hybf) build_pull(pl, R);
  }
  return UNIRES_OK;
}

static void free_tables(RepeatTables &R) {
  splat2_free(R.sched);
  pull2_free(R.pplan);
  shift_free(R.shift);
  ata1_free(R.f1);
  for (int v = 0; v < 2; ++v) {
    if (R.ctab_dev[v]) (void)hipFree(R.ctab_dev[v]), R.ctab_dev[v] = nullptr;
    if (R.xytab_dev[v]) (void)hipFree(R.xytab_dev[v]), R.xytab_dev[v] = nullptr;
    R.xytab_cap[v] = 0;
  }
  R.ctab_n = R.ctab_cap = 0;
}

static void free_mask(RepeatMask &R) {
  if (R.mask_u) (void)hipFree(R.mask_u);
  if (R.mask_c) (void)hipFree(R.mask_c);
  R.mask_u = R.mask_c = nullptr;
  R.mask_cap = 0, R.masked = false;
}

static void free_weights(RepeatWeights &R) {
  if (R.w_dev) (void)hipFree(R.w_dev);
  R.w_dev = nullptr;
  R.w_cap = 0, R.weighted = false;
}

// the observation's length along the caller's axis `axis`: the number of slices a per-slice table has
static int du_of(const Repeat &R, int axis) { return axis == 0 ? R.dim_xu.x : (axis == 1 ? R.dim_xu.y : R.dim_xu.z); }

static void free_gains(RepeatGains &R) {
  if (R.e_dev) (void)hipFree(R.e_dev);  // (one allocation: e, u e^2, u e)
  R.e_dev = R.wm_dev = R.wr_dev = nullptr;
  R.e_cap = 0, R.gained = false;
}

static void free_voxel(RepeatVoxel &R) {
  if (R.g_u) (void)hipFree(R.g_u);
  if (R.g_c) (void)hipFree(R.g_c);
  R.g_u = R.g_c = nullptr;
  R.g_cap = 0, R.voxw = false;
}

// the canonical-layout copy of a voxel-weighted, relabelled repeat's weights, for the orientation the repeat has now
static int canonical_voxel(Repeat &R, hipStream_t st) {
  if (!R.voxw || !R.oriented) return UNIRES_OK;
  if (!R.g_c && hipMalloc((void **)&R.g_c, R.g_cap * sizeof(float)) != hipSuccess) {
    R.g_c = nullptr;
    return fail(UNIRES_ERR_ALLOC, "hipMalloc voxel weights");
  }
  launch_voxel_permute(R.g_u, R.orient, R.dim_xu, R.g_c, st);
  return UNIRES_OK;
}

// the canonical-layout copy of a masked, relabelled repeat's mask, for the orientation the repeat has now
static int canonical_mask(Repeat &R, hipStream_t st) {
  if (!R.masked || !R.oriented) return UNIRES_OK;
  if (!R.mask_c && hipMalloc((void **)&R.mask_c, R.mask_cap) != hipSuccess) {
    R.mask_c = nullptr;
    return fail(UNIRES_ERR_ALLOC, "hipMalloc mask");
  }
  launch_mask_permute(R.mask_u, R.orient, R.dim_xu, R.mask_c, st);
  return UNIRES_OK;
}

// --------------------------------------------------------------------------
// entry points
// --------------------------------------------------------------------------
extern "C" int unires_plan_create(unires_plan_t **plan, const int32_t dim_y[3],
                                  const float vx_y[3], int32_t regime, int32_t n_repeats,
                                  const unires_repeat_t *repeats, float fov_tol) {
  if (!plan || !dim_y) return fail(UNIRES_ERR_NULL, "null argument");
  *plan = nullptr;
  if (!dims_ok(dim_y)) return fail(UNIRES_ERR_DIM, "bad dim_y");
  if (!vx_ok(vx_y)) return fail(UNIRES_ERR_ARG, "voxel size must be positive");
  if (regime < 0 || regime > 2) return fail(UNIRES_ERR_ARG, "Undefined method");
  if (n_repeats < 1 || !repeats) return fail(UNIRES_ERR_ARG, "need at least one repeat");
  unires_plan *pl = new (std::nothrow) unires_plan();
  if (!pl) return fail(UNIRES_ERR_ALLOC, "host allocation failed");
  pl->dy = mk(dim_y);
  pl->cg_epoch = next_cg_epoch();
  memcpy(pl->vx, vx_y, sizeof(pl->vx));
  pl->regime = regime;
  pl->fov_tol = fov_tol;
  pl->reps.resize(n_repeats);
  bool need_sep = false;
  for (int n = 0; n < n_repeats; ++n) {
    if (int rc = fill_repeat(pl, &repeats[n], pl->reps[n])) {
      unires_plan_destroy(pl);
      return rc;
    }
    if (regime != UNIRES_REGIME_IDENTITY) {
      pl->cap_g = std::max(pl->cap_g, pl->reps[n].dim_g.numel());
      pl->cap_x = std::max(pl->cap_x, pl->reps[n].dim_x.numel());
    }
    need_sep = need_sep || (regime == UNIRES_REGIME_SUPERRES && (pl->reps[n].sep || pl->reps[n].hyb));
  }
  const size_t ny = pl->dy.numel();
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    size_t o = off;
    off += align_up(bytes);
    return o;
  };
  const size_t o_r = carve(ny * 4), o_p = carve(ny * 4), o_ap = carve(ny * 4), o_ax = carve(ny * 4);
  const size_t o_g = carve(pl->cap_g * 4), o_x = carve(pl->cap_x * 4), o_xp = carve(pl->cap_x * 4);
  const size_t o_g2 = carve(need_sep ? pl->cap_g * 4 : 0);
  const size_t o_p0 = carve(kMaxPartials * 8), o_p1 = carve(kMaxPartials * 8);
  const size_t o_st = carve(sizeof(CgState));
  pl->ws_bytes = off;
  hipError_t e = hipMalloc((void **)&pl->ws, pl->ws_bytes);
  if (e != hipSuccess) {
    g_err = std::string("hipMalloc workspace: ") + hipGetErrorString(e);
    pl->ws = nullptr;
    unires_plan_destroy(pl);
    return UNIRES_ERR_ALLOC;
  }
  pl->r = (float *)(pl->ws + o_r);
  pl->p = (float *)(pl->ws + o_p);
  pl->ap = (float *)(pl->ws + o_ap);
  pl->ax = (float *)(pl->ws + o_ax);
  pl->gbuf = (float *)(pl->ws + o_g);
  pl->xbuf = (float *)(pl->ws + o_x);
  pl->xperm = (float *)(pl->ws + o_xp);
  pl->gbuf2 = need_sep ? (float *)(pl->ws + o_g2) : nullptr;
  pl->part0 = (double *)(pl->ws + o_p0);
  pl->part1 = (double *)(pl->ws + o_p1);
  pl->state = (CgState *)(pl->ws + o_st);
  e = hipMemset(pl->state, 0, sizeof(CgState));
  if (e != hipSuccess) {
    g_err = std::string("hipMemset: ") + hipGetErrorString(e);
    unires_plan_destroy(pl);
    return UNIRES_ERR_HIP;
  }
  for (Repeat &R : pl->reps)
    if (int rc = build_repeat_kernels(pl, R)) {
      unires_plan_destroy(pl);
      return rc;
    }
  *plan = pl;
  return UNIRES_OK;
}

extern "C" int unires_plan_destroy(unires_plan_t *plan) {
  if (!plan) return UNIRES_OK;
  if (plan->ws) (void)hipFree(plan->ws);
  if (plan->precM) (void)hipFree(plan->precM);
  if (plan->ring) (void)hipFree(plan->ring);
  cg_lockstep_forget(plan);
  plan->cg_whole.destroy(), plan->cg_chunks.destroy();
  if (plan->progress) (void)hipHostFree(plan->progress);
  if (plan->last_use) (void)hipEventDestroy(plan->last_use);
  drop_timing(plan);
  fftpre_destroy(plan->fft);
  for (Repeat &R : plan->reps) free_tables(R), free_mask(R), free_weights(R), free_voxel(R), free_gains(R);
  delete plan;
  return UNIRES_OK;
}

extern "C" int unires_plan_time_matvecs(unires_plan_t *plan, int32_t on) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null argument");
  const bool twice = on == 2;
  if (twice != plan->twice) drop_cg_graph(plan);  // (a captured solve has its launches baked in)
  plan->twice = twice;
  plan->timing = on == 1;
  if (!plan->timing) drop_timing(plan);
  return UNIRES_OK;
}

extern "C" int unires_plan_cg_ring(unires_plan_t *plan, int32_t k, int32_t *last) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null argument");
  if (k < 0) return fail(UNIRES_ERR_ARG, "ring size must be >= 0");
  if (k > 0) {
    const int v = std::min<int>(k, kMaxRing);
    if (v != plan->ring_req) drop_cg_graph(plan);  // (a captured solve has its ring baked in)
    plan->ring_req = v;
  }
  if (last) *last = plan->last.ring;
  return UNIRES_OK;
}

extern "C" int unires_plan_cg_lockstep(unires_plan_t *plan) { return plan ? plan->last.lockstep : 0; }

extern "C" int unires_plan_cg_ends(unires_plan_t *plan, int32_t *trimmed, int32_t *start_fused) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null argument");
  if (trimmed) *trimmed = plan->last.trim;
  if (start_fused) *start_fused = plan->last.fused;
  return UNIRES_OK;
}

extern "C" int unires_plan_matvec_time(unires_plan_t *plan, int32_t *launches, double *total_us) {
  if (!plan || !launches || !total_us) return fail(UNIRES_ERR_NULL, "null argument");
  *launches = 0, *total_us = 0.0;
  for (auto &e : plan->tev) {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(e.second));
    HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
    *total_us += 1e3 * (double)ms;
    ++*launches;
  }
  drop_timing(plan);
  return UNIRES_OK;
}

// Only the slice scaling (and tau) differ between two descriptions: same geometry, taps, layout and kernel family
static bool same_but_scaling(const RepeatDesc &a, const RepeatDesc &b) {
  auto taps_equal = [](const Taps &p, const Taps &q) {
    for (int d = 0; d < 3; ++d) {
      if (p.n[d] != q.n[d] || p.s[d] != q.s[d]) return false;
      for (int t = 0; t < p.n[d]; ++t)
        if (p.t[d][t] != q.t[d][t]) return false;
    }
    return true;
  };
  return !memcmp(&a.A, &b.A, sizeof(Affine)) && taps_equal(a.T, b.T) && !memcmp(&a.Af, &b.Af, sizeof(Affine)) &&
         taps_equal(a.Tf, b.Tf) && !memcmp(&a.dim_x, &b.dim_x, sizeof(Dim3i)) &&
         !memcmp(&a.dim_g, &b.dim_g, sizeof(Dim3i)) && !memcmp(&a.dim_gf, &b.dim_gf, sizeof(Dim3i)) &&
         !memcmp(&a.dim_xu, &b.dim_xu, sizeof(Dim3i)) && !memcmp(&a.orient, &b.orient, sizeof(Orient)) &&
         a.oriented == b.oriented && a.dim_thick == b.dim_thick && (a.scl != 0.f) == (b.scl != 0.f) &&
         a.sep0 == b.sep0;
}

extern "C" int unires_plan_set_repeat(unires_plan_t *plan, int32_t n,
                                      const unires_repeat_t *repeat) {
  if (!plan || !repeat) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 0 || n >= (int)plan->reps.size()) return fail(UNIRES_ERR_ARG, "repeat index");
  RepeatDesc tmp;
  int rc = fill_repeat(plan, repeat, tmp, plan->reps[n].mid());  // (a masked / weighted repeat stays so: no hybrid form)
  if (rc) return rc;
  if (plan->reps[n].masked && memcmp(&tmp.dim_xu, &plan->reps[n].dim_xu, sizeof(Dim3i)))
    return fail(UNIRES_ERR_DIM, "a masked repeat keeps its observation's dims (clear the mask first)");
  // (the weights stay too: one per slice of the same observation, in the caller's order - the canonical axis behind
  // them and its direction are read from the new orientation at every launch, no device work here)
  if (plan->reps[n].weighted && memcmp(&tmp.dim_xu, &plan->reps[n].dim_xu, sizeof(Dim3i)))
    return fail(UNIRES_ERR_DIM, "a weighted repeat keeps its observation's dims (clear the weights first)");
  if (plan->reps[n].voxw && memcmp(&tmp.dim_xu, &plan->reps[n].dim_xu, sizeof(Dim3i)))
    return fail(UNIRES_ERR_DIM, "a voxel-weighted repeat keeps its observation's dims (clear the weights first)");
  // (and the gains, with the tables composed from them: per slice in the caller's order, like the slice weights)
  if (plan->reps[n].gained && memcmp(&tmp.dim_xu, &plan->reps[n].dim_xu, sizeof(Dim3i)))
    return fail(UNIRES_ERR_DIM, "a gained repeat keeps its observation's dims (clear the gains first)");
  if (plan->regime != UNIRES_REGIME_IDENTITY &&
      (tmp.dim_g.numel() > plan->cap_g || tmp.dim_x.numel() > plan->cap_x))
    return fail(UNIRES_ERR_DIM, "new repeat exceeds the plan's workspace");
  if (plan->regime == UNIRES_REGIME_SUPERRES && (tmp.sep || tmp.hyb) && !plan->gbuf2)
    return fail(UNIRES_ERR_DIM, "new repeat needs the separable-conv scratch the plan was built without");
  // The tables rebuilt below (pull records, splat schedule, conv tables) are rewritten by kernels on
  // the NULL stream and synchronous copies; work queued on the caller's - possibly non-blocking -
  // streams may still be reading them: wait for the plan's last launches - every entry point REMEMBERS its stream
  // before it enqueues anything (mark_use), await_use records an event on each remembered stream and waits for it;
  // not the whole device: the other channels' streams keep running.
  await_use(plan);
  drop_cg_graph(plan);  // the captured solve has the old operator baked in
  plan->prec_ready = false;  // a preconditioner built for the old operator is stale
  Repeat &R = plan->reps[n];
  // A new slice scaling on the same geometry (the scaling Gauss-Newton step, unires/_update.py:270-393, once
  // per observation and ADMM iteration): window plan and splat schedule do not see it - only the conv_up
  // tables that carry S(scl) and the translated regime's factors are rewritten (the schedule build's kernels are
  // 1.2 ms at 256^3, waited for: 5.2 -> 3.9 ms per scaling step of three channels)
  static const bool no_fast = getenv("UNIRES_SET_REPEAT_FULL") != nullptr;
  const bool same = !no_fast && same_but_scaling(tmp, R);
  static const bool verbose = getenv("UNIRES_SET_REPEAT_VERBOSE") != nullptr;
  if (verbose) fprintf(stderr, "[set_repeat] %s (scl %g -> %g)\n", same ? "scaling only" : "full rebuild", (double)R.scl, (double)tmp.scl);
  if (same) {
    R.scl = tmp.scl, R.tau = tmp.tau;
    rc = build_sched(plan, R, true);
    if (!rc) build_shift(plan, R);
    return rc;
  }
  // the tables keep their device allocations; their contents are rebuilt for the new description
  static_cast<RepeatDesc &>(R) = tmp;
  R.ctab_n = 0;  // (no conv_up table of the new operator yet)
  sched_set_thorough(false);  // (an operator changing under a running reconstruction: the quick schedule builds)
  rc = build_repeat_kernels(plan, R);
  sched_set_thorough(true);
  // the mask stays (same observation, same dims); its canonical copy follows a new orientation - on the NULL stream
  // and waited for, like the tables above
  if (!rc && R.masked && R.oriented) {
    rc = canonical_mask(R, nullptr);
    if (!rc) HIP_TRY(hipStreamSynchronize(nullptr));
  }
  // ... and so do the voxel weights and their canonical copy
  if (!rc && R.voxw && R.oriented) {
    rc = canonical_voxel(R, nullptr);
    if (!rc) HIP_TRY(hipStreamSynchronize(nullptr));
  }
  return rc;
}

// The family of kernels and the tables of a repeat whose `masked` / `weighted` flags changed (choose_family): rebuilt where the family
// differs, as unires_plan_set_repeat rebuilds them, but with the thorough schedule builds of unires_plan_create - a mask
// is set once per observation, and a masked repeat then has the tables of a plan created without hybrid forms.
static int refamily(unires_plan *pl, Repeat &R) {
  const bool hyb = R.hyb, hybf = R.hybf, sep = R.sep;
  choose_family(pl, R, R.mid());
  // (a hybrid repeat whose kernels had turned out unavailable was rebuilt by build_repeat_kernels as what it is
  // chosen as now: rebuilding it once more is correct, only not needed)
  if (hyb == R.hyb && hybf == R.hybf && sep == R.sep) return UNIRES_OK;
  R.ctab_n = 0;  // (no conv_up table of the new family yet)
  return build_repeat_kernels(pl, R);
}

// sett.mask_zeros: voxels of repeat n's observation that are exactly 0 are missing data.  The plan keeps
// m(v) = [x(v) != 0] and its A^T A becomes A^T diag(m) A - in the CG matvec, in the Jacobi diagonal and in the mean
// diagonal the FFT preconditioner's symbol is built around, all of which go through ata_forward (api_operator.hip).
// A and A^T do not change.  Setting or clearing a mask changes which kernels the repeat runs on (choose_family; the
// one-kernel forms are skipped in api_operator.hip), so the tables are rebuilt where the family changed; the captured
// solves and the built preconditioner go, like set_diff's.
extern "C" int unires_plan_set_missing(unires_plan_t *plan, int32_t n, const float *x, void *stream) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null plan");
  if (n < 0 || n >= (int)plan->reps.size()) return fail(UNIRES_ERR_ARG, "repeat index");
  if (plan->regime == UNIRES_REGIME_IDENTITY)
    return fail(UNIRES_ERR_UNSUPPORTED,
                "regime A = I has no x-space intermediate to mask: build the plan in the denoising regime with the "
                "identity affine");
  Repeat &R = plan->reps[n];
  if (!x && !R.masked) return UNIRES_OK;
  hipStream_t st = (hipStream_t)stream;
  await_use(plan);  // (the mask is rewritten: earlier launches may still read it)
  drop_cg_graph(plan);
  plan->prec_ready = false;
  const bool was = R.masked, was_mid = R.mid();
  if (x) {
    // every allocation first: a failure leaves the repeat as it was
    const size_t nx = R.dim_xu.numel();
    if (R.mask_cap < nx) {
      free_mask(R);
      if (was_mid != R.mid()) (void)refamily(plan, R);  // (the old mask is gone with its allocation)
      if (hipMalloc((void **)&R.mask_u, nx) != hipSuccess) {
        R.mask_u = nullptr;
        return fail(UNIRES_ERR_ALLOC, "hipMalloc mask");
      }
      R.mask_cap = nx;
    }
    if (R.oriented && !R.mask_c && hipMalloc((void **)&R.mask_c, R.mask_cap) != hipSuccess) {
      R.mask_c = nullptr;
      return fail(UNIRES_ERR_ALLOC, "hipMalloc mask");
    }
    mark_use(plan, st);
    launch_mask_build(x, Orient(), R.dim_xu, R.mask_u, st);
    R.masked = true;
    (void)canonical_mask(R, st);  // (its buffer exists: nothing left to fail)
  } else {
    R.masked = false;
  }
  if (was_mid != R.mid()) {  // (a weighted repeat has the two-kernel family already)
    if (int rc = refamily(plan, R)) {
      // the tables of the new family could not be built: back to the state before the call
      R.masked = was;
      (void)refamily(plan, R);
      return rc;
    }
  }
  CHECK_LAUNCH();
  return UNIRES_OK;
}

// Per-slice weights of repeat n's data term: u_dev holds one float per slice along the caller's axis `axis`, on the
// device; the plan copies them into a buffer of its own and its A^T A becomes A^T diag(u . m) A (api_operator.hip:
// mid_pass), its right-hand side term A^T (u . x).  Three kinds of call:
//   a first set, a clear, a new axis: the repeat's forms change (a weighted repeat declines what a masked one declines:
//     choose_family, the gates of api_operator.hip), so the plan's earlier launches are waited for, the captured solves
//     and the preconditioner go, and the tables are rebuilt where the family differs;
//   new values on the same axis: nothing is rebuilt and nothing waited for.  The copy is enqueued on `stream`, in order
//     behind that stream's earlier solves; a captured solve is KEPT - it has the buffer's address baked in, which does
//     not change, and reads the values there when it is replayed.  (Dropping it would cost a capture per ADMM
//     iteration under sett.slice_robust, which changes the values every iteration.)  The preconditioner is dropped:
//     the Jacobi diagonal and the FFT symbol's mean follow u; it is rebuilt into the same allocations.
// The values are not looked at (they are on the device): u >= 0 is the caller's contract.
// On a gained repeat (unires_plan_set_slice_gains) every call also composes the tables u e^2 and u e again, on the same
// stream behind the copy, and an axis other than the gains' is refused.
extern "C" int unires_plan_set_slice_weights(unires_plan_t *plan, int32_t n, int32_t axis, const float *u_dev,
                                             void *stream) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null plan");
  if (n < 0 || n >= (int)plan->reps.size()) return fail(UNIRES_ERR_ARG, "repeat index");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "slice axis: 0, 1 or 2");
  if (plan->regime == UNIRES_REGIME_IDENTITY)
    return fail(UNIRES_ERR_UNSUPPORTED,
                "regime A = I has no x-space intermediate to weight: build the plan in the denoising regime with the "
                "identity affine");
  Repeat &R = plan->reps[n];
  if (!u_dev && !R.weighted) return UNIRES_OK;
  if (u_dev && R.gained && axis != R.e_axis)
    return fail(UNIRES_ERR_ARG, "slice weights and slice gains of a repeat run along the same axis");
  hipStream_t st = (hipStream_t)stream;
  const bool was = R.weighted, was_mid = R.mid();
  const int was_axis = R.w_axis;
  const bool values_only = u_dev && was && axis == R.w_axis;
  plan->prec_ready = false;
  if (!values_only) {
    await_use(plan);
    drop_cg_graph(plan);
  }
  if (u_dev) {
    const int du[3] = {R.dim_xu.x, R.dim_xu.y, R.dim_xu.z};
    const size_t cap = (size_t)std::max(du[0], std::max(du[1], du[2]));
    if (R.w_cap < cap) {  // (never while the repeat is weighted: its dims are kept, and the buffer was sized for them)
      if (R.w_dev) (void)hipFree(R.w_dev);
      R.w_dev = nullptr, R.w_cap = 0;
      if (hipMalloc((void **)&R.w_dev, cap * sizeof(float)) != hipSuccess) {
        R.w_dev = nullptr;
        return fail(UNIRES_ERR_ALLOC, "hipMalloc slice weights");
      }
      R.w_cap = cap;
    }
    mark_use(plan, st);
    HIP_TRY(hipMemcpyAsync(R.w_dev, u_dev, (size_t)du[axis] * sizeof(float), hipMemcpyDeviceToDevice, st));
    R.weighted = true, R.w_axis = axis;
  } else {
    R.weighted = false;
  }
  if (R.gained) {  // (its tables u e^2 and u e follow the weights, on the same stream behind the copy)
    mark_use(plan, st);
    launch_gain_compose(R.weighted ? R.w_dev : nullptr, R.e_dev, du_of(R, R.e_axis), R.wm_dev, R.wr_dev, st);
  }
  if (was_mid != R.mid()) {  // (a masked repeat has the two-kernel family already)
    if (int rc = refamily(plan, R)) {
      // the tables of the new family could not be built: back to the state before the call
      R.weighted = was, R.w_axis = was_axis;
      (void)refamily(plan, R);
      return rc;
    }
  }
  return UNIRES_OK;
}

// Per-slice intensity gains of repeat n's data term: e_dev holds one float per slice along the caller's axis `axis`, on
// the device.  The data term becomes 1/2 tau sum_v W (x - e[s(v)] (A y)(v))^2, W = g . u . m: the plan's A^T A becomes
// A^T diag(W . e^2) A and its right-hand side term A^T (W . e . x).  The plan copies the gains into a buffer of its own
// and composes two tables beside it, u e^2 and u e (u = 1 without slice weights; gain.hip), which the passes of a
// weighted repeat take where they took u (api_operator.hip: mid_pass, at_accumulate).  Call semantics as for the slice
// weights: a first set, a clear or a new axis changes the repeat's forms - the plan's earlier launches are waited for,
// the captured solves go, the tables are rebuilt where the family differs; new values rebuild nothing and wait for
// nothing - copy and compose are enqueued on `stream`, and a captured solve, which has the tables' addresses baked in,
// is KEPT and reads the new values when it is replayed.  Every set drops the built preconditioner.  The values are not
// looked at: e > 0 is the caller's contract.
extern "C" int unires_plan_set_slice_gains(unires_plan_t *plan, int32_t n, int32_t axis, const float *e_dev,
                                           void *stream) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null plan");
  if (n < 0 || n >= (int)plan->reps.size()) return fail(UNIRES_ERR_ARG, "repeat index");
  if (axis < 0 || axis > 2) return fail(UNIRES_ERR_ARG, "slice axis: 0, 1 or 2");
  if (plan->regime == UNIRES_REGIME_IDENTITY)
    return fail(UNIRES_ERR_UNSUPPORTED,
                "regime A = I has no x-space intermediate to scale: build the plan in the denoising regime with the "
                "identity affine");
  Repeat &R = plan->reps[n];
  if (!e_dev && !R.gained) return UNIRES_OK;
  if (e_dev && R.weighted && axis != R.w_axis)
    return fail(UNIRES_ERR_ARG, "slice gains run along the axis of the repeat's slice weights");
  hipStream_t st = (hipStream_t)stream;
  const bool was = R.gained, was_mid = R.mid();
  const int was_axis = R.e_axis;
  const bool values_only = e_dev && was && axis == R.e_axis;
  plan->prec_ready = false;
  if (!values_only) {
    await_use(plan);
    drop_cg_graph(plan);
  }
  if (e_dev) {
    const size_t cap = (size_t)std::max(R.dim_xu.x, std::max(R.dim_xu.y, R.dim_xu.z));
    if (R.e_cap < cap) {  // (never while the repeat is gained: its dims are kept, and the tables were sized for them)
      free_gains(R);
      if (was_mid != R.mid()) (void)refamily(plan, R);  // (the old gains are gone with their allocation)
      if (hipMalloc((void **)&R.e_dev, 3 * cap * sizeof(float)) != hipSuccess) {
        R.e_dev = nullptr;
        return fail(UNIRES_ERR_ALLOC, "hipMalloc slice gains");
      }
      R.wm_dev = R.e_dev + cap, R.wr_dev = R.e_dev + 2 * cap, R.e_cap = cap;
    }
    mark_use(plan, st);
    HIP_TRY(hipMemcpyAsync(R.e_dev, e_dev, (size_t)du_of(R, axis) * sizeof(float), hipMemcpyDeviceToDevice, st));
    launch_gain_compose(R.weighted ? R.w_dev : nullptr, R.e_dev, du_of(R, axis), R.wm_dev, R.wr_dev, st);
    R.gained = true, R.e_axis = axis;
  } else {
    R.gained = false;
  }
  if (was_mid != R.mid()) {  // (a masked or weighted repeat has the two-kernel family already)
    if (int rc = refamily(plan, R)) {
      // the tables of the new family could not be built: back to the state before the call
      R.gained = was, R.e_axis = was_axis;
      (void)refamily(plan, R);
      return rc;
    }
  }
  CHECK_LAUNCH();
  return UNIRES_OK;
}

// Per-voxel weights of repeat n's data term: g_dev holds one float per x-space voxel in the caller's layout, on the
// device; the plan copies them into a buffer of its own (and, where it relabels the observation, permutes that into a
// canonical-layout copy, as for the mask) and its A^T A becomes A^T diag(g . u . m) A (api_operator.hip: mid_pass), its
// right-hand side term A^T (g . u . x).  Two kinds of call, as for the slice weights:
//   a first set or a clear: the repeat's forms change (choose_family, the gates of api_operator.hip), so the plan's
//     earlier launches are waited for, the captured solves go, and the tables are rebuilt where the family differs;
//   new values: nothing is rebuilt and nothing waited for.  Copy and permute are enqueued on `stream`; a captured solve
//     is KEPT - it has the buffers' addresses baked in, which do not change, and reads the values there when it is
//     replayed (sett.voxel_robust changes the values every ADMM iteration).
// The built preconditioner is dropped either way.  The values are not looked at: g >= 0 is the caller's contract.
extern "C" int unires_plan_set_voxel_weights(unires_plan_t *plan, int32_t n, const float *g_dev, void *stream) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null plan");
  if (n < 0 || n >= (int)plan->reps.size()) return fail(UNIRES_ERR_ARG, "repeat index");
  if (plan->regime == UNIRES_REGIME_IDENTITY)
    return fail(UNIRES_ERR_UNSUPPORTED,
                "regime A = I has no x-space intermediate to weight: build the plan in the denoising regime with the "
                "identity affine");
  Repeat &R = plan->reps[n];
  if (!g_dev && !R.voxw) return UNIRES_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool was = R.voxw, was_mid = R.mid();
  const bool values_only = g_dev && was;
  plan->prec_ready = false;
  if (!values_only) {
    await_use(plan);
    drop_cg_graph(plan);
  }
  if (g_dev) {
    // every allocation first: a failure leaves the repeat as it was
    const size_t nx = R.dim_xu.numel();
    if (R.g_cap < nx) {  // (never while the repeat is weighted: its dims are kept, and the buffers were sized for them)
      free_voxel(R);
      if (hipMalloc((void **)&R.g_u, nx * sizeof(float)) != hipSuccess) {
        R.g_u = nullptr;
        return fail(UNIRES_ERR_ALLOC, "hipMalloc voxel weights");
      }
      R.g_cap = nx;
    }
    if (R.oriented && !R.g_c && hipMalloc((void **)&R.g_c, R.g_cap * sizeof(float)) != hipSuccess) {
      R.g_c = nullptr;
      return fail(UNIRES_ERR_ALLOC, "hipMalloc voxel weights");
    }
    mark_use(plan, st);
    HIP_TRY(hipMemcpyAsync(R.g_u, g_dev, nx * sizeof(float), hipMemcpyDeviceToDevice, st));
    R.voxw = true;
    (void)canonical_voxel(R, st);  // (its buffer exists: nothing left to fail)
  } else {
    R.voxw = false;
  }
  if (was_mid != R.mid()) {  // (a masked or slice-weighted repeat has the two-kernel family already)
    if (int rc = refamily(plan, R)) {
      // the tables of the new family could not be built: back to the state before the call
      R.voxw = was;
      (void)refamily(plan, R);
      return rc;
    }
  }
  CHECK_LAUNCH();
  return UNIRES_OK;
}

// How many solves of OTHER plans the caller keeps in flight next to this one's (the channels of a y-update, each
// on a stream of its own: unires/_update.py:122-150 has no cross-channel term).  The matvec's persistent kernels
// (k_splat2, k_ata1) normally take every wave slot / register the chip has - a channel's kernels then run one
// after the other's whatever the streams say.  With room left for them, the bandwidth-bound CG vector kernels of
// one channel run under the issue-bound splat of another: measured at 256^3 x 3 (profiles/r06_overlap_scan.txt)
// 4 879 -> 5 190 CG it/s with 384 - 448 splat workgroups of 1 024; at 384^3 x 4 a smaller grid LOSES (the pull and
// conv kernels between the splats leave room anyway): the cap applies below 2^25 output voxels.  A launch under a
// cap takes longer and the job as a whole gets faster.  n <= 1: the whole chip (the default).
// k_splat2's grid cap under the two-lane schedule, workgroups per 16 CUs (0: none) - E20's scan
static constexpr int kLockstepS2 = 0;

extern "C" int unires_plan_set_concurrency(unires_plan_t *plan, int32_t n_concurrent) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null argument");
  if (n_concurrent < 1 || n_concurrent > 64) return fail(UNIRES_ERR_ARG, "concurrency out of range (1 .. 64)");
  if (n_concurrent == plan->concurrency) return UNIRES_OK;
  int cap_s2 = 0, cap_f1 = 0, cap_s2_ls = 0;
  if (n_concurrent > 1 && plan->dy.numel() <= (1ull << 25)) {
    int dev = 0, ncu = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    static const int s2_16 = getenv("UNIRES_SHARE_S2") ? atoi(getenv("UNIRES_SHARE_S2")) : 28;  // workgroups per 16 CUs
    static const int f1_16 = getenv("UNIRES_SHARE_F1") ? atoi(getenv("UNIRES_SHARE_F1")) : 48;
    // (the two-lane schedule has a cap of its own, UNIRES_LOCKSTEP_S2 in the same unit; 0: none.  E20)
    static const int ls_16 = getenv("UNIRES_LOCKSTEP_S2") ? atoi(getenv("UNIRES_LOCKSTEP_S2")) : kLockstepS2;
    cap_s2 = std::max(8, ncu * s2_16 / 16 / 8 * 8);  // 448 of 1 024 on 256 CUs
    cap_s2_ls = ls_16 > 0 ? std::max(8, ncu * ls_16 / 16 / 8 * 8) : 0;
    cap_f1 = std::max(8, ncu * f1_16 / 16 / 8 * 8);  // 768 of 1 024
  }
  if (cap_s2 != plan->cap_s2 || cap_f1 != plan->cap_f1 || cap_s2_ls != plan->cap_s2_ls)
    drop_cg_graph(plan);  // (a captured solve has its grids baked in)
  plan->concurrency = n_concurrent, plan->cap_s2 = cap_s2, plan->cap_f1 = cap_f1, plan->cap_s2_ls = cap_s2_ls;
  return UNIRES_OK;
}

// The difference of the plan's D.  A captured solve has the matvec's kernels baked in and a built preconditioner
// the old symbol: both go, like set_repeat's.
extern "C" int unires_plan_set_diff(unires_plan_t *plan, int32_t which) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null argument");
  if (!diff_ok(which)) return fail(UNIRES_ERR_ARG, "which: forward (0), backward (1) or central (2)");
  if (which == plan->diff) return UNIRES_OK;
  await_use(plan);  // (the FFT preconditioner's eigenvalue tables are rewritten at the next build)
  drop_cg_graph(plan);
  plan->prec_ready = false;
  plan->diff = which;
  return UNIRES_OK;
}

extern "C" int64_t unires_plan_workspace_bytes(const unires_plan_t *plan) {
  return plan ? (int64_t)plan->ws_bytes : 0;
}

extern "C" int unires_orient_of(const float M[12], int32_t perm[3], int32_t flip[3]) {
  if (!M || !perm || !flip) return fail(UNIRES_ERR_NULL, "null argument");
  Affine A;
  memcpy(A.m, M, sizeof(A.m));
  for (int i = 0; i < 12; ++i)
    if (!isfinite(A.m[i])) return fail(UNIRES_ERR_ARG, "non-finite affine");
  const Orient O = orient_of(A);
  for (int j = 0; j < 3; ++j) perm[j] = O.perm[j], flip[j] = O.flip[j];
  return UNIRES_OK;
}

extern "C" int unires_plan_repeat_info(const unires_plan_t *plan, int32_t n, int32_t info[8]) {
  if (!plan || !info) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 0 || n >= (int)plan->reps.size()) return fail(UNIRES_ERR_ARG, "repeat index");
  const Repeat &R = plan->reps[n];
  const bool id = plan->regime == UNIRES_REGIME_IDENTITY;
  for (int j = 0; j < 3; ++j) info[j] = id ? j : R.orient.perm[j];
  info[3] = id ? 0 : (R.orient.flip[0] | (R.orient.flip[1] << 1) | (R.orient.flip[2] << 2));
  info[4] = R.pplan.valid ? 1 : 0;
  info[5] = R.sched.valid ? 2 + R.sched.axis : 0;
  // (the forms the matvec takes: a masked or weighted repeat skips the one-kernel matvec and the single-pass AtA kernel)
  info[6] = (R.shift.valid && !R.mid() ? 1 : 0) | (R.f1.valid && !R.mid() ? 2 : 0) | (R.masked ? 4 : 0) |
            (R.weighted ? 8 : 0) | (R.voxw ? 16 : 0) | (R.gained ? 32 : 0);
  info[7] = R.sep ? 1 : 0;
  return UNIRES_OK;
}
