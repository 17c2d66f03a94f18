// api_operator.hip - which kernels apply one repeat's A, A^T and A^T A, and the matvec of the y-update's system
// (sum_n tau_n AtA_n + rho lam^2 DtD); the entry points built on them: unires_proj_apply, unires_ata_matvec, the
// preconditioners and the RHS assembly.  Every choice is made from the repeat's description and the validity of
// its tables (api_plan.hip); nothing here builds or frees anything.
#include "aligned.hpp"
#include "api_internal.hpp"
#include "conv.hpp"
#include "pull.hpp"
#include "stencil.hpp"

using namespace unires;

static PushSrc push_src(const Repeat &R, const float *data, bool convup, float scl) {
  PushSrc src;
  src.data = data;
  src.convup = convup ? 1 : 0;
  src.xd = R.dim_x;
  src.gd = convup ? R.dim_gf : R.dim_g;
  src.T = R.Tf;
  src.S = make_scaling(scl, R.dim_thick);
  return src;
}

// scaling split for the hybrid path: the part along z goes with the fused kernels, the rest with
// the 1-D passes
static Scaling scaling_z(const Scaling &S) { return S.dim == 2 ? S : kNoScaling; }
static Scaling scaling_xy(const Scaling &S) { return S.dim == 2 ? kNoScaling : S; }

// The forward operator of one repeat in the plan's canonical layout: out = S conv_down pull(in) (denoising regime:
// out = pull(in), S unused).  One chain, first form that applies: hybrid (z profile in the window pull, x / y
// profiles as 1-D passes) -> separable passes -> window pull + conv -> tile pull + conv -> pull, then conv_down.
static void forward(unires_plan *pl, const Repeat &R, const float *in, const Scaling &S, float *out,
                    const int *done, hipStream_t st) {
  if (pl->regime == UNIRES_REGIME_DENOISE) {
    if (launch_pull_conv2(R.pplan, in, pl->dy, R.A, R.T, kNoScaling, out, R.dim_g, R.dim_g, pl->fov_tol, done, st))
      launch_pull(in, pl->dy, R.A, out, R.dim_g, pl->fov_tol, done, st);
    return;
  }
  if ((R.hyb || R.hybf) && pl->gbuf2 && R.pplan.valid &&
      !launch_pull_conv2(R.pplan, in, pl->dy, R.Af, R.Tz, scaling_z(S), pl->gbuf, R.dim_h, R.dim_gf, pl->fov_tol,
                         done, st)) {
    launch_conv_down_sep(pl->gbuf, R.dim_h, R.Txy, scaling_xy(S), out, R.dim_x, pl->gbuf, pl->gbuf2, done, st);
    return;
  }
  if (R.sep && pl->gbuf2) {
    launch_pull(in, pl->dy, R.Af, pl->gbuf, R.dim_gf, pl->fov_tol, done, st);
    launch_conv_down_sep(pl->gbuf, R.dim_gf, R.Tf, S, out, R.dim_x, pl->gbuf, pl->gbuf2, done, st);
    return;
  }
  if (launch_pull_conv2(R.pplan, in, pl->dy, R.Af, R.Tf, S, out, R.dim_x, R.dim_gf, pl->fov_tol, done, st) &&
      launch_pull_conv(in, pl->dy, R.Af, R.Tf, S, out, R.dim_x, R.dim_gf, pl->fov_tol, done, st)) {
    // Last resort, on the UNTRIMMED R.A / R.T / R.dim_g while every push runs on the trimmed R.Af / R.Tf: A and
    // A^T would differ by the dropped taps (trim_taps: <= 4e-7 relative) if this ran.  It does not: launch_pull_conv
    // (fused.hip) halves its output tile down to one voxel until the pulled tile fits 24 KB of LDS, so it fails
    // (over 64 KB) only when the product of the taps exceeds ~16k.  Such profiles are separable (R.sep: more than 64
    // taps in all) and took the separable passes above; the hybrid form, which resets sep, is kept only where the
    // window plan of pull2 exists (build_repeat_kernels) and took the first branch.
    launch_pull(in, pl->dy, R.A, pl->gbuf, R.dim_g, pl->fov_tol, done, st);
    launch_conv_down(pl->gbuf, R.dim_g, R.T, S, out, R.dim_x, done, st);
  }
}

// The pass on the x-space intermediate of a masked and / or weighted repeat's A^T A: A^T diag(u . m) A, mask and
// weights in ONE pass (slice.hip); the mask alone stays k_mask_apply's.  diag(u) is diagonal in observation space like
// diag(m) and commutes with it and with S.  `weights` false: the repeat's unweighted operator (unires_proj_apply's
// UNIRES_OP_ATA, which stays the reference's).  A gained repeat (unires_plan_set_slice_gains) runs the same passes with
// its table u e^2 where the others have u: A^T diag(g . u . e^2 . m) A.
static void mid_pass(const Repeat &R, float *buf, bool weights, const int *done, hipStream_t st) {
  const float *wm = R.w_mat();
  if (R.voxw && weights)  // (voxel weights: slice weights and mask in the same pass, voxel.hip)
    launch_voxel_apply(buf, buf, R.vox(), R.masked ? R.mask() : nullptr, wm, R.dim_x, R.w_caxis(), R.w_flip(), done, st);
  else if (wm && weights)
    launch_slice_apply(buf, buf, R.masked ? R.mask() : nullptr, wm, R.dim_x, R.w_caxis(), R.w_flip(), done, st);
  else if (R.masked)
    launch_mask_apply(buf, R.mask(), R.dim_x.numel(), done, st);
}

// x-space intermediate of AtA: xbuf = S(2 scl) conv_down pull(in)  (regime 2) or
// gbuf = pull(in) (regime 1); returns the push source that finishes the operator.  A masked repeat
// (unires_plan_set_missing) has its intermediate materialised - fill_repeat gave it no hybrid form, so the branch
// below that fuses conv_down with conv_up is not its - and zeroed where the observation is: A^T diag(m) A.  The mask
// is 0 / 1 in observation space, where it commutes with the even / odd scaling S.  A weighted repeat
// (unires_plan_set_slice_weights) likewise, multiplied by its slice's weight (mid_pass).
static PushSrc ata_forward(unires_plan *pl, const Repeat &R, const float *in, const int *done,
                           hipStream_t st, bool weights = true) {
  if (pl->regime == UNIRES_REGIME_DENOISE) {
    forward(pl, R, in, kNoScaling, pl->gbuf, done, st);
    mid_pass(R, pl->gbuf, weights, done, st);
    return push_src(R, pl->gbuf, false, 0.f);
  }
  // S(2 scl) once between conv and conv^T  (unires/_project.py:175-177)
  const Scaling S2 = make_scaling(2.f * R.scl, R.dim_thick);
  // A^T A with stride-2 profiles along x and y: the x-space volume is only a way station, so the passes on either
  // side of it run as one kernel (conv.hip: k_conv_ydown_xdownup2, k_conv1d_downup2_m) and the push gets a crafted
  // source - a volume that is x-complete (forward-only hybrid: conv_up_y and z follow as one kernel, then the
  // grid-source splat) or x- and y-complete (hybrid: the z-profile splat takes it as it is)
  const bool fwd_only = R.hybf && !R.hyb && R.sep && !(R.sched.valid && R.sched.axis >= 0);
  const bool both = R.hyb && R.sched.valid && R.sched.axis == 2 && R.Tf.s[1] == 2;
  if (!R.mid() && push_mode() == PushMode::kDefault && (fwd_only || both) && pl->gbuf2 && R.pplan.valid && R.Tf.s[0] == 2 &&
      !(R.Tf.n[0] == 1)) {
    // (x taps = Dirac for what follows the x pair; y taps too where conv_up_y went in)
    Taps Ty = R.Txy;
    set_dirac(Ty, 0);
    const Dim3i dxy = Dim3i{R.dim_h.x, R.dim_x.y, R.dim_x.z};
    const Scaling Sx = S2.dim == 0 ? S2 : kNoScaling, Srest = S2.dim == 0 ? kNoScaling : S2;
    const bool y_active = !is_dirac(Ty, 1) || Srest.dim == 1;
    if (y_active && !launch_pull_conv2(R.pplan, in, pl->dy, R.Af, R.Tz, scaling_z(Srest), pl->gbuf, R.dim_h, R.dim_gf,
                                       pl->fov_tol, done, st)) {
      // ... and conv_down_y in front of it in the same kernel where its taps are compiled in; where the z part
      // lives in the splat (`both`) conv_up_y goes in as well: the push source is then x- and y-complete
      const int gy = both ? R.dim_h.y : 0;
      if (!launch_conv_ydown_xdownup2(pl->gbuf, R.dim_h, R.Txy, scaling_xy(S2), R.dim_x.x, R.dim_x.y, gy, pl->gbuf2,
                                      done, st)) {
        PushSrc src = push_src(R, pl->gbuf2, true, 0.f);
        src.xd = both ? Dim3i{R.dim_h.x, R.dim_h.y, R.dim_x.z} : dxy;
        set_dirac(src.T, 0);
        if (both) set_dirac(src.T, 1);
        return src;
      }
      if (both && R.Tf.n[0] * R.Tf.n[1] <= 16) {  // (the fused 2-D kernels of conv.hip serve these taps)
        launch_conv_down_sep(pl->gbuf, R.dim_h, R.Txy, scaling_xy(S2), pl->xbuf, R.dim_x, pl->gbuf, pl->gbuf2, done, st);
        return push_src(R, pl->xbuf, true, 0.f);
      }
      launch_conv_down_sep(pl->gbuf, R.dim_h, Ty, scaling_xy(Srest), pl->gbuf2, dxy, pl->gbuf, pl->gbuf2, done, st);
      if (!launch_conv_downup2(pl->gbuf2, dxy, R.Tf, Sx, 0, R.dim_x.x, pl->gbuf, done, st)) {
        PushSrc src = push_src(R, pl->gbuf, true, 0.f);
        src.xd = dxy;
        set_dirac(src.T, 0);
        return src;
      }
      // not available for these taps: finish the x pass the usual way
      Taps Tx = R.Txy;
      set_dirac(Tx, 1);
      launch_conv_down_sep(pl->gbuf2, dxy, Tx, Sx, pl->xbuf, R.dim_x, pl->gbuf, pl->gbuf, done, st);
      return push_src(R, pl->xbuf, true, 0.f);
    }
  }
  forward(pl, R, in, S2, pl->xbuf, done, st);
  mid_pass(R, pl->xbuf, weights, done, st);
  return push_src(R, pl->xbuf, true, 0.f);
}

// An epilogue without the residual mode, i.e. what matvec() asks of the start's operator application when nothing
// fuses the residual: out stored, no partials.
static PushEpilogue without_residual(PushEpilogue ep) {
  if (ep.res_r) ep.partials = nullptr;
  ep.res_b = nullptr, ep.res_r = nullptr, ep.res_p = nullptr, ep.res_M = nullptr, ep.res_obj = nullptr;
  return ep;
}

// out = [out +] alpha * push(src) [+ epilogue]; falls back to a materialised conv_up when
// the conv_up fan-in is beyond what the fused kernel tabulates.
// The residual mode of the epilogue (ep.res_r) is k_splat2's alone and whether a push serves it is decided HERE, in
// one place: a launch_splat2 that takes the push of a repeat without mask or weights serves it and *served says so; every other
// kernel gets the epilogue without it.  (What is asked at all is matvec()'s: the mode belongs to the matvec's last
// push of a forward-difference operator.  ata_apply() strips it for k_ata1, which is not a push.)
static int push_any(unires_plan *pl, const PushSrc &src, const Repeat &R, float alpha,
                     const PushEpilogue &ep_in, float *out, const int *done, hipStream_t st, bool *served = nullptr) {
  const Affine &A = src.convup ? R.Af : R.A;
  const PushEpilogue ep = without_residual(ep_in);  // what every kernel but k_splat2 is given
  const PushEpilogue &ep2 = R.mid() ? ep : ep_in;   // ... and k_splat2 (a masked or weighted repeat declines the mode)
  const auto s2_done = [&] {
    if (served) *served = ep2.res_r != nullptr;
    return ep2.partials ? splat2_blocks(pl->dy, ep2.grid_cap) : 0;
  };
  if (served) *served = false;
  // default: the schedule-driven splat (k_splat2), then the r1 tile kernels where an operator is outside its
  // domain; UNIRES_PUSH=tile forces the general tile kernel (tests' cross-check)
  const bool use_tile = push_mode() == PushMode::kTile, sched_ok = push_mode() == PushMode::kDefault;
  if (sched_ok && R.hyb && src.convup && R.sched.valid && R.sched.axis == 2 && pl->gbuf2) {
    // conv_up along x / y as 1-D passes, then the z-profile splat with the intermediate as its source
    Taps Txy = src.T;  // (= R.Txy, or with the x part done already: ata_forward)
    set_dirac(Txy, 2);
    const Scaling Sxy = scaling_xy(src.S);
    const bool xy_done = Sxy.dim < 0 && is_dirac(Txy, 0) && is_dirac(Txy, 1);  // (ata_forward's one-kernel x / y part: nothing left)
    const float *h = xy_done ? src.data : launch_conv_up_sep(src.data, src.xd, Txy, Sxy, R.dim_h, pl->gbuf, pl->gbuf2, st);
    const float4 *tab = (const float4 *)R.ctab_dev[src.S.dim == 2 ? 1 : 0];
    if (!launch_splat2(R.sched, h, R.dim_h.numel(), tab, R.ctab_n, R.src_stride, R.ctab_step, R.src_stride,
                       R.ctab_step, A, alpha, ep2, out, pl->dy, done, st))
      return s2_done();
  }
  if (sched_ok && !R.hyb && R.sched.valid && (src.convup != 0) == (R.sched.axis >= 0)) {
    const float4 *tab = src.convup ? (const float4 *)R.ctab_dev[src.S.dim >= 0 ? 1 : 0] : nullptr;
    const size_t numel = src.convup ? src.xd.numel() : src.gd.numel();
    if (!launch_splat2(R.sched, src.data, numel, tab, R.ctab_n, R.src_stride, R.ctab_step, R.src_stride,
                       R.ctab_step, A, alpha, ep2, out, pl->dy, done, st))
      return s2_done();
  }
  if (!use_tile &&
      !launch_splat(src, A, R.Afinv, R.safe, alpha, pl->fov_tol, ep, out, pl->dy, done, st))
    return ep.partials ? splat_blocks(pl->dy, A) : 0;
  if (!use_tile && src.convup && R.sep && pl->gbuf2) {
    // many-tap profile: conv_up as 1-D passes into grid space, then the grid-source splat
    PushSrc d = src;
    d.data = launch_conv_up_sep(src.data, src.xd, src.T, src.S, src.gd, pl->gbuf, pl->gbuf2, st);
    d.convup = 0;
    if (sched_ok && R.sched.valid && R.sched.axis < 0 &&
        !launch_splat2(R.sched, d.data, d.gd.numel(), nullptr, 0, R.src_stride, 1, 0, 0, A, alpha, ep2, out,
                       pl->dy, done, st))
      return s2_done();
    if (!launch_splat(d, A, R.Afinv, R.safe, alpha, pl->fov_tol, ep, out, pl->dy, done, st))
      return ep.partials ? splat_blocks(pl->dy, A) : 0;
    (void)launch_push_tile(d, A, R.Afinv, R.safe, alpha, pl->fov_tol, ep, out, pl->dy, done, st);
    return ep.partials ? push_tile_blocks(pl->dy) : 0;
  }
  if (launch_push_tile(src, A, R.Afinv, R.safe, alpha, pl->fov_tol, ep, out, pl->dy, done, st)) {
    launch_conv_up(src.data, src.xd, src.T, src.S, pl->gbuf, src.gd, st);
    PushSrc d = src;
    d.data = pl->gbuf;
    d.convup = 0;
    (void)launch_push_tile(d, A, R.Afinv, R.safe, alpha, pl->fov_tol, ep, out, pl->dy, done, st);
  }
  return ep.partials ? push_tile_blocks(pl->dy) : 0;
}

// out (+)= alpha * At_n(x); with `weights`, of a weighted repeat: alpha * At_n(u_n . x) - the right-hand side's term.
// u . x is made in the plan's scratch (the observation is never written): in place on the canonical copy where the
// plan relabels the observation, else out of place from the caller's volume.
static void at_accumulate(unires_plan *pl, const Repeat &R, const float *x, float *out, float alpha,
                          bool accumulate, hipStream_t st, bool weights = false) {
  if (pl->regime == UNIRES_REGIME_IDENTITY) {
    launch_axpy(alpha, x, out, pl->dy.numel(), st);  // caller initialised out
    return;
  }
  const float *wr = weights ? R.w_rhs() : nullptr;  // (a gained repeat: its table u e - the term is At_n(u . e . x))
  const bool w = wr != nullptr;
  const bool v = weights && R.voxw;  // (g . u . x of a voxel-weighted repeat: one pass for both kinds of weight)
  if (R.oriented) {  // the caller's voxel layout -> the plan's
    launch_to_canonical(R.orient, x, R.dim_xu, pl->xperm, st);
    if (v)
      launch_voxel_apply(pl->xperm, pl->xperm, R.g_c, nullptr, wr, R.dim_x, R.w_caxis(), R.w_flip(), nullptr, st);
    else if (w) launch_slice_apply(pl->xperm, pl->xperm, nullptr, wr, R.dim_x, R.w_caxis(), R.w_flip(), nullptr, st);
    x = pl->xperm;
  } else if (v) {
    launch_voxel_apply(x, pl->xperm, R.g_u, nullptr, wr, R.dim_x, R.s_axis(), false, nullptr, st);
    x = pl->xperm;
  } else if (w) {
    launch_slice_apply(x, pl->xperm, nullptr, wr, R.dim_x, R.s_axis(), false, nullptr, st);
    x = pl->xperm;
  }
  PushEpilogue ep;
  ep.accumulate = accumulate ? 1 : 0;
  ep.grid_cap = pl->cap_s2;
  const bool sr = pl->regime == UNIRES_REGIME_SUPERRES;
  push_any(pl, push_src(R, x, sr, sr ? R.scl : 0.f), R, alpha, ep, out, nullptr, st);
}

// out (+)= alpha AtA_n(in) [+ epilogue]: pull, push, stencil and dot in ONE pass over `in` where the plan has it
// (denoising regime, ata1.hip; not a masked or weighted repeat, whose intermediate has to exist), else forward + push.  `share`: the persistent kernels' grids leave room for the
// other channels' solves (unires_plan_set_concurrency).  Returns the number of partials written.
static int ata_apply(unires_plan *pl, const Repeat &R, const float *in, float alpha, PushEpilogue ep, bool share,
                     float *out, const int *done, hipStream_t st, bool *served = nullptr, bool weights = true) {
  if (served) *served = false;
  if (pl->regime == UNIRES_REGIME_DENOISE && R.f1.valid && !R.mid()) {
    PushEpilogue e1 = without_residual(ep);  // (k_ata1 declines the residual mode)
    e1.grid_cap = share ? pl->cap_f1 : 0;
    if (!launch_ata1(R.f1, in, R.Af, alpha, e1, out, pl->dy, done, st)) return e1.partials ? ata1_blocks(pl->dy, e1.grid_cap) : 0;
  }
  ep.grid_cap = share ? (pl->lockstep ? pl->cap_s2_ls : pl->cap_s2) : 0;
  const PushSrc src = ata_forward(pl, R, in, done, st, weights);
  return push_any(pl, src, R, alpha, ep, out, done, st, served);
}

extern "C" int unires_proj_apply(unires_plan_t *plan, int32_t n, int32_t op, const float *in,
                                 float *out, void *stream) {
  if (!plan || !in || !out) return fail(UNIRES_ERR_NULL, "null argument");
  if (n < 0 || n >= (int)plan->reps.size()) return fail(UNIRES_ERR_ARG, "repeat index");
  if (op != UNIRES_OP_A && op != UNIRES_OP_AT && op != UNIRES_OP_ATA)
    return fail(UNIRES_ERR_ARG, "Undefined operator");
  if (in == out) return fail(UNIRES_ERR_ARG, "proj_apply cannot run in place");
  hipStream_t st = (hipStream_t)stream;
  mark_use(plan, st);  // (before anything is enqueued: an error return below is remembered too)
  const Repeat &R = plan->reps[n];
  const size_t ny = plan->dy.numel();
  if (plan->regime == UNIRES_REGIME_IDENTITY) {  // operator 'none': return dat
    HIP_TRY(hipMemcpyAsync(out, in, ny * sizeof(float), hipMemcpyDeviceToDevice, st));
    return UNIRES_OK;
  }
  if (op == UNIRES_OP_A) {
    // canonical layout first, re-ordered into the caller's after
    forward(plan, R, in, make_scaling(R.scl, R.dim_thick), R.oriented ? plan->xperm : out, nullptr, st);
    if (R.oriented) launch_from_canonical(R.orient, plan->xperm, out, R.dim_xu, st);
  } else if (op == UNIRES_OP_AT) {
    at_accumulate(plan, R, in, out, 1.f, false, st);
  } else {
    ata_apply(plan, R, in, 1.f, PushEpilogue(), false, out, nullptr, st, nullptr, false);  // (the unweighted operator)
  }
  CHECK_LAUNCH();
  return UNIRES_OK;
}

static bool no_aligned() {
  static const bool v = getenv("UNIRES_NO_ALIGNED") != nullptr;
  return v;
}

// The stencil pass of the matvec: q = a0 p + c DtD p (regime A = I: the whole matvec), or with `accumulate`
// q += c DtD p on a q that holds the data term (the pass that closes a backward / central matvec).  One flat
// streaming pass (stencil.hip); where the shape is outside its domain (lines shorter than 4, tiny volumes) the line
// kernel (forward only), then the general one.  wr, wq: c / vx_d^2 in matvec()'s two roundings.  Returns the number of
// partials written.
static int stencil_close(unires_plan *pl, float c, const float wr[3], const float wq[3], float a0, bool accumulate,
                         const float *p, float *q, double *part, const int *done, hipStream_t st, const float *objb) {
  static const bool no_flat = getenv("UNIRES_NO_FLAT") != nullptr;  // (a switch of forward's line kernel)
  const bool fwd = !diff_nonforward(pl->diff);
  const float h = diff_dtd_scale(pl->diff);
  if (!(fwd && no_flat) && !launch_dtd_flat(pl->diff, accumulate, p, q, pl->dy, a0, wr[0] * h, wr[1] * h, wr[2] * h, part,
                                            objb, done, st))
    return part ? dtd_flat_blocks(pl->dy, pl->diff) : 0;
  if (fwd && !no_aligned() && !launch_dtd_lines(p, q, pl->dy, a0, wq[0], wq[1], wq[2], part, objb, done, st))
    return part ? aligned_blocks(pl->dy) : 0;
  launch_dtd(p, pl->dy, pl->vx, a0, c, q, part, objb, done, st, pl->diff, accumulate);
  return part ? dtd_num_blocks(pl->dy) : 0;
}

// One chain for every difference of D: A = I is the stencil pass alone; one repeat tries the one-kernel forms; else
// one or two kernels per repeat.  The difference decides what the AtA kernels are given.  Forward's carry the
// stencil term (wr / wq) and close the matvec with the dot or the objective.  Backward's and central's run on the same
// kernels with zero weights and no partials, and stencil_close() then adds c DtD_W p and closes the matvec.
int unires::matvec(unires_plan *pl, float rho, float lam, const float *p, float *q, double *part, const int *done,
                   hipStream_t st, const float *objb, StartResidual *res) {
  if (res) res->served = false;
  // stencil weights rho lam^2 / vx_d^2, in the two roundings the kernels were validated with bit for bit:
  // wr = c * (1 / vx^2) (flat stencil, shift and aligned kernels), wq = c / vx^2 (line stencil, push epilogue)
  const float c = rho * (lam * lam);
  float wr[3], wq[3];
  for (int d = 0; d < 3; ++d) {
    const float v2 = pl->vx[d] * pl->vx[d];
    wr[d] = c * (1.f / v2), wq[d] = c / v2;
  }
  if (pl->regime == UNIRES_REGIME_IDENTITY) {
    float a0 = 0.f;
    for (const Repeat &R : pl->reps) a0 += R.tau;
    return stencil_close(pl, c, wr, wq, a0, false, p, q, part, done, st, objb);
  }
  const bool fwd = !diff_nonforward(pl->diff);
  const float zero[3] = {0.f, 0.f, 0.f};
  const float *kw = fwd ? wr : zero;  // what the one-kernel forms receive
  double *kpart = fwd ? part : nullptr;
  const float *kobjb = fwd ? objb : nullptr;
  const size_t nrep = pl->reps.size();
  // the one-kernel forms of a one-repeat plan: the partials written, or -1 where none applies
  const auto one_kernel = [&]() -> int {
    const Repeat &R = pl->reps[0];
    if (nrep != 1 || no_aligned() || R.mid()) return -1;  // (masked / weighted: no intermediate to multiply in one kernel)
    // translated by a fraction of a voxel (no rotation): the factorised one-kernel matvec.  Where the x-marching
    // kernel's fast form applies it serves integer shifts too (31.5 us against k_ata_aligned4x2's 36 - 37 at 256^3)
    // and is tried first
    const auto shift = [&] {
      return launch_ata_shift(R.shift, p, q, pl->dy, R.Af, R.tau, 0.f, kw[0], kw[1], kw[2], kpart, kobjb, done, st);
    };
    if (shift_fast(R.shift, pl->dy) && !shift()) return kpart ? shift_blocks(pl->dy) : 0;
    // grid-aligned observation (identity + integer shift, z slice profile): one streaming kernel
    if (!launch_ata_aligned(p, q, pl->dy, R.dim_gf, R.dim_x, R.Tf, make_scaling(2.f * R.scl, R.dim_thick), R.Af, R.tau,
                            0.f, kw[0], kw[1], kw[2], kpart, kobjb, done, st))
      return kpart ? aligned_blocks(pl->dy) : 0;
    if (!shift()) return kpart ? shift_blocks(pl->dy) : 0;
    return -1;
  };
  // The residual mode is asked of a forward-difference plan that takes the per-repeat route (the one-kernel forms do
  // not know it), on the last repeat's push; push_any() serves or declines it.
  const bool ask = res && fwd && !part && !objb;
  int npart = one_kernel();
  if (npart < 0) {
    // regimes 1/2: one or two kernels per repeat; forward's last one also adds c DtD p and the dot
    npart = 0;
    for (size_t n = 0; n < nrep; ++n) {
      const Repeat &R = pl->reps[n];
      PushEpilogue ep;
      ep.accumulate = n > 0;
      if (fwd) {
        // (ep.p stays unset otherwise: the push kernels take their stencil branch, and read p, wherever it is set)
        ep.p = p;
        if (n == 0) ep.cx = wq[0], ep.cy = wq[1], ep.cz = wq[2];  // the stencil term goes in once
        if (n + 1 == nrep) ep.partials = part, ep.objb = objb;
        if (n + 1 == nrep && ask)
          ep.partials = res->partials, ep.res_obj = res->obj_partials, ep.res_b = res->b, ep.res_r = res->r,
          ep.res_p = res->p, ep.res_M = res->M;
      }
      npart = ata_apply(pl, R, p, R.tau, ep, true, q, done, st, n + 1 == nrep && ask ? &res->served : nullptr);
    }
  }
  return fwd ? npart : stencil_close(pl, c, wr, wq, 0.f, true, p, q, part, done, st, objb);
}

extern "C" int unires_ata_matvec(unires_plan_t *plan, float rho, float lam, const float *p,
                                 float *q, double *dot_dev, void *stream) {
  if (!plan || !p || !q) return fail(UNIRES_ERR_NULL, "null argument");
  if (p == q) return fail(UNIRES_ERR_ARG, "matvec cannot run in place");
  hipStream_t st = (hipStream_t)stream;
  mark_use(plan, st);  // (before anything is enqueued: an error return below is remembered too)
  const int g = matvec(plan, rho, lam, p, q, dot_dev ? plan->part0 : nullptr, nullptr, st);
  if (dot_dev) launch_sum_to(plan->part0, g, dot_dev, st);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_precond_build(unires_plan_t *plan, int32_t precond_mode, float rho,
                                    float lam, float *m_out, void *stream) {
  if (!plan) return fail(UNIRES_ERR_NULL, "null plan");
  // The ADMM loop asks for the preconditioner every iteration: nothing to do while the mode,
  // rho, lam and the operator (set_repeat clears prec_ready) are what it was built for.  The
  // captured CG solve survives a rebuild too: it reads the diagonal at run time and its key
  // holds the mode, rho and lam.
  if (precond_mode == UNIRES_PRECOND_IDENTITY) {
    plan->prec_ready = false;
    return UNIRES_OK;
  }
  if (plan->prec_ready && plan->prec_mode == precond_mode && plan->prec_rho == rho && plan->prec_lam == lam &&
      !m_out)
    return UNIRES_OK;
  if (precond_mode != UNIRES_PRECOND_JACOBI && precond_mode != UNIRES_PRECOND_FFT)
    return fail(UNIRES_ERR_UNSUPPORTED, "preconditioner modes: identity (0), Jacobi (1), FFT (2)");
  hipStream_t st = (hipStream_t)stream;
  mark_use(plan, st);  // (before anything is enqueued: an error return below is remembered too)
  const size_t ny = plan->dy.numel();
  if (precond_mode == UNIRES_PRECOND_FFT) {
    if (int rc = fftpre_setup(plan->fft, plan->dy, plan->diff))
      return fail(rc == 2 ? UNIRES_ERR_ALLOC : UNIRES_ERR_HIP, "hipFFT plan / buffer creation failed");
    FftPre &F = plan->fft;
    // a = mean diagonal of the data term: mean_v sum_n tau_n (AtA_n 1)(v)
    double a = 0.0;
    if (plan->regime == UNIRES_REGIME_IDENTITY) {
      for (const Repeat &R : plan->reps) a += R.tau;
    } else {
      launch_fill(1.f, plan->ax, ny, st);
      for (size_t n = 0; n < plan->reps.size(); ++n) {
        const Repeat &R = plan->reps[n];
        const PushSrc src = ata_forward(plan, R, plan->ax, nullptr, st);
        PushEpilogue ep;
        ep.accumulate = n > 0;
        push_any(plan, src, R, R.tau, ep, F.z, nullptr, st);
      }
      launch_dot(F.z, plan->ax, ny, plan->part0, nullptr, st);
      launch_sum_to(plan->part0, vec_num_blocks(ny), &plan->state->rz, st);
      HIP_TRY(hipMemcpyAsync(&a, &plan->state->rz, sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      a /= (double)ny;
    }
    if (!(a > 0.0)) return fail(UNIRES_ERR_ARG, "data term has an empty diagonal");
    F.a = (float)a;
    for (int d = 0; d < 3; ++d) F.c[d] = rho * (lam * lam) / (plan->vx[d] * plan->vx[d]);
    if (m_out) return fail(UNIRES_ERR_ARG, "m_out is only defined for the Jacobi diagonal");
    CHECK_LAUNCH();
    plan->prec_rho = rho, plan->prec_lam = lam, plan->prec_mode = precond_mode, plan->prec_ready = true;
    return UNIRES_OK;
  }
  if (plan->reps.size() != 1)  // the reference raises ValueError here (_update.py:84-85)
    return fail(UNIRES_ERR_ARG, "CG pre-conditioning only supports one repeat per contrast.");
  if (!plan->precM) HIP_TRY(hipMalloc((void **)&plan->precM, ny * sizeof(float)));
  const Repeat &R = plan->reps[0];
  float c = 0.f;  // 2 rho lam^2 sum_d 1/vx_d^2, float32 like the reference's 0-d tensors
  for (int d = 0; d < 3; ++d) c += 1.f / (plan->vx[d] * plan->vx[d]);
  c = 2.f * rho * (lam * lam) * c;
  if (plan->regime == UNIRES_REGIME_IDENTITY) {
    launch_fill(R.tau + c, plan->precM, ny, st);
  } else {
    launch_fill(1.f, plan->ax, ny, st);
    const PushSrc src = ata_forward(plan, R, plan->ax, nullptr, st);
    push_any(plan, src, R, 1.f, PushEpilogue(), plan->precM, nullptr, st);
    launch_scale_shift(R.tau, c, plan->precM, ny, st);
  }
  if (m_out)
    HIP_TRY(hipMemcpyAsync(m_out, plan->precM, ny * sizeof(float), hipMemcpyDeviceToDevice, st));
  CHECK_LAUNCH();
  plan->prec_rho = rho, plan->prec_lam = lam, plan->prec_mode = precond_mode, plan->prec_ready = true;
  return UNIRES_OK;
}

extern "C" int unires_precond_apply(unires_plan_t *plan, const float *in, float *out, void *stream) {
  if (!plan || !in || !out) return fail(UNIRES_ERR_NULL, "null argument");
  if (in == out) return fail(UNIRES_ERR_ARG, "precond_apply cannot run in place");
  hipStream_t st = (hipStream_t)stream;
  mark_use(plan, st);  // (before anything is enqueued: an error return below is remembered too)
  const size_t ny = plan->dy.numel();
  if (!plan->prec_ready || plan->prec_mode == UNIRES_PRECOND_IDENTITY) {
    HIP_TRY(hipMemcpyAsync(out, in, ny * sizeof(float), hipMemcpyDeviceToDevice, st));
  } else if (plan->prec_mode == UNIRES_PRECOND_FFT) {
    if (fftpre_apply(plan->fft, in, out, st)) return fail(UNIRES_ERR_HIP, "hipFFT execution failed");
  } else {
    launch_div(in, plan->precM, out, ny, st);
  }
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rhs_assemble(unires_plan_t *plan, const float *const *x_ptrs,
                                   const float *w_c, const float *z_c, float rho, float lam,
                                   float *b, void *stream) {
  if (!plan || !x_ptrs || !w_c || !z_c || !b) return fail(UNIRES_ERR_NULL, "null argument");
  for (size_t n = 0; n < plan->reps.size(); ++n)
    if (!x_ptrs[n]) return fail(UNIRES_ERR_NULL, "null observation pointer");
  hipStream_t st = (hipStream_t)stream;
  mark_use(plan, st);  // (before anything is enqueued: an error return below is remembered too)
  // b = -lam * Dt(w - rho z)   (unires/_update.py:131-133)
  launch_div(w_c, z_c, 1.f, -rho, plan->dy, plan->vx, -lam, nullptr, b, st, plan->diff);
  // b += tau_n At_n x_n         (unires/_update.py:125-128; At_n (u_n . x_n) for a weighted repeat)
  for (size_t n = 0; n < plan->reps.size(); ++n)
    at_accumulate(plan, plan->reps[n], x_ptrs[n], b, plan->reps[n].tau, true, st, true);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_atx_assemble(unires_plan_t *plan, const float *const *x_ptrs, float *atx,
                                   void *stream) {
  if (!plan || !x_ptrs || !atx) return fail(UNIRES_ERR_NULL, "null argument");
  for (size_t n = 0; n < plan->reps.size(); ++n)
    if (!x_ptrs[n]) return fail(UNIRES_ERR_NULL, "null observation pointer");
  hipStream_t st = (hipStream_t)stream;
  mark_use(plan, st);  // (before anything is enqueued: an error return below is remembered too)
  if (plan->regime == UNIRES_REGIME_IDENTITY)
    HIP_TRY(hipMemsetAsync(atx, 0, plan->dy.numel() * sizeof(float), st));
  for (size_t n = 0; n < plan->reps.size(); ++n)
    at_accumulate(plan, plan->reps[n], x_ptrs[n], atx, plan->reps[n].tau,
                  n > 0 || plan->regime == UNIRES_REGIME_IDENTITY, st, true);
  CHECK_LAUNCH();
  return UNIRES_OK;
}

extern "C" int unires_rhs_from_atx(unires_plan_t *plan, const float *atx, const float *w_c,
                                   const float *z_c, float rho, float lam, float *b,
                                   void *stream) {
  if (!plan || !atx || !w_c || !z_c || !b) return fail(UNIRES_ERR_NULL, "null argument");
  launch_div(w_c, z_c, 1.f, -rho, plan->dy, plan->vx, -lam, atx, b, (hipStream_t)stream, plan->diff);
  CHECK_LAUNCH();
  return UNIRES_OK;
}
