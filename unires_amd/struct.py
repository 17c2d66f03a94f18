"""Data structures the hot path reads - counterparts of unires/struct.py:4-111.

``settings`` carries every field of the reference's, with the reference's defaults unless
noted; the atlas and plotting fields exist so that ``init`` can refuse them by name.
"""


class _input:
    """One observed image (unires/struct.py:4-22)."""

    def __init__(self, dat=None, mat=None, tau=1.0, po=None):
        self.dat = dat      # (X,Y,Z) float32 device tensor
        self.dim = None if dat is None else tuple(dat.shape)
        self.mat = mat      # (4,4) float64 affine
        self.tau = tau      # noise precision
        self.po = po        # _proj_op
        self.ct = False
        self.mu = 1.0
        self.sd = 1.0
        self.rigid_q = None
        self.label = None   # [dat, header] of a manual label volume (_util._read_label)
        # per-slice weights of the data term, float32 (dim[po.dim_thick],), >= 0: None - every slice has weight 1.
        # Set before fit() to distrust known slices (used as given with sett.slice_robust off; fit() validates them
        # once and moves them to the device); with sett.slice_robust fit() starts from ones where None and
        # re-estimates them every ADMM iteration.  They define the observation's data term: the y-update, the objective
        # and the scaling and rigid Gauss-Newton updates (sett.scaling, sett.unified_rigid) all minimise it - a slice
        # of weight 0 reaches none of them
        self.slice_w = None
        # per-voxel weights of the data term, float32 (X, Y, Z) like dat, >= 0: None - every voxel has weight 1.  Set
        # before fit() to distrust known voxels (a defect mask, a confidence map; fit() validates them once and moves
        # them to the device); with sett.voxel_robust they are the prior the Huber weights multiply, so a 0 stays 0.
        # They enter the y-update and the objective, and with sett.voxel_gn the scaling and rigid Gauss-Newton updates;
        # without it sett.scaling and sett.unified_rigid are refused with them
        self.weight = None
        # per-slice intensity gains of the data term, float32 (dim[po.dim_thick],), > 0: None - every slice has gain 1.
        # The observation is modelled as e[s(v)] (A y)(v): a slice that came out a few per cent brighter or darker than
        # its neighbours (banding) keeps its information.  Set before fit() where the gains are known (used as given
        # with sett.slice_gain off; fit() validates them once and moves them to the device); with sett.slice_gain
        # fit() starts from them, or from ones where None, and re-estimates them every ADMM iteration.  They enter the
        # y-update and the objective, and with sett.gain_gn the rigid Gauss-Newton update; sett.scaling is refused with
        # them, and so is sett.unified_rigid without sett.gain_gn
        self.slice_gain = None
        # coefficients of a smooth multiplicative bias field b = exp(beta) of the observation (receive-coil shading),
        # float64 (kx, ky, kz), kd <= min(8, dim[d]): None - no field.  beta(i, j, k) = sum_abc c_abc phi_a(i) phi_b(j)
        # phi_c(k) on the observation's own voxel grid, phi_m(i) = cos(pi m (2 i + 1) / (2 n)) (unnormalised DCT-II).
        # The observation is modelled as b . e . (A y).  Set before fit() where the field is known: used as given and
        # never re-estimated, with sett.bias on or off (fit() validates it once); with sett.bias every other non-CT
        # observation starts from zeros and takes one Gauss-Newton step after every ADMM iteration.  Refused with the
        # Rician model, sett.scaling, sett.unified_rigid and sett.slice_gain
        self.bias_coef = None
        # where the observation was read from (_core._read_data; None for in-memory data)
        self.file = None    # the header the file was read with
        self.fname = None
        self.direc = None
        self.nam = None


class _output:
    """One reconstructed channel (unires/struct.py:25-33)."""

    def __init__(self, dat=None, mat=None, lam=None):
        self.dat = dat      # (X,Y,Z) float32 device tensor, updated in place by the CG
        self.dim = None if dat is None else tuple(dat.shape)
        self.mat = mat
        self.lam = lam
        self.lam0 = lam
        self.label = None   # labels warped into the output space (_core._init_y_label)


class _proj_op:
    """Projection-operator descriptor (unires/struct.py:36-54)."""

    def __init__(self):
        self.dim_x = None
        self.mat_x = None
        self.vx_x = None
        self.dim_y = None
        self.mat_y = None
        self.vx_y = None
        self.dim_yx = None
        self.mat_yx = None
        self.ratio = None
        self.smo_ker = None     # dense (1,1,kx,ky,kz) float32, as the reference stores it
        self.smo_ker_1d = None  # its separable factors (what the kernels consume)
        self.rigid = None
        self.scl = None
        self.dim_thick = None
        self.D_x = None
        self.D_y = None


class settings:
    """The subset of unires/struct.py:57-111 that reaches the hot path
    (SURVEY.md Appendix A), same names and defaults."""

    def __init__(self):
        self.alpha = 1.0
        self.bound = 'zero'
        self.cgs_max_iter = 20
        self.cgs_tol = 1e-3
        self.cgs_verbose = False
        self.device = 'cuda'
        self.diff = 'forward'
        self.do_proj = None
        # build-side knob: voxels of an observation that are exactly 0 are missing data in the y-update's system too
        # (they already are in the likelihood, the scaling and rigid updates, the noise estimate and the initial
        # guess): the solve minimises the data term _compute_nll reports (ChannelPlan.set_missing).  Off: the
        # reference's system, which pulls the reconstruction towards 0 wherever an observation is zero-filled.
        self.mask_zeros = False
        # build-side knobs: robust slice outlier rejection.  slice_robust: after every ADMM iteration each observation's
        # slices get a weight from their residuals (_update.slice_rule): 1 unless a slice's residual variance exceeds
        # slice_k^2 times the median slice's, then the ratio.  The data term becomes
        # 1/2 tau sum_v u[s(v)] (x - A y)^2(v) - in the y-update (ChannelPlan.set_slice_weights), the objective and the
        # scaling and rigid updates, which see the weights just re-estimated.  slice_k = 3 is a modelling default
        # nobody has tuned on real data.  Off: every slice has weight 1 unless the user set _input.slice_w.
        self.slice_robust = False
        self.slice_k = 3.0
        # build-side knobs: robust voxel outlier rejection.  voxel_robust: after every ADMM iteration each voxel of each
        # observation gets the Huber weight of its residual r = x - A y (_update._update_voxel_weights): 1 unless |r|
        # exceeds voxel_k noise standard deviations, c = voxel_k / sqrt(tau), then c / |r|; times the user's
        # _input.weight where there is one.  The data term becomes 1/2 tau sum_v g(v) (x - A y)^2(v) in the y-update
        # (ChannelPlan.set_voxel_weights) and the objective.  voxel_k = 3 is a modelling default nobody has tuned on
        # real data.  Off: every voxel has weight 1 unless the user set _input.weight.
        self.voxel_robust = False
        self.voxel_k = 3.0
        # what the Huber threshold is a multiple of.  'noise': the image-noise sd 1 / sqrt(tau), as above.  'mad': the
        # robust sd of the residuals the rule judges, c = voxel_k 1.4826 median|x - A y| over the voxels with x != 0 and
        # prior > 0, re-taken for every repeat at every re-estimate - an exact median on the device, no read-back
        # (DESIGN 8.11).  Residuals carry model error too (slice profile, interpolation, partial volume), and tau may be
        # wrong; 'mad' follows both.  No floor at the noise sd, tau is not re-estimated.  fit() reports the last scale
        # of every repeat in info['voxel_scale'].  Any other name: ValueError in fit()
        self.voxel_scale = 'noise'
        # the scaling and rigid Gauss-Newton updates (sett.scaling, sett.unified_rigid) carry the voxel weights of every
        # repeat that has some: both minimise the data term above (_update._update_scaling, _rigid._update_rigid).
        # Off: fit() refuses those two settings with voxel weights, and the update functions ignore xn.weight, as they
        # did before the updates could carry them.  A switch only because that refusal is pinned by a test; not a
        # modelling choice - with voxel weights and either update, turn it on
        self.voxel_gn = False
        # build-side knobs: banding correction.  slice_gain: every non-CT observation gets one intensity gain per slice
        # along po.dim_thick, re-estimated after every ADMM iteration (_update._update_slice_gains): the exact minimiser
        # of 1/2 tau sum_v W (x - e_s A y)^2 + 1/2 kappa (e_s - 1)^2 over [1 / gain_max, gain_max], W the repeat's
        # weights and mask.  kappa = gain_reg tau (sum_{x != 0} x^2) / (slices with data), fixed for a whole fit().  The
        # reference's sett.scaling (one exp(+-s) for even / odd slices) is a special case and is refused with it, and so
        # is sett.unified_rigid unless sett.gain_gn lets its step carry the gains.  A factor common to all gains of a repeat trades
        # against y; the ridge towards 1 bounds it and does not remove it.  gain_reg = 0.1 and
        # gain_max = 2 are UNTUNED modelling defaults: nobody has chosen them on real data.  Off: every slice has gain 1
        # unless the user set _input.slice_gain
        self.slice_gain = False
        self.gain_reg = 0.1
        self.gain_max = 2.0
        # the rigid Gauss-Newton update (sett.unified_rigid) carries the gains of every repeat that has some: objective,
        # residual (times e, the chain rule through diag(e)) and Hessian weight W e^2 are those of
        # 1/2 tau sum_v W (x - e_s A y)^2 (_rigid._update_rigid).  Off: fit() refuses sett.unified_rigid
        # with gains, and the update ignores xn.slice_gain, as it did before it could carry them.  A switch only because
        # that refusal is pinned by a test; not a modelling choice - with gains and sett.unified_rigid, turn it on.
        # sett.scaling stays refused with gains either way
        self.gain_gn = False
        # build-side knob: the noise model of the data term.  'gaussian': 1/2 tau sum_v W (x - mu)^2, mu = e . A y - the
        # reference's, and what ran before the knob existed, bit for bit.  'rician': every non-CT observation is a
        # magnitude image with Rice noise of sigma = 1 / sqrt(tau) (what init() estimates): a voxel's term becomes
        # W [1/2 tau (x - mu)^2 + c(tau x mu)], c(z) = (z - |z|) - log i0e(|z|), which does not pull dark tissue, CSF
        # and air towards the Rician mean.  Minimised by majorisation: each ADMM iteration's y-update is the Gaussian
        # one on the effective observation x I1/I0(tau x mu) of the previous iteration's y (the first on x itself); one
        # A y and one streaming pass per repeat and iteration, and one more observation-sized buffer per repeat
        # (DESIGN 8.14).  CT repeats keep the Gaussian term.  Observations must be finite and >= 0.  sett.scaling,
        # sett.unified_rigid and sett.slice_gain minimise the Gaussian term and are refused with it, by name, unless
        # sett.rician_gn is set.  Any other name: ValueError in fit()
        self.noise_model = 'gaussian'
        # the rigid Gauss-Newton update (sett.unified_rigid) and the gain estimate (sett.slice_gain) carry the Rician
        # term of every repeat that has it: the rigid step's objective is the exact Rician term, its residual
        # W e (e A y - x I1/I0(z)) the exact gradient, its Hessian weight W e^2 the majoriser's curvature - the one the
        # step builds without the model (_rigid._update_rigid); the gain rule reads the effective observation
        # (_update._update_slice_gains).  Off: fit() refuses both with 'rician', and the two updates run
        # what they ran.  A switch only because those refusals are pinned by a test; not a modelling choice.
        # sett.scaling stays refused with 'rician' either way, and sett.unified_rigid with gains still needs sett.gain_gn
        self.rician_gn = False
        # build-side knobs: a smooth multiplicative bias field per observation (receive-coil shading).  bias: every
        # non-CT observation without a user's _input.bias_coef gets a field b = exp(beta), beta a separable cosine
        # series of order kd = clamp(ceil(2 n_d vx_d / bias_cutoff), 1, min(8, n_d)) along axis d - half-periods no
        # shorter than bias_cutoff mm; its coefficients take one Gauss-Newton step with a backtracking line search
        # after every ADMM iteration (_update._update_bias).  The data term becomes 1/2 tau sum_v W (x - b mu)^2 +
        # 1/2 c^T Lambda c, Lambda = kappa bias_reg diag(1 + sum_d (bias_cutoff m_d / (2 n_d vx_d))^2), kappa =
        # tau sum_{x != 0} x^2 fixed for a whole fit(); the ridge on the constant term is what fixes the scale between b
        # and y.  log b is clamped to +- log(bias_max).  The plan reads g b^2 for its voxel map and x / b for its
        # observation: no solve kernel changes, three more observation-sized buffers per repeat.  bias_cutoff = 60 mm,
        # bias_reg = 0.01 and bias_max = 4 are UNTUNED modelling defaults: nobody has chosen them on real data.
        # Refused, by name, with noise_model = 'rician', scaling, unified_rigid and slice_gain.  Off:
        # no observation has a field unless the user set _input.bias_coef
        self.bias = False
        self.bias_cutoff = 60.0
        self.bias_reg = 0.01
        self.bias_max = 4.0
        # per-voxel weight maps for init() / preproc(): a nested list shaped like the data (channels, then repeats),
        # each entry a NIfTI path, a tensor / array of the observation's shape, or None (_core._read_weights)
        self.weight = None
        # init() honours the weight maps too: a voxel whose weight is 0 is read by neither the noise / intensity
        # estimate (tau, mu, lam), nor the coregistration (quantisation range and every counted sample of the joint
        # histograms), nor the first guess of y (run.init).  Only the support of a map (> 0) counts
        # there; how large a positive weight is stays the data term's business.  Off: init() ignores the maps, as it
        # did before it could read them.  A switch only because tests pin init()'s results with sett.weight set; not
        # a modelling choice - with a defect mask, turn it on
        self.voxel_init = False
        # how init() estimates the noise sd (and so tau) of an observation.  'mixture': the reference's rule, the noise
        # class of a two-class mixture fitted to the intensity histogram - it needs an air background.  'mad': 1.4826 / 2
        # times the exact median magnitude of the in-plane Haar diagonal detail over the cells of usable voxels, and
        # mu = |mean of the usable voxels| - for background-free inputs (skull-stripped, masked, cropped);
        # WITH an air background it reads low, towards 0.655 sd.  Any other name: ValueError in init()
        self.noise_est = 'mixture'
        self.gap = 0.0
        self.interpolation = 'linear'
        self.method = None
        self.profile_ip = 2
        self.profile_tp = 0
        self.reg_scl = 4.0
        self.rho = None
        self.rho_scl = 1.0
        self.tolerance = 1e-4
        self.max_iter = 512
        self.sched_num = 3
        self.rigid_mod = 1
        self.scaling = False
        self.unified_rigid = False
        self.rigid_samp = 1
        self.rigid_basis = None  # set by _update_rigid / fit: affine_basis('SE')
        self.clean_fov = False
        self.do_print = 0
        # build-side knob: which nitorch-cg objective branch to reproduce
        # ('max_gain' = what the reference passes, unires/_update.py:145)
        self.cgs_stop = 'max_gain'
        # 'jacobi': _precond (the reference has it commented out, _update.py:136);
        # 'fft': build-side FFT-diagonal preconditioner (circulant a I + rho lam^2 DtD)
        self.cgs_precond = 'none'
        # build-side knob: enqueue the (independent) channels of the y-update on separate HIP streams
        # (True / False), or 'auto': streams whenever there are several channels.  Each plan is then told about
        # its neighbours (unires_plan_set_concurrency) and sizes its persistent kernels for them.  CG iterations/s,
        # streams vs one channel after the other (profiles/r06_overlap_scan.txt): 181 x 217 x 181 +20 .. +24 %,
        # 256^3 x 3 +6 %, thick axes x / y / z +8 %, 384^3 x 4 +5 %.  (Rounds 3 - 5 stopped at 10 M voxels: with
        # every matvec kernel filling the chip three streams bought nothing at 256^3.)
        self.channel_streams = 'auto'
        # ADMM iterations the host may run ahead of its GPU before it sleeps (blocking-sync events; 0: never
        # waits - the runtime then spins in the launch calls once the hardware queue is full), _host.Pacer
        self.host_pace = 2
        # build-side knob: keep sum_n tau_n At x_n across ADMM iterations (recomputed on change)
        self.cache_atx = True
        # manual labels of one observation, (path, (channel, repeat)) (unires/struct.py:86)
        self.label = None
        # resample observations to voxels no smaller than vx before fitting (_core._resample_inplane)
        self.force_inplane_res = False
        # reconstruction voxel size: a scalar or one per axis (unires/struct.py:109)
        self.vx = 1.0
        # coregistration of the observations (_core._init_reg; unires/struct.py:72-75, 90-93)
        self.do_coreg = True
        self.coreg_params = {'cost_fun': 'nmi', 'group': 'SE', 'samp': 1, 'fwhm': 7, 'mean_space': False}
        self.fix = 0  # flat index (channels, then repeats) of the observation the others align to
        self.do_atlas_align = False
        self.mat_coreg = None  # (N, 4, 4) float64 transforms _init_reg found
        # ---- init() / preproc() (run.py, _core._format_y / _read_data / _write_data; unires/struct.py) ----
        self.mat = None  # affine of the observations when they are given as one (X, Y, Z, C) array
        self.ct = False  # the data could be CT
        self.pow = 0  # output dimensions: an int > 0 (powers of two or 3 * powers of two, at most pow) or a 3-tuple
        self.dir_out = None  # output directory; None: the first input's, else 'UniRes-output'
        self.prefix = 'u_'
        self.bids = False  # add the '_space-unires_' tag to the written names
        self.write_out = True
        # the atlas, the CT origin reset, the JTV file and plotting are not built: init() / _format_y / _write_data
        # raise NotImplementedError when one of the switches below is set (atlas_rigid and fov only qualify them)
        self.atlas_rigid = False
        self.common_output = False
        self.crop = False
        self.do_res_origin = False
        self.fov = 'brain'
        self.write_jtv = False
        self.plot_conv = False
        self.show_hyperpar = False
        self.show_jtv = False
