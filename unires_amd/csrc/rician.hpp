// rician.hpp - the Rician data term of a magnitude observation (rician.hip; sett.noise_model = 'rician'): with
// mu = e . (A y) and z = tau x mu the negative log-likelihood of a voxel is 1/2 tau (x - mu)^2 + c(z) (up to a term
// without mu), c(z) = (z - |z|) - log i0e(|z|), and the tangent of log I0 at the current z majorises it by the
// Gaussian term on the effective observation x R(z), R = I1 / I0.
#pragma once
#include "common.hpp"

namespace unires {

// One pass over x and ay (z-fastest, dims d), slices counted along `axis`, S = d[axis]; g a volume or nullptr (1),
// e S floats or nullptr (1).  Per voxel p = fl32(e[s] ay) (launch_slice_apply's product; ay itself without e) and
// z = fl32(fl32(tau x) p), both in registers.
//   xt (nullptr: not written): fl32(x R(z)) with |R| <= 1, R odd, R(+-inf) = +-1; +0 where x == 0.  xt may be ay: a
//     voxel is read and stored by one thread, once.  g is not read for it.
//   sums (nullptr: not written): sums[s] = sum_{v in s} g(v) c(z(v)), float32 terms widened, weighted in float64 (one
//     product, rounded on its own) and added in float64 in launch_rigid_terms_e's fixed order: the same bits every
//     run, every one of the S entries written with a plain store.  part: S * slice_sums_parts(d, axis) doubles of
//     scratch (slice.hpp); not touched without sums.
// R and c in float32 from two fixed-degree forms (|z| <= 3.75: polynomials in z^2; beyond: in 1 / |z|), one select
// between them: no loops, no exp, no overflow.
void launch_rician_terms(const float *x, const float *ay, const float *g, const float *e, Dim3i d, int axis, float tau,
                         float *xt, double *part, double *sums, hipStream_t st);

// The terms of the rigid Gauss-Newton step of a Rician repeat in one pass over x, ay [and g] (sett.rician_gn): p and z
// as above, in registers; g a volume or nullptr (1), u and e S floats each or nullptr (1).
//   sums[s], sums[S + s]: launch_rigid_terms_e's bits - without e launch_slice_sums' / launch_voxel_sums' on (x, ay);
//   sums[2 S + s]: launch_rician_terms' sums;  part: 3 * S * slice_sums_parts(d, axis) doubles of scratch.
//   out (nullptr: not written): launch_rigid_resid's / launch_rigid_resid_g's bits on (x~, p), x~ = fl32(x R(z)) the
//     effective observation above, with t[s] = fl32(fl64(u[s]) fl64(e[s])) (1 for a missing table; neither: no factor)
//     for u; +0 where x == 0 or p == 0 - the mask reads the true x.  out may be ay: a voxel is read and stored by one
//     thread, once.
// launch_rigid_terms_e's walk, grid, shares and finish order: no atomics, the same bits every run.
void launch_rigid_terms_r(const float *x, const float *ay, const float *g, const float *u, const float *e, Dim3i d,
                          int axis, float tau, double *part, double *sums, float *out, hipStream_t st);

}  // namespace unires
