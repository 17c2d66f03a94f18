// stencil.hpp - the regulariser's launchers: the flat streaming form of q = a0 p + c DtD p for regime A = I
// (stencil.hip) and the any-shape gradient / divergence / DtD kernels it falls back to (diff.hip).
#pragma once
#include "common.hpp"

namespace unires {

// `which`: the difference of D (common.hpp).  Forward runs k_dtd_flat (or its marching form), backward / central
// k_dtd_flat_w; their grids, and so the partial counts, differ only where the marching form is on.
int dtd_flat_blocks(Dim3i dd, int which);  // partial sums written per launch
// q = a0 p + c DtD p with per-axis weights cx, cy, cz = c / vx^2, already times diff_dtd_scale(which) (+ partials of
// sum p*q, or of the objective sum (q - 2 objb) p without storing q).  accumulate: q += c DtD p (a0 unused; the
// partials are of the accumulated q) - the pass that closes a non-forward matvec; forward has no such form.
// Non-zero return: outside the kernels' domain, nothing launched.
int launch_dtd_flat(int which, bool accumulate, const float *p, float *q, Dim3i dd, float a0, float cx, float cy,
                    float cz, double *partials, const float *objb, const int *done, hipStream_t st);

// diff.hip: any shape.  `which`: the difference of D (kDiffForward / kDiffBackward / kDiffCentral, common.hpp)
void launch_grad(const float *src, Dim3i d, const float vx[3], float *dst3, hipStream_t st, int which = kDiffForward);
// dst = [add +] scale * Dt(ca*ua + cb*ub)   (ub, add may be NULL)
void launch_div(const float *ua, const float *ub, float ca, float cb, Dim3i d, const float vx[3],
                float scale, const float *add, float *dst, hipStream_t st, int which = kDiffForward);
int dtd_num_blocks(Dim3i d);
// dst = a*src + c*DtD(src); partials (nullable, dtd_num_blocks doubles) gets sum(src*dst) pieces;
// with objb (needs partials): partials = sum (dst - 2 objb) * src and dst is not stored.
// accumulate: dst += c*DtD(src) instead (a unused); the partials are then of the accumulated dst.
void launch_dtd(const float *src, Dim3i d, const float vx[3], float a, float c, float *dst,
                double *partials, const float *objb, const int *done, hipStream_t st, int which = kDiffForward,
                bool accumulate = false);

}  // namespace unires
