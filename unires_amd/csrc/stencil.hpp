// stencil.hpp - flat streaming form of q = a0 p + c DtD p for regime A = I (stencil.hip).
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

}  // namespace unires
