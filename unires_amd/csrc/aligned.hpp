// aligned.hpp - one-kernel CG matvec for grid-aligned observations (aligned.hip).
#pragma once
#include <stdlib.h>

#include "common.hpp"

namespace unires {

// UNIRES_MATVEC_VERBOSE=1: one line on stderr the first time each instantiation of a one-kernel matvec form
// (aligned.hip, shift.hip) is launched in the process - its name with the template arguments, the grid, and the
// run-time facts that select code inside the kernel (which form ran is decided by shape alone and is not visible in
// the plan).  Host code only.  Unset: one branch per launch, nothing else.
inline bool matvec_verbose() {
  static const bool v = getenv("UNIRES_MATVEC_VERBOSE") && atoi(getenv("UNIRES_MATVEC_VERBOSE")) != 0;
  return v;
}
__attribute__((format(printf, 1, 2))) void matvec_note(const char *fmt, ...);  // (the line without its "[matvec] ")
#define MATVEC_NOTE(...)                              \
  do {                                                \
    if (matvec_verbose()) matvec_note(__VA_ARGS__);   \
  } while (0)

bool affine_is_integer_shift(const Affine &A, int off[3]);
int aligned_blocks(Dim3i dd);
// q = tau AtA p + a0 p + c DtD p (+ partials of sum p*q, or of the objective
// sum (q - 2 objb) p without storing q).  Non-zero return: the operator is not
// an integer shift + z-only slice profile; nothing launched.
int launch_ata_aligned(const float *p, float *q, Dim3i dd, Dim3i gd, Dim3i xd, const Taps &T,
                       const Scaling &S2, const Affine &A, float tau, float a0, float cx,
                       float cy, float cz, double *partials, const float *objb, const int *done,
                       hipStream_t st);

// Regime A = I through the same line kernel: q = a0 p + c DtD p (+ partials).
int launch_dtd_lines(const float *p, float *q, Dim3i dd, float a0, float cx, float cy, float cz,
                     double *partials, const float *objb, const int *done, hipStream_t st);

}  // namespace unires
