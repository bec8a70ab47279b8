// Device helpers of the gammatone filter loop, shared by gammatone_kernel and gammatone_spikes_kernel (frontend.hip):
// the coefficient load, the second-order section and the quotient by a precomputed reciprocal.  This is the one place
// where the reference's order of operations is written down.  (The two-chain cascade of gammatone_spikes_kernel repeats
// section() by hand, and the chunked sample run and the hop walk stay in the kernels: shared as functions they changed
// the compiled filter loops, profiles/frontend_shared_filter.txt.)
//
// The reference filters every channel with scipy.signal.lfilter over four cascaded second-order sections, each in
// direct form II transposed with normalised coefficients (b/a0, a/a0):
//     y  = z0 + b0*u
//     z0 = (z1 + b1*u) - a1*y
//     z1 =       b2*u  - a2*y
// then divides by the channel's gain, squares, and per column sums nwin samples in ascending order, / nwin, sqrt.
// Every float64 operation below is one of these, in this order; the translation unit is compiled with
// -ffp-contract=off.  A change to one of the helpers shows in the assembly of all forty filter kernels; compare it
// with the parent's the way the profile above does.
//
// Exactness notes.  (1) A2 == 0 for every channel of this filter design, so u*b2 is a signed zero and
// z1 = u*b2 - y*a2 equals -(y*a2) up to the sign of an exact zero, which can never reach a non-zero value downstream;
// B2ZERO drops that product.  (2) n/d is evaluated as q = n*r, q' = fma(fma(-q, d, n), r, q) with r = RN(1/d):
// Markstein's sequence returns the correctly rounded quotient (= the IEEE division the reference performs) unless d's
// significand is all ones (or d leaves the normal range), which the caller checks before choosing this path.
#pragma once
#include "lsm_common.h"

namespace lsm_gt {

// One channel's four sections, normalised by a0.  The sections of this design share b0, b2, a1 and a2 and differ in b1
// (coefficient table: B0, B11..B14, B2, A0, A1, A2, gain: ten doubles per channel).
struct Sections {
    double b0, b1[4], b2, a1, a2, gain, rgain;
};

__device__ __forceinline__ Sections load_sections(const double *coefs, int ch)
{
    const double *k = coefs + (size_t)ch * 10;
    Sections s;
    const double a0 = k[6];
    s.b0 = k[0] / a0; s.b2 = k[5] / a0;
    s.b1[0] = k[1] / a0; s.b1[1] = k[2] / a0; s.b1[2] = k[3] / a0; s.b1[3] = k[4] / a0;
    s.a1 = k[7] / a0; s.a2 = k[8] / a0; s.gain = k[9];
    s.rgain = 1.0 / s.gain;
    return s;
}

// One section step on input u; returns the section's output.  The parameters stand in the order in which the step
// first touches them: with (u, b0, b1, b2, a1, a2, z0, z1) the compiler schedules the filter loops differently.
template <bool B2ZERO>
__device__ __forceinline__ double section(double &z0, double b0, double u, double &z1, double b1, double a1, double a2,
                                          double b2)
{
    const double y = z0 + b0 * u;
    z0 = (z1 + u * b1) - y * a1;
    z1 = B2ZERO ? -(y * a2) : u * b2 - y * a2;
    return y;
}

// q = n / d with r = RN(1/d): Markstein's sequence (FAST, see the notes above) or the true division.  The quotient
// leaves through a reference: as a return value the last fma would take the return's `noundef`, which is enough to
// change how the filter loop is vectorised and scheduled.
template <bool FAST>
__device__ __forceinline__ void quot(double &q, double n, double d, double r)
{
    if (FAST) {
        const double q0 = n * r;
        q = __builtin_fma(__builtin_fma(-q0, d, n), r, q0);
    } else {
        q = n / d;
    }
}

}  // namespace lsm_gt
