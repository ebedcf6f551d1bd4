/*
 * det_bind.h — second flavour of ref_probe: sin, cos and pow AS THE REFERENCE'S HEADERS SPELL THEM are bound, in the
 * driver's translation unit only, to the deterministic functions of oracle/pt_oracle_math.h (the arithmetic the HIP
 * kernels are held to).  Included before any header of the reference and after <cmath>, so that the standard library
 * itself is declared under its own names; the parser's translation units keep glibc.  tan (camera set-up) keeps glibc,
 * as the host pipeline's does.  The reference's ternary max / min stay as they are: they differ from IEEE maxNum /
 * minNum on NaN only, and the recorded fixtures hold none.
 */
#ifndef PT_REF_DET_BIND_H
#define PT_REF_DET_BIND_H

#include <algorithm>
#include <cmath>
#include <complex>
#include <filesystem>
#include <iostream>
#include <limits>
#include <random>
#include <sstream>
#include <variant>
#include <vector>

#include "../pt_oracle_math.h"

static inline float pt_ref_det_sin(float x) { float s, c; o_det_sincosf(x, &s, &c); return s; }
static inline float pt_ref_det_cos(float x) { float s, c; o_det_sincosf(x, &s, &c); return c; }
static inline float pt_ref_det_pow(float x, float y) { return o_det_powf(x, y); }
static inline float pt_ref_det_pow(float x, int n) {
    if (n != 5) { fprintf(stderr, "det_bind.h: pow(float, %d) has no deterministic binding\n", n); abort(); }
    return o_det_pow5(x);
}
/* anything else (double arguments, ...) must not reach these names unnoticed */
template <class A, class B> float pt_ref_det_pow(A, B) = delete;
template <class A> float pt_ref_det_sin(A) = delete;
template <class A> float pt_ref_det_cos(A) = delete;

#define sin(x) pt_ref_det_sin(x)
#define cos(x) pt_ref_det_cos(x)
#define pow(x, y) pt_ref_det_pow((x), (y))

#endif
