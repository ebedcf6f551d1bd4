/* curand_kernel.h — stand-in: the random state is the reference's own PCG32 (its pcg.h), one float draw per call. */
#ifndef PT_REF_SHIM_CURAND_KERNEL_H
#define PT_REF_SHIM_CURAND_KERNEL_H
#include "pcg.h"
typedef pcg32_state curandState;
static inline float curand_uniform(curandState* s) { return next_pcg32_real<float>(*s); }
#endif
