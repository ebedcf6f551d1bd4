/*
 * cuda_runtime.h — stand-in for the CUDA runtime header, for a HOST build of the reference's own sources
 * (oracle/ref_build/Makefile).  TEST INFRASTRUCTURE: our own text; nothing here restates the reference.
 * "Device memory" is the host heap, the execution-space qualifiers are empty.
 */
#ifndef PT_REF_SHIM_CUDA_RUNTIME_H
#define PT_REF_SHIM_CUDA_RUNTIME_H

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct uint2 { unsigned x, y; };
struct uint3 { unsigned x, y, z; };
struct uint4 { unsigned x, y, z, w; };
struct dim3 { unsigned x = 1, y = 1, z = 1; };

static inline float2 make_float2(float x, float y) { return float2{x, y}; }
static inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline int2 make_int2(int x, int y) { return int2{x, y}; }
static inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }
static inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
static inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }
static inline uint3 make_uint3(unsigned x, unsigned y, unsigned z) { return uint3{x, y, z}; }
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }

typedef int cudaError_t;
enum { cudaSuccess = 0, cudaErrorMemoryAllocation = 2 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };

/* A few bytes of slack and at least one byte: the callers copy "vertex count" elements out of arrays that may be shorter
 * (absent UVs), and allocate zero-sized pools. */
template <class T>
static inline cudaError_t cudaMalloc(T** p, size_t n) {
    *p = (T*)calloc(n ? n : 1, 1);
    return *p ? cudaSuccess : cudaErrorMemoryAllocation;
}
static inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t n, cudaMemcpyKind) {
    if (n) memcpy(dst, src, n);
    return cudaSuccess;
}
static inline cudaError_t cudaFree(void* p) { free(p); return cudaSuccess; }
static inline cudaError_t cudaDeviceReset() { return cudaSuccess; }
static inline const char* cudaGetErrorString(cudaError_t) { return "host stand-in"; }

static const uint3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0};
static const dim3 blockDim, gridDim;

#endif
