// ref_cuda_host.h -- TEST INFRASTRUCTURE: the few CUDA device built-ins the reference's BottomUpBuilder.cu and Tracer.cu
// use, written for a serial host run.  Force-included (g++ -include) ahead of ref_kernels_driver.cpp, which #includes
// those two files from the reference tree unmodified; only the CUDA runtime *headers* of the image are used besides.
//
// - launch coordinates are thread_local, so a driver may run rows of one launch on several host threads;
// - atomics are the GCC __atomic builtins (sequentially consistent), templated on (pointer type, operand type)
//   because the reference calls e.g. atomicAdd(unsigned*, int);
// - a fence or barrier is a no-op: ref_kernels_driver.cpp only emulates kernels that do not synchronise within a block.
//   ref_sah_driver.cpp (SharedTaskBuilder.cu: __shared__ variables, __syncthreads(), integer atomics) is compiled with
//   -DREF_BLOCK_BARRIER, under which __syncthreads() is a function that driver supplies;
// - surf2Dwrite writes into a RefSurface (ours), whose address is passed in place of a cudaSurfaceObject_t.
#ifndef REF_CUDA_HOST_H
#define REF_CUDA_HOST_H

#define __DEVICE_LAUNCH_PARAMETERS_H__   // skip the header that declares threadIdx & co. as extern const

#include <math.h>

#include <cstdint>
#include <cstring>

#include <cuda_runtime.h>

extern thread_local uint3 threadIdx;
extern thread_local uint3 blockIdx;
extern thread_local dim3 blockDim;
extern thread_local dim3 gridDim;

// CUDA's min / max overloads on floats, doubles and unsigned ints (math_functions.h: fminf / fmaxf, fmin / fmax, umin /
// umax; an int and an unsigned operand compare as unsigned).  Without these a host compile finds only min(int, int) /
// max(int, int) and truncates BottomUpBuilder.cuh's f3min / f3max and Tracer.cu's min(1.0f, ...) / max(dot(...), 0.0)
// to integers.
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
inline double min(float a, double b) { return fmin((double)a, b); }
inline double max(float a, double b) { return fmax((double)a, b); }
inline double min(double a, float b) { return fmin(a, (double)b); }
inline double max(double a, float b) { return fmax(a, (double)b); }
inline unsigned min(unsigned a, unsigned b) { return a < b ? a : b; }
inline unsigned max(unsigned a, unsigned b) { return a > b ? a : b; }
inline unsigned min(int a, unsigned b) { return min((unsigned)a, b); }
inline unsigned max(int a, unsigned b) { return max((unsigned)a, b); }
inline unsigned min(unsigned a, int b) { return min(a, (unsigned)b); }
inline unsigned max(unsigned a, int b) { return max(a, (unsigned)b); }

// helper_math.h is included here, once, as device code sees it.
// - Its host block (#ifndef __CUDACC__) defines fminf / fmaxf as `a < b ? a : b`, which is not CUDA's fminf / fmaxf
//   (IEEE minNum / maxNum: a NaN operand yields the other one; the slab test meets 0 * inf = NaN on box planes).  The
//   block is skipped; fminf / fmaxf are libm's, and its other three functions are given below, rsqrtf as 1 / sqrtf (the
//   project's arithmetic model; CUDA's rsqrtf is approximate).
// - It converts floats to bytes with uint8_t(x) (make_uchar3 / make_uchar4).  CUDA converts float to u8 with truncation
//   and clamping (cvt.rzi.u8.f32: NaN -> 0, out of range -> 0 or 255); a host cast outside [0, 256) is undefined, and
//   bilinear weights at a texture border do leave that range.  While helper_math.h is read, uint8_t names a type that
//   converts the way the device does; integer operands keep the modulo-256 conversion.
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
struct RefDeviceU8 {
    unsigned char v;
    RefDeviceU8(float f) : v(!(f > 0.0f) ? 0 : (f >= 255.0f ? 255 : (unsigned char)f)) {}
    RefDeviceU8(double f) : v(!(f > 0.0) ? 0 : (f >= 255.0 ? 255 : (unsigned char)f)) {}
    RefDeviceU8(int i) : v((unsigned char)i) {}
    RefDeviceU8(unsigned i) : v((unsigned char)i) {}
    operator unsigned char() const { return v; }
};
#define uint8_t RefDeviceU8
#define __CUDACC__
#include "helper_math.h"
#undef __CUDACC__
#undef uint8_t

inline int __clz(int x) { return x == 0 ? 32 : __builtin_clz((unsigned)x); }
inline int __ffs(int x) { return __builtin_ffs(x); }
inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }

// Called with the address of atomicAdd's operand before the add.  TraceRays hands atomicAdd the first member of its
// TraceStats (Tracer.cu: atomicAdd(num_tests, stats.box_tests)); ref_trace installs an observer there to read the
// triangle-test count of the same record, which the kernel keeps to itself.  Null everywhere else.
extern thread_local void (*ref_atomic_add_observer)(const void* operand);

template <class T, class U> inline T atomicAdd(T* a, const U& v)
{
    if (ref_atomic_add_observer) ref_atomic_add_observer(&v);
    return __atomic_fetch_add(a, (T)v, __ATOMIC_SEQ_CST);
}
template <class T, class U> inline T atomicMin(T* a, U v)
{
    T old = __atomic_load_n(a, __ATOMIC_SEQ_CST);
    while ((T)v < old && !__atomic_compare_exchange_n(a, &old, (T)v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
template <class T, class U> inline T atomicMax(T* a, U v)
{
    T old = __atomic_load_n(a, __ATOMIC_SEQ_CST);
    while ((T)v > old && !__atomic_compare_exchange_n(a, &old, (T)v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
template <class T, class U, class V> inline T atomicCAS(T* a, U expected, V desired)
{
    T e = (T)expected;
    __atomic_compare_exchange_n(a, &e, (T)desired, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
    return e;
}

#ifdef REF_BLOCK_BARRIER
void __syncthreads();   // ref_sah_driver.cpp: a real block barrier (one host thread per CUDA thread, run in turn)
#else
inline void __syncthreads() {}
#endif
inline void __threadfence() {}

struct RefSurface {
    uchar4* px;
    int w;
};

template <class T> inline void surf2Dwrite(T v, cudaSurfaceObject_t surf, int x_bytes, int y)
{
    static_assert(sizeof(T) == 4, "RefSurface holds 4-byte texels");
    RefSurface* s = reinterpret_cast<RefSurface*>(static_cast<uintptr_t>(surf));
    memcpy(&s->px[(size_t)y * s->w + x_bytes / 4], &v, 4);
}

#endif
