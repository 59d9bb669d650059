// arx_hd.h -- the attribute and atomic macros the device functors are written in: HIP's under hipcc, plain C++ everywhere else (the host test
// doubles under tests/, which run a launch as a loop over its items, and host-compiled product code that shares a header with the device).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ARX_DEV __device__
#define ARX_DEVI __device__ __forceinline__
#define ARX_HDI __host__ __device__ __forceinline__ // also used by the host tail of a stage
#define ARX_ATOMIC_OR(p, v) atomicOr((unsigned int *)(p), (unsigned int)(v))
#define ARX_ATOMIC_INC(p) atomicAdd((int *)(p), 1)
#define ARX_ATOMIC_ADD(p, v) atomicAdd((int *)(p), (int)(v))
#define ARX_ATOMIC_MIN(p, v) atomicMin((int *)(p), (int)(v))
#define ARX_ATOMIC_CAS(p, c, v) atomicCAS((int *)(p), (int)(c), (int)(v))
#define ARX_ATOMIC_ADD64(p, v) atomicAdd((unsigned long long *)(p), (unsigned long long)(v))
#define ARX_ATOMIC_MIN64(p, v) atomicMin((long long *)(p), (long long)(v))
#define ARX_ATOMIC_MAX64(p, v) atomicMax((long long *)(p), (long long)(v))
#define ARX_ATOMIC_MINU64(p, v) atomicMin((unsigned long long *)(p), (unsigned long long)(v))
// plain read of a word other lanes of the workgroup update with atomics (which execute in L2): bypass the per-CU L1
#define ARX_LOAD_SHARED(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define ARX_DEV
#define ARX_DEVI inline
#define ARX_HDI inline
#define ARX_ATOMIC_OR(p, v) (*(p) |= (v))
#define ARX_ATOMIC_INC(p) ((*(p))++)
#define ARX_ATOMIC_ADD(p, v) arx_host_fetch_add((p), (v))
#define ARX_ATOMIC_MIN(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define ARX_ATOMIC_CAS(p, c, v) arx_host_cas((p), (c), (v))
#define ARX_ATOMIC_ADD64(p, v) (*(p) += (v))
#define ARX_ATOMIC_MIN64(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define ARX_ATOMIC_MAX64(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define ARX_ATOMIC_MINU64(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define ARX_LOAD_SHARED(p) (*(p))
static inline int arx_host_fetch_add(int32_t *p, int v) { int o = *p; *p += v; return o; }
static inline int arx_host_cas(int32_t *p, int c, int v) { int o = *p; if (o == c) *p = v; return o; }
#endif
