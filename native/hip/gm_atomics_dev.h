// gm_atomics_dev.h — what the agent-scope atomics test (gm_atomics.hip) and the system-scope
// host-sync test (gm_hostsync.hip) share on the .hip side: the device policy of the steps in
// gm_atomics_steps.h, the pieces of their hand-off kernels, and the host helpers of their drivers.
// The hand-off pieces keep the form MI355X documents as valid: plain stores, every wave drains
// them, barrier, then one lane releases at the scope and stores the flag; the consumer warms its
// L1 first so that a missing invalidate shows. The flag poll and the acquire behind it differ
// between the two kernels (loop form, budget test, flag mask) and stay in them.
#pragma once
#include <hip/hip_runtime.h>

#include "gm_atomics_steps.h"
#include "gm_probe_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

#define GM_RLX __ATOMIC_RELAXED

constexpr int kThreads = GM_ATOMICS_THREADS;

// The steps' policy on the device: relaxed __hip_atomic_* at `Scope`. All ten add kinds at agent
// scope; at system scope the two integer adds, which is what travels as a PCIe AtomicOp.
template <int Scope>
struct DevOps {
  static constexpr uint32_t kKinds = Scope == __HIP_MEMORY_SCOPE_AGENT ? GM_ATOMICS_ADD_KINDS : 2;
  template <class T>
  static __device__ T fetch_add(T* p, T v) { return __hip_atomic_fetch_add(p, v, GM_RLX, Scope); }
  template <class T>
  static __device__ T fetch_xor(T* p, T v) { return __hip_atomic_fetch_xor(p, v, GM_RLX, Scope); }
  template <class T>
  static __device__ T fetch_max(T* p, T v) { return __hip_atomic_fetch_max(p, v, GM_RLX, Scope); }
  template <class T>
  static __device__ T fetch_min(T* p, T v) { return __hip_atomic_fetch_min(p, v, GM_RLX, Scope); }
  template <class T>
  static __device__ T fetch_and(T* p, T v) { return __hip_atomic_fetch_and(p, v, GM_RLX, Scope); }
  template <class T>
  static __device__ T fetch_or(T* p, T v) { return __hip_atomic_fetch_or(p, v, GM_RLX, Scope); }
  static __device__ void pk_add_bf16(uint32_t* p, uint32_t lo, uint32_t hi) {
    bf16x2 v;
    v[0] = (__bf16)(float)lo;
    v[1] = (__bf16)(float)hi;
    (void)__builtin_amdgcn_global_atomic_fadd_v2bf16((__attribute__((address_space(1))) bf16x2*)p,
                                                     v);
  }
  static __device__ uint32_t exchange(uint32_t* p, uint32_t v) {
    return __hip_atomic_exchange(p, v, GM_RLX, Scope);
  }
  static __device__ uint64_t load(const uint64_t* p) { return __hip_atomic_load(p, GM_RLX, Scope); }
  static __device__ bool cas(uint64_t* p, uint64_t* old, uint64_t want) {
    return __hip_atomic_compare_exchange_strong(p, old, want, GM_RLX, GM_RLX, Scope);
  }
};

// ---- the hand-off: a mailbox is `lines` x 4 KiB, 16 bytes per thread and line

// plain u32x4 stores of value(word) for every word of the mailbox
template <class Value>
__device__ __forceinline__ void store_box(uint32_t* box, uint32_t lines, Value value) {
  const uint32_t t = threadIdx.x;
  for (uint32_t l = 0; l < lines; ++l) {
    const uint32_t word = l * GM_ATOMICS_LINE_WORDS + 4 * t;
    const u32x4 q = {value(word), value(word + 1), value(word + 2), value(word + 3)};
    ((u32x4*)box)[l * kThreads + t] = q;
  }
}

// every wave drains its stores, barrier, then one lane releases at `Scope` and stores the flag
template <int Scope>
__device__ __forceinline__ void release_flag(uint32_t* flag, uint32_t value) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if constexpr (Scope == __HIP_MEMORY_SCOPE_AGENT)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    else
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    // the compiler may drop the fence's own wait when it can prove the counter empty
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(flag, value, GM_RLX, Scope);
  }
}

// pull a mailbox into this CU's L1 with plain loads before its flag is polled: bytes held from
// before the flag then show if the acquire does not drop them (an L1-cold reader would hide it)
__device__ __forceinline__ void warm_box(const uint32_t* box, uint32_t lines) {
  uint32_t sink = 0;
  for (uint32_t l = 0; l < lines; ++l) {
    const u32x4 q = ((const u32x4*)box)[l * kThreads + threadIdx.x];
    sink ^= q.x ^ q.y ^ q.z ^ q.w;
  }
  asm volatile("" ::"v"(sink) : "memory");
}

// every word of the mailbox against expect(word); on_bad(word, expected, got) per wrong one
template <class Expect, class OnBad>
__device__ __forceinline__ void compare_box(const uint32_t* box, uint32_t lines, Expect expect,
                                            OnBad on_bad) {
  const uint32_t t = threadIdx.x;
  for (uint32_t l = 0; l < lines; ++l) {
    const u32x4 q = ((const u32x4*)box)[l * kThreads + t];
    const uint32_t got[4] = {q.x, q.y, q.z, q.w};
    const uint32_t word = l * GM_ATOMICS_LINE_WORDS + 4 * t;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t e = expect(word + i);
      if (got[i] != e) on_bad(word + i, e, got[i]);
    }
  }
}

// ---------------------------------------------------------------------------------- host side

// The step form of a public injection (gm_atomics_inject_t, gm_hostsync_inject_t) for `test`, of
// the ADD test for `kind`; none where it is meant for another. The host-sync hand-off keeps its
// direction in `kind`.
template <class Inject>
gm_atomics_inj_t inj_for(const Inject* in, uint32_t test, uint32_t kind, bool dir_in_kind = false) {
  gm_atomics_inj_t j;
  if (in && in->test == test && (test != GM_ATOMICS_ADD || in->kind == kind)) {
    j.a = in->a;
    j.b = in->b;
    j.word = in->word;
    j.mask = in->mask;
    j.dir = dir_in_kind ? in->kind : 0;
    j.on = 1;
  }
  return j;
}

// an injection into a step (g, s) of `test`: a thread and a step of the run, an add kind of the
// test, and a mask where the test uses one
template <class Inject>
bool inject_step_ok(const Inject* in, uint32_t test, uint32_t threads, uint32_t iters,
                    uint32_t add_kinds) {
  if (in->a >= threads || in->b >= iters) return false;
  if (test == GM_ATOMICS_TICKET) return true;
  if (test == GM_ATOMICS_ADD && in->kind >= add_kinds) return false;
  return in->mask != 0;
}

// wall_clock64() ticks in budget_us on the current device
inline int budget_ticks_of(uint32_t budget_us, double* ticks_per_us, uint64_t* ticks) {
  int dev = 0, khz = 0;
  GM_CHECK(hipGetDevice(&dev));
  GM_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
  if (khz <= 0) return (int)hipErrorInvalidDevice;
  *ticks_per_us = khz / 1000.0;
  *ticks = (uint64_t)(budget_us * *ticks_per_us + 0.5);
  if (*ticks == 0) *ticks = 1;
  return 0;
}

// a zeroed table of the kernels' own counters on the stream's device, read back into `host`
// after the stream has drained
template <class T>
struct Tab {
  DevBuf buf;
  T host{};
  T* dev() const { return (T*)buf.p; }
  int create(hipStream_t st) {
    GM_CHECK(buf.alloc(sizeof(T)));
    return (int)hipMemsetAsync(buf.p, 0, sizeof(T), st);
  }
  int read(hipStream_t st) {
    GM_CHECK(hipStreamSynchronize(st));
    return (int)hipMemcpy(&host, buf.p, sizeof(T), hipMemcpyDeviceToHost);
  }
};

}  // namespace
