// The hand-off between the workgroups of a weight-stationary LSTM launch (lstm_fwd_persist.hip, lstm_fwd_ns.hip,
// lstm_bwd_persist.hip, lstm_f32_persist.hip): the status area, the bounded wait, the XCD agreement, the chunk-level
// round counters, the sc1 / write-through 16-byte accesses and the diagnostic stamp.  The protocol itself is described
// in the header comment of lstm_fwd_persist.hip.
//
// The rule: a wait in these kernels is written with bounded_spin, or -- in the two loops that redo work while they
// wait -- with spin_expired / raise_timeout / status_clear.  Never by hand: a wait that does not end on the time-out and
// on the sticky status word hangs a machine that others share.
#pragma once
#include "csn_common.h"

namespace csn {

// ---- the status area of a workspace (WsLayout::status; PersistFwdArgs / PersistBwdArgs / F32Persist*Args::error_flag):
// kStatusBytes of 32-bit words, zeroed by csn_lstm_workspace_init and csn_lstm_status_clear, sticky in between.
// csn_lstm_status_read maps the first three words to the CSN_STATUS_* bits.
enum StatusWord : int {
  kStatusTimeout = 0,        // a bounded wait ran out (or csn_lstm_status_raise): every later wait returns at once
  kStatusNonFinite = 1,      // a non-finite gradient reached the backward
  kStatusStaleSlot = 2,      // CSN_SLAB_TAGS builds: a consumer was served a stale occupant of a ring slot
  kStatusDumpClaim = 7,      // CSN_SLAB_TAGS_DUMP builds: the first detection claims the dump ...
  kStatusDump = 8,           // ... and writes its 16 words here
};
static constexpr size_t kStatusBytes = 256;

// ---- bounded waits
static constexpr unsigned long long kSpinTimeoutTicks = 20000000ull;   // 0.2 s of the 100 MHz wall clock

__device__ __forceinline__ bool status_clear(const unsigned* error_flag) {
  return __hip_atomic_load(error_flag + kStatusTimeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
}
__device__ __forceinline__ void raise_status(unsigned* error_flag, StatusWord w) {
  __hip_atomic_store(error_flag + w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void raise_timeout(unsigned* error_flag) { raise_status(error_flag, kStatusTimeout); }
__device__ __forceinline__ bool spin_expired(unsigned long long t0) { return wall_clock64() - t0 > kSpinTimeoutTicks; }

// Spins until done() -- which polls with relaxed agent-scope (sc1) loads, this CU's L1 bypassed -- or until the status
// word is set (by anyone: sticky, later waits return at once) or the time-out has passed (then sets it).
// Callers capture by VALUE, and never the kernel-argument struct: a reference to it changes the register allocation of
// kernels that sit at the limit.
template <typename Done>
__device__ __forceinline__ void bounded_spin(unsigned* error_flag, Done done) {
  const unsigned long long t0 = wall_clock64();
  while (!done()) {
    __builtin_amdgcn_s_sleep(1);
    if (!status_clear(error_flag)) break;
    if (spin_expired(t0)) {
      raise_timeout(error_flag);
      break;
    }
  }
}

// ---- is hand-off group `grp` of a grouped launch on one XCD?  Evaluated by all threads of every workgroup of the group,
// `a` being the launch's PersistFwdArgs / PersistBwdArgs and `tid` the kernel's copy of threadIdx.x.  Thread 0 adds
// (1, 1 << its XCC field) to the group's agreement word a.agree[grp] and waits for all `nslices` arrivals; all workgroups
// then see the same word and take the same decision.  `lds`: 4 bytes of the workgroup's LDS, free again afterwards.
// A macro, because of what the alternatives did to kernels that sit at the register limit: the arguments are read where
// the kernels have always read them -- inside thread 0's branch, the status pointer inside the wait.  As a function with
// by-value arguments the same instructions came out in another order in every kernel, and one N-split instantiation
// changed its address arithmetic; with `a` by reference the K-split forward changed its register allocation; and with
// threadIdx.x read again instead of `tid` the fused N-split kernels changed theirs.
// (Count: the width in which the arrivals are compared.  The K-split forward has always compared 32 bits and the other
// kernels the 64 of the word; either is right, and each keeps its own so that its device code stays what it was.)
__device__ __forceinline__ unsigned xcc_id() { return __builtin_amdgcn_s_getreg(6164) & 7u; }      // hwreg(HW_REG_XCC_ID, 0, 4)
// (LDS address space: no flat_ instruction in these kernels -- FLAT retires out of order)
#define CSN_LDS_INT(p) ((__attribute__((address_space(3))) int*)(__attribute__((address_space(3))) void*)(p))
#define CSN_XCD_GROUP_IS_LOCAL(Count, a, grp, nslices, lds)                                                            \
  ({                                                                                                                   \
    if (tid == 0) {                                                                                                    \
      const unsigned xcc_ = csn::xcc_id();                                                                             \
      const unsigned long long mine_ = 1ull | (1ull << (8 + 6 * xcc_));                                                \
      __hip_atomic_fetch_add((a).agree + (grp), mine_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                    \
      const unsigned long long t0_ = wall_clock64();                                                                   \
      unsigned long long v_;                                                                                           \
      while ((Count)((v_ = __hip_atomic_load((a).agree + (grp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xffull) < \
             (Count)(nslices)) {                                                                                       \
        __builtin_amdgcn_s_sleep(1);                                                                                   \
        if (!csn::status_clear((a).error_flag)) break;                                                                 \
        if (csn::spin_expired(t0_)) {                                                                                  \
          csn::raise_timeout((a).error_flag);                                                                          \
          break;                                                                                                       \
        }                                                                                                              \
      }                                                                                                                \
      CSN_LDS_INT(lds)[0] = (int)(((v_ >> (8 + 6 * xcc_)) & 63ull) == (unsigned long long)(nslices));                  \
    }                                                                                                                  \
    __syncthreads();                                                                                                   \
    const bool local_ = CSN_LDS_INT(lds)[0] != 0;                                                                      \
    __syncthreads();                                                                                                   \
    local_;                                                                                                            \
  })

// ---- chunk-level hand-off between the rounds of a merged launch (PersistBwdArgs::nrounds): row-major dgates and dx cross
// XCDs through plain / nt stores, so visibility is an agent-scope release by the producers and an agent-scope acquire by
// every consuming workgroup.  Both are called by ALL threads of a workgroup, under a uniform condition.
// Publish: every wave's stores have left it, then ONE lane writes the XCD's L2 back and counts the workgroup in.
// (the one lane: compared afresh at every use -- as a loop invariant the lane mask was a pair of SGPRs kept, and spilled,
// across the step loop)
__device__ __forceinline__ bool round_leader() {
  unsigned t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t == 0u;
}
__device__ __forceinline__ void round_publish(unsigned* word) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (round_leader()) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the fence's own wait can be dropped by the compiler)
    __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// Wait: ONE lane polls the counter, then the acquire; the barrier holds the other waves until the invalidate has
// completed.  No load of the handed-off bytes may be issued in front of this.
__device__ __forceinline__ void round_wait(const unsigned* word, unsigned want, unsigned* error_flag) {
  if (round_leader()) {
    bounded_spin(error_flag, [word, want] { return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want; });
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}

// ---- the handed-off bytes: 16 per lane through a buffer resource, as any 16-byte vector type V
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// aux = 16: sc1 (agent-coherent, bypasses this CU's L1; MI355X_MICROARCH.md visibility table)
template <typename V>
__device__ __forceinline__ V load_sc1_b128(__amdgpu_buffer_rsrc_t rsrc, int byte_off, int soff = 0) {
  static_assert(sizeof(V) == 16, "a 16-byte vector");
  return __builtin_bit_cast(V, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off, soff, 16));
}
// WT: sc1 = written through to memory (placement-independent groups); otherwise a plain store that stays in this XCD's L2
template <bool WT, typename V>
__device__ __forceinline__ void store_b128(__amdgpu_buffer_rsrc_t rsrc, int byte_off, const V& v, int soff = 0) {
  static_assert(sizeof(V) == 16, "a 16-byte vector");
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc, byte_off, soff, WT ? 16 : 0);
}

}  // namespace csn

// ---- diagnostic builds (`make diag`, tools/persist_bench.hip): per-phase wall-clock sums of ONE workgroup's thread 0.
// CSN_HANDOFF_STAMP(g_pstamps, CSN_STAMP_BLOCK, i) adds the ticks since the last stamp to g_pstamps[i]; the kernel
// provides `tid` and a running `unsigned long long last_`.
#ifdef CSN_PSTAMPS
#ifndef CSN_STAMP_BLOCK
#define CSN_STAMP_BLOCK 11     // group 3 (layer 0 at cfg2), slice 1; 15 = group 7 (layer 1)
#endif
#define CSN_HANDOFF_STAMP(stamps, wg, i)                                       \
  do {                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                         \
    if (tid == 0 && blockIdx.x == (wg)) {                                      \
      const unsigned long long now_ = wall_clock64();                          \
      atomicAdd(&stamps[i], now_ - last_);                                     \
      last_ = now_;                                                            \
    }                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                         \
  } while (0)
#else
#define CSN_HANDOFF_STAMP(stamps, wg, i)
#endif
