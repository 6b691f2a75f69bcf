// Device-side memory access shared by the kernels (gfx950): address-space pointer types, loads / stores / LDS-DMA through a raw buffer
// descriptor, and the s_waitcnt forms the kernels use.  One definition each; every kernel file takes them from here.
#pragma once
#include "crg_common.h"

namespace crg_buf {

typedef const __attribute__((address_space(1))) void* gptr_t;  // global pointer operand of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr_t;        // LDS pointer operand of the LDS-DMA builtins
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Word 3 of the raw buffer descriptor (V#): DATA_FORMAT = 4 (one 32-bit component, bits 15-18) and nothing else - stride 0, no swizzle,
// no index: raw byte offsets with the range check on - a lane whose offset lies outside [0, bytes) loads zeros and its store is dropped.
constexpr int BUF_RSRC_FLAGS = 0x00020000;

// One LDS-DMA piece through a raw buffer descriptor: lane -> 16 bytes at base + voff + soff, zeros when out of [0, bytes).
__device__ __forceinline__ void buf_dma16(const void* base, unsigned bytes, char* lds, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, BUF_RSRC_FLAGS);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lptr_t)lds, 16, voff, soff, 0, 0);
#endif
}

// Stores through a buffer descriptor: an out-of-range lane (offset forced past the end) is DROPPED by the range check, so the store
// INSTRUCTION COUNT per wave is a compile-time constant whatever the tails are - which is what lets counted vmcnt waits leave exactly
// these stores in flight (vmcnt counts stores on gfx950).
__device__ __forceinline__ void buf_store16(void* base, unsigned bytes, int voff, const bf16x8& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, BUF_RSRC_FLAGS);
  u32x4 r;
  __builtin_memcpy(&r, &v, 16);
  __builtin_amdgcn_raw_buffer_store_b128(r, rs, voff, 0, 0);
#endif
}
// DROP: timing ablation only (CRG_LN_ABL_NOSTORE / CRG_RG_ABL_NOSTORE of the calling file): the store goes out of range - dropped by the
// range check, still issued and counted in vmcnt
template <bool DROP = false>
__device__ __forceinline__ void buf_store8(void* base, unsigned bytes, int voff, const bf16x4& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, BUF_RSRC_FLAGS);
  u32x2 r;
  __builtin_memcpy(&r, &v, 8);
  if constexpr (DROP) voff = (int)0x80000000;
  __builtin_amdgcn_raw_buffer_store_b64(r, rs, voff, 0, 0);
#endif
}
__device__ __forceinline__ void buf_store2(void* base, unsigned bytes, int voff, bf16 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, BUF_RSRC_FLAGS);
  short r;
  __builtin_memcpy(&r, &v, 2);
  __builtin_amdgcn_raw_buffer_store_b16(r, rs, voff, 0, 0);
#endif
}
__device__ __forceinline__ bf16x8 buf_load16(const void* base, unsigned bytes, int voff) {
  bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, BUF_RSRC_FLAGS);
  const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
  __builtin_memcpy(&v, &r, 16);
#endif
  return v;
}
__device__ __forceinline__ bf16x4 buf_load8(const void* base, unsigned bytes, int voff) {
  bf16x4 v = {0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, BUF_RSRC_FLAGS);
  const u32x2 r = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 0, 0);
  __builtin_memcpy(&v, &r, 8);
#endif
  return v;
}

// s_waitcnt (gfx9 encoding): vmcnt in bits 0-3 and 14-15, expcnt in bits 4-6, lgkmcnt in bits 8-11; a field at its maximum does not wait.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {  // s_waitcnt vmcnt(N) only (expcnt / lgkmcnt fields left at "no wait")
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}
__device__ __forceinline__ void wait_vmcnt0() { wait_vmcnt<0>(); }  // s_waitcnt vmcnt(0) only: every vector-memory access of the wave has returned
__device__ __forceinline__ void wait_lgkmcnt0() {  // s_waitcnt lgkmcnt(0) only (0xc07f): every LDS / scalar-memory access of the wave has returned
  __builtin_amdgcn_s_waitcnt(15 | (3 << 14) | (7 << 4) | (0 << 8));
}

}  // namespace crg_buf
