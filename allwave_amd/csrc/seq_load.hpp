// seq_load.hpp -- how a record kernel reads the bases a lane's columns touch (cs.hip): a lane's 16 columns consume at
// most 16 consecutive bytes of a sequence, read as five aligned dwords and shifted into place.
#pragma once

#include "planner_device.hpp"  // SEQ_PAD_BYTES
#include "wave_ops.hpp"        // u32x4

namespace awvw {

// 16 bytes of a sequence of `len` bytes from position `pos` on: five aligned dwords, shifted into place.  Dwords that start at or
// behind the sequence's end are not read (their bytes are 0); a dword that starts inside it ends at most 3 bytes behind it, inside
// the engine's padding.
static_assert(awp::SEQ_PAD_BYTES >= 3, "load16 reads whole dwords that start inside a sequence: the layout must pad every sequence by 3 bytes or more");
__device__ __forceinline__ u32x4 load16(const uint8_t* seq, int len, int pos) {
  const uintptr_t addr = (uintptr_t)seq + (uintptr_t)pos, end = (uintptr_t)seq + (uintptr_t)max(len, 0);
  const unsigned* a = (const unsigned*)(addr & ~(uintptr_t)3);
  const unsigned s = (unsigned)(addr & 3);
  unsigned d[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) d[k] = (uintptr_t)(a + k) < end ? a[k] : 0u;
  u32x4 x;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], s);
  return x;
}

}  // namespace awvw
