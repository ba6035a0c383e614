// Row table and wave fence shared by the batched decode attention modules
// (decode_attn_batched.hip: bf16 caches, decode_attn_fp8.hip: e4m3 caches).
#pragma once

#include "common.h"

// len, start and slot of a row from the device tables; len = 0 is "empty".
struct DbRow {
  int len, start, slot;
};

DEV_INLINE DbRow db_row(const int* __restrict__ lengths,
                        const int* __restrict__ slots, int row, int S,
                        int max_len, int window) {
  const int len = min(lengths[row], max_len);
  const int slot = slots[row];
  const bool ok = len > 0 && slot >= 0 && slot < S;
  DbRow r;
  r.len = ok ? len : 0;
  r.slot = ok ? slot : 0;
  r.start = (ok && window > 0) ? max(0, len - window) : 0;
  return r;
}

// Orders the wave's own LDS writes and reads of its V image against each
// other (the lanes exchange data); LDS operations of one wave execute in
// order, so no instruction is needed, only the compiler must not move them.
DEV_INLINE void db_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
