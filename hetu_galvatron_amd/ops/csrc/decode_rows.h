// Row table, addressing tags and wave fence of batched decode attention: the
// chunk body and the merge kernel (decode_body.h), instantiated by
// decode_attn_batched.hip for bf16 and e4m3 caches, contiguous and paged.
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

// Where a row's keys live: the addressing tag of the chunk body
// (decode_body.h).  The kernel fills in what it was launched with; the body
// binds the tag to its row's slot.  Contiguous:
// one cache row of max_s positions, base() is the element offset of
// (slot, position 0, head hk).
struct DbContig {
  static constexpr bool paged = false;
  int max_s;
  DEV_INLINE void bind(int) {}
  DEV_INLINE long base(int slot, int hkv, int hk, int d) const {
    return ((long)slot * max_s * hkv + hk) * d;
  }
};

// Paged: position p is row p & (page - 1) of pool page trow[p >> lg].  A
// wave step is 32 keys on the absolute 32-key grid and 32 | page, so a step
// has one page id, a wave-uniform value.
struct DbPaged {
  static constexpr bool paged = true;
  const int* __restrict__ trow;      // the table; bound: the slot's row
  int max_pages, lg, P;              // table columns, log2(page), pool pages
  DEV_INLINE void bind(int slot) { trow += (long)slot * max_pages; }
  // element offset of head hk in a pool row
  DEV_INLINE long base(int, int, int hk, int d) const { return (long)hk * d; }
  DEV_INLINE int page_id(int k0) const { return trow[k0 >> lg]; }
  DEV_INLINE bool ok(int id) const { return (unsigned)id < (unsigned)P; }
  // pool row of position k0 in page id
  DEV_INLINE long pool_row(int id, int k0) const {
    return ((long)id << lg) + (k0 & ((1 << lg) - 1));
  }
};

// First position of a row's tile grid and the chunks the row has: the
// contiguous kernels start at r.start, the paged ones on the 32-key grid.
template <class A>
DEV_INLINE int db_grid_start(const DbRow& r) {
  return A::paged ? (r.start & ~31) : r.start;
}

// Orders the wave's own LDS writes and reads of its V image against each
// other (the lanes exchange data); LDS operations of one wave execute in
// order, so no instruction is needed, only the compiler must not move them.
DEV_INLINE void db_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
