// Batched decode attention on a paged KV cache, bf16 and e4m3 pools (serving
// path, gfx950).
//
//   q [n, hq, D] bf16, pools [P, page, hkv, D] bf16 or e4m3 bytes, o [n, hq, D]
//   page_table: int32 [S, max_pages]; lengths, slots: int32 [n]; all in
//   device memory.  slots[i] is a row of the table.  Position p of q row i is
//   pool[page_table[slots[i], p >> lg(page)], p & (page - 1)]; page is a
//   power of two >= 32.
//
// Row contract, grid (n_chunks, hkv, n) from host arguments alone, empty
// rows, work split, per-step arithmetic, combine, split-KV and merge are
// those of decode_attn_batched.hip and decode_attn_fp8.hip: the two kernels
// here instantiate the same chunk bodies (decode_batched_body.h,
// decode_fp8_body.h) with the paged addressing tag.  What differs:
//
// Steps on the absolute 32-key grid.  A wave step covers keys [k0, k0 + 32)
// with k0 % 32 == 0 in absolute positions and 32 | page, so a step lies in
// one page: one page id per wave step, a wave-uniform value read with a
// scalar load, no per-lane lookup.  A row's first tile starts at
// a0 = start_i & ~31 and chunk c covers [a0 + c chunk, a0 + (c + 1) chunk)
// cut to [start_i, len_i); the merge counts a row's chunks from a0 as well
// and the host sizes chunk * n_chunks >= window + 31.  Without a window
// a0 = start_i = 0: chunks, tiles and the order of accumulation are those of
// the contiguous kernels, and so are the bits of the result.
//
// Lower edge.  Only the step that contains start_i has keys below it.  It
// takes the bounded load path, which clamps row addresses into
// [start_i, p1), zeroes V by value and scores -1e30 on both sides.  A step
// with start_i <= k0 and k0 + 32 <= p1 has no bounds checks in its loads.
//
// Lookups ahead of the loads.  The K and V loads of step k0 + 128 are issued
// in the middle of step k0, and their base depends on a table entry.  A wave
// holds the ids of its current and next step in scalar registers and reads
// the id of step k0 + 256 at the top of step k0, a full step before the
// loads that use it.
//
// An id outside [0, P) skips its step: nothing is loaded or staged, no
// address is formed, and the step adds nothing to the wave's max, sum or O.
// A row all of whose attended pages are invalid sums to l = 0 and is written
// as zeros.
#include "common.h"

#include <stdint.h>

// Packed fp32 instructions are kept out of this module's device code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif
#include "decode_batched_body.h"
#include "decode_fp8_body.h"

namespace {

template <int D>
__global__ __launch_bounds__(256) void decode_paged_kernel(
    const __bf16* __restrict__ q,    // [n, hq, D]
    const __bf16* __restrict__ kc,   // [P, page, hkv, D]
    const __bf16* __restrict__ vc,
    __bf16* __restrict__ o,          // [n, hq, D]
    float* __restrict__ part,        // [n*hq, n_chunks, D+2]; null: write o
    const int* __restrict__ table,   // [S, max_pages]
    const int* __restrict__ lengths, const int* __restrict__ slots, int hq,
    int hkv, int S, int max_pages, int lg, int P, int max_len, int window,
    int chunk, float scale) {
  db_chunk<D>(q, kc, vc, o, part, lengths, slots,
              DbPaged{table, max_pages, lg, P}, hq, hkv, S, max_len, window,
              chunk, scale);
}

template <int D>
__global__ __launch_bounds__(256) void decode_paged_fp8_kernel(
    const __bf16* __restrict__ q,    // [n, hq, D]
    const uint8_t* __restrict__ kc,  // [P, page, hkv, D] e4m3
    const uint8_t* __restrict__ vc,
    const float* __restrict__ k_scale,   // [hkv] or null
    const float* __restrict__ v_scale,
    __bf16* __restrict__ o,          // [n, hq, D]
    float* __restrict__ part,        // [n*hq, n_chunks, D+2]; null: write o
    const int* __restrict__ table,   // [S, max_pages]
    const int* __restrict__ lengths, const int* __restrict__ slots, int hq,
    int hkv, int S, int max_pages, int lg, int P, int max_len, int window,
    int chunk, float scale) {
  f8_chunk<D>(q, kc, vc, k_scale, v_scale, o, part, lengths, slots,
              DbPaged{table, max_pages, lg, P}, hq, hkv, S, max_len, window,
              chunk, scale);
}

// One block of D threads per (row, q head): log-sum-exp merge of the chunks
// this row has, counted from the row's first tile; the others were never
// written.  v_scale is null for bf16 pools.  A row without a valid page has
// l = 0 in every chunk and is written as zeros.
template <int D>
__global__ void decode_paged_merge_kernel(
    const float* __restrict__ part, const float* __restrict__ v_scale,
    __bf16* __restrict__ o, const int* __restrict__ lengths,
    const int* __restrict__ slots, int hq, int hkv, int S, int max_len,
    int window, int chunk, int n_chunks) {
  const int bh = blockIdx.x, tid = threadIdx.x;
  const DbRow r = db_row(lengths, slots, bh / hq, S, max_len, window);
  if (r.len == 0) {
    o[(long)bh * D + tid] = (__bf16)0.f;
    return;
  }
  const int nch = min(
      (r.len - db_grid_start<DbPaged>(r) + chunk - 1) / chunk, n_chunks);
  const float* base = part + (long)bh * n_chunks * (D + 2);
  float gm = DB_NEG;
  for (int ci = 0; ci < nch; ++ci) gm = fmaxf(gm, base[ci * (D + 2) + D]);
  float gl = 0.f, acc = 0.f;
  for (int ci = 0; ci < nch; ++ci) {
    const float f = __expf(base[ci * (D + 2) + D] - gm);
    gl += f * base[ci * (D + 2) + D + 1];
    acc += f * base[ci * (D + 2) + tid];
  }
  if (gl == 0.f) gl = 1.f;
  float res = acc / gl;
  if (v_scale) res *= v_scale[(bh % hq) / (hq / hkv)];
  o[(long)bh * D + tid] = (__bf16)res;
}

struct PagedArgs {
  const int* table;
  const int* lengths;
  const int* slots;
  int n, hq, hkv, S, max_pages, lg, P, max_len, window, chunk, n_chunks;
  float scale;
};

template <int D>
void launch(const __bf16* q, const void* kc, const void* vc,
            const float* k_scale, const float* v_scale, bool fp8, __bf16* o,
            float* part, const PagedArgs& a, hipStream_t st) {
  const dim3 grid(a.n_chunks, a.hkv, a.n);
  float* pp = a.n_chunks > 1 ? part : nullptr;
  if (fp8)
    hipLaunchKernelGGL((decode_paged_fp8_kernel<D>), grid, dim3(256), 0, st, q,
                       static_cast<const uint8_t*>(kc),
                       static_cast<const uint8_t*>(vc), k_scale, v_scale, o,
                       pp, a.table, a.lengths, a.slots, a.hq, a.hkv, a.S,
                       a.max_pages, a.lg, a.P, a.max_len, a.window, a.chunk,
                       a.scale);
  else
    hipLaunchKernelGGL((decode_paged_kernel<D>), grid, dim3(256), 0, st, q,
                       static_cast<const __bf16*>(kc),
                       static_cast<const __bf16*>(vc), o, pp, a.table,
                       a.lengths, a.slots, a.hq, a.hkv, a.S, a.max_pages,
                       a.lg, a.P, a.max_len, a.window, a.chunk, a.scale);
  if (a.n_chunks > 1)
    hipLaunchKernelGGL((decode_paged_merge_kernel<D>), dim3(a.n * a.hq),
                       dim3(D), 0, st, part, fp8 ? v_scale : nullptr, o,
                       a.lengths, a.slots, a.hq, a.hkv, a.S, a.max_len,
                       a.window, a.chunk, a.n_chunks);
}

}  // namespace

int decode_paged_tile() {
  static_assert(DB_TILE == F8_TILE, "one split for both pool dtypes");
  return DB_TILE;
}

// Pools [P, 1 << lg, hkv, d], bf16 (fp8 false; the scales are unused) or
// e4m3 bytes; table int32 [S, max_pages].  chunk is a multiple of
// decode_paged_tile() with chunk * n_chunks >= the longest row's tiles from
// its first 32-key boundary (window + 31 with a window); part is
// [n*hq, n_chunks, d+2] fp32 (unused, may be null, when n_chunks == 1).
void decode_attn_paged_launch(const __bf16* q, const void* kc, const void* vc,
                              const float* k_scale, const float* v_scale,
                              bool fp8, __bf16* o, float* part,
                              const int* table, const int* lengths,
                              const int* slots, int n, int hq, int hkv, int S,
                              int max_pages, int lg, int P, int max_len,
                              int window, int chunk, int n_chunks, int d,
                              float scale, hipStream_t st) {
  const PagedArgs a{table, lengths, slots, n, hq, hkv, S, max_pages, lg, P,
                    max_len, window, chunk, n_chunks, scale};
  if (d == 64)
    launch<64>(q, kc, vc, k_scale, v_scale, fp8, o, part, a, st);
  else
    launch<128>(q, kc, vc, k_scale, v_scale, fp8, o, part, a, st);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif
