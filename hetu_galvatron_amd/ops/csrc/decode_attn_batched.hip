// Batched single-token decode attention for gfx950 (serving path): bf16 and
// e4m3 KV caches, contiguous or paged.  The four kernels are one chunk body
// (decode_body.h, where the design is described) under a cache format tag
// and an addressing tag (decode_rows.h).  What the paged kernels add:
//
//   page_table: int32 [S, max_pages] in device memory; slots[i] is a row of
//   the table.  Position p of q row i is
//   pool[page_table[slots[i], p >> lg(page)], p & (page - 1)]; page is a
//   power of two >= 32.
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
#include "decode_launch.h"

// Packed fp32 instructions are kept out of this module's device code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif
#include "decode_body.h"

namespace {

template <int D>
__global__ __launch_bounds__(256) void decode_batched_kernel(
    const __bf16* __restrict__ q,    // [n, hq, D]
    const __bf16* __restrict__ kc,   // [S, max_s, hkv, D]
    const __bf16* __restrict__ vc,
    __bf16* __restrict__ o,          // [n, hq, D]
    float* __restrict__ part,        // [n*hq, n_chunks, D+2]; null: write o
    const int* __restrict__ lengths, const int* __restrict__ slots, int hq,
    int hkv, int S, int max_s, int max_len, int window, int chunk,
    float scale) {
  decode_chunk<D>(q, kc, vc, DbBf16{}, o, part, lengths, slots,
                  DbContig{max_s}, hq, hkv, S, max_len, window, chunk, scale);
}

template <int D>
__global__ __launch_bounds__(256) void decode_batched_fp8_kernel(
    const __bf16* __restrict__ q,    // [n, hq, D]
    const uint8_t* __restrict__ kc,  // [S, max_s, hkv, D] e4m3
    const uint8_t* __restrict__ vc,
    const float* __restrict__ k_scale,   // [hkv] or null
    const float* __restrict__ v_scale,
    __bf16* __restrict__ o,          // [n, hq, D]
    float* __restrict__ part,        // [n*hq, n_chunks, D+2]; null: write o
    const int* __restrict__ lengths, const int* __restrict__ slots, int hq,
    int hkv, int S, int max_s, int max_len, int window, int chunk,
    float scale) {
  decode_chunk<D>(q, kc, vc, DbE4m3{k_scale, v_scale}, o, part, lengths,
                  slots, DbContig{max_s}, hq, hkv, S, max_len, window, chunk,
                  scale);
}

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
  decode_chunk<D>(q, kc, vc, DbBf16{}, o, part, lengths, slots,
                  DbPaged{table, max_pages, lg, P}, hq, hkv, S, max_len,
                  window, chunk, scale);
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
  decode_chunk<D>(q, kc, vc, DbE4m3{k_scale, v_scale}, o, part, lengths,
                  slots, DbPaged{table, max_pages, lg, P}, hq, hkv, S,
                  max_len, window, chunk, scale);
}

template <int D>
void launch(const DecodeBatchedArgs& a, hipStream_t st) {
  const dim3 grid(a.n_chunks, a.hkv, a.n), block(256);
  float* part = a.n_chunks > 1 ? a.part : nullptr;
  const __bf16* kb = static_cast<const __bf16*>(a.k_cache);
  const __bf16* vb = static_cast<const __bf16*>(a.v_cache);
  const uint8_t* k8 = static_cast<const uint8_t*>(a.k_cache);
  const uint8_t* v8 = static_cast<const uint8_t*>(a.v_cache);
  if (a.table && a.fp8)
    hipLaunchKernelGGL((decode_paged_fp8_kernel<D>), grid, block, 0, st, a.q,
                       k8, v8, a.k_scale, a.v_scale, a.o, part, a.table,
                       a.lengths, a.slots, a.hq, a.hkv, a.S, a.max_pages,
                       a.lg, a.P, a.max_len, a.window, a.chunk, a.scale);
  else if (a.table)
    hipLaunchKernelGGL((decode_paged_kernel<D>), grid, block, 0, st, a.q, kb,
                       vb, a.o, part, a.table, a.lengths, a.slots, a.hq,
                       a.hkv, a.S, a.max_pages, a.lg, a.P, a.max_len,
                       a.window, a.chunk, a.scale);
  else if (a.fp8)
    hipLaunchKernelGGL((decode_batched_fp8_kernel<D>), grid, block, 0, st,
                       a.q, k8, v8, a.k_scale, a.v_scale, a.o, part,
                       a.lengths, a.slots, a.hq, a.hkv, a.S, a.max_s,
                       a.max_len, a.window, a.chunk, a.scale);
  else
    hipLaunchKernelGGL((decode_batched_kernel<D>), grid, block, 0, st, a.q,
                       kb, vb, a.o, part, a.lengths, a.slots, a.hq, a.hkv,
                       a.S, a.max_s, a.max_len, a.window, a.chunk, a.scale);
  if (a.n_chunks == 1) return;
  const float* vs = a.fp8 ? a.v_scale : nullptr;
  if (a.table)
    hipLaunchKernelGGL((decode_merge_kernel<D, DbPaged>), dim3(a.n * a.hq),
                       dim3(D), 0, st, a.part, vs, a.o, a.lengths, a.slots,
                       a.hq, a.hkv, a.S, a.max_len, a.window, a.chunk,
                       a.n_chunks);
  else
    hipLaunchKernelGGL((decode_merge_kernel<D, DbContig>), dim3(a.n * a.hq),
                       dim3(D), 0, st, a.part, vs, a.o, a.lengths, a.slots,
                       a.hq, a.hkv, a.S, a.max_len, a.window, a.chunk,
                       a.n_chunks);
}

}  // namespace

int decode_batched_tile() { return DB_TILE; }

void decode_batched_launch(const DecodeBatchedArgs& a, hipStream_t st) {
  if (a.d == 64)
    launch<64>(a, st);
  else
    launch<128>(a, st);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif
