// Batched single-token decode attention for gfx950 (serving path).
//
//   q [n, hq, D] bf16, caches [S, max_s, hkv, D] bf16, o [n, hq, D] bf16
//   lengths, slots: int32 [n] in device memory.  Row i attends to positions
//   [start_i, len_i) of cache row slots[i]; len_i = min(lengths[i], max_len),
//   start_i = max(0, len_i - window) (0 without a window).
//
// Nothing is read back: the grid is (n_chunks, hkv, n) from host arguments
// alone, so a captured graph replays after lengths and slots change in place.
// A row with len_i <= 0 or a slot outside [0, S) is empty: its o row is
// zeros and no address is formed from it.
//
// One 256-thread workgroup per (row, kv head, chunk) serves all qpg = hq/hkv
// (<= 16) query heads of the group, so every K and V row is fetched once per
// group.  The four waves are independent: wave w takes keys 32w .. 32w+31 of
// every 128-key tile of the chunk, keeps its own online softmax and meets
// the others once, after the last tile, in LDS.  Per 32-key step of a wave
// (v_mfma_f32_16x16x32_bf16; lane l: g = l >> 4, c = l & 15):
//
//   S^T[keys x heads] = K . Q^T   two 16-key blocks x D/32 k-steps.  The A
//       fragment is 8 contiguous bf16 of key row 16*blk + c, straight from
//       global memory with a 16-byte load; the B fragment is q of head c
//       (zero for c >= qpg), held in registers.  D layout: register r of
//       block blk is key 16*blk + 4g + r of head c, so a lane's scores
//       belong to one head and the running max and sum are per-lane scalars;
//       the tile max is combined across the four 16-lane groups, the sum
//       only once at the end.
//   O^T[d x heads] += V^T . P^T   D/16 row blocks.  The sum over keys does
//       not depend on the order, so k-slot 8g + j of the product is key
//       4g + j (j < 4) or 16 + 4g + j - 4: the P^T fragment is then the
//       lane's own eight weights.  V^T is read with that same map by two
//       ds_read_b64_tr_b16 per row block from the wave's own LDS image of
//       its 32 V rows (staged by rows with 16-byte loads, row stride D + 16
//       elements: the four rows of a 16-lane group are 32 B apart modulo
//       256, so the reads do not collide).
//
// The weights enter the second product as three bf16 terms (p = hi + lo +
// lo2, each the rounding of what the ones before left over): one bf16 term
// alone is a relative error of 2^-9 per weight, which the decode element
// rule (ulp of o plus 2^-20 of the absolute-value sum) does not allow where
// the weighted V rows cancel.  MFMA work is far below the memory time, so the
// two extra products are free.
//
// The next step's K fragments and V rows are loaded into registers after the
// first product of the current one, before its softmax and second product.
// Only a step that reaches past the chunk's end clamps its row addresses and
// selects zeros for V and -1e30 for the scores.
//
// LDS is a constant of the tile (4 x 32 x (D + 16) bf16 + 512 B), reused for
// the final combine of the waves.  With n_chunks > 1 every non-empty chunk
// writes an unnormalised partial [D] + (m, l) in fp32 and the merge kernel
// reads, per row, only the chunks that row has.
#include "common.h"

// Packed fp32 instructions are kept out of this module's device code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif
#include "decode_batched_body.h"

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
  db_chunk<D>(q, kc, vc, o, part, lengths, slots, DbContig{max_s}, hq, hkv,
              S, max_len, window, chunk, scale);
}

// One block of D threads per (row, q head): log-sum-exp merge of the chunks
// this row has, counted from its own length; the others were never written.
template <int D>
__global__ void decode_batched_merge_kernel(
    const float* __restrict__ part, __bf16* __restrict__ o,
    const int* __restrict__ lengths, const int* __restrict__ slots, int hq,
    int S, int max_len, int window, int chunk, int n_chunks) {
  const int bh = blockIdx.x, tid = threadIdx.x;
  const DbRow r = db_row(lengths, slots, bh / hq, S, max_len, window);
  if (r.len == 0) {
    o[(long)bh * D + tid] = (__bf16)0.f;
    return;
  }
  const int nch = min((r.len - r.start + chunk - 1) / chunk, n_chunks);
  const float* base = part + (long)bh * n_chunks * (D + 2);
  float gm = DB_NEG;
  for (int ci = 0; ci < nch; ++ci) gm = fmaxf(gm, base[ci * (D + 2) + D]);
  float gl = 0.f, acc = 0.f;
  for (int ci = 0; ci < nch; ++ci) {
    const float f = __expf(base[ci * (D + 2) + D] - gm);
    gl += f * base[ci * (D + 2) + D + 1];
    acc += f * base[ci * (D + 2) + tid];
  }
  o[(long)bh * D + tid] = (__bf16)(acc / gl);
}

template <int D>
void launch(const __bf16* q, const __bf16* kc, const __bf16* vc, __bf16* o,
            float* part, const int* lengths, const int* slots, int n, int hq,
            int hkv, int S, int max_s, int max_len, int window, int chunk,
            int n_chunks, float scale, hipStream_t st) {
  hipLaunchKernelGGL((decode_batched_kernel<D>), dim3(n_chunks, hkv, n),
                     dim3(256), 0, st, q, kc, vc, o,
                     n_chunks > 1 ? part : nullptr, lengths, slots, hq, hkv,
                     S, max_s, max_len, window, chunk, scale);
  if (n_chunks > 1)
    hipLaunchKernelGGL((decode_batched_merge_kernel<D>), dim3(n * hq),
                       dim3(D), 0, st, part, o, lengths, slots, hq, S,
                       max_len, window, chunk, n_chunks);
}

}  // namespace

int decode_batched_tile() { return DB_TILE; }

// chunk is a multiple of decode_batched_tile() with chunk * n_chunks >= the
// longest window; part is [n*hq, n_chunks, d+2] fp32 (unused, may be null,
// when n_chunks == 1).
void decode_attn_batched_launch(const __bf16* q, const __bf16* kc,
                                const __bf16* vc, __bf16* o, float* part,
                                const int* lengths, const int* slots, int n,
                                int hq, int hkv, int S, int max_s,
                                int max_len, int window, int chunk,
                                int n_chunks, int d, float scale,
                                hipStream_t st) {
  if (d == 64)
    launch<64>(q, kc, vc, o, part, lengths, slots, n, hq, hkv, S, max_s,
               max_len, window, chunk, n_chunks, scale, st);
  else
    launch<128>(q, kc, vc, o, part, lengths, slots, n, hq, hkv, S, max_s,
                max_len, window, chunk, n_chunks, scale, st);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif
