// Host launchers of the batched decode modules, declared once:
// decode_attn_batched.hip and decode_attn_fp8.hip include this next to their
// definitions and bindings.hip next to its calls, so a definition and a call
// cannot drift apart.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

// One batched decode call.  Row i of q [n, hq, d] attends to positions
// [max(0, len_i - window), len_i), len_i = min(lengths[i], max_len), of row
// slots[i] of
//   table == null: the caches [S, max_s, hkv, d];
//   otherwise: the int32 table [S, max_pages] over pools [P, 1 << lg, hkv, d].
// The caches are bf16, or e4m3 bytes (fp8) with real = stored * scale[h];
// either scale may be null (ones) and both are unused for bf16.  chunk is a
// multiple of decode_batched_tile() with chunk * n_chunks >= the longest
// row's tiles (paged with a window: from its first 32-key boundary, window +
// 31); part is [n*hq, n_chunks, d+2] fp32 (unused, may be null, when
// n_chunks == 1).  d is 64 or 128.
struct DecodeBatchedArgs {
  const __bf16* q;
  const void* k_cache;
  const void* v_cache;
  bool fp8;
  const float* k_scale;
  const float* v_scale;
  const int* table;
  const int* lengths;
  const int* slots;
  const int* q_lens;         // multi-token only
  __bf16* o;
  float* part;
  int n, hq, hkv, d;
  int T;                     // multi-token only: query tokens per row
  int S;
  int max_s;                 // contiguous only
  int max_pages, lg, P;      // paged only
  int max_len, window, chunk, n_chunks;
  float scale;
};

int decode_batched_tile();
void decode_batched_launch(const DecodeBatchedArgs& a, hipStream_t st);

// The multi-token call (decode_attn_multi.hip): q and o are [n, T, hq, d],
// T <= 16, and q_lens int32 [n] counts each row's real tokens.  Token
// t < q_lens[i] sits at pos = lengths[i] - q_lens[i] + t and attends to
// [max(0, pos + 1 - window), pos]; lengths[i] must lie in (0, max_len] or the
// row is empty.  With a window the split covers window + T - 1 positions
// (paged: + 31); part is [n*T*hq, n_chunks, d+2].  decode_multi_groups: the
// workgroups per (row, kv head, chunk), one per 16 or 32 columns of the
// T * hq / hkv.
int decode_multi_groups(int T, int hq, int hkv);
void decode_multi_launch(const DecodeBatchedArgs& a, hipStream_t st);

// The prefill-shaped call (decode_attn_prefill.hip): the multi-token call's
// arguments and semantics for any T >= 1, chunks and part included.
// decode_prefill_groups: the workgroups per (row, kv head, chunk), one per
// 128 columns of the T * hq / hkv.
int decode_prefill_groups(int T, int hq, int hkv);
void decode_prefill_launch(const DecodeBatchedArgs& a, hipStream_t st);

// k, v: [n, hkv, d] bf16 with row and head strides in elements (multiples of
// 8, 16-byte aligned bases) and a contiguous last dim; d is 64 or 128.
void kv_append_fp8_launch(const __bf16* k, const __bf16* v, long k_rs,
                          long k_hs, long v_rs, long v_hs, uint8_t* kc,
                          uint8_t* vc, const float* k_scale,
                          const float* v_scale, const int* slots,
                          const int* positions, int n, int hkv, int d, int S,
                          int max_s, hipStream_t st);
