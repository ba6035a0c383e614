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

// The decode prologue (decode_prologue.hip): per-row RoPE of q and k and the
// cache write of k and v, one launch for the n*T rows of the packed qkv
// [n, T, G, qpg+2, d] (slots 0..qpg-1 of a group its q heads, qpg k, qpg+1
// v).  Token t of row i sits at p = lengths[i] - q_lens[i] + t and is live
// when t < q_lens[i], slots[i] is in [0, S) and 0 <= p < lim, where lim is
// min(rows of cos/sin, positions of a cache row or of a table row's pages),
// set by the caller.  q [n, T, G*qpg, d] gets the rotated heads of a live
// token and zeros otherwise; a live token's rotated k and its v go to
// cache[slots[i], p] (contiguous) or to pool[table[slots[i], p >> lg],
// p & (page - 1)], nowhere when that page id is outside [0, P).  cos, sin:
// fp32 [rows, d/2], both null for no rotation.  Caches, scales, table, S,
// max_s, max_pages, lg and P as in DecodeBatchedArgs with hkv = G; d is 64 or
// 128.
struct DecodePrologueArgs {
  const __bf16* qkv;
  const float* cos;
  const float* sin;
  bool interleaved;          // pairs (2m, 2m+1), not (m, m + d/2)
  const int* lengths;
  const int* q_lens;
  const int* slots;
  const int* table;
  __bf16* q;
  void* k_cache;
  void* v_cache;
  bool fp8;
  const float* k_scale;
  const float* v_scale;
  int n, T, G, qpg, d;
  int lim;
  int S;
  int max_s;                 // contiguous only
  int max_pages, lg, P;      // paged only
};

void decode_prologue_launch(const DecodePrologueArgs& a, hipStream_t st);
