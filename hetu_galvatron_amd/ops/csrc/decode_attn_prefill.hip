// Cache-reading prefill attention for gfx950 (chunked prefill on the serving
// caches): T > 16 consecutive query tokens of a row against that row's bf16
// or e4m3 cache, contiguous or paged.  The kernels are one chunk body
// (decode_prefill_body.h, where the design is described) under the format and
// addressing tags of the decode kernels, 128 (token, head) columns per
// workgroup; split-KV partials are merged by decode_multi_merge_kernel.
#include "common.h"
#include "decode_launch.h"
#include "decode_prefill_body.h"

namespace {

template <int D>
__global__ __launch_bounds__(256) void decode_prefill_kernel(
    const __bf16* __restrict__ q,    // [n, T, hq, D]
    const __bf16* __restrict__ kc,   // [S, max_s, hkv, D]
    const __bf16* __restrict__ vc,
    __bf16* __restrict__ o,          // [n, T, hq, D]
    float* __restrict__ part,        // [n*T*hq, n_chunks, D+2]; null: write o
    const int* __restrict__ lengths, const int* __restrict__ q_lens,
    const int* __restrict__ slots, int T, int hq, int hkv, int nct, int S,
    int max_s, int max_len, int window, int chunk, float scale) {
  decode_prefill_chunk<D, DbBf16, DbContig>(
      q, kc, vc, DbBf16{}, o, part, lengths, q_lens, slots, DbContig{max_s},
      T, hq, hkv, nct, S, max_len, window, chunk, scale);
}

template <int D>
__global__ __launch_bounds__(256) void decode_prefill_fp8_kernel(
    const __bf16* __restrict__ q, const uint8_t* __restrict__ kc,
    const uint8_t* __restrict__ vc,
    const float* __restrict__ k_scale,   // [hkv] or null
    const float* __restrict__ v_scale, __bf16* __restrict__ o,
    float* __restrict__ part, const int* __restrict__ lengths,
    const int* __restrict__ q_lens, const int* __restrict__ slots, int T,
    int hq, int hkv, int nct, int S, int max_s, int max_len, int window,
    int chunk, float scale) {
  decode_prefill_chunk<D, DbE4m3, DbContig>(
      q, kc, vc, DbE4m3{k_scale, v_scale}, o, part, lengths, q_lens, slots,
      DbContig{max_s}, T, hq, hkv, nct, S, max_len, window, chunk, scale);
}

template <int D>
__global__ __launch_bounds__(256) void decode_prefill_paged_kernel(
    const __bf16* __restrict__ q,
    const __bf16* __restrict__ kc,   // [P, page, hkv, D]
    const __bf16* __restrict__ vc, __bf16* __restrict__ o,
    float* __restrict__ part,
    const int* __restrict__ table,   // [S, max_pages]
    const int* __restrict__ lengths, const int* __restrict__ q_lens,
    const int* __restrict__ slots, int T, int hq, int hkv, int nct, int S,
    int max_pages, int lg, int P, int max_len, int window, int chunk,
    float scale) {
  decode_prefill_chunk<D, DbBf16, DbPaged>(
      q, kc, vc, DbBf16{}, o, part, lengths, q_lens, slots,
      DbPaged{table, max_pages, lg, P}, T, hq, hkv, nct, S, max_len, window,
      chunk, scale);
}

template <int D>
__global__ __launch_bounds__(256) void decode_prefill_paged_fp8_kernel(
    const __bf16* __restrict__ q, const uint8_t* __restrict__ kc,
    const uint8_t* __restrict__ vc, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, __bf16* __restrict__ o,
    float* __restrict__ part, const int* __restrict__ table,
    const int* __restrict__ lengths, const int* __restrict__ q_lens,
    const int* __restrict__ slots, int T, int hq, int hkv, int nct, int S,
    int max_pages, int lg, int P, int max_len, int window, int chunk,
    float scale) {
  decode_prefill_chunk<D, DbE4m3, DbPaged>(
      q, kc, vc, DbE4m3{k_scale, v_scale}, o, part, lengths, q_lens, slots,
      DbPaged{table, max_pages, lg, P}, T, hq, hkv, nct, S, max_len, window,
      chunk, scale);
}

template <int D>
void launch(const DecodeBatchedArgs& a, hipStream_t st) {
  const int nct = decode_prefill_groups(a.T, a.hq, a.hkv);
  const dim3 grid(a.n_chunks, a.hkv * nct, a.n), block(256);
  float* part = a.n_chunks > 1 ? a.part : nullptr;
  const __bf16* kb = static_cast<const __bf16*>(a.k_cache);
  const __bf16* vb = static_cast<const __bf16*>(a.v_cache);
  const uint8_t* k8 = static_cast<const uint8_t*>(a.k_cache);
  const uint8_t* v8 = static_cast<const uint8_t*>(a.v_cache);
  if (a.table && a.fp8)
    hipLaunchKernelGGL((decode_prefill_paged_fp8_kernel<D>), grid, block, 0,
                       st, a.q, k8, v8, a.k_scale, a.v_scale, a.o, part,
                       a.table, a.lengths, a.q_lens, a.slots, a.T, a.hq,
                       a.hkv, nct, a.S, a.max_pages, a.lg, a.P, a.max_len,
                       a.window, a.chunk, a.scale);
  else if (a.table)
    hipLaunchKernelGGL((decode_prefill_paged_kernel<D>), grid, block, 0, st,
                       a.q, kb, vb, a.o, part, a.table, a.lengths, a.q_lens,
                       a.slots, a.T, a.hq, a.hkv, nct, a.S, a.max_pages, a.lg,
                       a.P, a.max_len, a.window, a.chunk, a.scale);
  else if (a.fp8)
    hipLaunchKernelGGL((decode_prefill_fp8_kernel<D>), grid, block, 0, st,
                       a.q, k8, v8, a.k_scale, a.v_scale, a.o, part,
                       a.lengths, a.q_lens, a.slots, a.T, a.hq, a.hkv, nct,
                       a.S, a.max_s, a.max_len, a.window, a.chunk, a.scale);
  else
    hipLaunchKernelGGL((decode_prefill_kernel<D>), grid, block, 0, st, a.q,
                       kb, vb, a.o, part, a.lengths, a.q_lens, a.slots, a.T,
                       a.hq, a.hkv, nct, a.S, a.max_s, a.max_len, a.window,
                       a.chunk, a.scale);
  if (a.n_chunks == 1) return;
  // the chunk grid is decode_multi's, so its merge fits unchanged
  const float* vs = a.fp8 ? a.v_scale : nullptr;
  const dim3 mgrid(a.n * a.T * a.hq), mblock(D);
  if (a.table)
    hipLaunchKernelGGL((decode_multi_merge_kernel<D, DbPaged>), mgrid, mblock,
                       0, st, a.part, vs, a.o, a.lengths, a.q_lens, a.slots,
                       a.T, a.hq, a.hkv, PF_COLS, a.S, a.max_len, a.window,
                       a.chunk, a.n_chunks);
  else
    hipLaunchKernelGGL((decode_multi_merge_kernel<D, DbContig>), mgrid,
                       mblock, 0, st, a.part, vs, a.o, a.lengths, a.q_lens,
                       a.slots, a.T, a.hq, a.hkv, PF_COLS, a.S, a.max_len,
                       a.window, a.chunk, a.n_chunks);
}

}  // namespace

int decode_prefill_groups(int T, int hq, int hkv) {
  return (T * (hq / hkv) + PF_COLS - 1) / PF_COLS;
}

void decode_prefill_launch(const DecodeBatchedArgs& a, hipStream_t st) {
  if (a.d == 64)
    launch<64>(a, st);
  else
    launch<128>(a, st);
}
