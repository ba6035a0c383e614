// Batched decode attention on an FP8 (OCP e4m3) KV cache, and the quantising
// cache write that fills it (serving path, gfx950).
//
//   q [n, hq, D] bf16, caches [S, max_s, hkv, D] e4m3 bytes, o [n, hq, D] bf16
//   k_scale, v_scale: fp32 [hkv] (null: ones), real = stored * scale[h]
//   lengths, slots: int32 [n] in device memory, as in decode_attn_batched.hip
//
// Contract, work split, online softmax, split-KV and merge are those of
// decode_batched_kernel (decode_attn_batched.hip): grid (n_chunks, hkv, n)
// from host arguments alone, one 256-thread workgroup per (row, kv head,
// chunk), wave w takes keys 32w .. 32w+31 of every 128-key tile, the three-
// term bf16 split of the weights.  What differs is how the bytes move.
//
// Arithmetic.  e4m3 -> bf16 is exact (3 mantissa bits; the smallest denormal
// 2^-9 is a bf16 normal), one v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 per
// two values, so both products stay v_mfma_f32_16x16x32_bf16 on exactly
// dequantised operands.  k_scale[h] is folded into the softmax scale (one
// fp32 product per workgroup), v_scale[h] multiplies the normalised fp32 row
// once, in the direct write or in the merge kernel.
//
// K (lane l: g = l >> 4, c = l & 15).  A K row is D bytes.  A lane reads 16
// contiguous bytes of a row with one 16-byte load: bytes 64t + 16g ..
// 64t + 16g + 15 (t < D/64).  They are its A fragments of the two k-steps
// 2t and 2t + 1: k-slot 8g + j of k-step 2t + h is column 64t + 16g + 8h + j.
// The contraction over d does not depend on the order, and q's B fragments
// are loaded once per chunk with the same map (8 bf16 from column
// 64t + 16g + 8h of head c).  Row c of A block blk is key 8(c >> 2) + 4 blk
// + (c & 3) of the wave's 32, so the D layout (register r of block blk =
// A row 16 blk + 4g + r) gives lane (g, c) the scores of the contiguous keys
// 8g .. 8g + 7 of head c: s[4 blk + r] is key 8g + 4 blk + r.
//
// V goes through LDS as bytes: the wave's image is 32 rows of D bytes (half
// the bf16 image and half its ds_write_b128 traffic), row stride D + 16
// bytes.  ds_read_b64_tr_b8 on a 16-lane group: lane 2q + p gives the
// address of bytes 8p .. 8p + 7 of row q (q < 8), and lane i receives byte i
// of rows 0 .. 7.  With row q = key 8g + q and the 16 bytes = columns
// 16 dt .. 16 dt + 15, lane (g, c) receives V[8g + j][16 dt + c], j < 8:
// the A fragment of O^T[d x heads] += V^T . P^T with k-slot 8g + j = key
// 8g + j, so one read per 16-row block of d (the bf16 kernel needs two) and
// the P^T fragment is the lane's own eight weights, no cross-lane move.
// Four conversions turn the 8 bytes into the bf16x8 fragment.
//
// Banks (bank = (byte / 4) % 64 for the transposed read, served by 32-lane
// halves; % 32 for ds_write_b128, served by 8 consecutive lanes).  A half of
// a transposed read holds keys 16h .. 16h + 15, 16 bytes each at
// key (D + 16) + 16 dt: in 16-byte units key u + dt with u = 9 (D = 128) or
// 5 (D = 64), odd, so the 16 keys fall on the 16 different units of the 256
// bytes.  Writes, D = 128: 8 lanes hold one row, 128 contiguous bytes.
// D = 64: a row is four lanes; with rows r and r + 1 in one group of 8 the
// second 64 bytes would start 80 bytes on and overlap the first by 16 modulo
// 128, so a load's 16 rows are dealt x -> (x & 8) | ((x & 1) << 2) |
// ((x >> 1) & 3): 8 lanes hold rows r and r + 4, 320 = 64 (mod 128) bytes
// apart, which tile the 128 bytes.  All three are conflict-free.
//
// The next step's K bytes and V rows are loaded (raw, 16 + 16 VGPRs at
// D = 128) after the first product, before the softmax and second product.
// Full steps carry no bounds checks; a step that reaches past the chunk's
// end clamps its row addresses and selects zero bytes for V and -1e30 for
// the scores.  LDS: the V images are 4 x 32 x (D + 16) B; the fp32 combine
// of the four waves (4 x 16 x D x 4 B) is the larger of the two and sizes
// the block.
#include "common.h"

#include <stdint.h>

// Packed fp32 instructions are kept out of this module's device code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif
#include "decode_fp8_body.h"

namespace {

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
  f8_chunk<D>(q, kc, vc, k_scale, v_scale, o, part, lengths, slots,
              DbContig{max_s}, hq, hkv, S, max_len, window, chunk, scale);
}

// One block of D threads per (row, q head): log-sum-exp merge of the chunks
// this row has, counted from its own length; the others were never written.
template <int D>
__global__ void decode_batched_fp8_merge_kernel(
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
  const int nch = min((r.len - r.start + chunk - 1) / chunk, n_chunks);
  const float* base = part + (long)bh * n_chunks * (D + 2);
  float gm = F8_NEG;
  for (int ci = 0; ci < nch; ++ci) gm = fmaxf(gm, base[ci * (D + 2) + D]);
  float gl = 0.f, acc = 0.f;
  for (int ci = 0; ci < nch; ++ci) {
    const float f = __expf(base[ci * (D + 2) + D] - gm);
    gl += f * base[ci * (D + 2) + D + 1];
    acc += f * base[ci * (D + 2) + tid];
  }
  const float vs = v_scale ? v_scale[(bh % hq) / (hq / hkv)] : 1.f;
  o[(long)bh * D + tid] = (__bf16)(acc / gl * vs);
}

// Quantising cache write.  One thread per 16 elements of one (row, head) of
// k (blockIdx.y = 0) or v (1): two 16-byte loads, the correctly rounded fp32
// quotient by scale[h], an explicit clamp to +-448, round-to-nearest-even to
// e4m3 and one 16-byte store to cache[slots[i], positions[i], h].  A row
// whose slot or position is outside the cache is skipped before any address
// is formed from it.
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(
    const __bf16* __restrict__ k, const __bf16* __restrict__ v, long k_rs,
    long k_hs, long v_rs, long v_hs, uint8_t* __restrict__ kc,
    uint8_t* __restrict__ vc, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ slots,
    const int* __restrict__ positions, int n, int hkv, int d, int S,
    int max_s) {
  const int cpr = d / 16;            // 16-element chunks per (row, head)
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)n * hkv * cpr) return;
  const int ch = (int)(idx % cpr), h = (int)(idx / cpr % hkv);
  const int i = (int)(idx / ((long)cpr * hkv));
  const int slot = slots[i], pos = positions[i];
  if (slot < 0 || slot >= S || pos < 0 || pos >= max_s) return;
  const bool is_v = blockIdx.y != 0;
  const __bf16* src = (is_v ? v + i * v_rs + h * v_hs
                            : k + i * k_rs + h * k_hs) + 16 * ch;
  const float* sp = is_v ? v_scale : k_scale;
  const float sc = sp ? sp[h] : 1.f;
  const bf16x8 lo = *reinterpret_cast<const bf16x8*>(src);
  const bf16x8 hi = *reinterpret_cast<const bf16x8*>(src + 8);
  float x[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) { x[j] = (float)lo[j]; x[8 + j] = (float)hi[j]; }
  f8_uint4 out;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    x[j] = fminf(fmaxf(x[j] / sc, -F8_MAX), F8_MAX);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int wd = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j], x[4 * j + 1], 0, false);
    wd = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j + 2], x[4 * j + 3], wd, true);
    out[j] = (unsigned)wd;
  }
  uint8_t* dst = (is_v ? vc : kc) +
                 (((long)slot * max_s + pos) * hkv + h) * d + 16 * ch;
  *reinterpret_cast<f8_uint4*>(dst) = out;
}

template <int D>
void launch(const __bf16* q, const uint8_t* kc, const uint8_t* vc,
            const float* k_scale, const float* v_scale, __bf16* o,
            float* part, const int* lengths, const int* slots, int n, int hq,
            int hkv, int S, int max_s, int max_len, int window, int chunk,
            int n_chunks, float scale, hipStream_t st) {
  hipLaunchKernelGGL((decode_batched_fp8_kernel<D>), dim3(n_chunks, hkv, n),
                     dim3(256), 0, st, q, kc, vc, k_scale, v_scale, o,
                     n_chunks > 1 ? part : nullptr, lengths, slots, hq, hkv,
                     S, max_s, max_len, window, chunk, scale);
  if (n_chunks > 1)
    hipLaunchKernelGGL((decode_batched_fp8_merge_kernel<D>), dim3(n * hq),
                       dim3(D), 0, st, part, v_scale, o, lengths, slots, hq,
                       hkv, S, max_len, window, chunk, n_chunks);
}

}  // namespace

int decode_fp8_tile() { return F8_TILE; }

// Arguments as decode_attn_batched_launch, plus the byte caches and the two
// scale vectors (either may be null: ones).
void decode_attn_batched_fp8_launch(
    const __bf16* q, const uint8_t* kc, const uint8_t* vc,
    const float* k_scale, const float* v_scale, __bf16* o, float* part,
    const int* lengths, const int* slots, int n, int hq, int hkv, int S,
    int max_s, int max_len, int window, int chunk, int n_chunks, int d,
    float scale, hipStream_t st) {
  if (d == 64)
    launch<64>(q, kc, vc, k_scale, v_scale, o, part, lengths, slots, n, hq,
               hkv, S, max_s, max_len, window, chunk, n_chunks, scale, st);
  else
    launch<128>(q, kc, vc, k_scale, v_scale, o, part, lengths, slots, n, hq,
                hkv, S, max_s, max_len, window, chunk, n_chunks, scale, st);
}

// k, v: [n, hkv, d] bf16 with row and head strides in elements (multiples of
// 8, 16-byte aligned bases) and a contiguous last dim; d is 64 or 128.
void kv_append_fp8_launch(const __bf16* k, const __bf16* v, long k_rs,
                          long k_hs, long v_rs, long v_hs, uint8_t* kc,
                          uint8_t* vc, const float* k_scale,
                          const float* v_scale, const int* slots,
                          const int* positions, int n, int hkv, int d, int S,
                          int max_s, hipStream_t st) {
  const long items = (long)n * hkv * (d / 16);
  hipLaunchKernelGGL(kv_append_fp8_kernel,
                     dim3((unsigned)((items + 255) / 256), 2), dim3(256), 0,
                     st, k, v, k_rs, k_hs, v_rs, v_hs, kc, vc, k_scale,
                     v_scale, slots, positions, n, hkv, d, S, max_s);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif
