// The quantising write that fills an FP8 (OCP e4m3) KV cache (serving path,
// gfx950): caches [S, max_s, hkv, D] e4m3 bytes, real = stored * scale[h] with
// k_scale, v_scale fp32 [hkv] (null: ones).  The kernels that read such a
// cache are in decode_attn_batched.hip (format tag DbE4m3 of decode_body.h).
#include "common.h"
#include "decode_launch.h"

// Packed fp32 instructions are kept out of this module's device code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "decode_quant.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned f8_uint4;

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
  for (int j = 0; j < 4; ++j) out[j] = db_quant_e4m3x4(x + 4 * j, sc);
  uint8_t* dst = (is_v ? vc : kc) +
                 (((long)slot * max_s + pos) * hkv + h) * d + 16 * ch;
  *reinterpret_cast<f8_uint4*>(dst) = out;
}

}  // namespace

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
