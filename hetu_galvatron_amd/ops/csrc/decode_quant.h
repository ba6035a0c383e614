// The e4m3 quantisation of the serving caches, written once: the quantising
// append (decode_attn_fp8.hip) and the decode prologue (decode_prologue.hip)
// store the same bytes for the same bf16 value.  Include this inside the
// module's packed-fp32 pragma.
#pragma once

#include "common.h"

constexpr float DB_F8_MAX = 448.f;              // largest finite e4m3

// Four values -> four e4m3 bytes (x[0] in the low byte): the correctly
// rounded fp32 quotient by sc, an explicit clamp to +-448, then
// round-to-nearest-even to e4m3.
DEV_INLINE unsigned db_quant_e4m3x4(const float* x, float sc) {
  float y[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    y[j] = fminf(fmaxf(x[j] / sc, -DB_F8_MAX), DB_F8_MAX);
  int wd = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  wd = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], wd, true);
  return (unsigned)wd;
}
