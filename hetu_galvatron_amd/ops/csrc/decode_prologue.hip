// The decode prologue (serving path, gfx950): what stands between the qkv
// linear and the attention launch of a decode, speculative or chunked-prefill
// step, in one launch.  For the n*T token rows of the packed qkv
// [n, T, G, qpg+2, D] it rotates q and k at the token's own position, writes
// q [n, T, G*qpg, D] and appends the rotated k and the v to the serving cache
// (bf16 or e4m3, contiguous rows or pages), reading positions, cache rows and
// page ids from the device tables that the attention kernels read.  The
// contract is DecodePrologueArgs in decode_launch.h.
//
// Lane map.  A lane owns 16 elements of one head and everything that pairs
// with them: with the half pairing the 8-element chunk c and the chunk D/2
// on, with the interleaved pairing the 16 contiguous elements 16c..16c+15,
// whose 8 pairs lie inside.  Either way the lane needs cos/sin[8c..8c+8), two
// 16-byte loads of qkv, and nothing from another lane; a head is D/16 lanes.
// Stores are 16 bytes of bf16, and for e4m3 two 8-byte stores (half) or one
// 16-byte store (interleaved).
//
// Launch shape.  The lanes are a flat index over (token, head, chunk) in two
// regions: first every rotated head (the G*(qpg+1) q and k heads of a token),
// then, from a workgroup boundary on, the G v heads.  The v test is
// therefore workgroup-uniform and the v workgroups carry no rotation code
// path at run time.  A workgroup is not tied to a token, so the large case
// (8 x 1024 chunked prefill, 393k heads) fills every lane of every workgroup
// but the last of a region.  The small case (one token: 48 heads, 384 lanes
// at D = 128) is latency-bound, one dependent chain per lane, so up to 64k
// lanes run as 64-lane workgroups that spread over the CUs; above that,
// 256-lane workgroups keep the dispatch count down.
//
// cos and sin go straight through L1, not through LDS.  What a lane waits on
// is the chain lengths/q_lens/slots -> position (-> page id) -> cos/sin and
// store address.  Staging a token's cos/sin row in LDS would put an LDS
// write, a barrier and an LDS read behind the position on that chain, and a
// workgroup that spans tokens would need a row per token; through L1 the
// 8 heads of a wave read the same 8 chunks (one request, broadcast) and the
// other waves of the token hit L1 or L2.  The qkv loads depend on the lane
// index alone and are issued before the tables are read.
//
// Arithmetic: x1*c - x2*s and x2*c + x1*s in fp32 with each product and the
// sum rounded on its own (contraction off, no packed fp32), then
// round-to-nearest-even to bf16: the bits of the torch composition.  An e4m3
// cache stores db_quant_e4m3x4 of the bf16-rounded value (decode_quant.h).
#include "common.h"
#include "decode_launch.h"

// Packed fp32 instructions are kept out of this module's device code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "decode_quant.h"
#include "decode_rows.h"

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned dp_uint2;
typedef __attribute__((ext_vector_type(4))) unsigned dp_uint4;

// Rotates the lane's 16 elements in place: x[0..8) and x[8..16) are its two
// chunks, c and s its 8 cos and sin values.  Half: pair (x[j], x[8 + j]);
// interleaved: pair (x[2j], x[2j + 1]).  Every result is rounded to bf16.
template <bool IL>
DEV_INLINE void dp_rotate(float* x, const float* c, const float* s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i1 = IL ? 2 * j : j, i2 = IL ? 2 * j + 1 : 8 + j;
    const float x1 = x[i1], x2 = x[i2];
    const float a = x1 * c[j], b = x2 * s[j];
    const float e = x2 * c[j], f = x1 * s[j];
    x[i1] = (float)(__bf16)(a - b);
    x[i2] = (float)(__bf16)(e + f);
  }
}

template <int D, bool FP8, class A, bool IL>
__global__ __launch_bounds__(256) void decode_prologue_kernel(
    DecodePrologueArgs a, A adr, int rot_blocks) {
  constexpr int CPR = D / 16;                  // lanes per head
  const bool is_v = (int)blockIdx.x >= rot_blocks;      // workgroup-uniform
  const int hpg = is_v ? 1 : a.qpg + 1;        // this region's heads per group
  // the launcher keeps every region below 2^31 lanes: 32-bit index math
  const unsigned idx =
      (blockIdx.x - (is_v ? rot_blocks : 0)) * blockDim.x + threadIdx.x;
  if (idx >= (unsigned)(a.n * a.T) * (a.G * hpg * CPR)) return;
  const int c = (int)(idx % CPR);
  const int hh = (int)(idx / CPR % (unsigned)(a.G * hpg));
  const long tok = idx / (unsigned)(CPR * a.G * hpg);
  const int g = hh / hpg, s = is_v ? a.qpg + 1 : hh - g * hpg;
  const int o0 = IL ? 16 * c : 8 * c, o1 = IL ? 16 * c + 8 : 8 * c + D / 2;

  const __bf16* src = a.qkv + ((tok * a.G + g) * (a.qpg + 2) + s) * D;
  const bf16x8 in0 = *reinterpret_cast<const bf16x8*>(src + o0);
  const bf16x8 in1 = *reinterpret_cast<const bf16x8*>(src + o1);

  const int i = (int)((unsigned)tok / (unsigned)a.T);
  const int t = (int)tok - i * a.T;
  const int len = a.lengths[i], ql = a.q_lens[i], slot = a.slots[i];
  const long pl = (long)len - ql + t;
  const bool live = t < ql && (unsigned)slot < (unsigned)a.S && pl >= 0 &&
                    pl < a.lim;
  const bool is_q = s < a.qpg;
  __bf16* qdst = a.q + ((tok * a.G + g) * a.qpg + s) * D;   // is_q only
  if (!live) {
    if (is_q) {
      const bf16x8 z = {};
      *reinterpret_cast<bf16x8*>(qdst + o0) = z;
      *reinterpret_cast<bf16x8*>(qdst + o1) = z;
    }
    return;
  }
  const int p = (int)pl;                       // checked: 0 <= p < lim

  // where a k or v head goes, in cache elements
  long off = 0;
  if (!is_q) {
    if constexpr (A::paged) {
      A row = adr;
      row.bind(slot);
      const int id = row.page_id(p);
      if (!row.ok(id)) return;
      off = row.pool_row(id, p) * a.G * D + row.base(slot, a.G, g, D);
    } else {
      off = adr.base(slot, a.G, g, D) + (long)p * a.G * D;
    }
  }

  float x[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = (float)in0[j];
    x[8 + j] = (float)in1[j];
  }
  bf16x8 out0 = in0, out1 = in1;
  if (!is_v && a.cos) {
    const long cs = (long)p * (D / 2) + 8 * c;
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(a.cos + cs);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>(a.cos + cs + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(a.sin + cs);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(a.sin + cs + 4);
    float cv[8], sv[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cv[j] = c0[j]; cv[4 + j] = c1[j]; sv[j] = s0[j]; sv[4 + j] = s1[j];
    }
    dp_rotate<IL>(x, cv, sv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      out0[j] = (__bf16)x[j];
      out1[j] = (__bf16)x[8 + j];
    }
  }

  if (is_q) {
    *reinterpret_cast<bf16x8*>(qdst + o0) = out0;
    *reinterpret_cast<bf16x8*>(qdst + o1) = out1;
    return;
  }
  if constexpr (FP8) {
    const float* sp = is_v ? a.v_scale : a.k_scale;
    const float sc = sp ? sp[g] : 1.f;
    uint8_t* dst = static_cast<uint8_t*>(is_v ? a.v_cache : a.k_cache) + off;
    dp_uint4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = db_quant_e4m3x4(x + 4 * j, sc);
    if constexpr (IL) {
      *reinterpret_cast<dp_uint4*>(dst + o0) = w;
    } else {
      const dp_uint2 lo = {w[0], w[1]}, hi = {w[2], w[3]};
      *reinterpret_cast<dp_uint2*>(dst + o0) = lo;
      *reinterpret_cast<dp_uint2*>(dst + o1) = hi;
    }
  } else {
    __bf16* dst = static_cast<__bf16*>(is_v ? a.v_cache : a.k_cache) + off;
    *reinterpret_cast<bf16x8*>(dst + o0) = out0;
    *reinterpret_cast<bf16x8*>(dst + o1) = out1;
  }
}

template <int D, bool FP8, class A>
void launch_pairing(const DecodePrologueArgs& a, const A& adr, hipStream_t st) {
  constexpr int CPR = D / 16;
  const long tokens = (long)a.n * a.T;
  const long rot = tokens * a.G * (a.qpg + 1) * CPR, v = tokens * a.G * CPR;
  const int bs = rot + v <= 65536 ? 64 : 256;
  const long rot_blocks = (rot + bs - 1) / bs, v_blocks = (v + bs - 1) / bs;
  const dim3 grid((unsigned)(rot_blocks + v_blocks)), block(bs);
  if (a.interleaved)
    hipLaunchKernelGGL((decode_prologue_kernel<D, FP8, A, true>), grid, block,
                       0, st, a, adr, (int)rot_blocks);
  else
    hipLaunchKernelGGL((decode_prologue_kernel<D, FP8, A, false>), grid, block,
                       0, st, a, adr, (int)rot_blocks);
}

template <int D, bool FP8>
void launch_addressing(const DecodePrologueArgs& a, hipStream_t st) {
  if (a.table) {
    DbPaged adr;
    adr.trow = a.table;
    adr.max_pages = a.max_pages;
    adr.lg = a.lg;
    adr.P = a.P;
    launch_pairing<D, FP8>(a, adr, st);
  } else {
    DbContig adr;
    adr.max_s = a.max_s;
    launch_pairing<D, FP8>(a, adr, st);
  }
}

}  // namespace

void decode_prologue_launch(const DecodePrologueArgs& a, hipStream_t st) {
  if (a.d == 128) {
    if (a.fp8) launch_addressing<128, true>(a, st);
    else launch_addressing<128, false>(a, st);
  } else {
    if (a.fp8) launch_addressing<64, true>(a, st);
    else launch_addressing<64, false>(a, st);
  }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif
