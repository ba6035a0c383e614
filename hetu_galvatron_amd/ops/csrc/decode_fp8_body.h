// The per-chunk body of batched decode attention on e4m3 caches: what one
// 256-thread workgroup does for one (row, kv head, chunk).  The design is
// described at the head of decode_attn_fp8.hip.  The body is parametrised by
// an addressing tag (decode_rows.h): DbContig, instantiated by
// decode_attn_fp8.hip, reads one cache row; DbPaged, instantiated by
// decode_attn_paged.hip, reads pool pages through a page table.  Include it
// inside the module's packed-fp32 pragma.
#pragma once

#include <stdint.h>

#include "common.h"
#include "decode_rows.h"

namespace {

constexpr int F8_WAVES = 4;
constexpr int F8_WKEYS = 32;                    // keys per wave step
constexpr int F8_TILE = F8_WAVES * F8_WKEYS;    // keys per workgroup tile
constexpr float F8_NEG = -1e30f;
constexpr float F8_MAX = 448.f;                 // largest finite e4m3

typedef __attribute__((ext_vector_type(2))) __bf16 f8_bf16x2;
typedef __attribute__((ext_vector_type(2))) int f8_int2;
typedef __attribute__((ext_vector_type(4))) unsigned f8_uint4;
typedef __attribute__((address_space(3))) f8_int2 f8_lds_int2;

// Eight e4m3 bytes (two dwords) -> the bf16x8 fragment, exactly.
DEV_INLINE bf16x8 f8_to_bf16x8(unsigned a, unsigned b) {
  union { f8_bf16x2 p[4]; bf16x8 f; } u;
  u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false);
  u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true);
  u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false);
  u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true);
  return u.f;
}

// Row of a load's 64 / (D/16) rows that lanes x CH .. x CH + CH - 1 stage.
template <int D>
DEV_INLINE int f8_stage_row(int x) {
  return D == 64 ? ((x & 8) | ((x & 1) << 2) | ((x >> 1) & 3)) : x;
}

// Raw K bytes and V rows of the wave's 32 keys from key k0 on.  FULL: all 32
// are inside [lo, p1).  Otherwise rows past p1 - 1 are read from row p1 - 1
// (inside the chunk) and V is zeroed by value; the scores are masked later.
// REL (paged): kb and vb point at key k0's row, and keys below lo (the
// row's first attended position, inside this step) are read from row lo.
template <int D, bool FULL, bool REL>
DEV_INLINE void f8_load(const uint8_t* __restrict__ kb,
                        const uint8_t* __restrict__ vb, int rs, int k0, int lo,
                        int p1, int lane, f8_uint4 (&kr)[2][D / 64],
                        f8_uint4 (&vr)[D / 32]) {
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    int key = k0 + 8 * (c >> 2) + 4 * blk + (c & 3);
    if (!FULL) key = min(key, p1 - 1);
    if (!FULL && REL) key = max(key, lo);
    if (REL) key -= k0;
    const uint8_t* kp = kb + (long)key * rs + 16 * g;
#pragma unroll
    for (int t = 0; t < D / 64; ++t)
      kr[blk][t] = *reinterpret_cast<const f8_uint4*>(kp + 64 * t);
  }
  constexpr int CH = D / 16;         // 16-byte chunks per row
  constexpr int RPL = 64 / CH;       // rows per load of the wave
  const int row = f8_stage_row<D>(lane / CH);
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int key = k0 + i * RPL + row;
    int kc = FULL ? key : min(key, p1 - 1);
    if (!FULL && REL) kc = max(kc, lo);
    if (REL) kc -= k0;
    f8_uint4 v = *reinterpret_cast<const f8_uint4*>(vb + (long)kc * rs +
                                                    16 * (lane % CH));
    if (!FULL && (key >= p1 || (REL && key < lo)))
      v = f8_uint4{0u, 0u, 0u, 0u};
    vr[i] = v;
  }
}

// Issues the loads of the wave step at k0.  Paged: `id` is the step's page
// id, fetched at least one step earlier; an id outside the pool loads
// nothing and forms no address.
template <int D, class A>
DEV_INLINE void f8_fetch(const A& ad, const uint8_t* __restrict__ kb,
                         const uint8_t* __restrict__ vb, int rs, int k0, int lo,
                         int p1, int id, int lane, f8_uint4 (&kr)[2][D / 64],
                         f8_uint4 (&vr)[D / 32]) {
  if constexpr (A::paged) {
    if (!ad.ok(id)) return;
    const long off = ad.pool_row(id, k0) * rs;
    if (lo <= k0 && k0 + F8_WKEYS <= p1)
      f8_load<D, true, true>(kb + off, vb + off, rs, k0, lo, p1, lane, kr, vr);
    else
      f8_load<D, false, true>(kb + off, vb + off, rs, k0, lo, p1, lane, kr,
                              vr);
  } else {
    if (k0 + F8_WKEYS <= p1)
      f8_load<D, true, false>(kb, vb, rs, k0, lo, p1, lane, kr, vr);
    else
      f8_load<D, false, false>(kb, vb, rs, k0, lo, p1, lane, kr, vr);
  }
}

template <int D, class A>
DEV_INLINE void f8_chunk(const __bf16* q,         // [n, hq, D]
                         const uint8_t* kc,       // cache or pool, e4m3
                         const uint8_t* vc,
                         const float* k_scale,    // [hkv] or null
                         const float* v_scale,
                         __bf16* o,               // [n, hq, D]
                         float* part,             // null: write o
                         const int* lengths, const int* slots, A ad, int hq,
                         int hkv, int S, int max_len, int window, int chunk,
                         float scale) {
  constexpr int VSTR = D + 16;       // LDS row stride of the V image, bytes
  constexpr int VIMG = F8_WKEYS * VSTR;
  constexpr int NDT = D / 16;
  constexpr int COMB = F8_WAVES * 16 * D * 4;
  static_assert(F8_WAVES * VIMG <= COMB, "the combine sizes the block");
  // the V images of the four waves, then the waves' fp32 O for the combine
  __shared__ __align__(16) uint8_t lds[COMB];
  __shared__ float ml[F8_WAVES][16][2];

  const int row = blockIdx.z, hk = blockIdx.y, ci = blockIdx.x;
  const int qpg = hq / hkv;
  const int tid = threadIdx.x;
  const DbRow r = db_row(lengths, slots, row, S, max_len, window);
  const int p0 = db_grid_start<A>(r) + ci * chunk;
  if (p0 >= r.len) {                 // workgroup-uniform; also the empty row
    if (r.len == 0 && part == nullptr)
      for (int i = tid; i < qpg * D; i += 256)
        o[((long)row * hq + hk * qpg) * D + i] = (__bf16)0.f;
    return;
  }
  const int p1 = min(p0 + chunk, r.len);
  const int lo = r.start;            // paged: the only bound below a step

  // the wave index as a scalar: the step loop branches on it
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const int rs = hkv * D;
  ad.bind(r.slot);
  const long base = ad.base(r.slot, hkv, hk, D);
  const uint8_t* kb = kc + base;
  const uint8_t* vb = vc + base;
  const float sc = k_scale ? scale * k_scale[hk] : scale;

  bf16x8 qf[D / 32];
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[ks][j] = (__bf16)0.f;
    if (c < qpg)
      qf[ks] = *reinterpret_cast<const bf16x8*>(
          q + ((long)row * hq + hk * qpg + c) * D + 64 * (ks >> 1) + 16 * g +
          8 * (ks & 1));
  }

  uint8_t* vimg = lds + w * VIMG;
  constexpr int CH = D / 16, RPL = 64 / CH;
  const int wr_off = f8_stage_row<D>(lane / CH) * VSTR + 16 * (lane % CH);
  // lane 2q + p of a 16-lane group addresses bytes 8p .. 8p+7 of key 8g + q
  const int tr_off = (8 * g + (c >> 1)) * VSTR + 8 * (c & 1);

  f32x4 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = F8_NEG, l = 0.f;

  f8_uint4 kr[2][D / 64];
  f8_uint4 vr[D / 32];
  int k0 = p0 + w * F8_WKEYS;
  // paged: the page ids of this step and the next, as wave-uniform values
  int id0 = -1, id1 = -1;
  if constexpr (A::paged) {
    if (k0 < p1) id0 = ad.page_id(k0);
    if (k0 + F8_TILE < p1) id1 = ad.page_id(k0 + F8_TILE);
  }
  if (k0 < p1) f8_fetch<D>(ad, kb, vb, rs, k0, lo, p1, id0, lane, kr, vr);
  while (k0 < p1) {                  // wave-uniform
    // the id of the step after the next, a full step ahead of its loads
    int id2 = -1;
    if constexpr (A::paged) {
      if (k0 + 2 * F8_TILE < p1) id2 = ad.page_id(k0 + 2 * F8_TILE);
    }
    bool live = true;                // paged: the step's page is in the pool
    if constexpr (A::paged) live = ad.ok(id0);

    f32x4 sacc[2];
    if (live) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
      *reinterpret_cast<f8_uint4*>(vimg + wr_off + i * RPL * VSTR) = vr[i];
    db_wave_fence();

#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      sacc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        const f8_uint4 raw = kr[blk][ks >> 1];
        const bf16x8 kf = f8_to_bf16x8(raw[2 * (ks & 1)],
                                       raw[2 * (ks & 1) + 1]);
        sacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            kf, qf[ks], sacc[blk], 0, 0, 0);
      }
    }
    }

    const int kn = k0 + F8_TILE;
    if (kn < p1) f8_fetch<D>(ad, kb, vb, rs, kn, lo, p1, id1, lane, kr, vr);

    if (live) {
    float s[8];
    float mx = F8_NEG;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = k0 + 8 * g + j;
      const bool in = A::paged
          ? (unsigned)(key - lo) < (unsigned)(p1 - lo) : key < p1;
      s[j] = in ? sacc[j >> 2][j & 3] * sc : F8_NEG;
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mn = fmaxf(m, mx);
    const float alpha = __expf(m - mn);
    m = mn;
    float ps = 0.f;
    bf16x8 ph, pl, pl2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = __expf(s[j] - mn);
      ps += p;
      const __bf16 h = (__bf16)p;
      const float r1 = p - (float)h;
      const __bf16 lo16 = (__bf16)r1;
      ph[j] = h;
      pl[j] = lo16;
      pl2[j] = (__bf16)(r1 - (float)lo16);
    }
    l = l * alpha + ps;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const f8_int2 raw = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
          (f8_lds_int2*)(vimg + tr_off + 16 * dt));
      const bf16x8 vf = f8_to_bf16x8(raw[0], raw[1]);
      f32x4 a = oacc[dt];
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] *= alpha;
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pl2, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pl, a, 0, 0, 0);
      oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, ph, a, 0, 0, 0);
    }
    db_wave_fence();
    }
    k0 = kn;
    id0 = id1;
    id1 = id2;
  }

  // the lane groups summed different keys against the same max
  l += __shfl_xor(l, 16, WAVE);
  l += __shfl_xor(l, 32, WAVE);

  __syncthreads();                   // every wave is done with its V image
  float* comb = reinterpret_cast<float*>(lds);   // [wave][head][D]
  if (c < qpg) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      *reinterpret_cast<f32x4*>(comb + (w * 16 + c) * D + 16 * dt + 4 * g) =
          oacc[dt];
    if (g == 0) { ml[w][c][0] = m; ml[w][c][1] = l; }
  }
  __syncthreads();
  const float vs = v_scale ? v_scale[hk] : 1.f;
  for (int i = tid; i < qpg * D; i += 256) {
    const int hh = i / D, d = i - hh * D;
    float gm = ml[0][hh][0];
#pragma unroll
    for (int ww = 1; ww < F8_WAVES; ++ww) gm = fmaxf(gm, ml[ww][hh][0]);
    float gl = 0.f, acc = 0.f;
#pragma unroll
    for (int ww = 0; ww < F8_WAVES; ++ww) {
      const float f = __expf(ml[ww][hh][0] - gm);
      gl += f * ml[ww][hh][1];
      acc += f * comb[(ww * 16 + hh) * D + d];
    }
    const long bh = (long)row * hq + hk * qpg + hh;
    if (part == nullptr) {
      // paged: every attended page was outside the pool -> zeros
      if (A::paged && gl == 0.f) gl = 1.f;
      o[bh * D + d] = (__bf16)(acc / gl * vs);
    } else {
      float* out = part + (bh * gridDim.x + ci) * (D + 2);
      out[d] = acc;
      if (d == 0) { out[D] = gm; out[D + 1] = gl; }
    }
  }
}

}  // namespace
