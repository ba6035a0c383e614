// The per-chunk body of batched decode attention on bf16 caches: what one
// 256-thread workgroup does for one (row, kv head, chunk).  The design is
// described at the head of decode_attn_batched.hip.  The body is parametrised
// by an addressing tag (decode_rows.h): DbContig, instantiated by
// decode_attn_batched.hip, reads one cache row; DbPaged, instantiated by
// decode_attn_paged.hip, reads pool pages through a page table.  Include it
// inside the module's packed-fp32 pragma.
#pragma once

#include "common.h"
#include "decode_rows.h"

namespace {

constexpr int DB_WAVES = 4;
constexpr int DB_WKEYS = 32;                    // keys per wave step
constexpr int DB_TILE = DB_WAVES * DB_WKEYS;    // keys per workgroup tile
constexpr float DB_NEG = -1e30f;

typedef __attribute__((ext_vector_type(4))) short db_short4;
typedef __attribute__((address_space(3))) db_short4 db_lds_short4;

// K fragments and V rows of the wave's 32 keys from key k0 on.  FULL: all 32
// are inside [lo, p1).  Otherwise rows past p1 - 1 are read from row p1 - 1
// (inside the chunk) and V is zeroed by value; the scores are masked later.
// REL (paged): kb and vb point at key k0's row, and keys below lo (the
// row's first attended position, inside this step) are read from row lo.
template <int D, bool FULL, bool REL>
DEV_INLINE void db_load(const __bf16* __restrict__ kb,
                        const __bf16* __restrict__ vb, int rs, int k0, int lo,
                        int p1, int lane, bf16x8 (&kf)[2][D / 32],
                        bf16x8 (&vr)[D / 16]) {
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    int key = k0 + 16 * blk + c;
    if (!FULL) key = min(key, p1 - 1);
    if (!FULL && REL) key = max(key, lo);
    if (REL) key -= k0;
    const __bf16* kp = kb + (long)key * rs + 8 * g;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks)
      kf[blk][ks] = *reinterpret_cast<const bf16x8*>(kp + 32 * ks);
  }
  constexpr int CH = D / 8;          // 16-byte chunks per row
  constexpr int RPL = 64 / CH;       // rows per load of the wave
#pragma unroll
  for (int i = 0; i < D / 16; ++i) {
    const int key = k0 + i * RPL + lane / CH;
    int kc = FULL ? key : min(key, p1 - 1);
    if (!FULL && REL) kc = max(kc, lo);
    if (REL) kc -= k0;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(vb + (long)kc * rs +
                                                8 * (lane % CH));
    if (!FULL && (key >= p1 || (REL && key < lo))) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
    }
    vr[i] = v;
  }
}

// Issues the loads of the wave step at k0.  Paged: `id` is the step's page
// id, fetched at least one step earlier; an id outside the pool loads
// nothing and forms no address.
template <int D, class A>
DEV_INLINE void db_fetch(const A& ad, const __bf16* __restrict__ kb,
                         const __bf16* __restrict__ vb, int rs, int k0, int lo,
                         int p1, int id, int lane, bf16x8 (&kf)[2][D / 32],
                         bf16x8 (&vr)[D / 16]) {
  if constexpr (A::paged) {
    if (!ad.ok(id)) return;
    const long off = ad.pool_row(id, k0) * rs;
    if (lo <= k0 && k0 + DB_WKEYS <= p1)
      db_load<D, true, true>(kb + off, vb + off, rs, k0, lo, p1, lane, kf, vr);
    else
      db_load<D, false, true>(kb + off, vb + off, rs, k0, lo, p1, lane, kf,
                              vr);
  } else {
    if (k0 + DB_WKEYS <= p1)
      db_load<D, true, false>(kb, vb, rs, k0, lo, p1, lane, kf, vr);
    else
      db_load<D, false, false>(kb, vb, rs, k0, lo, p1, lane, kf, vr);
  }
}

template <int D, class A>
DEV_INLINE void db_chunk(const __bf16* q,    // [n, hq, D]
                         const __bf16* kc,   // cache or pool
                         const __bf16* vc,
                         __bf16* o,          // [n, hq, D]
                         float* part,  // null: write o
                         const int* lengths,
                         const int* slots, A ad, int hq, int hkv,
                         int S, int max_len, int window, int chunk,
                         float scale) {
  constexpr int VSTR = D + 16;       // LDS row stride of the V image
  constexpr int VIMG = DB_WKEYS * VSTR;
  constexpr int NDT = D / 16;
  // the V images of the four waves, then the waves' fp32 O for the combine
  __shared__ __align__(16) __bf16 lds[DB_WAVES * VIMG];
  __shared__ float ml[DB_WAVES][16][2];
  static_assert(DB_WAVES * VIMG * 2 >= DB_WAVES * 16 * D * 4,
                "the combine does not fit the V images");

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
  const __bf16* kb = kc + base;
  const __bf16* vb = vc + base;

  bf16x8 qf[D / 32];
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[ks][j] = (__bf16)0.f;
    if (c < qpg)
      qf[ks] = *reinterpret_cast<const bf16x8*>(
          q + ((long)row * hq + hk * qpg + c) * D + 32 * ks + 8 * g);
  }

  __bf16* vimg = lds + w * VIMG;
  constexpr int CH = D / 8, RPL = 64 / CH;
  const int wr_off = (lane / CH) * VSTR + 8 * (lane % CH);
  // lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a
  // 4 x 16 block and receives column (lane & 15) of its four rows
  const int tr_off = (4 * g + ((lane >> 2) & 3)) * VSTR + 4 * (lane & 3);

  f32x4 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = DB_NEG, l = 0.f;

  bf16x8 kf[2][D / 32];
  bf16x8 vr[NDT];
  int k0 = p0 + w * DB_WKEYS;
  // paged: the page ids of this step and the next, as wave-uniform values
  int id0 = -1, id1 = -1;
  if constexpr (A::paged) {
    if (k0 < p1) id0 = ad.page_id(k0);
    if (k0 + DB_TILE < p1) id1 = ad.page_id(k0 + DB_TILE);
  }
  if (k0 < p1) db_fetch<D>(ad, kb, vb, rs, k0, lo, p1, id0, lane, kf, vr);
  while (k0 < p1) {                  // wave-uniform
    // the id of the step after the next, a full step ahead of its loads
    int id2 = -1;
    if constexpr (A::paged) {
      if (k0 + 2 * DB_TILE < p1) id2 = ad.page_id(k0 + 2 * DB_TILE);
    }
    bool live = true;                // paged: the step's page is in the pool
    if constexpr (A::paged) live = ad.ok(id0);

    f32x4 sacc[2];
    if (live) {
#pragma unroll
      for (int i = 0; i < NDT; ++i)
        *reinterpret_cast<bf16x8*>(vimg + wr_off + i * RPL * VSTR) = vr[i];
      db_wave_fence();

#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        sacc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks)
          sacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kf[blk][ks], qf[ks], sacc[blk], 0, 0, 0);
      }
    }

    const int kn = k0 + DB_TILE;
    if (kn < p1) db_fetch<D>(ad, kb, vb, rs, kn, lo, p1, id1, lane, kf, vr);

    if (live) {
      float s[8];
      float mx = DB_NEG;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = k0 + 16 * (j >> 2) + 4 * g + (j & 3);
        const bool in = A::paged
            ? (unsigned)(key - lo) < (unsigned)(p1 - lo) : key < p1;
        s[j] = in ? sacc[j >> 2][j & 3] * scale : DB_NEG;
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
        union { db_short4 h[2]; bf16x8 f; } u;
        u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (db_lds_short4*)(vimg + tr_off + 16 * dt));
        u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (db_lds_short4*)(vimg + tr_off + 16 * dt + 16 * VSTR));
        f32x4 a = oacc[dt];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] *= alpha;
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u.f, pl2, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u.f, pl, a, 0, 0, 0);
        oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u.f, ph, a, 0, 0, 0);
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
  for (int i = tid; i < qpg * D; i += 256) {
    const int hh = i / D, d = i - hh * D;
    float gm = ml[0][hh][0];
#pragma unroll
    for (int ww = 1; ww < DB_WAVES; ++ww) gm = fmaxf(gm, ml[ww][hh][0]);
    float gl = 0.f, acc = 0.f;
#pragma unroll
    for (int ww = 0; ww < DB_WAVES; ++ww) {
      const float f = __expf(ml[ww][hh][0] - gm);
      gl += f * ml[ww][hh][1];
      acc += f * comb[(ww * 16 + hh) * D + d];
    }
    const long bh = (long)row * hq + hk * qpg + hh;
    if (part == nullptr) {
      // paged: every attended page was outside the pool -> zeros
      if (A::paged && gl == 0.f) gl = 1.f;
      o[bh * D + d] = (__bf16)(acc / gl);
    } else {
      float* out = part + (bh * gridDim.x + ci) * (D + 2);
      out[d] = acc;
      if (d == 0) { out[D] = gm; out[D + 1] = gl; }
    }
  }
}

}  // namespace
