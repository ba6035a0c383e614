// The per-chunk body of batched decode attention: what one 256-thread
// workgroup does for one (row, kv head, chunk).  One function,
// decode_chunk<D, F, A>, parametrised by
//   F, the cache format tag below: DbBf16 or DbE4m3 -- the element type, the
//      lane maps of the loads, the V image and its transposed read, the
//      scales;
//   A, the addressing tag of decode_rows.h: DbContig reads one cache row,
//      DbPaged reads pool pages through a page table.
// decode_attn_batched.hip instantiates the four combinations.  Include this
// inside the module's packed-fp32 pragma.
//
//   q [n, hq, D] bf16, caches [S, max_s, hkv, D] (pools [P, page, hkv, D]),
//   o [n, hq, D] bf16; lengths, slots: int32 [n] in device memory.  Row i
//   attends to positions [start_i, len_i) of cache row slots[i];
//   len_i = min(lengths[i], max_len), start_i = max(0, len_i - window)
//   (0 without a window).
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
// the others once, after the last tile, in LDS.  Per 32-key step a wave
// forms S^T[keys x heads] = K . Q^T (two 16-key blocks x D/32 k-steps of
// v_mfma_f32_16x16x32_bf16; the B fragment is q of head c = lane & 15, zero
// for c >= qpg, held in registers) and O^T[d x heads] += V^T . P^T (D/16 row
// blocks).  A lane's scores belong to one head, so the running max and sum
// are per-lane scalars; the tile max is combined across the four 16-lane
// groups, the sum only once at the end.  How the fragments are made is the
// format's business and is described at each tag.
//
// The weights enter the second product as three bf16 terms (p = hi + lo +
// lo2, each the rounding of what the ones before left over): one bf16 term
// alone is a relative error of 2^-9 per weight, which the decode element
// rule (ulp of o plus 2^-20 of the absolute-value sum) does not allow where
// the weighted V rows cancel.  MFMA work is far below the memory time, so the
// two extra products are free.
//
// The next step's K and V registers are loaded (raw) after the first product
// of the current one, before its softmax and second product.  Full steps
// carry no bounds checks; a step that reaches past the chunk's end (paged:
// or below the row's start) clamps its row addresses and selects zeros for V
// and -1e30 for the scores.
//
// LDS is a constant of the tile: the larger of the four waves' V images and
// their fp32 O for the final combine, which reuses the block, plus 512 B.
// With n_chunks > 1 every non-empty chunk writes an unnormalised partial
// [D] + (m, l) in fp32 and the merge kernel reads, per row, only the chunks
// that row has.
#pragma once

#include <stdint.h>

#include "common.h"
#include "decode_rows.h"

namespace {

constexpr int DB_WAVES = 4;
constexpr int DB_WKEYS = 32;                    // keys per wave step
constexpr int DB_TILE = DB_WAVES * DB_WKEYS;    // keys per workgroup tile
constexpr float DB_NEG = -1e30f;

typedef __attribute__((ext_vector_type(4))) short db_short4;
typedef __attribute__((address_space(3))) db_short4 db_lds_short4;
typedef __attribute__((ext_vector_type(2))) __bf16 f8_bf16x2;
typedef __attribute__((ext_vector_type(2))) int f8_int2;
typedef __attribute__((ext_vector_type(4))) unsigned f8_uint4;
typedef __attribute__((address_space(3))) f8_int2 f8_lds_int2;

// A format tag F gives (lane l: g = l >> 4, c = l & 15):
//   elem, raw, EPL: the cache element, 16 bytes of a row as loaded, and the
//     elements in them.  Lane l loads columns EPL (4t + g) .. + EPL - 1 of
//     its K rows, t < D / (4 EPL), and stages V by rows with D / EPL lanes
//     per row.
//   k_key(k0, blk, c): the key in A row c of block blk of the step at k0.
//   q_frag(p, ks, g): where the 8 columns of q row p in k-slots 8g .. 8g + 7
//     of k-step ks start.
//   a_frag(kr, ks): the A fragment of k-step ks from a block's raw K.
//   score_key(k0, j, g): the key that score j (register j & 3 of block
//     j >> 2) of the step at k0 belongs to.
//   stage_row(x): the row, of a V load's rows, that lane group x stages.
//   tr_off(l, g, c, vstr): the lane's offset in the V image for the
//     transposed read; vt_frag(p): the V^T fragment of a 16-row block of d,
//     p = image + tr_off + 16 dt.
//   k_mul, v_mul: what the format puts on the softmax scale and on the
//     normalised row of kv head hk (bf16: nothing, at compile time).
//   zero, ZERO_BY_LANE: the zeros for V rows outside a bounded step, written
//     into the loaded value lane by lane (bf16: the compiler selects) or
//     assigned as one constant (e4m3: it branches round the load).  The one
//     place where the body asks which: either form for both formats changes
//     the other's paged kernel (profiles/decode_unify_isa.md).
// The hooks add to k0 and p in a fixed order so that the address arithmetic
// the compiler sees stays what it was tuned with.

// bf16 caches (v_mfma_f32_16x16x32_bf16 throughout).
//
//   S^T = K . Q^T   The A fragment is 8 contiguous bf16 of key row
//       16*blk + c, straight from global memory with a 16-byte load.  D
//       layout: register r of block blk is key 16*blk + 4g + r of head c.
//   O^T += V^T . P^T   The sum over keys does not depend on the order, so
//       k-slot 8g + j of the product is key 4g + j (j < 4) or
//       16 + 4g + j - 4: the P^T fragment is then the lane's own eight
//       weights.  V^T is read with that same map by two ds_read_b64_tr_b16
//       per row block from the wave's own LDS image of its 32 V rows (staged
//       by rows with 16-byte loads, row stride D + 16 elements: the four
//       rows of a 16-lane group are 32 B apart modulo 256, so the reads do
//       not collide).
struct DbBf16 {
  typedef __bf16 elem;
  typedef bf16x8 raw;
  static constexpr int EPL = 8;
  static constexpr bool ZERO_BY_LANE = true;
  static DEV_INLINE void zero(raw& v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
  }
  static DEV_INLINE int k_key(int k0, int blk, int c) {
    return k0 + 16 * blk + c;
  }
  static DEV_INLINE const __bf16* q_frag(const __bf16* p, int ks, int g) {
    return p + 32 * ks + 8 * g;
  }
  template <int D>
  static DEV_INLINE bf16x8 a_frag(const raw (&kr)[D / 32], int ks) {
    return kr[ks];
  }
  static DEV_INLINE int score_key(int k0, int j, int g) {
    return k0 + 16 * (j >> 2) + 4 * g + (j & 3);
  }
  template <int D>
  static DEV_INLINE int stage_row(int x) { return x; }
  // lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a
  // 4 x 16 block and receives column (lane & 15) of its four rows
  static DEV_INLINE int tr_off(int lane, int g, int, int vstr) {
    return (4 * g + ((lane >> 2) & 3)) * vstr + 4 * (lane & 3);
  }
  template <int VSTR>
  static DEV_INLINE bf16x8 vt_frag(const elem* p) {
    union { db_short4 h[2]; bf16x8 f; } u;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((db_lds_short4*)p);
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (db_lds_short4*)(p + 16 * VSTR));
    return u.f;
  }
  DEV_INLINE float k_mul(float scale, int) const { return scale; }
  DEV_INLINE float v_mul(int) const { return 1.f; }
};

// Eight e4m3 bytes (two dwords) -> the bf16x8 fragment, exactly.
DEV_INLINE bf16x8 f8_to_bf16x8(unsigned a, unsigned b) {
  union { f8_bf16x2 p[4]; bf16x8 f; } u;
  u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false);
  u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true);
  u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false);
  u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true);
  return u.f;
}

// FP8 (OCP e4m3) caches: bytes, real = stored * scale[h] with k_scale,
// v_scale fp32 [hkv] (null: ones).
//
// Arithmetic.  e4m3 -> bf16 is exact (3 mantissa bits; the smallest denormal
// 2^-9 is a bf16 normal), one v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 per
// two values, so both products stay v_mfma_f32_16x16x32_bf16 on exactly
// dequantised operands.  k_scale[h] is folded into the softmax scale (one
// fp32 product per workgroup), v_scale[h] multiplies the normalised fp32 row
// once, in the direct write or in the merge kernel.
//
// K.  A K row is D bytes.  A lane reads 16 contiguous bytes of a row with
// one 16-byte load: bytes 64t + 16g .. 64t + 16g + 15 (t < D/64).  They are
// its A fragments of the two k-steps 2t and 2t + 1: k-slot 8g + j of k-step
// 2t + h is column 64t + 16g + 8h + j.  The contraction over d does not
// depend on the order, and q's B fragments are loaded once per chunk with
// the same map (8 bf16 from column 64t + 16g + 8h of head c).  Row c of A
// block blk is key 8(c >> 2) + 4 blk + (c & 3) of the wave's 32, so the D
// layout (register r of block blk = A row 16 blk + 4g + r) gives lane (g, c)
// the scores of the contiguous keys 8g .. 8g + 7 of head c: s[4 blk + r] is
// key 8g + 4 blk + r.
//
// V goes through LDS as bytes: the wave's image is 32 rows of D bytes (half
// the bf16 image and half its ds_write_b128 traffic), row stride D + 16
// bytes.  ds_read_b64_tr_b8 on a 16-lane group: lane 2q + p gives the
// address of bytes 8p .. 8p + 7 of row q (q < 8), and lane i receives byte i
// of rows 0 .. 7.  With row q = key 8g + q and the 16 bytes = columns
// 16 dt .. 16 dt + 15, lane (g, c) receives V[8g + j][16 dt + c], j < 8:
// the A fragment of O^T[d x heads] += V^T . P^T with k-slot 8g + j = key
// 8g + j, so one read per 16-row block of d (bf16 needs two) and the P^T
// fragment is the lane's own eight weights, no cross-lane move.  Four
// conversions turn the 8 bytes into the bf16x8 fragment.
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
// The raw registers of a step are 16 + 16 VGPRs at D = 128.  LDS: the V
// images are 4 x 32 x (D + 16) B; the fp32 combine of the four waves
// (4 x 16 x D x 4 B) is the larger of the two and sizes the block.
struct DbE4m3 {
  typedef uint8_t elem;
  typedef f8_uint4 raw;
  static constexpr int EPL = 16;
  const float* __restrict__ k_scale;   // [hkv] or null
  const float* __restrict__ v_scale;
  static constexpr bool ZERO_BY_LANE = false;
  static DEV_INLINE raw zero() { return raw{0u, 0u, 0u, 0u}; }
  static DEV_INLINE int k_key(int k0, int blk, int c) {
    return k0 + 8 * (c >> 2) + 4 * blk + (c & 3);
  }
  static DEV_INLINE const __bf16* q_frag(const __bf16* p, int ks, int g) {
    return p + 64 * (ks >> 1) + 16 * g + 8 * (ks & 1);
  }
  template <int D>
  static DEV_INLINE bf16x8 a_frag(const raw (&kr)[D / 64], int ks) {
    const raw r = kr[ks >> 1];
    return f8_to_bf16x8(r[2 * (ks & 1)], r[2 * (ks & 1) + 1]);
  }
  static DEV_INLINE int score_key(int k0, int j, int g) {
    return k0 + 8 * g + j;
  }
  template <int D>
  static DEV_INLINE int stage_row(int x) {
    return D == 64 ? ((x & 8) | ((x & 1) << 2) | ((x >> 1) & 3)) : x;
  }
  // lane 2q + p of a 16-lane group addresses bytes 8p .. 8p+7 of key 8g + q
  static DEV_INLINE int tr_off(int, int g, int c, int vstr) {
    return (8 * g + (c >> 1)) * vstr + 8 * (c & 1);
  }
  template <int VSTR>
  static DEV_INLINE bf16x8 vt_frag(const elem* p) {
    const f8_int2 r = __builtin_amdgcn_ds_read_tr8_b64_v2i32((f8_lds_int2*)p);
    return f8_to_bf16x8(r[0], r[1]);
  }
  DEV_INLINE float k_mul(float scale, int hk) const {
    return k_scale ? scale * k_scale[hk] : scale;
  }
  DEV_INLINE float v_mul(int hk) const { return v_scale ? v_scale[hk] : 1.f; }
};

// Raw K and V rows of the wave's 32 keys from key k0 on.  FULL: all 32 are
// inside [lo, p1).  Otherwise rows past p1 - 1 are read from row p1 - 1
// (inside the chunk) and V is zeroed by value; the scores are masked later.
// REL (paged): kb and vb point at key k0's row, and keys below lo (the
// row's first attended position, inside this step) are read from row lo.
template <int D, class F, bool FULL, bool REL>
DEV_INLINE void db_load(const typename F::elem* __restrict__ kb,
                        const typename F::elem* __restrict__ vb, int rs,
                        int k0, int lo, int p1, int lane,
                        typename F::raw (&kr)[2][D / (4 * F::EPL)],
                        typename F::raw (&vr)[D / (2 * F::EPL)]) {
  typedef typename F::raw raw;
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    int key = F::k_key(k0, blk, c);
    if (!FULL) key = min(key, p1 - 1);
    if (!FULL && REL) key = max(key, lo);
    if (REL) key -= k0;
    const typename F::elem* kp = kb + (long)key * rs + F::EPL * g;
#pragma unroll
    for (int t = 0; t < D / (4 * F::EPL); ++t)
      kr[blk][t] = *reinterpret_cast<const raw*>(kp + 4 * F::EPL * t);
  }
  constexpr int CH = D / F::EPL;     // 16-byte chunks per row
  constexpr int RPL = 64 / CH;       // rows per load of the wave
  const int row = F::template stage_row<D>(lane / CH);
#pragma unroll
  for (int i = 0; i < D / (2 * F::EPL); ++i) {
    const int key = k0 + i * RPL + row;
    int kc = FULL ? key : min(key, p1 - 1);
    if (!FULL && REL) kc = max(kc, lo);
    if (REL) kc -= k0;
    raw v = *reinterpret_cast<const raw*>(vb + (long)kc * rs +
                                          F::EPL * (lane % CH));
    if (!FULL && (key >= p1 || (REL && key < lo))) {
      if constexpr (F::ZERO_BY_LANE) F::zero(v); else v = F::zero();
    }
    vr[i] = v;
  }
}

// Issues the loads of the wave step at k0.  Paged: `id` is the step's page
// id, fetched at least one step earlier; an id outside the pool loads
// nothing and forms no address.
template <int D, class F, class A>
DEV_INLINE void db_fetch(const A& ad, const typename F::elem* __restrict__ kb,
                         const typename F::elem* __restrict__ vb, int rs,
                         int k0, int lo, int p1, int id, int lane,
                         typename F::raw (&kr)[2][D / (4 * F::EPL)],
                         typename F::raw (&vr)[D / (2 * F::EPL)]) {
  if constexpr (A::paged) {
    if (!ad.ok(id)) return;
    const long off = ad.pool_row(id, k0) * rs;
    if (lo <= k0 && k0 + DB_WKEYS <= p1)
      db_load<D, F, true, true>(kb + off, vb + off, rs, k0, lo, p1, lane, kr,
                                vr);
    else
      db_load<D, F, false, true>(kb + off, vb + off, rs, k0, lo, p1, lane, kr,
                                 vr);
  } else {
    if (k0 + DB_WKEYS <= p1)
      db_load<D, F, true, false>(kb, vb, rs, k0, lo, p1, lane, kr, vr);
    else
      db_load<D, F, false, false>(kb, vb, rs, k0, lo, p1, lane, kr, vr);
  }
}

template <int D, class F, class A>
DEV_INLINE void decode_chunk(const __bf16* q,    // [n, hq, D]
                             const typename F::elem* kc,   // cache or pool
                             const typename F::elem* vc, F fmt,
                             __bf16* o,          // [n, hq, D]
                             float* part,        // null: write o
                             const int* lengths, const int* slots, A ad,
                             int hq, int hkv, int S, int max_len, int window,
                             int chunk, float scale) {
  typedef typename F::elem elem;
  typedef typename F::raw raw;
  constexpr int VSTR = D + 16;       // LDS row stride of the V image, elements
  constexpr int VIMG = DB_WKEYS * VSTR;
  constexpr int NDT = D / 16;
  constexpr int NVR = D / (2 * F::EPL);   // V loads of a step
  // the V images of the four waves, then the waves' fp32 O for the combine:
  // the larger of the two sizes the block
  constexpr int IMGS = DB_WAVES * VIMG * (int)sizeof(elem);
  constexpr int COMB = DB_WAVES * 16 * D * 4;
  __shared__ __align__(16) elem lds[(IMGS > COMB ? IMGS : COMB) / sizeof(elem)];
  __shared__ float ml[DB_WAVES][16][2];

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
  const elem* kb = kc + base;
  const elem* vb = vc + base;
  const float sc = fmt.k_mul(scale, hk);

  bf16x8 qf[D / 32];
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[ks][j] = (__bf16)0.f;
    if (c < qpg)
      qf[ks] = *reinterpret_cast<const bf16x8*>(
          F::q_frag(q + ((long)row * hq + hk * qpg + c) * D, ks, g));
  }

  elem* vimg = lds + w * VIMG;
  constexpr int CH = D / F::EPL, RPL = 64 / CH;
  const int wr_off =
      F::template stage_row<D>(lane / CH) * VSTR + F::EPL * (lane % CH);
  const int tr_off = F::tr_off(lane, g, c, VSTR);

  f32x4 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = DB_NEG, l = 0.f;

  raw kr[2][D / (4 * F::EPL)];
  raw vr[NVR];
  int k0 = p0 + w * DB_WKEYS;
  // paged: the page ids of this step and the next, as wave-uniform values
  int id0 = -1, id1 = -1;
  if constexpr (A::paged) {
    if (k0 < p1) id0 = ad.page_id(k0);
    if (k0 + DB_TILE < p1) id1 = ad.page_id(k0 + DB_TILE);
  }
  if (k0 < p1)
    db_fetch<D, F>(ad, kb, vb, rs, k0, lo, p1, id0, lane, kr, vr);
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
      for (int i = 0; i < NVR; ++i)
        *reinterpret_cast<raw*>(vimg + wr_off + i * RPL * VSTR) = vr[i];
      db_wave_fence();

#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        sacc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks)
          sacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              F::template a_frag<D>(kr[blk], ks), qf[ks], sacc[blk], 0, 0, 0);
      }
    }

    const int kn = k0 + DB_TILE;
    if (kn < p1)
      db_fetch<D, F>(ad, kb, vb, rs, kn, lo, p1, id1, lane, kr, vr);

    if (live) {
      float s[8];
      float mx = DB_NEG;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = F::score_key(k0, j, g);
        const bool in = A::paged
            ? (unsigned)(key - lo) < (unsigned)(p1 - lo) : key < p1;
        s[j] = in ? sacc[j >> 2][j & 3] * sc : DB_NEG;
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
        const bf16x8 vf = F::template vt_frag<VSTR>(vimg + tr_off + 16 * dt);
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
  const float vs = fmt.v_mul(hk);
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
      o[bh * D + d] = (__bf16)(acc / gl * vs);
    } else {
      float* out = part + (bh * gridDim.x + ci) * (D + 2);
      out[d] = acc;
      if (d == 0) { out[D] = gm; out[D + 1] = gl; }
    }
  }
}

// One block of D threads per (row, q head): log-sum-exp merge of the chunks
// this row has, counted from the first position of its tile grid (its own
// start, or the 32-key boundary below it for paged rows); the others were
// never written.  v_scale is null for bf16 caches.  A paged row without a
// valid page has l = 0 in every chunk and is written as zeros.
template <int D, class A>
__global__ void decode_merge_kernel(
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
  const int nch =
      min((r.len - db_grid_start<A>(r) + chunk - 1) / chunk, n_chunks);
  const float* base = part + (long)bh * n_chunks * (D + 2);
  float gm = DB_NEG;
  for (int ci = 0; ci < nch; ++ci) gm = fmaxf(gm, base[ci * (D + 2) + D]);
  float gl = 0.f, acc = 0.f;
  for (int ci = 0; ci < nch; ++ci) {
    const float f = __expf(base[ci * (D + 2) + D] - gm);
    gl += f * base[ci * (D + 2) + D + 1];
    acc += f * base[ci * (D + 2) + tid];
  }
  if (A::paged && gl == 0.f) gl = 1.f;
  float res = acc / gl;
  if (v_scale) res *= v_scale[(bh % hq) / (hq / hkv)];
  o[(long)bh * D + tid] = (__bf16)res;
}

}  // namespace
