// CDNA4 MFMA flash attention (forward with LSE, backward) for gfx950.
//
// Replaces the reference's FlashAttention-2 CUDA dependency
// (galvatron/core/runtime/transformer/attention_impl.py:18-108 and the raw
// _flash_attn_forward/_backward used by ring attention at :561-729).
// LSE is a first-class output (ring-CP merge needs it).
//
// Layout: q [b, sq, hq, D], k/v [b, skv, hkv, D] bf16, GQA (hq % hkv == 0),
// causal = bottom-right aligned. lse [b, hq, sq] fp32 (natural log).
//
// v2 forward structure (guide §B 8-warp ladder, plain HIP):
//   8 waves x 32 q rows (QB=256/workgroup), KV tiles of 64;
//   swapped QK^T (S^T = mfma(K, Q^T)) so each lane owns one q column ->
//   softmax fully in-register (per-lane m/l scalars, exp2 units);
//   P redistributed to PV fragments by cvt_pk_bf16 + permlane32_swap
//   (no LDS round-trip); PV computed as O^T = mfma(V^T, P^T) so the
//   running rescale is a plain per-lane multiply;
//   V staged by rows like K (16-byte loads -> b128 LDS writes) into a
//   swizzled image and read transposed with ds_read_b64_tr_b16 (the v1
//   scalar ds_write_b16 transpose was 14-37% of wave cycles in
//   SQ_LDS_BANK_CONFLICT; v2 staged a second, transposed image from
//   strided 2-byte global loads);
//   async-stage split (T14): next tile's global loads issue before the
//   current tile's compute, LDS writes land after the barrier;
//   per-wave causal tile skip.
// Backward keeps the v1 two-kernel (dq + expanded dkv) structure; K (dq)
// and Q / dO (dkv) are held once and read both by rows and transposed.
//
// This header holds what the four flash modules share: the tile helpers, the
// block bodies and their tile geometry.  Each module (flash_attn.hip dense,
// flash_attn_varlen.hip, flash_attn_qkv.hip, flash_attn_qkv_varlen.hip)
// includes it and adds its own addressing, kernels and launchers.  They are
// separate modules because the bodies are file-local noinline functions
// whose LDS base the compiler folds to a constant while the dense kernel is
// their only caller; a second caller in the same module undoes that folding
// and costs the dense kernels SGPRs and scratch.
#pragma once

#include <type_traits>

#include "common.h"

// [[clang::always_inline]] on a call statement: a body with one call site in
// its module is inlined into it.  The attribute draws -Wignored-attributes.
#pragma clang diagnostic ignored "-Wignored-attributes"
#define FLASH_INLINE_CALL [[clang::always_inline]]

namespace {

// Tile geometry of the three bodies, read by the body and by every kernel
// that sizes its LDS for it; the launchers take the rows per workgroup.
template <int D>
struct FwdTile {
  static constexpr int KB = 64;            // kv tile
  static constexpr int QBF = 256;          // q rows per workgroup (8 waves x 32)
  static constexpr int BUFSZ = 2 * KB * D;  // K rows + V rows (tile_off images)
};
template <int D>
struct DqTile {
  static constexpr int KB = 32;            // kv tile
  static constexpr int QBF = 256;          // q rows per workgroup (8 waves x 32)
  static constexpr int BUFSZ = 2 * KB * D;  // K rows + V rows (tile_off images)
};
template <int D>
struct DkvTile {
  static constexpr int QT = 64;            // q tile (2 mfma halves per stage)
  static constexpr int KBW = 256;          // keys per workgroup (8 waves x 32)
  static constexpr int BUFSZ = 2 * QT * D;  // q rows + dO rows, both phases
};

DEV_INLINE float neg_big() { return -1e30f; }

// Two of the forms that spare VALU work compute the same bits as the plain
// ones but move registers about: skipping the forward's O rescale while no
// running max of the wave moves, and a wave-uniform branch around a masked
// and an unmasked element loop in dq.  A module whose bodies of a
// head dimension D they would cost scratch or occupancy defines the step to
// 0 for that D before it includes this header and keeps the plain form
// (docs/KERNELS.md, "Softmax VALU work").
#ifndef FLASH_SKIP_RESCALE
#define FLASH_SKIP_RESCALE(D) 1
#endif
#ifndef FLASH_DQ_MASK_SPLIT
#define FLASH_DQ_MASK_SPLIT(D) 1
#endif

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// (lo, hi) rounded to bf16 in one word: the vector conversion is a single
// v_cvt_pk_bf16_f32, the rounding of two scalar conversions.
DEV_INLINE unsigned pack_bf16(float lo, float hi) {
  union { bf16x2 h2; unsigned u; } cv;
  cv.h2 = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
  return cv.u;
}

// Combine x of lane l with x of lane l ^ 32 without LDS: permlane32_swap of
// x with itself leaves the lower half's x in every lane of the first word
// and the upper half's in the second.  Both lanes of a pair combine the same
// two values, in either order: use with commutative operations only.
DEV_INLINE void both_halves(float x, float& lower, float& upper) {
  const unsigned u = __float_as_uint(x);
  auto r2 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  lower = __uint_as_float(r2[0]);
  upper = __uint_as_float(r2[1]);
}

// 16 bias values for one 32-key D-layout column: row(r) = 8*(r>>2) +
// 4*hi + (r&3) — each r-quad is 4 contiguous bf16, so 4 8-byte loads
// cover the column.  base must be 4-element aligned (callers pass
// kv0 + 4*hi with kv0 % 32 == 0).  A quad that reaches past the row end is
// loaded from the row's last 4 elements and shifted down, so that the keys
// of a row whose length is no multiple of 4 still get their own bias
// (clamping the quad to a 4-aligned start gave the last limit % 4 keys the
// bias of earlier ones); what is shifted in belongs to masked keys.
DEV_INLINE void load_bias16(const __bf16* brow, int base, int limit,
                            float* out /*16*/) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int idx = base + 8 * g;
    const int cl = min(idx, max(limit - 4, 0));
    union { bf16x4 v; unsigned long long u; } b4;
    b4.v = *reinterpret_cast<const bf16x4*>(brow + cl);
    b4.u >>= 16 * min(idx - cl, 3);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * g + j] = (float)b4.v[j];
  }
}

// ---------------------------------------------------------------------------
// One LDS image per staged [rows][D] tile, read both by rows (ds_read_b128,
// the first product of every body) and by columns (ds_read_b64_tr_b16, the
// second product), so no tile is fetched or held twice.
//
// tile_off(row, ch) is the element offset of 16-byte chunk ch (0..D/8-1) of
// row `row`: 8-row x 32-column subtiles of 512 B, the four chunks of a
// subtile row XORed with bits 2..3 of the row.  The image is dense
// (rows*D elements, no padding).  By the bank rule (bank = (byte/4) % 64
// for b128 / b64 / tr reads, % 32 for writes):
//   row read   lane l reads row l & 31 (+ const), all lanes of a half one
//              ch.  ds_read_b128 is served in groups of 16 lanes made of
//              four aligned 4-lane runs (lanes 0-3, 12-15, 20-27 and so
//              on), i.e. rows 4n..4n+3 for four different n, each n with
//              its own n & 3: row & 3 picks the 64-byte quarter, the XOR
//              key n & 3 the slot in it -> 16 distinct slots, conflict-free;
//   tr read    a 32-lane half holds rows r0..r0+3 (r0 % 4 == 0) x the four
//              chunks of one subtile = 256 contiguous bytes, conflict-free;
//   write      8 consecutive lanes hold two rows x four chunks of a subtile
//              (stage_map) = 128 contiguous bytes, conflict-free.
// Reads that differ by ks / dt / +32 rows differ by constants (or by the
// ks&1 bit inside the XOR), so each kind needs two address registers.
// ---------------------------------------------------------------------------
#define TILE_FN __host__ __device__ __forceinline__ constexpr
template <int D>
TILE_FN int tile_off(int row, int ch) {
  return 8 * D * (row >> 3) + 256 * (ch >> 2) + 32 * (row & 7) +
         8 * ((ch & 3) ^ ((row >> 2) & 3));
}

// staging pack p of thread tid -> (row, chunk): 4 lanes cover 64 B of a
// row, the next 4 the row below, then the next subtile of the row pair; a
// wave covers whole rows (D=128: 4, D=64: 8), so the 16-byte global loads
// stay coalesced.  A thread's packs are 4096/D rows apart in one chunk, so
// they share their addresses up to a constant.
template <int D>
DEV_INLINE void stage_map(int tid, int p, int& row, int& ch) {
  const int rest = tid >> 3;
  row = 2 * (rest / (D / 32)) + ((tid >> 2) & 1) + p * (4096 / D);
  ch = 4 * (rest % (D / 32)) + (tid & 3);
}

// Offset of a row read, tile_off(rb + col, 2*ks + hi) for lane l (col =
// l & 31, hi = l >> 5) and rb % 16 == 0, with the constants split off: one
// lane term, XOR 16 for odd ks.  tile_reads_match_tile_off ties it to
// tile_off at compile time.
template <int D>
TILE_FN int tile_row_off(int lane, int rb, int ks) {
  const int col = lane & 31, hi = lane >> 5;
  const int lane_off = 8 * D * (col >> 3) + 32 * (col & 7) +
                       8 * (hi ^ ((col >> 2) & 3));
  return (lane_off ^ (16 * (ks & 1))) + D * rb + 256 * (ks >> 1);
}

// A/B fragment of a row read: T[rb + col][16*ks + 8*hi + j], j = 0..7
template <int D>
DEV_INLINE bf16x8 tile_row_frag(const __bf16* t, int rb, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(t + tile_row_off<D>(lane, rb, ks));
}

// A fragment of the transposed product: lane l (col = l & 31, hi = l >> 5)
// gets T[row0 + 8*hi + j][32*dt + col], j = 0..7 — what one b128 read of a
// transposed image would give.  ds_read_b64_tr_b16 serves 16-lane groups:
// lane 4q+p of a group supplies the address of row q, columns 4p..4p+3 of a
// 4 x 16 block and lane i receives column i.  Group g = l >> 4 has hi = g>>1
// and columns 32*dt + 16*(g&1) + (0..15), i.e. chunk 4*dt + 2*(g&1) +
// (p>>1), half p & 1; the first read takes rows row0 + 8*hi + q (j = 0..3),
// the second the rows 4 below (j = 4..7).  With row0 % 16 == 0 the XOR key
// (row >> 2) & 3 is 2*hi for the first read and 2*hi + 1 for the second, so
// tile_off reduces to one lane term; the second read is 4 rows (128
// elements) on with the chunk's low bit flipped (XOR 8).
// Every lane's address is 8-byte aligned and inside the tile.  EXEC must be
// all ones: call only under wave-uniform control flow.
template <int D>
TILE_FN int tile_tr_off(int lane, int row0, int dt, int second) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int hi = g >> 1;
  const int lane_off = 8 * D * hi + 32 * q + 16 * ((g & 1) ^ hi) + 4 * p;
  return D * row0 + 256 * dt + (second ? (lane_off ^ 8) + 128 : lane_off);
}

typedef __attribute__((ext_vector_type(4))) short tr_short4;
template <int D>
DEV_INLINE bf16x8 tile_tr_frag(const __bf16* t, int row0, int dt, int lane) {
  typedef __attribute__((address_space(3))) tr_short4 lds_short4;
  union { tr_short4 h[2]; bf16x8 f; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_short4*)(t + tile_tr_off<D>(lane, row0, dt, 0)));
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_short4*)(t + tile_tr_off<D>(lane, row0, dt, 1)));
  return u.f;
}

// The reduced read offsets against tile_off, for every lane, 16-row step,
// ks and dt of a 64-row tile (the largest staged): the row read is chunk
// 2*ks + hi of row rb + col; lane 4q+p of group g of the transposed read
// is half p & 1 of chunk 4*dt + 2*(g&1) + (p>>1) of row row0 + 8*(g>>1) + q
// (+ 4 for the second read), 8-byte aligned.
template <int D>
constexpr bool tile_reads_match_tile_off() {
  for (int lane = 0; lane < 64; ++lane)
    for (int r16 = 0; r16 < 64; r16 += 16) {
      const int col = lane & 31, hi = lane >> 5;
      for (int ks = 0; ks < D / 16; ++ks)
        if (tile_row_off<D>(lane, r16, ks) !=
            tile_off<D>(r16 + col, 2 * ks + hi))
          return false;
      const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
      for (int dt = 0; dt < D / 32; ++dt)
        for (int second = 0; second < 2; ++second) {
          const int off = tile_tr_off<D>(lane, r16, dt, second);
          const int row = r16 + 8 * (g >> 1) + q + 4 * second;
          const int ch = 4 * dt + 2 * (g & 1) + (p >> 1);
          if (off != tile_off<D>(row, ch) + 4 * (p & 1) || off % 4 != 0)
            return false;
        }
    }
  return true;
}
static_assert(tile_reads_match_tile_off<64>() &&
                  tile_reads_match_tile_off<128>(),
              "tile_row_off / tile_tr_off diverge from tile_off");

// four D-layout registers r = 4g..4g+3 are 4 contiguous columns of the
// lane's output row (mfma32_d_row): one 8-byte store
DEV_INLINE void store_d_quad(__bf16* row, int dt, int g, int hi, float a,
                             float b, float c, float d) {
  bf16x4 pk;
  pk[0] = (__bf16)a; pk[1] = (__bf16)b; pk[2] = (__bf16)c; pk[3] = (__bf16)d;
  *reinterpret_cast<bf16x4*>(row + dt * 32 + 8 * g + 4 * hi) = pk;
}

// Where the o / dout rows of a head live.  The dense and varlen kernels keep
// them at q's base and row stride (OutLikeQ: an empty tag, nothing is
// passed and the address arithmetic is unchanged); the packed-QKV kernels
// read q from the linear_qkv buffer while o / dout stay [s, b, hq, D], so
// they pass a base and a stride of their own (OutOwn).
struct OutLikeQ {
  DEV_INLINE long base(long q_base) const { return q_base; }
  DEV_INLINE int stride(int q_stride) const { return q_stride; }
};
struct OutOwn {
  long o_base;
  int o_stride;
  DEV_INLINE long base(long) const { return o_base; }
  DEV_INLINE int stride(int) const { return o_stride; }
};

// Segment `seg` of a cu_seqlens table (token offsets into the batch-major
// flattened [b*s] stream): t0 = cu[seg] is row p0 of batch row bi.  A
// malformed entry (negative offset, past the last row, straddling a row)
// maps to len = 0, "empty", so no address is ever formed from it.
struct Seg {
  int len;  // tokens in the segment (0 = nothing to do)
  int t0, bi, p0;
};

DEV_INLINE Seg cu_seg(const int* __restrict__ cu, int seg, int b, int s) {
  const int t0 = cu[seg];
  const int len = cu[seg + 1] - t0;
  const int bi = t0 / s;
  const int p0 = t0 - bi * s;
  const bool ok = t0 >= 0 && len > 0 && bi < b && p0 + len <= s;
  return Seg{ok ? len : 0, t0, bi, p0};
}

// Head h of batch row bi, from row p0 on, of the linear_qkv output
// [s, b, G, qpg+2, D] (G local kv groups; slots 0..qpg-1 of a group are its
// q heads, slot qpg is k, slot qpg+1 is v), g = h/qpg, slot = h%qpg,
// hq = G*qpg:
//   row stride (q, k, v, dq)   b*G*(qpg+2)*D
//   q / dq base                (((p0*b + bi)*G + g)*(qpg+2) + slot)*D
//   k, v                       slots qpg, qpg+1 of group g: the kernels
//                              pre-offset the k and v pointers by qpg*D,
//                              (qpg+1)*D, so both share the group base
//   o, dout, dk_exp, dv_exp    [s, b, hq, D]: base ((p0*b + bi)*hq + h)*D,
//                              row stride b*hq*D
//   lse, di                    [b, hq, s]: base (bi*hq + h)*s + p0
// Every offset is a multiple of D, so the 16-byte vector accesses stay
// aligned.
struct PackedAddr {
  long q_base, kv_base, o_base, lse_base;
  int qkv_str, o_str;
};

template <int D>
DEV_INLINE PackedAddr packed_addr(int p0, int bi, int h, int b, int s, int G,
                                  int qpg) {
  PackedAddr p;
  const int hq = G * qpg;
  const int g = h / qpg;
  const int slot = h - g * qpg;
  const long row = (long)p0 * b + bi;
  const long grp = (row * G + g) * (qpg + 2);
  p.q_base = (grp + slot) * D;
  p.kv_base = grp * D;
  p.o_base = (row * hq + h) * D;
  p.lse_base = ((long)bi * hq + h) * s + p0;
  p.qkv_str = b * G * (qpg + 2) * D;
  p.o_str = b * hq * D;
  return p;
}

// ---------------------------------------------------------------------------
// forward (v2)
// ---------------------------------------------------------------------------
template <int D, bool BIASED = false, bool WINDOWED = false,
          class OA = OutLikeQ>
__device__ __attribute__((noinline))
void flash_fwd_block(int qblk, const __bf16* __restrict__ q,
                     const __bf16* __restrict__ k,
                     const __bf16* __restrict__ v,
                     __bf16* __restrict__ o, float* __restrict__ lse,
                     __bf16* smem_base, long q_base, long kv_base,
                     long lse_base, int q_stride, int kv_stride, int off,
                     int sq, int skv, float sl2e, bool causal,
                     const __bf16* __restrict__ bias = nullptr,
                     long bias_base = 0, int window = 0, OA oa = OA()) {
  constexpr int KB = FwdTile<D>::KB;
  constexpr int QBF = FwdTile<D>::QBF;
  constexpr int NK = D / 16;        // S^T K-slices
  constexpr int ND = D / 32;        // 32-wide d tiles of O^T
  constexpr int KPT = D / 64;       // staging packs per thread (512 thr)
  constexpr int BUFSZ = FwdTile<D>::BUFSZ;
  __bf16* smem = smem_base;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int col = lane & 31;
  const int hi = lane >> 5;
  const int wid = tid >> 6;
  const int q0w = qblk * QBF + wid * 32;

  // Q fragments (B-operand of S^T): lane holds Q[q0w+col][ks*16 + 8*hi + j]
  bf16x8 qf[NK];
  {
    const int qg = min(q0w + col, sq - 1);
    const __bf16* qp = q + q_base + (long)qg * q_stride + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks)
      qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
  }

  f32x16 ot[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) ot[dt] = (f32x16)(0.f);
  float m_run = neg_big(), l_run = 0.f;

  int kv_end = causal ? min(skv, qblk * QBF + QBF + off) : skv;
  const int kv_last_w = causal ? min(skv, q0w + 32 + off) : skv;  // wave's own
  // sliding window (mistral): keys visible to q are [q+off-window+1, q+off];
  // whole-workgroup start tile + per-wave lower skip + per-element mask
  int kv_begin = 0;
  int kv_first_w = 0;
  if (WINDOWED) {
    kv_begin = max(0, (qblk * QBF + off - window + 1) / KB * KB);
    kv_first_w = max(0, q0w + off - window + 1);
  }

  // staged registers for the next tile
  bf16x8 kst[KPT], vst[KPT];

  // Guards are hoisted out of the load loops: per-element branches around
  // staged loads make hipcc wait vmcnt(0) after EACH load (32 serialized
  // memory round trips per tile, ~13 us/tile measured — guide §5 trap (c)).
  // Fast path is branch-free; the tail tile loads clamped addresses and
  // zeroes by value-select.
  auto stage_load = [&](int kv0) {
    const bool full = (kv0 + KB <= skv);
#pragma unroll
    for (int p = 0; p < KPT; ++p) {
      int row, ch;
      stage_map<D>(tid, p, row, ch);
      const int kg = kv0 + row;
      if (full) {
        const long g = kv_base + (long)kg * kv_stride + ch * 8;
        kst[p] = *reinterpret_cast<const bf16x8*>(k + g);
        vst[p] = *reinterpret_cast<const bf16x8*>(v + g);
      } else {
        const long g = kv_base + (long)min(kg, skv - 1) * kv_stride + ch * 8;
        bf16x8 tk = *reinterpret_cast<const bf16x8*>(k + g);
        bf16x8 tv = *reinterpret_cast<const bf16x8*>(v + g);
        kst[p] = kg < skv ? tk : (bf16x8)(__bf16(0.f));
        vst[p] = kg < skv ? tv : (bf16x8)(__bf16(0.f));
      }
    }
  };
  auto stage_write = [&](int buf) {
    __bf16* k_lds = smem + buf * BUFSZ;
    __bf16* v_lds = k_lds + KB * D;
#pragma unroll
    for (int p = 0; p < KPT; ++p) {
      int row, ch;
      stage_map<D>(tid, p, row, ch);
      *reinterpret_cast<bf16x8*>(k_lds + tile_off<D>(row, ch)) = kst[p];
      *reinterpret_cast<bf16x8*>(v_lds + tile_off<D>(row, ch)) = vst[p];
    }
  };

  stage_load(kv_begin);
  stage_write(0);
  __syncthreads();
  int cur = 0;

  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += KB) {
    const bool have_next = kv0 + KB < kv_end;
    const __bf16* k_lds = smem + cur * BUFSZ;
    const __bf16* v_lds = k_lds + KB * D;
    if (have_next) stage_load(kv0 + KB);  // async: lands at stage_write

    if (kv0 < kv_last_w && kv0 + KB > kv_first_w) {  // per-wave skips
      // ---- S^T = K Q^T (two 32-key tiles) ----
      f32x16 st0 = (f32x16)(0.f), st1 = (f32x16)(0.f);
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        bf16x8 k0 = tile_row_frag<D>(k_lds, 0, ks, lane);
        bf16x8 k1 = tile_row_frag<D>(k_lds, 32, ks, lane);
        st0 = mfma32_bf16(k0, qf[ks], st0);
        st1 = mfma32_bf16(k1, qf[ks], st1);
      }

      // ---- scale (+ additive bias, + mask on straddle/tail tiles) ----
      float pv[32];
      const int qg = q0w + col;
      const __bf16* brow = nullptr;
      if (BIASED)
        brow = bias + bias_base + (long)min(qg, sq - 1) * skv;
      const bool need_mask =
          (causal && kv0 + KB > q0w + off + 1) || (kv0 + KB > skv) ||
          (WINDOWED && kv0 < q0w + 32 + off - window + 1);
      constexpr float LOG2E = 1.4426950408889634f;
      float bv[32];
      if (BIASED) {
        load_bias16(brow, kv0 + 4 * hi, skv, bv);
        load_bias16(brow, kv0 + 32 + 4 * hi, skv, bv + 16);
      }
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key0 = kv0 + mfma32_d_row(lane, r);
          float x0 = st0[r] * sl2e, x1 = st1[r] * sl2e;
          if (BIASED) {
            x0 += LOG2E * bv[r];
            x1 += LOG2E * bv[16 + r];
          }
          if (key0 >= skv || (causal && key0 > qg + off) ||
              (WINDOWED && key0 <= qg + off - window)) x0 = neg_big();
          if (key0 + 32 >= skv || (causal && key0 + 32 > qg + off) ||
              (WINDOWED && key0 + 32 <= qg + off - window))
            x1 = neg_big();
          pv[r] = x0;
          pv[16 + r] = x1;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          pv[r] = st0[r] * sl2e + (BIASED ? LOG2E * bv[r] : 0.f);
          pv[16 + r] = st1[r] * sl2e + (BIASED ? LOG2E * bv[16 + r] : 0.f);
        }
      }

      // ---- in-register online softmax (per-lane q column) ----
      float mt = pv[0];
#pragma unroll
      for (int i = 1; i < 32; ++i) mt = fmaxf(mt, pv[i]);
      float m_lo, m_hi;
      both_halves(mt, m_lo, m_hi);
      mt = fmaxf(m_lo, m_hi);
      const float mn = fmaxf(m_run, mt);
      // exp2 here is the bare v_exp_f32.  exp2f() wraps it for results in
      // the denormal range: for an argument >= -126 the wrapper adds 0 and
      // scales by 2^0, i.e. returns this instruction's result; below -126
      // it returns a denormal where the instruction returns 0.  Such a P or
      // alpha is at most 2^-126 beside a row sum >= 1 (the row's maximum
      // contributes exp2(0)), so it cannot move an fp32 accumulator.
      const float alpha = (m_run <= neg_big())
                              ? 0.f : __builtin_amdgcn_exp2f(m_run - mn);
      // A row is dead while every key seen so far is masked: mn and all of
      // pv are neg_big().  Subtracting 0 there gives exp2(neg_big()) = 0
      // exactly; one select per tile, not one per element.
      const float msub = (mn <= neg_big()) ? 0.f : mn;
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        pv[i] = __builtin_amdgcn_exp2f(pv[i] - msub);
        ps += pv[i];
      }
      float ps_lo, ps_hi;
      both_halves(ps, ps_lo, ps_hi);
      ps = ps_lo + ps_hi;
      l_run = l_run * alpha + ps;
      m_run = mn;
      // alpha == 1 in every lane (no running max of the wave moved): the
      // rescale would multiply by one.  The ballot is wave-uniform.
      if (!FLASH_SKIP_RESCALE(D) ||
          __builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
      }

      // ---- P -> bf16 PV fragments via cvt_pk + permlane32_swap ----
      // frag[ks] holds P[q=lane][16*ks + 8*hi + j], j=0..7, as 4 u32 words
      unsigned w[16];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float* pt = pv + 16 * t;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            // pairs (8i+2g, 8i+2g+1) with (8i+2g+4, 8i+2g+5)
            unsigned a = pack_bf16(pt[8 * i + 2 * g], pt[8 * i + 2 * g + 1]);
            unsigned bb = pack_bf16(pt[8 * i + 2 * g + 4],
                                    pt[8 * i + 2 * g + 5]);
            auto r2 = __builtin_amdgcn_permlane32_swap(a, bb, false, false);
            // words of frag (2t + i): position 2g -> r2[0], 2g+1... see map
            w[(2 * t + i) * 4 + g] = r2[0];      // keys (8hi + 2g, +1)
            w[(2 * t + i) * 4 + 2 + g] = r2[1];  // keys (8hi + 4 + 2g, +1)
          }
        }
      }

      // ---- O^T += V^T P^T ----
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        union { unsigned u[4]; bf16x8 f; } pb;
#pragma unroll
        for (int g = 0; g < 4; ++g) pb.u[g] = w[ks * 4 + g];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          bf16x8 va = tile_tr_frag<D>(v_lds, ks * 16, dt, lane);
          ot[dt] = mfma32_bf16(va, pb.f, ot[dt]);
        }
      }
    }

    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: O^T[d][q=lane], per-lane stats ----
  const int qg = q0w + col;
  if (qg < sq) {
    const float invl = l_run > 0.f ? 1.f / l_run : 0.f;
    __bf16* orow = o + oa.base(q_base) + (long)qg * oa.stride(q_stride);
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        orow[dt * 32 + mfma32_d_row(lane, r)] = (__bf16)(ot[dt][r] * invl);
    if (hi == 0)
      lse[lse_base + qg] =
          l_run > 0.f ? (m_run + log2f(l_run)) * 0.6931471805599453f
                      : -INFINITY;
  }
}

// ---------------------------------------------------------------------------
// backward dQ (v2): same swapped structure as the forward — 8 waves x 32 q
// rows, per-lane lse/di scalars, dS^T packed to MFMA fragments with
// cvt_pk + permlane32_swap (no dS LDS round-trip, no per-row stat arrays:
// the v1 form spilled 34 dwords/lane to scratch).
// dQ^T[d][q] += K^T dS accumulated in D-layout, epilogue like the forward.
// ---------------------------------------------------------------------------
template <int D, bool BIASED = false, bool WINDOWED = false,
          class OA = OutLikeQ>
__device__ __attribute__((noinline))
void flash_bwd_dq_block(int qblk, const __bf16* __restrict__ dout,
                        const __bf16* __restrict__ q,
                        const __bf16* __restrict__ k,
                        const __bf16* __restrict__ v,
                        const float* __restrict__ lse,
                        const float* __restrict__ di,
                        __bf16* __restrict__ dq, __bf16* smem_base,
                        long q_base, long kv_base, long lse_base,
                        int q_stride, int kv_stride, int off, int sq,
                        int skv, float scale, bool causal,
                        const __bf16* __restrict__ bias = nullptr,
                        long bias_base = 0, int window = 0, OA oa = OA()) {
  constexpr int KB = DqTile<D>::KB;
  constexpr int QBF = DqTile<D>::QBF;
  constexpr int NK = D / 16;
  constexpr int ND = D / 32;
  constexpr int KPT = (KB * D / 8 + 511) / 512;  // row packs per thread
  constexpr int BUFSZ = DqTile<D>::BUFSZ;
  __bf16* smem = smem_base;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int col = lane & 31;
  const int hi = lane >> 5;
  const int wid = tid >> 6;
  const int q0w = qblk * QBF + wid * 32;

  bf16x8 qf[NK], dof[NK];
  float lse_c, di_c;
  {
    const int qg = min(q0w + col, sq - 1);
    const __bf16* qp = q + q_base + (long)qg * q_stride + 8 * hi;
    const __bf16* dop = dout + oa.base(q_base) +
                        (long)qg * oa.stride(q_stride) + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
      dof[ks] = *reinterpret_cast<const bf16x8*>(dop + ks * 16);
    }
    const float l0 = lse[lse_base + qg];
    const float d0 = di[lse_base + qg];
    const bool live = q0w + col < sq;
    lse_c = live ? l0 : INFINITY;  // exp(x - inf) = 0 -> dead rows silent
    di_c = live ? d0 : 0.f;
  }

  f32x16 dq_acc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) dq_acc[dt] = (f32x16)(0.f);

  const int kv_end = causal ? min(skv, qblk * QBF + QBF + off) : skv;
  const int kv_last_w = causal ? min(skv, q0w + 32 + off) : skv;
  int kv_begin = 0, kv_first_w = 0;
  if (WINDOWED) {
    kv_begin = max(0, (qblk * QBF + off - window + 1) / KB * KB);
    kv_first_w = max(0, q0w + off - window + 1);
  }

  bf16x8 kst[KPT], vst_r[KPT];

  auto stage_load = [&](int kv0) {
    const bool full = (kv0 + KB <= skv);
#pragma unroll
    for (int p = 0; p < KPT; ++p) {
      const int idx = tid + p * 512;
      if (idx >= KB * D / 8) break;
      int row, ch;
      stage_map<D>(tid, p, row, ch);
      const int kg = full ? kv0 + row : min(kv0 + row, skv - 1);
      kst[p] = *reinterpret_cast<const bf16x8*>(
          k + kv_base + (long)kg * kv_stride + ch * 8);
      vst_r[p] = *reinterpret_cast<const bf16x8*>(
          v + kv_base + (long)kg * kv_stride + ch * 8);
      if (!full && kv0 + row >= skv) {
        kst[p] = (bf16x8)(__bf16(0.f));
        vst_r[p] = (bf16x8)(__bf16(0.f));
      }
    }
  };
  auto stage_write = [&](int buf) {
    __bf16* k_lds = smem + buf * BUFSZ;
    __bf16* v_lds = k_lds + KB * D;
#pragma unroll
    for (int p = 0; p < KPT; ++p) {
      const int idx = tid + p * 512;
      if (idx >= KB * D / 8) break;
      int row, ch;
      stage_map<D>(tid, p, row, ch);
      *reinterpret_cast<bf16x8*>(k_lds + tile_off<D>(row, ch)) = kst[p];
      *reinterpret_cast<bf16x8*>(v_lds + tile_off<D>(row, ch)) = vst_r[p];
    }
  };

  stage_load(kv_begin);
  stage_write(0);
  __syncthreads();
  int cur = 0;

  const float sl2e = scale;  // bwd stays in natural-log units (lse is ln)

  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += KB) {
    const bool have_next = kv0 + KB < kv_end;
    const __bf16* k_lds = smem + cur * BUFSZ;
    const __bf16* v_lds = k_lds + KB * D;
    if (have_next) stage_load(kv0 + KB);

    if (kv0 < kv_last_w && kv0 + KB > kv_first_w) {
      // S^T = K Q^T ; dP^T = V dO^T
      f32x16 st = (f32x16)(0.f), dp = (f32x16)(0.f);
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        bf16x8 kb = tile_row_frag<D>(k_lds, 0, ks, lane);
        st = mfma32_bf16(kb, qf[ks], st);
        bf16x8 vb = tile_row_frag<D>(v_lds, 0, ks, lane);
        dp = mfma32_bf16(vb, dof[ks], dp);
      }

      // dS^T = P^T (dP^T - Di), branchless mask
      const int qg = q0w + col;
      const __bf16* brow = nullptr;
      if (BIASED)
        brow = bias + bias_base + (long)min(qg, sq - 1) * skv;
      // The test is the same in every lane of the wave, but q0w comes from
      // the thread index and a noinline body gets its arguments in vector
      // registers: read it from the first lane, so that it is a scalar
      // branch around two plain loops and not an exec-masked region per
      // element.
      constexpr bool SPLIT = FLASH_DQ_MASK_SPLIT(D);
      bool need_mask =
          (causal && kv0 + KB > q0w + off + 1) || (kv0 + KB > skv) ||
          (WINDOWED && kv0 < q0w + 32 + off - window + 1);
      if (SPLIT) need_mask = __builtin_amdgcn_readfirstlane(need_mask);
      float dsv[16];
      float bv[16];
      if (BIASED)
        load_bias16(brow, kv0 + 4 * hi, skv, bv);
      auto element = [&](int r, bool masked) {
        float sc = st[r] * sl2e;
        if (BIASED) sc += bv[r];
        const float e = __expf(sc - lse_c);
        float pr = e;
        if (masked) {
          const int key = kv0 + mfma32_d_row(lane, r);
          const bool ok = key < skv && !(causal && key > qg + off) &&
                          !(WINDOWED && key <= qg + off - window);
          pr = ok ? e : 0.f;
        }
        dsv[r] = pr * (dp[r] - di_c) * scale;
      };
      if (!SPLIT) {
#pragma unroll
        for (int r = 0; r < 16; ++r) element(r, need_mask);
      } else if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) element(r, true);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) element(r, false);
      }

      // pack dS^T to MFMA B-fragments (cvt_pk + permlane32_swap)
      unsigned w[8];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          unsigned a = pack_bf16(dsv[8 * i + 2 * g], dsv[8 * i + 2 * g + 1]);
          unsigned bb = pack_bf16(dsv[8 * i + 2 * g + 4],
                                  dsv[8 * i + 2 * g + 5]);
          auto r2 = __builtin_amdgcn_permlane32_swap(a, bb, false, false);
          w[i * 4 + g] = r2[0];
          w[i * 4 + 2 + g] = r2[1];
        }
      }

      // dQ^T += K^T dS
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        union { unsigned u[4]; bf16x8 f; } db;
#pragma unroll
        for (int g = 0; g < 4; ++g) db.u[g] = w[kh * 4 + g];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          bf16x8 ka = tile_tr_frag<D>(k_lds, kh * 16, dt, lane);
          dq_acc[dt] = mfma32_bf16(ka, db.f, dq_acc[dt]);
        }
      }
    }

    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: dQ^T[d][q=lane]
  const int qg = q0w + col;
  if (qg < sq) {
    __bf16* dqr = dq + q_base + (long)qg * q_stride;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store_d_quad(dqr, dt, g, hi, dq_acc[dt][4 * g], dq_acc[dt][4 * g + 1],
                     dq_acc[dt][4 * g + 2], dq_acc[dt][4 * g + 3]);
  }
}


// ---------------------------------------------------------------------------
// backward dK/dV (v5): expanded per q-head (host reduces over the GQA
// group), 8 waves x 32 keys (256 keys/workgroup), async-staged q tiles.
//
// v5 = two SEQUENTIAL phases in one kernel (dV pass, then dK pass), each
// with only 64 accumulator VGPRs so the wave's K (and V) fragments are
// PRELOADED into loop-invariant registers.  The v3/v4 single-pass variant
// kept 128 accumulator VGPRs live (dkt+dvt) and the compiler was forced
// to re-load every K/V fragment from L2 one at a time with a full
// vmcnt(0) drain before EACH MFMA — rocprofv3 PMC showed the waves parked
// (SQ_WAIT_ANY 73.7% of wave cycles, MFMA busy 28%) while the healthy dq
// kernel sits at 46%/51%.  The S matrix is computed twice (once per
// phase): +25% MFMA work for register room — measured net win.
//   phase dV:  S = mfma(Q_frag[from q_lds rows], K^T_frag[kfr regs])
//              dV^T[d][key] = mfma(dO^T_frag[from t_lds], P_frag[permlane])
//   phase dK:  S again; dP = mfma(dO_frag[from do_lds rows], V^T[vfr regs])
//              dK^T[d][key] = mfma(Q^T_frag[from t_lds], dS_frag[permlane])
// ---------------------------------------------------------------------------
template <int D, bool DKPH, bool BIASED = false, bool WINDOWED = false,
          class OA = OutLikeQ>
__device__ __attribute__((noinline))
void flash_bwd_dkv_phase(int kvblk, const __bf16* __restrict__ dout,
                         const __bf16* __restrict__ q,
                         const __bf16* __restrict__ k,
                         const __bf16* __restrict__ v,
                         const float* __restrict__ lse,
                         const float* __restrict__ di,
                         __bf16* __restrict__ dk_exp,
                         __bf16* __restrict__ dv_exp, __bf16* smem_base,
                         float* lsedi_base, long q_base, long kv_base,
                         long dkv_base, long lse_base, int q_stride,
                         int kv_stride, int dkv_stride, int off, int sq,
                         int skv, float scale, bool causal,
                         const __bf16* __restrict__ bias = nullptr,
                         float* __restrict__ dbias = nullptr,
                         long bias_base = 0, int window = 0, OA oa = OA()) {
  constexpr int QT = DkvTile<D>::QT;
  constexpr int KBW = DkvTile<D>::KBW;
  constexpr int NK = D / 16;
  constexpr int ND = D / 32;
  constexpr int QPT = (QT * D / 8 + 511) / 512;   // row packs per thread

  // LDS per buffer: q rows + dO rows (tile_off images), in both phases
  constexpr int BUFSZ = DkvTile<D>::BUFSZ;
  __bf16* smem = smem_base;
  float (*lse_lds)[QT] = reinterpret_cast<float (*)[QT]>(lsedi_base);
  float (*di_lds)[QT] = reinterpret_cast<float (*)[QT]>(lsedi_base + 2 * QT);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int col = lane & 31;   // this wave's key index
  const int hi = lane >> 5;
  const int k0w = kvblk * KBW + wid * 32;  // this wave's first key row

  // loop-invariant K (and V) fragments, preloaded into registers — the
  // whole point of the phase split
  const int kg_f = min(k0w + col, skv - 1);
  bf16x8 kfr[NK];
  bf16x8 vfr[DKPH ? NK : 1];
  {
    const __bf16* kp_f = k + kv_base + (long)kg_f * kv_stride + 8 * hi;
    const __bf16* vp_f = v + kv_base + (long)kg_f * kv_stride + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      kfr[ks] = *reinterpret_cast<const bf16x8*>(kp_f + ks * 16);
      if (DKPH)
        vfr[ks] = *reinterpret_cast<const bf16x8*>(vp_f + ks * 16);
    }
  }

  f32x16 acc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) acc[dt] = (f32x16)(0.f);

  // first q tile that can attend any key of this block (per-wave causal
  // skipping happens per 32-q half inside the loop); with a sliding
  // window, also the LAST q that can see any of this block's keys:
  // q <= key - off + window - 1
  int qstart = 0;
  if (causal) qstart = max(0, ((kvblk * KBW - off) / QT) * QT);
  int qstop = sq;
  if (WINDOWED)
    qstop = min(sq, kvblk * KBW + KBW - 1 - off + window);

  // staged registers: q rows and dO rows.  The dV phase reads the dO image
  // only by columns, the dK phase reads it by rows and the q image both ways
  bf16x8 qst[QPT], dost[QPT];
  float lse_st, di_st;
  const long do_base = oa.base(q_base);
  const int do_stride = oa.stride(q_stride);

  auto stage_load = [&](int qt0) {
    const bool full = (qt0 + QT <= sq);
#pragma unroll
    for (int p = 0; p < QPT; ++p) {
      const int idx = tid + p * 512;
      if (idx >= QT * D / 8) break;
      int row, ch;
      stage_map<D>(tid, p, row, ch);
      const int qg = full ? qt0 + row : min(qt0 + row, sq - 1);
      qst[p] = *reinterpret_cast<const bf16x8*>(
          q + q_base + (long)qg * q_stride + ch * 8);
      dost[p] = *reinterpret_cast<const bf16x8*>(
          dout + do_base + (long)qg * do_stride + ch * 8);
      if (!full && qt0 + row >= sq) {
        qst[p] = (bf16x8)(__bf16(0.f));
        dost[p] = (bf16x8)(__bf16(0.f));
      }
    }
    if (tid < QT) {
      const int qg = qt0 + tid;
      lse_st = qg < sq ? lse[lse_base + qg] : INFINITY;
      if (DKPH) di_st = qg < sq ? di[lse_base + qg] : 0.f;
    }
  };
  auto stage_write = [&](int buf) {
    __bf16* q_lds = smem + buf * BUFSZ;
    __bf16* do_lds = q_lds + QT * D;
#pragma unroll
    for (int p = 0; p < QPT; ++p) {
      const int idx = tid + p * 512;
      if (idx >= QT * D / 8) break;
      int row, ch;
      stage_map<D>(tid, p, row, ch);
      *reinterpret_cast<bf16x8*>(q_lds + tile_off<D>(row, ch)) = qst[p];
      *reinterpret_cast<bf16x8*>(do_lds + tile_off<D>(row, ch)) = dost[p];
    }
    if (tid < QT) {
      lse_lds[buf][tid] = lse_st;
      if (DKPH) di_lds[buf][tid] = di_st;
    }
  };

  stage_load(qstart);
  stage_write(0);
  __syncthreads();
  int cur = 0;

  for (int qt0 = qstart; qt0 < qstop; qt0 += QT) {
    const bool have_next = qt0 + QT < qstop;
    const __bf16* q_lds = smem + cur * BUFSZ;
    const __bf16* do_lds = q_lds + QT * D;
    const __bf16* t_lds = DKPH ? q_lds : do_lds;  // read by columns
    if (have_next) stage_load(qt0 + QT);

    // two 32-q mfma halves per staged tile
#pragma unroll
    for (int qh = 0; qh < QT / 32; ++qh) {
      const int q0h = qt0 + qh * 32;
      // per-half skips (wave-uniform): any key of this wave live?
      if (causal && q0h + 31 + off < k0w) continue;
      if (WINDOWED && q0h + off - window + 1 > k0w + 31) continue;
      if (q0h >= sq) continue;

      // S = Q K^T (; dP = dO V^T)  D-layout rows=q(crow), cols=key(lane);
      // A-frag lane l&31 = q row of the half, B-frag lane = key
      f32x16 s_acc = (f32x16)(0.f), dp_acc = (f32x16)(0.f);
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        bf16x8 qa = tile_row_frag<D>(q_lds, qh * 32, ks, lane);
        s_acc = mfma32_bf16(qa, kfr[ks], s_acc);
        if (DKPH) {
          bf16x8 doa = tile_row_frag<D>(do_lds, qh * 32, ks, lane);
          dp_acc = mfma32_bf16(doa, vfr[ks], dp_acc);
        }
      }

      float wv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = mfma32_d_row(lane, r);
        const float lse_r = lse_lds[cur][qh * 32 + qrow];
        float sc = s_acc[r] * scale;
        if (BIASED) {
          const long bq = (long)min(q0h + qrow, sq - 1);
          sc += (float)bias[bias_base + bq * skv +
                            min(k0w + col, skv - 1)];
        }
        const float e = __expf(sc - lse_r);
        float p = e;
        if (WINDOWED) {
          const int keyg = k0w + col;
          const int qo = q0h + qrow + off;
          const bool ok = keyg < skv && (!causal || keyg <= qo) &&
                          keyg > qo - window;
          p = ok ? e : 0.f;
        } else if (causal) {
          const int keyg = k0w + col;
          const bool ok = keyg < skv && keyg <= q0h + qrow + off;
          p = ok ? e : 0.f;
        } else if (k0w + col >= skv) {
          p = 0.f;
        }
        if (DKPH) {
          const float di_r = di_lds[cur][qh * 32 + qrow];
          const float t = p * (dp_acc[r] - di_r);
          if (BIASED) {
            // d(bias) = dS (un-scaled); batch contributions accumulate
            // via fp32 atomics into [hq, sq, skv]
            const int bq = q0h + qrow, bk = k0w + col;
            if (bq < sq && bk < skv)
              atomicAdd(dbias + bias_base + (long)bq * skv + bk, t);
          }
          wv[r] = t * scale;
        } else {
          wv[r] = p;
        }
      }

      // convert P / dS (D-layout rows=q) to B-fragments (lane=key,
      // in-lane=q) via cvt_pk + permlane32_swap
      unsigned w[8];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          unsigned a = pack_bf16(wv[8 * i + 2 * g], wv[8 * i + 2 * g + 1]);
          unsigned bb = pack_bf16(wv[8 * i + 2 * g + 4],
                                  wv[8 * i + 2 * g + 5]);
          auto r2 = __builtin_amdgcn_permlane32_swap(a, bb, false, false);
          w[i * 4 + g] = r2[0];
          w[i * 4 + 2 + g] = r2[1];
        }
      }

      // dV^T += dO^T P  /  dK^T += Q^T dS  (two K=16 slices of the half)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        union { unsigned u[4]; bf16x8 f; } fb;
#pragma unroll
        for (int g = 0; g < 4; ++g) fb.u[g] = w[kh * 4 + g];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          bf16x8 ta = tile_tr_frag<D>(t_lds, qh * 32 + kh * 16, dt, lane);
          acc[dt] = mfma32_bf16(ta, fb.f, acc[dt]);
        }
      }
    }

    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: dK^T/dV^T D-layout rows=d(crow), cols=key(lane)
  const int keyg = k0w + col;
  if (keyg < skv) {
    __bf16* outr = (DKPH ? dk_exp : dv_exp) + dkv_base +
                   (long)keyg * dkv_stride;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store_d_quad(outr, dt, g, hi, acc[dt][4 * g], acc[dt][4 * g + 1],
                     acc[dt][4 * g + 2], acc[dt][4 * g + 3]);
  }
}

template <int D, bool BIASED = false, bool WINDOWED = false,
          class OA = OutLikeQ>
__device__ void flash_bwd_dkv_block(
    int kvblk, const __bf16* __restrict__ dout, const __bf16* __restrict__ q,
    const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ di,
    __bf16* __restrict__ dk_exp, __bf16* __restrict__ dv_exp,
    __bf16* smem_base, float* lsedi_base, long q_base, long kv_base,
    long dkv_base, long lse_base, int q_stride, int kv_stride,
    int dkv_stride, int off, int sq, int skv, float scale, bool causal,
    const __bf16* bias = nullptr, float* dbias = nullptr,
    long bias_base = 0, int window = 0, OA oa = OA()) {
  flash_bwd_dkv_phase<D, false, BIASED, WINDOWED, OA>(
      kvblk, dout, q, k, v, lse, di, dk_exp, dv_exp, smem_base, lsedi_base,
      q_base, kv_base, dkv_base, lse_base, q_stride, kv_stride, dkv_stride,
      off, sq, skv, scale, causal, bias, dbias, bias_base, window, oa);
  __syncthreads();
  flash_bwd_dkv_phase<D, true, BIASED, WINDOWED, OA>(
      kvblk, dout, q, k, v, lse, di, dk_exp, dv_exp, smem_base, lsedi_base,
      q_base, kv_base, dkv_base, lse_base, q_stride, kv_stride, dkv_stride,
      off, sq, skv, scale, causal, bias, dbias, bias_base, window, oa);
}

// Host: run f with the head dimension as a compile-time constant,
// f(std::integral_constant<int, D>()).  The bindings admit d = 64 | 128 only.
template <class F>
void with_head_dim(int d, F f) {
  if (d == 64)
    f(std::integral_constant<int, 64>());
  else
    f(std::integral_constant<int, 128>());
}

// Host: complementary-pair causal scheduling (block x also runs block
// nblk-1-x) halves grid.x; skipped when the halved grid underfills the
// 256-CU chip (small-seq shapes).
inline bool flash_paired(int nblk, int b, int hq, bool causal) {
  return causal && ((nblk + 1) / 2) * (long)b * hq >= 256;
}

}  // namespace
