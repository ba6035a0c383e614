// Batched single-token decode attention for gfx950 (serving path).
//
//   q [n, hq, D] bf16, caches [S, max_s, hkv, D] bf16, o [n, hq, D] bf16
//   lengths, slots: int32 [n] in device memory.  Row i attends to positions
//   [start_i, len_i) of cache row slots[i]; len_i = min(lengths[i], max_len),
//   start_i = max(0, len_i - window) (0 without a window).
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
// the others once, after the last tile, in LDS.  Per 32-key step of a wave
// (v_mfma_f32_16x16x32_bf16; lane l: g = l >> 4, c = l & 15):
//
//   S^T[keys x heads] = K . Q^T   two 16-key blocks x D/32 k-steps.  The A
//       fragment is 8 contiguous bf16 of key row 16*blk + c, straight from
//       global memory with a 16-byte load; the B fragment is q of head c
//       (zero for c >= qpg), held in registers.  D layout: register r of
//       block blk is key 16*blk + 4g + r of head c, so a lane's scores
//       belong to one head and the running max and sum are per-lane scalars;
//       the tile max is combined across the four 16-lane groups, the sum
//       only once at the end.
//   O^T[d x heads] += V^T . P^T   D/16 row blocks.  The sum over keys does
//       not depend on the order, so k-slot 8g + j of the product is key
//       4g + j (j < 4) or 16 + 4g + j - 4: the P^T fragment is then the
//       lane's own eight weights.  V^T is read with that same map by two
//       ds_read_b64_tr_b16 per row block from the wave's own LDS image of
//       its 32 V rows (staged by rows with 16-byte loads, row stride D + 16
//       elements: the four rows of a 16-lane group are 32 B apart modulo
//       256, so the reads do not collide).
//
// The weights enter the second product as three bf16 terms (p = hi + lo +
// lo2, each the rounding of what the ones before left over): one bf16 term
// alone is a relative error of 2^-9 per weight, which the decode element
// rule (ulp of o plus 2^-20 of the absolute-value sum) does not allow where
// the weighted V rows cancel.  MFMA work is far below the memory time, so the
// two extra products are free.
//
// The next step's K fragments and V rows are loaded into registers after the
// first product of the current one, before its softmax and second product.
// Only a step that reaches past the chunk's end clamps its row addresses and
// selects zeros for V and -1e30 for the scores.
//
// LDS is a constant of the tile (4 x 32 x (D + 16) bf16 + 512 B), reused for
// the final combine of the waves.  With n_chunks > 1 every non-empty chunk
// writes an unnormalised partial [D] + (m, l) in fp32 and the merge kernel
// reads, per row, only the chunks that row has.
#include "common.h"

// Packed fp32 instructions are kept out of this module's device code.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif
#include "decode_rows.h"

namespace {

constexpr int DB_WAVES = 4;
constexpr int DB_WKEYS = 32;                    // keys per wave step
constexpr int DB_TILE = DB_WAVES * DB_WKEYS;    // keys per workgroup tile
constexpr float DB_NEG = -1e30f;

typedef __attribute__((ext_vector_type(4))) short db_short4;
typedef __attribute__((address_space(3))) db_short4 db_lds_short4;

// K fragments and V rows of the wave's 32 keys from key k0 on.  FULL: all 32
// are inside [.., p1).  Otherwise rows past p1 - 1 are read from row p1 - 1
// (inside the chunk) and V is zeroed by value; the scores are masked later.
template <int D, bool FULL>
DEV_INLINE void db_load(const __bf16* __restrict__ kb,
                        const __bf16* __restrict__ vb, int rs, int k0, int p1,
                        int lane, bf16x8 (&kf)[2][D / 32],
                        bf16x8 (&vr)[D / 16]) {
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    int key = k0 + 16 * blk + c;
    if (!FULL) key = min(key, p1 - 1);
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
    const int kc = FULL ? key : min(key, p1 - 1);
    bf16x8 v = *reinterpret_cast<const bf16x8*>(vb + (long)kc * rs +
                                                8 * (lane % CH));
    if (!FULL && key >= p1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
    }
    vr[i] = v;
  }
}

template <int D>
__global__ __launch_bounds__(256) void decode_batched_kernel(
    const __bf16* __restrict__ q,    // [n, hq, D]
    const __bf16* __restrict__ kc,   // [S, max_s, hkv, D]
    const __bf16* __restrict__ vc,
    __bf16* __restrict__ o,          // [n, hq, D]
    float* __restrict__ part,        // [n*hq, n_chunks, D+2]; null: write o
    const int* __restrict__ lengths, const int* __restrict__ slots, int hq,
    int hkv, int S, int max_s, int max_len, int window, int chunk,
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
  const int p0 = r.start + ci * chunk;
  if (p0 >= r.len) {                 // workgroup-uniform; also the empty row
    if (r.len == 0 && part == nullptr)
      for (int i = tid; i < qpg * D; i += 256)
        o[((long)row * hq + hk * qpg) * D + i] = (__bf16)0.f;
    return;
  }
  const int p1 = min(p0 + chunk, r.len);

  // the wave index as a scalar: the step loop branches on it
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const int rs = hkv * D;
  const long base = ((long)r.slot * max_s * hkv + hk) * D;
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
  if (k0 < p1) {
    if (k0 + DB_WKEYS <= p1)
      db_load<D, true>(kb, vb, rs, k0, p1, lane, kf, vr);
    else
      db_load<D, false>(kb, vb, rs, k0, p1, lane, kf, vr);
  }
  while (k0 < p1) {                  // wave-uniform
#pragma unroll
    for (int i = 0; i < NDT; ++i)
      *reinterpret_cast<bf16x8*>(vimg + wr_off + i * RPL * VSTR) = vr[i];
    db_wave_fence();

    f32x4 sacc[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      sacc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks)
        sacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            kf[blk][ks], qf[ks], sacc[blk], 0, 0, 0);
    }

    const int kn = k0 + DB_TILE;
    if (kn < p1) {
      if (kn + DB_WKEYS <= p1)
        db_load<D, true>(kb, vb, rs, kn, p1, lane, kf, vr);
      else
        db_load<D, false>(kb, vb, rs, kn, p1, lane, kf, vr);
    }

    float s[8];
    float mx = DB_NEG;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = k0 + 16 * (j >> 2) + 4 * g + (j & 3);
      s[j] = key < p1 ? sacc[j >> 2][j & 3] * scale : DB_NEG;
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
      const __bf16 lo = (__bf16)r1;
      ph[j] = h;
      pl[j] = lo;
      pl2[j] = (__bf16)(r1 - (float)lo);
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
    k0 = kn;
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
      o[bh * D + d] = (__bf16)(acc / gl);
    } else {
      float* out = part + (bh * gridDim.x + ci) * (D + 2);
      out[d] = acc;
      if (d == 0) { out[D] = gm; out[D + 1] = gl; }
    }
  }
}

// One block of D threads per (row, q head): log-sum-exp merge of the chunks
// this row has, counted from its own length; the others were never written.
template <int D>
__global__ void decode_batched_merge_kernel(
    const float* __restrict__ part, __bf16* __restrict__ o,
    const int* __restrict__ lengths, const int* __restrict__ slots, int hq,
    int S, int max_len, int window, int chunk, int n_chunks) {
  const int bh = blockIdx.x, tid = threadIdx.x;
  const DbRow r = db_row(lengths, slots, bh / hq, S, max_len, window);
  if (r.len == 0) {
    o[(long)bh * D + tid] = (__bf16)0.f;
    return;
  }
  const int nch = min((r.len - r.start + chunk - 1) / chunk, n_chunks);
  const float* base = part + (long)bh * n_chunks * (D + 2);
  float gm = DB_NEG;
  for (int ci = 0; ci < nch; ++ci) gm = fmaxf(gm, base[ci * (D + 2) + D]);
  float gl = 0.f, acc = 0.f;
  for (int ci = 0; ci < nch; ++ci) {
    const float f = __expf(base[ci * (D + 2) + D] - gm);
    gl += f * base[ci * (D + 2) + D + 1];
    acc += f * base[ci * (D + 2) + tid];
  }
  o[(long)bh * D + tid] = (__bf16)(acc / gl);
}

template <int D>
void launch(const __bf16* q, const __bf16* kc, const __bf16* vc, __bf16* o,
            float* part, const int* lengths, const int* slots, int n, int hq,
            int hkv, int S, int max_s, int max_len, int window, int chunk,
            int n_chunks, float scale, hipStream_t st) {
  hipLaunchKernelGGL((decode_batched_kernel<D>), dim3(n_chunks, hkv, n),
                     dim3(256), 0, st, q, kc, vc, o,
                     n_chunks > 1 ? part : nullptr, lengths, slots, hq, hkv,
                     S, max_s, max_len, window, chunk, scale);
  if (n_chunks > 1)
    hipLaunchKernelGGL((decode_batched_merge_kernel<D>), dim3(n * hq),
                       dim3(D), 0, st, part, o, lengths, slots, hq, S,
                       max_len, window, chunk, n_chunks);
}

}  // namespace

int decode_batched_tile() { return DB_TILE; }

// chunk is a multiple of decode_batched_tile() with chunk * n_chunks >= the
// longest window; part is [n*hq, n_chunks, d+2] fp32 (unused, may be null,
// when n_chunks == 1).
void decode_attn_batched_launch(const __bf16* q, const __bf16* kc,
                                const __bf16* vc, __bf16* o, float* part,
                                const int* lengths, const int* slots, int n,
                                int hq, int hkv, int S, int max_s,
                                int max_len, int window, int chunk,
                                int n_chunks, int d, float scale,
                                hipStream_t st) {
  if (d == 64)
    launch<64>(q, kc, vc, o, part, lengths, slots, n, hq, hkv, S, max_s,
               max_len, window, chunk, n_chunks, scale, st);
  else
    launch<128>(q, kc, vc, o, part, lengths, slots, n, hq, hkv, S, max_s,
                max_len, window, chunk, n_chunks, scale, st);
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif
