// The per-chunk body of cache-reading prefill attention: many consecutive
// query tokens of a row (a prompt chunk, T > 16) against that row's cache,
// which already holds their own K/V.  One function,
// decode_prefill_chunk<D, F, A>, under the format and addressing tags of
// decode_body.h and decode_rows.h; decode_attn_prefill.hip instantiates it.
// The semantics are those of decode_multi_chunk (decode_multi_body.h): q, o
// [n, T, hq, D], token t < q_lens[i] at pos = lengths[i] - q_lens[i] + t
// attends [max(0, pos + 1 - window), pos], zeros for every other token and
// for empty rows, invalid pages skipped, nothing read back.
//
// The shape is the flash forward's, not decode's.
//
// Columns.  A (row, kv head) has T * qpg columns j = t * qpg + h, token major
// as in decode_multi.  A 256-thread workgroup owns 128 of them, a wave 32:
// lane l of a wave is column 32 w + (l & 31) in both products, so its limits
// clo <= key <= cpos, its running max and its sum are per-lane scalars.  qpg
// need not divide 32 or 128: a token's heads may lie in two waves or two
// workgroups.  Every wave walks all keys of the workgroup's span (the flash
// split); there is no combine across waves.
//
// Products.  Swapped, as in flash_fwd_block: S^T = K . Q^T (two 32-key halves
// of a 64-key tile, D / 16 k-steps of v_mfma_f32_32x32x16_bf16, q fragments
// held in registers) and O^T += V^T . P^T.  The softmax is in exp2 units with
// the bare v_exp_f32.  P enters the second product as ONE bf16 term, packed
// with v_cvt_pk_bf16_f32 and turned into the B operand by permlane32_swap;
// the row sum is taken from the fp32 weights.  That is the accuracy of the
// flash forward (a relative 2^-9 per weight), not the three-term split of the
// decode kernels: prefill is MFMA-bound and the split would double its MFMA
// work.
//
// Staging.  The workgroup stages each 64-key tile of K and of V once, by rows
// with 16-byte loads, into the conflict-free tile_off images of
// flash_attn_body.h, double-buffered with one barrier per tile; the loads of
// the next tile are issued before the products of the current one.  All four
// waves read the same images: K by rows, V transposed (ds_read_b64_tr_b16).
// e4m3 caches are dequantised to bf16 while staging (f8_to_bf16x8, exact),
// once per tile, so the tile loop does not know the format; k_scale[hk] is
// folded into the softmax scale and v_scale[hk] multiplies the normalised row.
//
// Key range.  The workgroup's columns cover tokens [t0, t1]; it needs the keys
// [lo(t0), pos(t1)] (dm_span), cut to its chunk: [ka, kb).  Tiles start at ka
// (contiguous) or on the absolute 64-key grid (paged: the two 32-key halves
// of a tile then have one page id each; the ids are read one tile before the
// loads that use them).  A wave skips the tiles that none of its columns
// needs.  A tile inside every column's limits, inside [ka, kb) and on valid
// pages takes a path without masks and without bounds checks; a seam tile
// (causal diagonal, window edge, first or last tile of the range, invalid
// page) clamps its row addresses into [ka, kb), stages zeros for rows outside
// and for invalid pages (no address is formed from such an id) and masks its
// scores by value-select.  Every branch round a transposed read or an MFMA is
// wave-uniform.
//
// Columns without a key.  Masked scores are -1e30; while a column's max is
// still -1e30 nothing is subtracted, so its weights are exp2(-1e30) = 0 and l
// and O stay untouched (the rule of decode_multi).  l = 0 writes zeros.  q
// rows of tokens t >= q_lens[i] are not loaded.
//
// Split-KV.  Chunks are those of decode_multi (dm_grid_start, dm_chunks), so
// decode_multi_merge_kernel merges them unchanged with 128 columns per group;
// the partial max is stored in natural-log units for it.
#pragma once

#include "flash_attn_body.h"
#include "decode_multi_body.h"

namespace {

constexpr int PF_KB = 64;                 // keys per staged tile
constexpr int PF_WAVES = 4;
constexpr int PF_COLS = 32 * PF_WAVES;    // columns per workgroup
constexpr float PF_LOG2E = 1.4426950408889634f;
constexpr float PF_LN2 = 0.6931471805599453f;

// Pack p of thread tid -> (row, 16-byte bf16 chunk) of a staged tile.  bf16:
// stage_map's layout for 256 threads, which cover 2048 / D rows per pack.
// e4m3: a 16-byte load is 16 elements, the chunks ch and ch + 1; D / 16 lanes
// per row.
template <int D, class F>
DEV_INLINE void pf_stage_map(int tid, int p, int& row, int& ch) {
  if constexpr (F::EPL == 8) {
    stage_map<D>(tid, 0, row, ch);
    row += p * (2048 / D);
  } else {
    constexpr int LPR = D / 16;
    row = tid / LPR + p * (256 / LPR);
    ch = 2 * (tid % LPR);
  }
}

template <int D, class F, class A>
DEV_INLINE void decode_prefill_chunk(
    const __bf16* q,                 // [n, T, hq, D]
    const typename F::elem* kc,      // cache or pool
    const typename F::elem* vc, F fmt,
    __bf16* o,                       // [n, T, hq, D]
    float* part,                     // null: write o
    const int* lengths, const int* q_lens, const int* slots, A ad, int T,
    int hq, int hkv, int nct, int S, int max_len, int window, int chunk,
    float scale) {
  typedef typename F::elem elem;
  typedef typename F::raw raw;
  constexpr int KB = PF_KB;
  constexpr int NK = D / 16;         // k-steps of S^T
  constexpr int ND = D / 32;         // 32-row blocks of O^T
  constexpr int NP = D / (4 * F::EPL);   // staging packs per thread and image
  constexpr int BUFSZ = 2 * KB * D;  // K rows + V rows of one buffer
  __shared__ __align__(16) __bf16 smem[2 * BUFSZ];

  const int row = blockIdx.z, ci = blockIdx.x;
  const int hk = blockIdx.y / nct, c0 = (blockIdx.y - hk * nct) * PF_COLS;
  const int qpg = hq / hkv, ncol = T * qpg;
  const int tid = threadIdx.x, lane = tid & 63;
  const int col = lane & 31, hi = lane >> 5;
  // the wave index as a scalar: the tile loop branches on what follows from it
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const DmRow r = dm_row(lengths, q_lens, slots, row, S, max_len, T, window);
  const DmSpan sp = dm_span(r, c0, PF_COLS, qpg, window);

  // the lane's column
  const int j = c0 + 32 * w + col, t = j / qpg;
  const bool real = t < r.ql;        // implies j < ncol
  const long bh = ((long)row * T + t) * hq + hk * qpg + j - t * qpg;

  if (sp.lo >= sp.hi) {              // workgroup-uniform: no real token here
    if (part == nullptr && j < ncol) {
      bf16x8 z = {};
#pragma unroll
      for (int i = 0; i < D / 16; ++i)
        *reinterpret_cast<bf16x8*>(o + bh * D + hi * (D / 2) + 8 * i) = z;
    }
    return;
  }
  const int g0 = dm_grid_start<A>(r);
  const DmChunks cs = dm_chunks(g0, chunk, gridDim.x, sp);
  if (ci < cs.first || ci > cs.last) return;
  const int p0 = g0 + ci * chunk;
  const int ka = max(p0, sp.lo), kb = min(p0 + chunk, sp.hi);   // ka < kb

  const int rs = hkv * D;
  ad.bind(r.slot);
  const long base = ad.base(r.slot, hkv, hk, D);
  const elem* kg = kc + base;
  const elem* vg = vc + base;
  const float sl2e = fmt.k_mul(scale, hk) * PF_LOG2E;

  // the lane's limits, cut to the chunk, and its q fragments (B operand of
  // S^T): Q[column][16 ks + 8 hi + 0..7]
  const int cpos = real ? r.len - r.ql + t : -1;
  const int clo = real ? max(dm_lo(cpos, window), ka) : 0x7fffffff;
  const int chi = min(cpos, kb - 1);
  bf16x8 qf[NK];
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    bf16x8 z = {};
    qf[ks] = z;
    if (real)
      qf[ks] = *reinterpret_cast<const bf16x8*>(q + bh * D + 16 * ks + 8 * hi);
  }

  // the wave's 32 columns: the keys some column needs, [w_lo, w_hi), and the
  // keys every column attends, [f_lo, f_hi) (non-empty only if all are real)
  const int cw = c0 + 32 * w;
  const int t0w = cw / qpg, t1w = min((cw + 31) / qpg, r.ql - 1);
  const int pos0 = r.len - r.ql + t0w, pos1 = r.len - r.ql + t1w;
  const bool wave_live = t0w <= t1w;
  const bool all_real = (cw + 31) / qpg < r.ql;
  const int w_lo = max(ka, dm_lo(pos0, window)), w_hi = min(kb, pos1 + 1);
  const int f_lo = max(ka, dm_lo(pos1, window));
  const int f_hi = all_real ? min(kb, pos0 + 1) : 0;

  f32x16 ot[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) ot[dt] = (f32x16)(0.f);
  float m_run = DB_NEG, l_run = 0.f;

  // page ids of the two 32-key halves of the tile at kv0; -1 where the half
  // starts past the range (its table entry may not exist)
  auto tile_ids = [&](int kv0, int& a, int& b) {
    a = b = -1;
    if constexpr (A::paged) {
      if (kv0 < kb) a = ad.page_id(kv0);
      if (kv0 + 32 < kb) b = ad.page_id(kv0 + 32);
    }
  };
  auto tile_full = [&](int kv0, int a, int b) {
    bool full = kv0 >= ka && kv0 + KB <= kb;
    if constexpr (A::paged) full = full && ad.ok(a) && ad.ok(b);
    return full;
  };

  raw kst[NP], vst[NP];
  // Guards are hoisted out of the load loops: the full tile is branch-free,
  // a seam tile loads clamped addresses and zeroes by value-select.
  auto stage_load = [&](int kv0, int a, int b) {
    const bool full = tile_full(kv0, a, b);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      int srow, ch;
      pf_stage_map<D, F>(tid, p, srow, ch);
      const int key = kv0 + srow;
      if (full) {
        long off;
        if constexpr (A::paged)
          off = ad.pool_row(srow < 32 ? a : b, key) * rs + ch * 8;
        else
          off = (long)key * rs + ch * 8;
        kst[p] = *reinterpret_cast<const raw*>(kg + off);
        vst[p] = *reinterpret_cast<const raw*>(vg + off);
      } else {
        const int kcl = min(max(key, ka), kb - 1);   // inside the tile
        bool valid = key >= ka && key < kb;
        long off;
        if constexpr (A::paged) {
          const int id = kcl - kv0 < 32 ? a : b;
          const bool good = ad.ok(id);
          valid = valid && good;
          off = ad.pool_row(good ? id : 0, kcl) * rs + ch * 8;
        } else {
          off = (long)kcl * rs + ch * 8;
        }
        const raw tk = *reinterpret_cast<const raw*>(kg + off);
        const raw tv = *reinterpret_cast<const raw*>(vg + off);
        const raw z = {};
        kst[p] = valid ? tk : z;
        vst[p] = valid ? tv : z;
      }
    }
  };
  auto stage_write = [&](int buf) {
    __bf16* k_lds = smem + buf * BUFSZ;
    __bf16* v_lds = k_lds + KB * D;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      int srow, ch;
      pf_stage_map<D, F>(tid, p, srow, ch);
      if constexpr (F::EPL == 8) {
        *reinterpret_cast<bf16x8*>(k_lds + tile_off<D>(srow, ch)) = kst[p];
        *reinterpret_cast<bf16x8*>(v_lds + tile_off<D>(srow, ch)) = vst[p];
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          *reinterpret_cast<bf16x8*>(k_lds + tile_off<D>(srow, ch + h)) =
              f8_to_bf16x8(kst[p][2 * h], kst[p][2 * h + 1]);
          *reinterpret_cast<bf16x8*>(v_lds + tile_off<D>(srow, ch + h)) =
              f8_to_bf16x8(vst[p][2 * h], vst[p][2 * h + 1]);
        }
      }
    }
  };

  const int kv_begin = A::paged ? (ka & ~(KB - 1)) : ka;
  int idA, idB, nxA, nxB;
  tile_ids(kv_begin, idA, idB);
  tile_ids(kv_begin + KB, nxA, nxB);
  stage_load(kv_begin, idA, idB);
  stage_write(0);
  __syncthreads();
  int cur = 0;

  for (int kv0 = kv_begin; kv0 < kb; kv0 += KB) {   // workgroup-uniform
    const bool have_next = kv0 + KB < kb;
    const __bf16* k_lds = smem + cur * BUFSZ;
    const __bf16* v_lds = k_lds + KB * D;
    if (have_next) stage_load(kv0 + KB, nxA, nxB);  // lands at stage_write
    int n2A, n2B;                    // a tile ahead of the loads that use them
    tile_ids(kv0 + 2 * KB, n2A, n2B);

    if (wave_live && kv0 < w_hi && kv0 + KB > w_lo) {   // wave-uniform
      // ---- S^T = K Q^T (two 32-key halves) ----
      f32x16 st0 = (f32x16)(0.f), st1 = (f32x16)(0.f);
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const bf16x8 k0 = tile_row_frag<D>(k_lds, 0, ks, lane);
        const bf16x8 k1 = tile_row_frag<D>(k_lds, 32, ks, lane);
        st0 = mfma32_bf16(k0, qf[ks], st0);
        st1 = mfma32_bf16(k1, qf[ks], st1);
      }

      // ---- scale, and the masks of a seam tile ----
      float pv[32];
      bool okA = true, okB = true;
      if constexpr (A::paged) { okA = ad.ok(idA); okB = ad.ok(idB); }
      const bool need_mask =
          !(kv0 >= f_lo && kv0 + KB <= f_hi && okA && okB);
      if (need_mask) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const int key0 = kv0 + mfma32_d_row(lane, rr), key1 = key0 + 32;
          const bool in0 = key0 >= clo && key0 <= chi && okA;
          const bool in1 = key1 >= clo && key1 <= chi && okB;
          const float x0 = st0[rr] * sl2e, x1 = st1[rr] * sl2e;
          pv[rr] = in0 ? x0 : DB_NEG;
          pv[16 + rr] = in1 ? x1 : DB_NEG;
        }
      } else {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          pv[rr] = st0[rr] * sl2e;
          pv[16 + rr] = st1[rr] * sl2e;
        }
      }

      // ---- in-register online softmax (per-lane column) ----
      float mt = pv[0];
#pragma unroll
      for (int i = 1; i < 32; ++i) mt = fmaxf(mt, pv[i]);
      float m_lo, m_hi;
      both_halves(mt, m_lo, m_hi);
      mt = fmaxf(m_lo, m_hi);
      const float mn = fmaxf(m_run, mt);
      // the bare v_exp_f32: see flash_fwd_block
      const float alpha = (m_run <= DB_NEG)
                              ? 0.f : __builtin_amdgcn_exp2f(m_run - mn);
      // A column that has seen no key has mn and all of pv at -1e30:
      // subtracting 0 there gives exp2(-1e30) = 0 exactly.
      const float msub = (mn <= DB_NEG) ? 0.f : mn;
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
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
          for (int rr = 0; rr < 16; ++rr) ot[dt][rr] *= alpha;
      }

      // ---- P -> one bf16 term, B fragments via cvt_pk + permlane32_swap:
      // fragment ks holds P[column][16 ks + 8 hi + 0..7] as 4 words ----
      unsigned pw[16];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const float* pt = pv + 16 * tt;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            const unsigned a =
                pack_bf16(pt[8 * i + 2 * g], pt[8 * i + 2 * g + 1]);
            const unsigned b =
                pack_bf16(pt[8 * i + 2 * g + 4], pt[8 * i + 2 * g + 5]);
            auto r2 = __builtin_amdgcn_permlane32_swap(a, b, false, false);
            pw[(2 * tt + i) * 4 + g] = r2[0];
            pw[(2 * tt + i) * 4 + 2 + g] = r2[1];
          }
        }
      }

      // ---- O^T += V^T P^T ----
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        union { unsigned u[4]; bf16x8 f; } pb;
#pragma unroll
        for (int g = 0; g < 4; ++g) pb.u[g] = pw[ks * 4 + g];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          const bf16x8 va = tile_tr_frag<D>(v_lds, ks * 16, dt, lane);
          ot[dt] = mfma32_bf16(va, pb.f, ot[dt]);
        }
      }
    }

    if (have_next) stage_write(cur ^ 1);
    __syncthreads();
    cur ^= 1;
    idA = nxA; idB = nxB;
    nxA = n2A; nxB = n2B;
  }

  // ---- epilogue: O^T[d][column = lane], per-lane m and l ----
  if (j >= ncol) return;             // columns past the last token's heads
  if (part == nullptr) {
    // a column without a key (or only invalid pages) -> zeros
    const float inv = l_run > 0.f ? fmt.v_mul(hk) / l_run : 0.f;
    __bf16* orow = o + bh * D;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store_d_quad(orow, dt, g, hi, ot[dt][4 * g] * inv,
                     ot[dt][4 * g + 1] * inv, ot[dt][4 * g + 2] * inv,
                     ot[dt][4 * g + 3] * inv);
  } else {
    float* out = part + (bh * gridDim.x + ci) * (D + 2);
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float* p = out + dt * 32 + 8 * g + 4 * hi;   // 8-byte aligned
        *reinterpret_cast<f32x2*>(p) =
            f32x2{ot[dt][4 * g], ot[dt][4 * g + 1]};
        *reinterpret_cast<f32x2*>(p + 2) =
            f32x2{ot[dt][4 * g + 2], ot[dt][4 * g + 3]};
      }
    if (hi == 0) {                   // the merge works in natural-log units
      out[D] = m_run <= DB_NEG ? DB_NEG : m_run * PF_LN2;
      out[D + 1] = l_run;
    }
  }
}

}  // namespace
