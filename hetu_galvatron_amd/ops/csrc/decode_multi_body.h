// The per-chunk body of multi-token decode attention: a short block of T
// consecutive query tokens of a row against that row's cache, with a causal
// edge inside the block (speculative verification, chunked decode).  One
// function, decode_multi_chunk<D, F, A, CB>, under the format and addressing
// tags of decode_body.h and decode_rows.h; decode_attn_multi.hip instantiates
// it.  Include this inside the module's packed-fp32 pragma.
//
//   q, o [n, T, hq, D] bf16; caches and pools as in decode_body.h; lengths,
//   q_lens, slots: int32 [n] in device memory.  lengths[i] counts the row's
//   cached positions, the new tokens included; q_lens[i] of the T tokens are
//   real.  Token t < q_lens[i] sits at pos = lengths[i] - q_lens[i] + t and
//   attends to [max(0, pos + 1 - window), pos] (from 0 without a window).
//
// Columns.  A (row, kv head) has T * qpg columns, j = t * qpg + h, token
// major: the 16 columns of one MFMA block are neighbouring tokens, so their
// causal limits and window starts differ by at most 16 / qpg + 1 positions
// and the block's key range is hardly wider than a single token's.  qpg need
// not divide 16; a token's heads may lie in two blocks.
//
// Work split.  One 256-thread workgroup per (row, kv head, column group,
// chunk); a column group is CB blocks of 16 columns, blockIdx.y = hk * ncg +
// group.  The workgroup keeps CB sets of q fragments (B operands) and CB sets
// of O accumulators in registers.  Per 32-key wave step the K fragments (A
// operands of S^T = K . Q^T) and the V^T fragments (A operands of
// O^T += V^T . P^T) are made once, from one load of the step's rows and one
// LDS image, and used for every block: the K/V stream of a (row, kv head) is
// read once per 16 CB columns.  Waves, tiles, chunks, the V image, the
// three-term bf16 split of the weights and the loads one step ahead are those
// of decode_chunk.
//
// Masks.  A lane's eight scores of a block belong to one column, so the
// column's limits (clo, cpos) are two per-lane scalars per block and a score
// is kept iff clo <= key <= cpos.  The running max and sum stay per lane and
// per block.
//
// Key range.  A workgroup needs the keys from the window start of its first
// token to the position of its last real one, [sp.lo, sp.hi).  Wave steps
// outside it are skipped, the row loads are clamped into it, and a workgroup
// whose chunk does not meet it (dm_chunks) returns before any barrier or
// memory access beyond the three row words.
//
// Columns without a key.  With m = -1e30 a masked score would weigh
// exp(-1e30 - m) = 1 as long as the column has seen no key: a step wholly
// below a later token's window, a chunk wholly above an earlier token's
// position, a token t >= q_lens[i].  The weights of a column whose max is
// still -1e30 are therefore zeros by selection, so such a step leaves l and O
// untouched; once the max is real, exp(-1e30 - m) is an exact zero.  A column
// that never sees a key ends with l = 0 and is written as zeros.  q rows of
// tokens t >= q_lens[i] are not loaded (their B fragments are zeros).
//
// With T = 1 and q_lens = 1 every step of this body performs the arithmetic
// of decode_chunk in its order: the results are the same bits.
#pragma once

#include "decode_body.h"

namespace {

// A row of the multi-token call; ql = 0 is "empty": lengths outside
// (0, max_len], q_lens outside [0, T] or above the length, a slot outside
// [0, S).  lo0: the first key of token 0, where the row's tile grid starts.
struct DmRow {
  int len, ql, slot, lo0;
};

DEV_INLINE int dm_lo(int pos, int window) {
  return window > 0 ? max(0, pos + 1 - window) : 0;
}

DEV_INLINE DmRow dm_row(const int* __restrict__ lengths,
                        const int* __restrict__ q_lens,
                        const int* __restrict__ slots, int row, int S,
                        int max_len, int T, int window) {
  const int len = lengths[row], ql = q_lens[row], slot = slots[row];
  const bool ok = len > 0 && len <= max_len && ql > 0 && ql <= T &&
                  ql <= len && slot >= 0 && slot < S;
  DmRow r;
  r.len = ok ? len : 0;
  r.ql = ok ? ql : 0;
  r.slot = ok ? slot : 0;
  r.lo0 = ok ? dm_lo(len - ql, window) : 0;
  return r;
}

template <class A>
DEV_INLINE int dm_grid_start(const DmRow& r) {
  return A::paged ? (r.lo0 & ~31) : r.lo0;
}

// The keys [lo, hi) that the columns [c0, c0 + cols) of a row need: from the
// window start of their first token to the position of their last real one.
// lo >= hi: no real token among them.
struct DmSpan {
  int lo, hi;
};

DEV_INLINE DmSpan dm_span(const DmRow& r, int c0, int cols, int qpg,
                          int window) {
  const int t0 = c0 / qpg, t1 = min((c0 + cols - 1) / qpg, r.ql - 1);
  DmSpan s{0, 0};
  if (t0 <= t1) {
    s.lo = dm_lo(r.len - r.ql + t0, window);
    s.hi = r.len - r.ql + t1 + 1;
  }
  return s;
}

// The chunks [first, last] of the row's grid (chunk c = [g0 + c chunk,
// g0 + (c + 1) chunk)) that meet a non-empty span: what a column group's
// workgroups compute and write, and what the merge reads.
struct DmChunks {
  int first, last;
};

DEV_INLINE DmChunks dm_chunks(int g0, int chunk, int n_chunks,
                              const DmSpan& s) {
  return DmChunks{(s.lo - g0) / chunk,
                  min((s.hi - 1 - g0) / chunk, n_chunks - 1)};
}

template <int D, class F, class A, int CB>
DEV_INLINE void decode_multi_chunk(
    const __bf16* q,                 // [n, T, hq, D]
    const typename F::elem* kc,      // cache or pool
    const typename F::elem* vc, F fmt,
    __bf16* o,                       // [n, T, hq, D]
    float* part,                     // null: write o
    const int* lengths, const int* q_lens, const int* slots, A ad, int T,
    int hq, int hkv, int ncg, int S, int max_len, int window, int chunk,
    float scale) {
  typedef typename F::elem elem;
  typedef typename F::raw raw;
  constexpr int VSTR = D + 16;       // LDS row stride of the V image, elements
  constexpr int VIMG = DB_WKEYS * VSTR;
  constexpr int NDT = D / 16;
  constexpr int NVR = D / (2 * F::EPL);   // V loads of a step
  constexpr int COLS = 16 * CB;
  // the V images of the four waves, then the waves' fp32 O of one column
  // block at a time for the combine: the block of decode_chunk
  constexpr int IMGS = DB_WAVES * VIMG * (int)sizeof(elem);
  constexpr int COMB = DB_WAVES * 16 * D * 4;
  __shared__ __align__(16) elem lds[(IMGS > COMB ? IMGS : COMB) / sizeof(elem)];
  __shared__ float ml[DB_WAVES][16][2];

  const int row = blockIdx.z, ci = blockIdx.x;
  const int hk = blockIdx.y / ncg, c0 = (blockIdx.y - hk * ncg) * COLS;
  const int qpg = hq / hkv, ncol = T * qpg;
  const int tid = threadIdx.x;
  const DmRow r = dm_row(lengths, q_lens, slots, row, S, max_len, T, window);
  const DmSpan sp = dm_span(r, c0, COLS, qpg, window);
  if (sp.lo >= sp.hi) {              // workgroup-uniform: no real token here
    if (part == nullptr)
      for (int i = tid; i < COLS * D; i += 256) {
        const int j = c0 + i / D, t = j / qpg;
        if (j < ncol)
          o[(((long)row * T + t) * hq + hk * qpg + j - t * qpg) * D + i % D] =
              (__bf16)0.f;
      }
    return;
  }
  const int g0 = dm_grid_start<A>(r);
  const DmChunks cs = dm_chunks(g0, chunk, gridDim.x, sp);
  if (ci < cs.first || ci > cs.last) return;
  const int p0 = g0 + ci * chunk;
  const int p1 = min(p0 + chunk, sp.hi);
  const int lo = sp.lo;

  // the wave index as a scalar: the step loop branches on it
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const int rs = hkv * D;
  ad.bind(r.slot);
  const long base = ad.base(r.slot, hkv, hk, D);
  const elem* kb = kc + base;
  const elem* vb = vc + base;
  const float sc = fmt.k_mul(scale, hk);

  // the lane's column of each block: its limits and its q fragments
  bf16x8 qf[CB][D / 32];
  int clo[CB], cpos[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int j = c0 + 16 * cb + c, t = j / qpg;
    const bool real = t < r.ql;      // implies j < ncol
    cpos[cb] = real ? r.len - r.ql + t : -1;
    clo[cb] = real ? dm_lo(cpos[cb], window) : 0x7fffffff;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[cb][ks][e] = (__bf16)0.f;
      if (real)
        qf[cb][ks] = *reinterpret_cast<const bf16x8*>(F::q_frag(
            q + (((long)row * T + t) * hq + hk * qpg + j - t * qpg) * D, ks,
            g));
    }
  }

  elem* vimg = lds + w * VIMG;
  constexpr int CH = D / F::EPL, RPL = 64 / CH;
  const int wr_off =
      F::template stage_row<D>(lane / CH) * VSTR + F::EPL * (lane % CH);
  const int tr_off = F::tr_off(lane, g, c, VSTR);

  f32x4 oacc[CB][NDT];
  float m[CB], l[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      oacc[cb][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[cb] = DB_NEG;
    l[cb] = 0.f;
  }

  raw kr[2][D / (4 * F::EPL)];
  raw vr[NVR];
  // the wave's first step that reaches the span
  int k0 = p0 + w * DB_WKEYS;
  if (k0 + DB_WKEYS <= lo) k0 += ((lo - DB_WKEYS - k0) / DB_TILE + 1) * DB_TILE;
  // paged: the page ids of this step and the next, as wave-uniform values
  int id0 = -1, id1 = -1;
  if constexpr (A::paged) {
    if (k0 < p1) id0 = ad.page_id(k0);
    if (k0 + DB_TILE < p1) id1 = ad.page_id(k0 + DB_TILE);
  }
  if (k0 < p1)
    db_fetch<D, F>(ad, kb, vb, rs, k0, lo, p1, id0, lane, kr, vr);
  while (k0 < p1) {                  // wave-uniform
    int id2 = -1;
    if constexpr (A::paged) {
      if (k0 + 2 * DB_TILE < p1) id2 = ad.page_id(k0 + 2 * DB_TILE);
    }
    bool live = true;                // paged: the step's page is in the pool
    if constexpr (A::paged) live = ad.ok(id0);

    f32x4 sacc[CB][2];
    if (live) {
#pragma unroll
      for (int i = 0; i < NVR; ++i)
        *reinterpret_cast<raw*>(vimg + wr_off + i * RPL * VSTR) = vr[i];
      db_wave_fence();

#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
        sacc[cb][0] = sacc[cb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks) {
          const bf16x8 a = F::template a_frag<D>(kr[blk], ks);
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            sacc[cb][blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, qf[cb][ks], sacc[cb][blk], 0, 0, 0);
        }
      }
    }

    const int kn = k0 + DB_TILE;
    if (kn < p1)
      db_fetch<D, F>(ad, kb, vb, rs, kn, lo, p1, id1, lane, kr, vr);

    if (live) {
      float alpha[CB];
      bf16x8 ph[CB], pl[CB], pl2[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        float s[8];
        float mx = DB_NEG;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int key = F::score_key(k0, j, g);
          const bool in = key >= clo[cb] && key <= cpos[cb];
          s[j] = in ? sacc[cb][j >> 2][j & 3] * sc : DB_NEG;
          mx = fmaxf(mx, s[j]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
        const float mn = fmaxf(m[cb], mx);
        alpha[cb] = __expf(m[cb] - mn);
        m[cb] = mn;
        const bool seen = mn > 0.5f * DB_NEG;   // the column has had a key
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = seen ? __expf(s[j] - mn) : 0.f;
          ps += p;
          const __bf16 h = (__bf16)p;
          const float r1 = p - (float)h;
          const __bf16 lo16 = (__bf16)r1;
          ph[cb][j] = h;
          pl[cb][j] = lo16;
          pl2[cb][j] = (__bf16)(r1 - (float)lo16);
        }
        l[cb] = l[cb] * alpha[cb] + ps;
      }
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const bf16x8 vf = F::template vt_frag<VSTR>(vimg + tr_off + 16 * dt);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          f32x4 a = oacc[cb][dt];
#pragma unroll
          for (int e = 0; e < 4; ++e) a[e] *= alpha[cb];
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pl2[cb], a, 0, 0, 0);
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pl[cb], a, 0, 0, 0);
          oacc[cb][dt] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, ph[cb], a, 0, 0, 0);
        }
      }
      db_wave_fence();
    }
    k0 = kn;
    id0 = id1;
    id1 = id2;
  }

  // the lane groups summed different keys against the same max
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    l[cb] += __shfl_xor(l[cb], 16, WAVE);
    l[cb] += __shfl_xor(l[cb], 32, WAVE);
  }

  // the cross-wave combine, one column block at a time through the LDS block
  float* comb = reinterpret_cast<float*>(lds);   // [wave][column][D]
  const float vs = fmt.v_mul(hk);
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    __syncthreads();                 // V images / the block before are read
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
      *reinterpret_cast<f32x4*>(comb + (w * 16 + c) * D + 16 * dt + 4 * g) =
          oacc[cb][dt];
    if (g == 0) { ml[w][c][0] = m[cb]; ml[w][c][1] = l[cb]; }
    __syncthreads();
    for (int i = tid; i < 16 * D; i += 256) {
      const int cc = i / D, d = i - cc * D;
      const int j = c0 + 16 * cb + cc, t = j / qpg;
      if (j >= ncol) break;          // columns past the last token's heads
      float gm = ml[0][cc][0];
#pragma unroll
      for (int ww = 1; ww < DB_WAVES; ++ww) gm = fmaxf(gm, ml[ww][cc][0]);
      float gl = 0.f, acc = 0.f;
#pragma unroll
      for (int ww = 0; ww < DB_WAVES; ++ww) {
        const float f = __expf(ml[ww][cc][0] - gm);
        gl += f * ml[ww][cc][1];
        acc += f * comb[(ww * 16 + cc) * D + d];
      }
      const long bh = ((long)row * T + t) * hq + hk * qpg + j - t * qpg;
      if (part == nullptr) {
        // a column without a key (or only invalid pages) -> zeros
        if (gl == 0.f) gl = 1.f;
        o[bh * D + d] = (__bf16)(acc / gl * vs);
      } else {
        float* out = part + (bh * gridDim.x + ci) * (D + 2);
        out[d] = acc;
        if (d == 0) { out[D] = gm; out[D + 1] = gl; }
      }
    }
  }
}

// One block of D threads per (row, token, q head): log-sum-exp merge of the
// chunks that the column group of this output wrote, found with dm_span and
// dm_chunks as the chunk kernel found them; the others were never written.
// cols: the columns of a group (16 CB of the chunk kernel).  A token past
// q_lens, an empty row and a column whose chunks all have l = 0 give zeros.
template <int D, class A>
__global__ void decode_multi_merge_kernel(
    const float* __restrict__ part, const float* __restrict__ v_scale,
    __bf16* __restrict__ o, const int* __restrict__ lengths,
    const int* __restrict__ q_lens, const int* __restrict__ slots, int T,
    int hq, int hkv, int cols, int S, int max_len, int window, int chunk,
    int n_chunks) {
  const int bh = blockIdx.x, tid = threadIdx.x;
  const int head = bh % hq, t = (bh / hq) % T, qpg = hq / hkv;
  const DmRow r = dm_row(lengths, q_lens, slots, bh / (hq * T), S, max_len,
                         T, window);
  if (t >= r.ql) {
    o[(long)bh * D + tid] = (__bf16)0.f;
    return;
  }
  const int j = t * qpg + head % qpg;
  const DmSpan sp = dm_span(r, j / cols * cols, cols, qpg, window);
  const DmChunks cs = dm_chunks(dm_grid_start<A>(r), chunk, n_chunks, sp);
  const float* base = part + (long)bh * n_chunks * (D + 2);
  float gm = DB_NEG;
  for (int ci = cs.first; ci <= cs.last; ++ci)
    gm = fmaxf(gm, base[ci * (D + 2) + D]);
  float gl = 0.f, acc = 0.f;
  for (int ci = cs.first; ci <= cs.last; ++ci) {
    const float f = __expf(base[ci * (D + 2) + D] - gm);
    gl += f * base[ci * (D + 2) + D + 1];
    acc += f * base[ci * (D + 2) + tid];
  }
  if (gl == 0.f) gl = 1.f;
  float res = acc / gl;
  if (v_scale) res *= v_scale[head / qpg];
  o[(long)bh * D + tid] = (__bf16)res;
}

}  // namespace
