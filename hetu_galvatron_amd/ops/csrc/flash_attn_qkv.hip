// Packed-QKV self-attention: the block bodies of flash_attn_body.h reading
// q, k and v straight from the linear_qkv output [s, b, G, qpg+2, D] (see
// packed_addr there), so nothing has to separate them in memory first.
// sbhd only, sq = skv = s, off = 0, no bias, no window.  o, dout, dk_exp,
// dv_exp stay [s, b, hq, D] and lse, di [b, hq, s]; dq is written into the
// q slots of a dqkv buffer of the packed geometry.
//
// Unlike the varlen kernels, these keep complementary-pair causal
// scheduling: they run the flagship's shape, where dropping it costs
// 1.5-1.8x.  dq and dkv keep the dense structure (noinline bodies, two call
// sites); the forward inlines one copy of its body in a two-pass loop.
#include "flash_attn_body.h"
#include "flash_attn_launch.h"

namespace {

template <int D>
DEV_INLINE PackedAddr packed_head(int b, int s, int G, int qpg) {
  const int hq = G * qpg;
  const int bh = blockIdx.y;
  const int bi = bh / hq;
  const int h = bh - bi * hq;
  return packed_addr<D>(0, bi, h, b, s, G, qpg);
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_packed_fwd_kernel(const __bf16* __restrict__ qkv,
                             __bf16* __restrict__ o, float* __restrict__ lse,
                             int b, int s, int G, int qpg, float scale,
                             bool causal, bool paired) {
  constexpr int QBF = FwdTile<D>::QBF;
  __shared__ __align__(16) __bf16 smem[2 * FwdTile<D>::BUFSZ];
  const PackedAddr p = packed_head<D>(b, s, G, qpg);
  const __bf16* k = qkv + (long)qpg * D;
  const __bf16* v = k + D;
  const OutOwn oa{p.o_base, p.o_str};
  const float sl2e = scale * 1.4426950408889634f;
  const int nqb = (s + QBF - 1) / QBF;
  // one inlined copy of the body, run for the block and then for its
  // complementary partner: out of line (as in the dense kernel) the
  // compiler serialised the V staging loads of the full-tile path here
  for (int pass = 0; pass < 2; ++pass) {
    const int qb = pass == 0 ? (int)blockIdx.x : nqb - 1 - (int)blockIdx.x;
    if (pass == 1) {
      if (!(causal && paired && qb > (int)blockIdx.x)) break;
      __syncthreads();
    }
    FLASH_INLINE_CALL flash_fwd_block<D, false, false, OutOwn>(
        qb, qkv, k, v, o, lse, smem, p.q_base, p.kv_base, p.lse_base,
        p.qkv_str, p.qkv_str, 0, s, s, sl2e, causal, nullptr, 0, 0, oa);
  }
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_packed_bwd_dq_kernel(const __bf16* __restrict__ dout,
                                const __bf16* __restrict__ qkv,
                                const float* __restrict__ lse,
                                const float* __restrict__ di,
                                __bf16* __restrict__ dqkv, int b, int s,
                                int G, int qpg, float scale, bool causal,
                                bool paired) {
  constexpr int QBF = DqTile<D>::QBF;
  __shared__ __align__(16) __bf16 smem[2 * DqTile<D>::BUFSZ];
  const PackedAddr p = packed_head<D>(b, s, G, qpg);
  const __bf16* k = qkv + (long)qpg * D;
  const __bf16* v = k + D;
  const OutOwn oa{p.o_base, p.o_str};
  const int nqb = (s + QBF - 1) / QBF;
  flash_bwd_dq_block<D, false, false, OutOwn>(
      blockIdx.x, dout, qkv, k, v, lse, di, dqkv, smem, p.q_base, p.kv_base,
      p.lse_base, p.qkv_str, p.qkv_str, 0, s, s, scale, causal, nullptr, 0,
      0, oa);
  const int qb2 = nqb - 1 - (int)blockIdx.x;
  if (causal && paired && qb2 > (int)blockIdx.x) {
    __syncthreads();
    flash_bwd_dq_block<D, false, false, OutOwn>(
        qb2, dout, qkv, k, v, lse, di, dqkv, smem, p.q_base, p.kv_base,
        p.lse_base, p.qkv_str, p.qkv_str, 0, s, s, scale, causal, nullptr,
        0, 0, oa);
  }
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_packed_bwd_dkv_kernel(const __bf16* __restrict__ dout,
                                 const __bf16* __restrict__ qkv,
                                 const float* __restrict__ lse,
                                 const float* __restrict__ di,
                                 __bf16* __restrict__ dk_exp,  // [s,b,hq,D]
                                 __bf16* __restrict__ dv_exp, int b, int s,
                                 int G, int qpg, float scale, bool causal,
                                 bool paired) {
  constexpr int KBW = DkvTile<D>::KBW;
  __shared__ __align__(16) __bf16 smem[2 * DkvTile<D>::BUFSZ];
  __shared__ __align__(16) float lsedi[4 * DkvTile<D>::QT];
  const PackedAddr p = packed_head<D>(b, s, G, qpg);
  const __bf16* k = qkv + (long)qpg * D;
  const __bf16* v = k + D;
  const OutOwn oa{p.o_base, p.o_str};
  const int nkb = (s + KBW - 1) / KBW;
  // dk_exp / dv_exp carry hq heads in o's layout
  flash_bwd_dkv_block<D, false, false, OutOwn>(
      blockIdx.x, dout, qkv, k, v, lse, di, dk_exp, dv_exp, smem, lsedi,
      p.q_base, p.kv_base, p.o_base, p.lse_base, p.qkv_str, p.qkv_str,
      p.o_str, 0, s, s, scale, causal, nullptr, nullptr, 0, 0, oa);
  const int kb2 = nkb - 1 - (int)blockIdx.x;
  if (causal && paired && kb2 > (int)blockIdx.x) {
    __syncthreads();
    flash_bwd_dkv_block<D, false, false, OutOwn>(
        kb2, dout, qkv, k, v, lse, di, dk_exp, dv_exp, smem, lsedi,
        p.q_base, p.kv_base, p.o_base, p.lse_base, p.qkv_str, p.qkv_str,
        p.o_str, 0, s, s, scale, causal, nullptr, nullptr, 0, 0, oa);
  }
}

}  // namespace

// the dense grids (and their underfill-aware pairing rule) with hq = G*qpg
// heads
void flash_packed_fwd_launch(const __bf16* qkv, __bf16* o, float* lse, int b,
                             int s, int G, int qpg, int d, float scale,
                             bool causal, hipStream_t st) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    const int hq = G * qpg;
    const int nqb = (s + FwdTile<D>::QBF - 1) / FwdTile<D>::QBF;
    const bool paired = flash_paired(nqb, b, hq, causal);
    dim3 grid(paired ? (nqb + 1) / 2 : nqb, b * hq);
    hipLaunchKernelGGL((flash_packed_fwd_kernel<D>), grid, dim3(512), 0, st,
                       qkv, o, lse, b, s, G, qpg, scale, causal, paired);
  });
}

void flash_packed_bwd_launch(const __bf16* dout, const __bf16* qkv,
                             const float* lse, const float* di, __bf16* dqkv,
                             __bf16* dk_exp, __bf16* dv_exp, int b, int s,
                             int G, int qpg, int d, float scale, bool causal,
                             hipStream_t st) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    // q blocks == key blocks (sq == skv)
    static_assert(DqTile<D>::QBF == DkvTile<D>::KBW, "one grid for both");
    const int hq = G * qpg;
    const int nb = (s + DqTile<D>::QBF - 1) / DqTile<D>::QBF;
    const bool paired = flash_paired(nb, b, hq, causal);
    dim3 grid(paired ? (nb + 1) / 2 : nb, b * hq);
    hipLaunchKernelGGL((flash_packed_bwd_dq_kernel<D>), grid, dim3(512), 0,
                       st, dout, qkv, lse, di, dqkv, b, s, G, qpg, scale,
                       causal, paired);
    hipLaunchKernelGGL((flash_packed_bwd_dkv_kernel<D>), grid, dim3(512), 0,
                       st, dout, qkv, lse, di, dk_exp, dv_exp, b, s, G, qpg,
                       scale, causal, paired);
  });
}
