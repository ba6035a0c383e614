// Packed-document (varlen) self-attention: the block bodies of
// flash_attn_body.h, mapped one workgroup per (segment, head, 256-row
// block).  cu[nseg+1] holds token offsets into the batch-major flattened
// [b*s] stream; a segment never straddles a batch row, so it is a contiguous
// run of rows in both layouts and only the bases change.  sq = skv = len,
// off = 0.  lse/di keep the dense [b, hq, s] layout.  No complementary
// pairing: blocks past the end of a short segment leave before touching
// memory, and mixed lengths are left to the hardware scheduler.
//
// Each body has one call site here and is inlined into it (off = 0 and
// sq == skv fold away; no scratch at D=64).
//
// The dq mask split raises the D = 64 dq kernel past 128 VGPRs, i.e. from
// two resident workgroups per CU to one; it is left out at that D.
#define FLASH_DQ_MASK_SPLIT(D) ((D) == 128)
#include "flash_attn_body.h"
#include "flash_attn_launch.h"

namespace {

struct VarlenSeg {
  int len;        // tokens in the segment (0 = nothing to do)
  long q_base, kv_base, lse_base;
  int q_str, kv_str;
};

template <int D>
DEV_INLINE VarlenSeg varlen_seg(const int* __restrict__ cu, int b, int s,
                                int hq, int hkv, bool sbhd) {
  VarlenSeg g;
  const int seg = blockIdx.y / hq;
  const int h = blockIdx.y - seg * hq;
  const int hk = h / (hq / hkv);
  // cu_seg's decoding, kept in its own words: through cu_seg the compiler
  // orders the validity compares differently in all six kernels
  const int t0 = cu[seg];
  const int len = cu[seg + 1] - t0;
  const int bi = t0 / s;
  const int p0 = t0 - bi * s;
  const bool ok = t0 >= 0 && len > 0 && bi < b && p0 + len <= s;
  g.len = ok ? len : 0;
  g.q_base = sbhd ? (((long)p0 * b + bi) * hq + h) * D
                  : ((long)t0 * hq + h) * D;
  g.kv_base = sbhd ? (((long)p0 * b + bi) * hkv + hk) * D
                   : ((long)t0 * hkv + hk) * D;
  g.q_str = (sbhd ? b * hq : hq) * D;
  g.kv_str = (sbhd ? b * hkv : hkv) * D;
  g.lse_base = ((long)bi * hq + h) * s + p0;
  return g;
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_varlen_fwd_kernel(const __bf16* __restrict__ q,
                             const __bf16* __restrict__ k,
                             const __bf16* __restrict__ v,
                             __bf16* __restrict__ o, float* __restrict__ lse,
                             const int* __restrict__ cu, int b, int s,
                             int hq, int hkv, float scale, bool causal,
                             bool sbhd) {
  __shared__ __align__(16) __bf16 smem[2 * FwdTile<D>::BUFSZ];
  const VarlenSeg g = varlen_seg<D>(cu, b, s, hq, hkv, sbhd);
  // workgroup-uniform, before any barrier; also covers len == 0
  if ((int)blockIdx.x * FwdTile<D>::QBF >= g.len) return;
  const float sl2e = scale * 1.4426950408889634f;
  FLASH_INLINE_CALL flash_fwd_block<D>(
      blockIdx.x, q, k, v, o, lse, smem, g.q_base, g.kv_base, g.lse_base,
      g.q_str, g.kv_str, 0, g.len, g.len, sl2e, causal);
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_varlen_bwd_dq_kernel(const __bf16* __restrict__ dout,
                                const __bf16* __restrict__ q,
                                const __bf16* __restrict__ k,
                                const __bf16* __restrict__ v,
                                const float* __restrict__ lse,
                                const float* __restrict__ di,
                                __bf16* __restrict__ dq,
                                const int* __restrict__ cu, int b, int s,
                                int hq, int hkv, float scale, bool causal,
                                bool sbhd) {
  __shared__ __align__(16) __bf16 smem[2 * DqTile<D>::BUFSZ];
  const VarlenSeg g = varlen_seg<D>(cu, b, s, hq, hkv, sbhd);
  if ((int)blockIdx.x * DqTile<D>::QBF >= g.len) return;
  FLASH_INLINE_CALL flash_bwd_dq_block<D>(
      blockIdx.x, dout, q, k, v, lse, di, dq, smem, g.q_base, g.kv_base,
      g.lse_base, g.q_str, g.kv_str, 0, g.len, g.len, scale, causal);
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_varlen_bwd_dkv_kernel(const __bf16* __restrict__ dout,
                                 const __bf16* __restrict__ q,
                                 const __bf16* __restrict__ k,
                                 const __bf16* __restrict__ v,
                                 const float* __restrict__ lse,
                                 const float* __restrict__ di,
                                 __bf16* __restrict__ dk_exp,
                                 __bf16* __restrict__ dv_exp,
                                 const int* __restrict__ cu, int b, int s,
                                 int hq, int hkv, float scale, bool causal,
                                 bool sbhd) {
  __shared__ __align__(16) __bf16 smem[2 * DkvTile<D>::BUFSZ];
  __shared__ __align__(16) float lsedi[4 * DkvTile<D>::QT];
  const VarlenSeg g = varlen_seg<D>(cu, b, s, hq, hkv, sbhd);
  if ((int)blockIdx.x * DkvTile<D>::KBW >= g.len) return;
  // the two phases of flash_bwd_dkv_block, dV then dK; dk_exp / dv_exp
  // carry hq heads, so q's base and stride address them too
  FLASH_INLINE_CALL flash_bwd_dkv_phase<D, false>(
      blockIdx.x, dout, q, k, v, lse, di, dk_exp, dv_exp, smem, lsedi,
      g.q_base, g.kv_base, g.q_base, g.lse_base, g.q_str, g.kv_str, g.q_str,
      0, g.len, g.len, scale, causal);
  __syncthreads();
  FLASH_INLINE_CALL flash_bwd_dkv_phase<D, true>(
      blockIdx.x, dout, q, k, v, lse, di, dk_exp, dv_exp, smem, lsedi,
      g.q_base, g.kv_base, g.q_base, g.lse_base, g.q_str, g.kv_str, g.q_str,
      0, g.len, g.len, scale, causal);
}

}  // namespace

// grid.x covers the longest segment, grid.y = (segment, head)
void flash_varlen_fwd_launch(const __bf16* q, const __bf16* k,
                             const __bf16* v, __bf16* o, float* lse,
                             const int* cu, int nseg, int max_seqlen, int b,
                             int s, int hq, int hkv, int d, float scale,
                             bool causal, bool sbhd, hipStream_t st) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    dim3 grid((max_seqlen + FwdTile<D>::QBF - 1) / FwdTile<D>::QBF,
              nseg * hq);
    hipLaunchKernelGGL((flash_varlen_fwd_kernel<D>), grid, dim3(512), 0, st,
                       q, k, v, o, lse, cu, b, s, hq, hkv, scale, causal,
                       sbhd);
  });
}

void flash_varlen_bwd_launch(const __bf16* dout, const __bf16* q,
                             const __bf16* k, const __bf16* v,
                             const float* lse, const float* di, __bf16* dq,
                             __bf16* dk_exp, __bf16* dv_exp, const int* cu,
                             int nseg, int max_seqlen, int b, int s, int hq,
                             int hkv, int d, float scale, bool causal,
                             bool sbhd, hipStream_t st) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    static_assert(DqTile<D>::QBF == DkvTile<D>::KBW, "one grid for both");
    dim3 grid((max_seqlen + DqTile<D>::QBF - 1) / DqTile<D>::QBF, nseg * hq);
    hipLaunchKernelGGL((flash_varlen_bwd_dq_kernel<D>), grid, dim3(512), 0,
                       st, dout, q, k, v, lse, di, dq, cu, b, s, hq, hkv,
                       scale, causal, sbhd);
    hipLaunchKernelGGL((flash_varlen_bwd_dkv_kernel<D>), grid, dim3(512), 0,
                       st, dout, q, k, v, lse, di, dk_exp, dv_exp, cu, b, s,
                       hq, hkv, scale, causal, sbhd);
  });
}
