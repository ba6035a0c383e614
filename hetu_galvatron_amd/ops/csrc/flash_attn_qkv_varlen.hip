// Packed documents on the packed-QKV buffer: the varlen work mapping (one
// workgroup per (segment, head, 256-row block) of a cu_seqlens table, see
// cu_seg in flash_attn_body.h) with the packed-QKV addressing (packed_addr
// there).  sbhd only, sq = skv = len, off = 0, no bias, no window.  As in
// the varlen module there is no complementary pairing, blocks past the end
// of a short segment leave before touching memory, a malformed entry is an
// empty segment, and each body has one call site and is inlined into it.
//
// The dq mask split raises the D = 64 dq kernel past 128 VGPRs, i.e. from
// two resident workgroups per CU to one; it is left out at that D.
#define FLASH_DQ_MASK_SPLIT(D) ((D) == 128)
#include "flash_attn_body.h"
#include "flash_attn_launch.h"

namespace {

// -> the addresses of this workgroup's (segment, head); len = tokens in the
// segment (0 = nothing to do)
template <int D>
DEV_INLINE PackedAddr packed_seg(const int* __restrict__ cu, int b, int s,
                                 int G, int qpg, int& len) {
  const int hq = G * qpg;
  const int seg = blockIdx.y / hq;
  const int h = blockIdx.y - seg * hq;
  const Seg c = cu_seg(cu, seg, b, s);
  len = c.len;
  return packed_addr<D>(c.p0, c.bi, h, b, s, G, qpg);
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_packed_varlen_fwd_kernel(const __bf16* __restrict__ qkv,
                                    __bf16* __restrict__ o,
                                    float* __restrict__ lse,
                                    const int* __restrict__ cu, int b, int s,
                                    int G, int qpg, float scale,
                                    bool causal) {
  __shared__ __align__(16) __bf16 smem[2 * FwdTile<D>::BUFSZ];
  int len;
  const PackedAddr p = packed_seg<D>(cu, b, s, G, qpg, len);
  // workgroup-uniform, before any barrier; also covers len == 0
  if ((int)blockIdx.x * FwdTile<D>::QBF >= len) return;
  const __bf16* k = qkv + (long)qpg * D;
  const __bf16* v = k + D;
  const OutOwn oa{p.o_base, p.o_str};
  const float sl2e = scale * 1.4426950408889634f;
  FLASH_INLINE_CALL flash_fwd_block<D, false, false, OutOwn>(
      blockIdx.x, qkv, k, v, o, lse, smem, p.q_base, p.kv_base, p.lse_base,
      p.qkv_str, p.qkv_str, 0, len, len, sl2e, causal, nullptr, 0, 0, oa);
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_packed_varlen_bwd_dq_kernel(const __bf16* __restrict__ dout,
                                       const __bf16* __restrict__ qkv,
                                       const float* __restrict__ lse,
                                       const float* __restrict__ di,
                                       __bf16* __restrict__ dqkv,
                                       const int* __restrict__ cu, int b,
                                       int s, int G, int qpg, float scale,
                                       bool causal) {
  __shared__ __align__(16) __bf16 smem[2 * DqTile<D>::BUFSZ];
  int len;
  const PackedAddr p = packed_seg<D>(cu, b, s, G, qpg, len);
  if ((int)blockIdx.x * DqTile<D>::QBF >= len) return;
  const __bf16* k = qkv + (long)qpg * D;
  const __bf16* v = k + D;
  const OutOwn oa{p.o_base, p.o_str};
  FLASH_INLINE_CALL flash_bwd_dq_block<D, false, false, OutOwn>(
      blockIdx.x, dout, qkv, k, v, lse, di, dqkv, smem, p.q_base, p.kv_base,
      p.lse_base, p.qkv_str, p.qkv_str, 0, len, len, scale, causal, nullptr,
      0, 0, oa);
}

template <int D>
__global__ __launch_bounds__(512, 2)
void flash_packed_varlen_bwd_dkv_kernel(const __bf16* __restrict__ dout,
                                        const __bf16* __restrict__ qkv,
                                        const float* __restrict__ lse,
                                        const float* __restrict__ di,
                                        __bf16* __restrict__ dk_exp,
                                        __bf16* __restrict__ dv_exp,
                                        const int* __restrict__ cu, int b,
                                        int s, int G, int qpg, float scale,
                                        bool causal) {
  __shared__ __align__(16) __bf16 smem[2 * DkvTile<D>::BUFSZ];
  __shared__ __align__(16) float lsedi[4 * DkvTile<D>::QT];
  int len;
  const PackedAddr p = packed_seg<D>(cu, b, s, G, qpg, len);
  if ((int)blockIdx.x * DkvTile<D>::KBW >= len) return;
  const __bf16* k = qkv + (long)qpg * D;
  const __bf16* v = k + D;
  const OutOwn oa{p.o_base, p.o_str};
  // the two phases of flash_bwd_dkv_block, dV then dK; dk_exp / dv_exp
  // carry hq heads in o's layout
  FLASH_INLINE_CALL flash_bwd_dkv_phase<D, false, false, false, OutOwn>(
      blockIdx.x, dout, qkv, k, v, lse, di, dk_exp, dv_exp, smem, lsedi,
      p.q_base, p.kv_base, p.o_base, p.lse_base, p.qkv_str, p.qkv_str,
      p.o_str, 0, len, len, scale, causal, nullptr, nullptr, 0, 0, oa);
  __syncthreads();
  FLASH_INLINE_CALL flash_bwd_dkv_phase<D, true, false, false, OutOwn>(
      blockIdx.x, dout, qkv, k, v, lse, di, dk_exp, dv_exp, smem, lsedi,
      p.q_base, p.kv_base, p.o_base, p.lse_base, p.qkv_str, p.qkv_str,
      p.o_str, 0, len, len, scale, causal, nullptr, nullptr, 0, 0, oa);
}

}  // namespace

// the varlen grid with hq = G*qpg heads
void flash_packed_varlen_fwd_launch(const __bf16* qkv, __bf16* o, float* lse,
                                    const int* cu, int nseg, int max_seqlen,
                                    int b, int s, int G, int qpg, int d,
                                    float scale, bool causal,
                                    hipStream_t st) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    dim3 grid((max_seqlen + FwdTile<D>::QBF - 1) / FwdTile<D>::QBF,
              nseg * G * qpg);
    hipLaunchKernelGGL((flash_packed_varlen_fwd_kernel<D>), grid, dim3(512),
                       0, st, qkv, o, lse, cu, b, s, G, qpg, scale, causal);
  });
}

void flash_packed_varlen_bwd_launch(const __bf16* dout, const __bf16* qkv,
                                    const float* lse, const float* di,
                                    __bf16* dqkv, __bf16* dk_exp,
                                    __bf16* dv_exp, const int* cu, int nseg,
                                    int max_seqlen, int b, int s, int G,
                                    int qpg, int d, float scale, bool causal,
                                    hipStream_t st) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    static_assert(DqTile<D>::QBF == DkvTile<D>::KBW, "one grid for both");
    dim3 grid((max_seqlen + DqTile<D>::QBF - 1) / DqTile<D>::QBF,
              nseg * G * qpg);
    hipLaunchKernelGGL((flash_packed_varlen_bwd_dq_kernel<D>), grid,
                       dim3(512), 0, st, dout, qkv, lse, di, dqkv, cu, b, s,
                       G, qpg, scale, causal);
    hipLaunchKernelGGL((flash_packed_varlen_bwd_dkv_kernel<D>), grid,
                       dim3(512), 0, st, dout, qkv, lse, di, dk_exp, dv_exp,
                       cu, b, s, G, qpg, scale, causal);
  });
}
