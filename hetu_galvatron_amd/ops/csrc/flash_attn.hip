// Dense flash attention for gfx950: q [b, sq, hq, D], k/v [b, skv, hkv, D]
// (or [s, b, h, D] with sbhd), bias, sliding window, cross lengths.  The
// block bodies are in flash_attn_body.h; this module adds the dense
// kernels, attn_di and the MFMA layout probe.
//
// The dense bodies are noinline and already spill; of the body header's
// optional steps they keep only the rescale skip at D = 128.  The skip at
// D = 64 and the mask split of dq each cost these kernels scratch.
#define FLASH_SKIP_RESCALE(D) ((D) == 128)
#define FLASH_DQ_MASK_SPLIT(D) 0
#include "flash_attn_body.h"
#include "flash_attn_launch.h"

namespace {

// thin kernel: common indexing + complementary-pair causal load balance
// (block x runs q blocks {x, nqb-1-x}: constant total KV tiles per block,
// so the makespan matches the average instead of 2x the deepest block)
template <int D, bool BIASED = false, bool WINDOWED = false>
__global__ __launch_bounds__(512, 2)
void flash_fwd_kernel(const __bf16* __restrict__ q,
                      const __bf16* __restrict__ k,
                      const __bf16* __restrict__ v,
                      __bf16* __restrict__ o, float* __restrict__ lse,
                      int b, int sq, int skv, int hq, int hkv, float scale,
                      bool causal, const __bf16* __restrict__ bias = nullptr,
                      bool paired = true, bool sbhd = false,
                      int window = 0) {
  constexpr int QBF = FwdTile<D>::QBF;
  __shared__ __align__(16) __bf16 smem[2 * FwdTile<D>::BUFSZ];
  const int bh = blockIdx.y;
  const int bi = bh / hq;
  const int h = bh - bi * hq;
  const int hk = h / (hq / hkv);
  // sbhd: tensors are [s, b, h, d] (the runtime's native activation
  // layout) — only the per-(b,h) base and the s-stride change
  const long q_base = sbhd ? ((long)bi * hq + h) * D
                           : ((long)bi * sq * hq + h) * D;
  const long kv_base = sbhd ? ((long)bi * hkv + hk) * D
                            : ((long)bi * skv * hkv + hk) * D;
  const int q_str = (sbhd ? b * hq : hq) * D;
  const int kv_str = (sbhd ? b * hkv : hkv) * D;
  const long lse_base = ((long)bi * hq + h) * sq;
  const long bias_base = (long)h * sq * skv;  // bias [hq, sq, skv]
  const float sl2e = scale * 1.4426950408889634f;
  const int off = skv - sq;
  const int nqb = (sq + QBF - 1) / QBF;
  flash_fwd_block<D, BIASED, WINDOWED>(blockIdx.x, q, k, v, o, lse, smem, q_base,
                             kv_base, lse_base, q_str, kv_str, off, sq,
                             skv, sl2e, causal, bias, bias_base, window);
  const int qb2 = nqb - 1 - (int)blockIdx.x;
  if (causal && paired && qb2 > (int)blockIdx.x) {
    __syncthreads();
    flash_fwd_block<D, BIASED, WINDOWED>(qb2, q, k, v, o, lse, smem, q_base, kv_base,
                               lse_base, q_str, kv_str, off, sq, skv,
                               sl2e, causal, bias, bias_base, window);
  }
}

// ---------------------------------------------------------------------------
// Di = rowsum(dO * O)  — one wave per (b, s, h) row
// ---------------------------------------------------------------------------
template <int D>
__global__ void attn_di_kernel(const __bf16* __restrict__ dout,
                               const __bf16* __restrict__ o,
                               float* __restrict__ di, int b, int sq, int hq,
                               bool sbhd = false) {
  // row index = (bi*sq + s)*hq + h (bshd) or (s*b + bi)*hq + h (sbhd)
  const long rows = (long)b * sq * hq;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  constexpr int EPL = D / 64;  // elems per lane
  for (long row = blockIdx.x * 4 + wid; row < rows; row += (long)gridDim.x * 4) {
    const __bf16* dp = dout + row * D;
    const __bf16* op = o + row * D;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
      const int c = lane * EPL + i;
      acc += (float)dp[c] * (float)op[c];
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      // di layout [b, hq, sq]
      long bi, s, h;
      if (sbhd) {
        s = row / ((long)b * hq);
        const long rem = row - s * b * hq;
        bi = rem / hq;
        h = rem - bi * hq;
      } else {
        bi = row / ((long)sq * hq);
        const long rem = row - bi * sq * hq;
        s = rem / hq;
        h = rem - s * hq;
      }
      di[(bi * hq + h) * sq + s] = acc;
    }
  }
}

template <int D, bool BIASED = false, bool WINDOWED = false>
__global__ __launch_bounds__(512, 2)
void flash_bwd_dq_kernel(const __bf16* __restrict__ dout,
                         const __bf16* __restrict__ q,
                         const __bf16* __restrict__ k,
                         const __bf16* __restrict__ v,
                         const float* __restrict__ lse,
                         const float* __restrict__ di,
                         __bf16* __restrict__ dq,
                         int b, int sq, int skv, int hq, int hkv,
                         float scale, bool causal,
                         const __bf16* __restrict__ bias = nullptr,
                         bool paired = true, bool sbhd = false,
                         int window = 0) {
  constexpr int QBF = DqTile<D>::QBF;
  __shared__ __align__(16) __bf16 smem[2 * DqTile<D>::BUFSZ];
  const int bh = blockIdx.y;
  const int bi = bh / hq;
  const int h = bh - bi * hq;
  const int hk = h / (hq / hkv);
  const long q_base = sbhd ? ((long)bi * hq + h) * D
                           : ((long)bi * sq * hq + h) * D;
  const long kv_base = sbhd ? ((long)bi * hkv + hk) * D
                            : ((long)bi * skv * hkv + hk) * D;
  const int q_str = (sbhd ? b * hq : hq) * D;
  const int kv_str = (sbhd ? b * hkv : hkv) * D;
  const long lse_base = ((long)bi * hq + h) * sq;
  const long bias_base = (long)h * sq * skv;
  const int off = skv - sq;
  const int nqb = (sq + QBF - 1) / QBF;
  flash_bwd_dq_block<D, BIASED, WINDOWED>(blockIdx.x, dout, q, k, v, lse, di, dq,
                                smem, q_base, kv_base, lse_base, q_str,
                                kv_str, off, sq, skv, scale, causal, bias,
                                bias_base, window);
  const int qb2 = nqb - 1 - (int)blockIdx.x;
  if (causal && paired && qb2 > (int)blockIdx.x) {
    __syncthreads();
    flash_bwd_dq_block<D, BIASED, WINDOWED>(qb2, dout, q, k, v, lse, di, dq, smem,
                                  q_base, kv_base, lse_base, q_str,
                                  kv_str, off, sq, skv, scale, causal,
                                  bias, bias_base, window);
  }
}

template <int D, bool BIASED = false, bool WINDOWED = false>
__global__ __launch_bounds__(512, 2)
void flash_bwd_dkv_kernel(const __bf16* __restrict__ dout,
                          const __bf16* __restrict__ q,
                          const __bf16* __restrict__ k,
                          const __bf16* __restrict__ v,
                          const float* __restrict__ lse,
                          const float* __restrict__ di,
                          __bf16* __restrict__ dk_exp,   // [b, skv, hq, D]
                          __bf16* __restrict__ dv_exp,
                          int b, int sq, int skv, int hq, int hkv,
                          float scale, bool causal,
                          const __bf16* __restrict__ bias = nullptr,
                          float* __restrict__ dbias = nullptr,
                          bool paired = true, bool sbhd = false,
                          int window = 0) {
  constexpr int KBW = DkvTile<D>::KBW;
  __shared__ __align__(16) __bf16 smem[2 * DkvTile<D>::BUFSZ];
  __shared__ __align__(16) float lsedi[4 * DkvTile<D>::QT];
  const int bh = blockIdx.y;
  const int bi = bh / hq;
  const int h = bh - bi * hq;
  const int hk = h / (hq / hkv);
  const long q_base = sbhd ? ((long)bi * hq + h) * D
                           : ((long)bi * sq * hq + h) * D;
  const long kv_base = sbhd ? ((long)bi * hkv + hk) * D
                            : ((long)bi * skv * hkv + hk) * D;
  // dk_exp/dv_exp are [b, skv, hq, D] (bshd) or [skv, b, hq, D] (sbhd)
  const long dkv_base = sbhd ? ((long)bi * hq + h) * D
                             : ((long)bi * skv * hq + h) * D;
  const int q_str = (sbhd ? b * hq : hq) * D;
  const int kv_str = (sbhd ? b * hkv : hkv) * D;
  const int dkv_str = (sbhd ? b * hq : hq) * D;
  const long lse_base = ((long)bi * hq + h) * sq;
  const int off = skv - sq;
  const int nkb = (skv + KBW - 1) / KBW;
  const long bias_base = (long)h * sq * skv;
  flash_bwd_dkv_block<D, BIASED, WINDOWED>(blockIdx.x, dout, q, k, v, lse, di, dk_exp,
                                 dv_exp, smem, lsedi, q_base, kv_base,
                                 dkv_base, lse_base, q_str, kv_str,
                                 dkv_str, off, sq, skv, scale, causal, bias,
                                 dbias, bias_base, window);
  const int kb2 = nkb - 1 - (int)blockIdx.x;
  if (causal && paired && kb2 > (int)blockIdx.x) {
    __syncthreads();
    flash_bwd_dkv_block<D, BIASED, WINDOWED>(kb2, dout, q, k, v, lse, di, dk_exp,
                                   dv_exp, smem, lsedi, q_base, kv_base,
                                   dkv_base, lse_base, q_str, kv_str,
                                   dkv_str, off, sq, skv, scale, causal,
                                   bias, dbias, bias_base, window);
  }
}

// ---------------------------------------------------------------------------
// MFMA layout probe: one-wave 32x32x16 GEMM from global memory laid out by
// the assumed fragment maps. Validated against torch matmul on-device.
// ---------------------------------------------------------------------------
template <bool ALT>
__global__ void mfma_probe_kernel(const __bf16* __restrict__ A,  // [32][16]
                                  const __bf16* __restrict__ B,  // [16][32]
                                  float* __restrict__ Dst) {     // [32][32]
  const int lane = threadIdx.x & 63;
  bf16x8 a, bfrag;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int kk = ALT ? mfma32_ab_k_alt(lane, j) : mfma32_ab_k(lane, j);
    a[j] = A[(lane & 31) * 16 + kk];
    bfrag[j] = B[kk * 32 + (lane & 31)];
  }
  f32x16 d = mfma32_bf16(a, bfrag, (f32x16)(0.f));
#pragma unroll
  for (int i = 0; i < 16; ++i)
    Dst[mfma32_d_row(lane, i) * 32 + mfma32_d_col(lane)] = d[i];
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
void flash_fwd_launch(const __bf16* q, const __bf16* k, const __bf16* v,
                      __bf16* o, float* lse, int b, int sq, int skv, int hq,
                      int hkv, int d, float scale, bool causal,
                      hipStream_t st, const __bf16* bias, bool sbhd,
                      int window) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    const int nqb = (sq + FwdTile<D>::QBF - 1) / FwdTile<D>::QBF;
    const bool paired = flash_paired(nqb, b, hq, causal);
    dim3 grid(paired ? (nqb + 1) / 2 : nqb, b * hq);
    if (bias != nullptr)
      hipLaunchKernelGGL((flash_fwd_kernel<D, true>), grid, dim3(512), 0, st,
                         q, k, v, o, lse, b, sq, skv, hq, hkv, scale, causal,
                         bias, paired, sbhd, window);
    else if (window > 0)
      hipLaunchKernelGGL((flash_fwd_kernel<D, false, true>), grid, dim3(512),
                         0, st, q, k, v, o, lse, b, sq, skv, hq, hkv, scale,
                         causal, nullptr, paired, sbhd, window);
    else
      hipLaunchKernelGGL((flash_fwd_kernel<D>), grid, dim3(512), 0, st, q, k,
                         v, o, lse, b, sq, skv, hq, hkv, scale, causal,
                         nullptr, paired, sbhd, 0);
  });
}

void attn_di_launch(const __bf16* dout, const __bf16* o, float* di, int b,
                    int sq, int hq, int d, hipStream_t st, bool sbhd) {
  const long rows = (long)b * sq * hq;
  const int grid = galv_grid((rows + 3) / 4);
  with_head_dim(d, [&](auto dc) {
    hipLaunchKernelGGL((attn_di_kernel<decltype(dc)::value>), dim3(grid),
                       dim3(256), 0, st, dout, o, di, b, sq, hq, sbhd);
  });
}

void flash_bwd_launch(const __bf16* dout, const __bf16* q, const __bf16* k,
                      const __bf16* v, const float* lse, const float* di,
                      __bf16* dq, __bf16* dk_exp, __bf16* dv_exp, int b,
                      int sq, int skv, int hq, int hkv, int d, float scale,
                      bool causal, hipStream_t st, const __bf16* bias,
                      float* dbias, bool sbhd, int window) {
  with_head_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    const int nqb = (sq + DqTile<D>::QBF - 1) / DqTile<D>::QBF;
    const bool pq = flash_paired(nqb, b, hq, causal);
    dim3 gq(pq ? (nqb + 1) / 2 : nqb, b * hq);
    const int nkb = (skv + DkvTile<D>::KBW - 1) / DkvTile<D>::KBW;
    const bool pkv = flash_paired(nkb, b, hq, causal);
    dim3 gkv(pkv ? (nkb + 1) / 2 : nkb, b * hq);
    if (bias != nullptr) {
      hipLaunchKernelGGL((flash_bwd_dq_kernel<D, true>), gq, dim3(512), 0, st,
                         dout, q, k, v, lse, di, dq, b, sq, skv, hq, hkv,
                         scale, causal, bias, pq, sbhd, window);
      hipLaunchKernelGGL((flash_bwd_dkv_kernel<D, true>), gkv, dim3(512), 0,
                         st, dout, q, k, v, lse, di, dk_exp, dv_exp, b, sq,
                         skv, hq, hkv, scale, causal, bias, dbias, pkv, sbhd,
                         window);
    } else if (window > 0) {
      hipLaunchKernelGGL((flash_bwd_dq_kernel<D, false, true>), gq,
                         dim3(512), 0, st, dout, q, k, v, lse, di, dq, b, sq,
                         skv, hq, hkv, scale, causal, nullptr, pq, sbhd,
                         window);
      hipLaunchKernelGGL((flash_bwd_dkv_kernel<D, false, true>), gkv,
                         dim3(512), 0, st, dout, q, k, v, lse, di, dk_exp,
                         dv_exp, b, sq, skv, hq, hkv, scale, causal, nullptr,
                         nullptr, pkv, sbhd, window);
    } else {
      hipLaunchKernelGGL((flash_bwd_dq_kernel<D>), gq, dim3(512), 0, st,
                         dout, q, k, v, lse, di, dq, b, sq, skv, hq, hkv,
                         scale, causal, nullptr, pq, sbhd, 0);
      hipLaunchKernelGGL((flash_bwd_dkv_kernel<D>), gkv, dim3(512), 0, st,
                         dout, q, k, v, lse, di, dk_exp, dv_exp, b, sq, skv,
                         hq, hkv, scale, causal, nullptr, nullptr, pkv, sbhd,
                         0);
    }
  });
}

void mfma_probe_launch(const __bf16* A, const __bf16* B, float* Dst, bool alt,
                       hipStream_t st) {
  if (alt)
    hipLaunchKernelGGL((mfma_probe_kernel<true>), dim3(1), dim3(64), 0, st,
                       A, B, Dst);
  else
    hipLaunchKernelGGL((mfma_probe_kernel<false>), dim3(1), dim3(64), 0, st,
                       A, B, Dst);
}
