// Fused AdamW for gfx950: fp32 master update + low-precision param copy.
//
// Replaces apex FusedAdam (reference: galvatron/core/runtime/optimizer/
// utils.py:8-11). One launch per flat-param shard (shards are large, so
// per-tensor launches are launch-overhead-free); all state streams
// (master/m/v fp32, grad bf16|fp32, out bf16|fp32) read/written vectorized.
#include "common.h"

namespace {

template <typename TG, typename TO>
__global__ void adamw_kernel(float* __restrict__ master,
                             const TG* __restrict__ grad,
                             float* __restrict__ m, float* __restrict__ v,
                             TO* __restrict__ out, long n, float lr,
                             float beta1, float beta2, float eps, float wd,
                             float bc1, float bc2, float gscale) {
  // fully vectorized (8-wide VecIO): the scalar-indexed form measured only
  // ~5 TB/s of the 30 B/param stream; this is a pure-bandwidth kernel
  const long n8 = n & ~7L;
  for (long i = (blockIdx.x * (long)blockDim.x + threadIdx.x) * 8; i < n8;
       i += (long)gridDim.x * blockDim.x * 8) {
    float gv[8], mv8[8], vv8[8], ma8[8], ov[8];
    VecIO<TG>::load(gv, grad + i);
    VecIO<float>::load(mv8, m + i);
    VecIO<float>::load(vv8, v + i);
    VecIO<float>::load(ma8, master + i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float g = gv[k] * gscale;
      const float mv = beta1 * mv8[k] + (1.f - beta1) * g;
      const float vv = beta2 * vv8[k] + (1.f - beta2) * g * g;
      const float denom = sqrtf(vv / bc2) + eps;
      const float upd = (mv / bc1) / denom + wd * ma8[k];
      const float p = ma8[k] - lr * upd;
      mv8[k] = mv;
      vv8[k] = vv;
      ma8[k] = p;
      ov[k] = p;
    }
    VecIO<float>::store(m + i, mv8);
    VecIO<float>::store(v + i, vv8);
    VecIO<float>::store(master + i, ma8);
    VecIO<TO>::store(out + i, ov);
  }
  // tail
  for (long j = n8 + blockIdx.x * (long)blockDim.x + threadIdx.x; j < n;
       j += (long)gridDim.x * blockDim.x) {
    const float g = (float)grad[j] * gscale;
    float mv = m[j] = beta1 * m[j] + (1.f - beta1) * g;
    float vv = v[j] = beta2 * v[j] + (1.f - beta2) * g * g;
    const float denom = sqrtf(vv / bc2) + eps;
    const float upd = (mv / bc1) / denom + wd * master[j];
    const float p = master[j] - lr * upd;
    master[j] = p;
    out[j] = (TO)p;
  }
}

// Fused microbatch gradient accumulation: flat_fp32[off:off+n] += (f32)g.
// Replaces the eager `flat_grad[slice].add_(grad.flatten().float())` pair
// (bf16->f32 temp + f32 add measured ~600 ms/step on the 8B bench; this
// single pass is ~80 GB/microbatch instead of ~144).
template <typename TG>
__global__ void grad_accum_kernel(float* __restrict__ flat,
                                  const TG* __restrict__ g, long n) {
  const long n8 = n & ~7L;
  for (long i = (blockIdx.x * (long)blockDim.x + threadIdx.x) * 8; i < n8;
       i += (long)gridDim.x * blockDim.x * 8) {
    float gv[8], fv[8];
    VecIO<TG>::load(gv, g + i);
    VecIO<float>::load(fv, flat + i);
#pragma unroll
    for (int k = 0; k < 8; ++k) fv[k] += gv[k];
    VecIO<float>::store(flat + i, fv);
  }
  for (long i = n8 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    flat[i] += (float)g[i];
}

// Multi-tensor sum-of-squares for the global grad norm: one launch over
// ALL flat grad shards (replaces the per-block eager pow+reduce chain —
// ~105 launch pairs per step on the 8B bench).  chunks: [n,3] int64
// (ptr, offset, count); every block writes its partial to out[blockIdx.x]
// (the caller sums them in a fixed order: same bits on every run).
__global__ void multi_sumsq_kernel(const long* __restrict__ chunks,
                                   int n_chunks, float* __restrict__ out) {
  float acc = 0.f;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const float* p = reinterpret_cast<const float*>(chunks[3 * c]) +
                     chunks[3 * c + 1];
    const long cnt = chunks[3 * c + 2];
    const long cnt4 = cnt & ~3L;
    for (long i = threadIdx.x * 4L; i < cnt4; i += (long)blockDim.x * 4) {
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += g4[k] * g4[k];
    }
    for (long i = cnt4 + threadIdx.x; i < cnt; i += blockDim.x) {
      const float g = p[i];
      acc += g * g;
    }
  }
  acc = wave_sum(acc);
  __shared__ float warp_acc[8];
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) warp_acc[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += warp_acc[w];
    out[blockIdx.x] = t;
  }
}

}  // namespace

int multi_sumsq_grid(int n_chunks) {
  int grid = galv_grid(n_chunks * 4);
  return grid < 1 ? 1 : grid;
}

// out: multi_sumsq_grid(n_chunks) per-block partial sums
void multi_sumsq_launch(const long* chunks, int n_chunks, float* out,
                        hipStream_t st) {
  const int grid = multi_sumsq_grid(n_chunks);
  hipLaunchKernelGGL((multi_sumsq_kernel), dim3(grid), dim3(512), 0, st,
                     chunks, n_chunks, out);
}

template <typename TG>
void grad_accum_launch_t(float* flat, const TG* g, long n, hipStream_t st) {
  int grid = galv_grid((n / 8 + 255) / 256);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((grad_accum_kernel<TG>), dim3(grid), dim3(256), 0, st,
                     flat, g, n);
}

template void grad_accum_launch_t<__bf16>(float*, const __bf16*, long, hipStream_t);
template void grad_accum_launch_t<float>(float*, const float*, long, hipStream_t);

template <typename TG, typename TO>
void adamw_launch_t(float* master, const TG* grad, float* m, float* v,
                    TO* out, long n, int step, float lr, float beta1,
                    float beta2, float eps, float wd, float gscale,
                    hipStream_t st) {
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2 = 1.f - powf(beta2, (float)step);
  int grid = galv_grid((n / 8 + 255) / 256);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((adamw_kernel<TG, TO>), dim3(grid), dim3(256), 0, st,
                     master, grad, m, v, out, n, lr, beta1, beta2, eps, wd,
                     bc1, bc2, gscale);
}

template void adamw_launch_t<float, float>(float*, const float*, float*, float*, float*, long, int, float, float, float, float, float, float, hipStream_t);
template void adamw_launch_t<float, __bf16>(float*, const float*, float*, float*, __bf16*, long, int, float, float, float, float, float, float, hipStream_t);
template void adamw_launch_t<__bf16, float>(float*, const __bf16*, float*, float*, float*, long, int, float, float, float, float, float, float, hipStream_t);
template void adamw_launch_t<__bf16, __bf16>(float*, const __bf16*, float*, float*, __bf16*, long, int, float, float, float, float, float, float, hipStream_t);
