// Fused RMSNorm / LayerNorm forward+backward for gfx950.
//
// Replaces the reference's flash-attn CUDA fused norms
// (galvatron/core/runtime/transformer/norm.py:3-30 hard-imports
// flash_attn.ops.rms_norm / dropout_layer_norm) with CDNA4-native kernels.
//
// Memory-bound: bf16 loads vectorized as 16 B/lane packets (guide G13),
// 256-thread blocks, one row per block iteration, grid-stride over rows.
// Column ownership per thread is a fixed stride-2048 comb, so backward
// accumulates per-thread dw/db partials in registers (VPT packets) and
// commits them into a per-block partial buffer [grid][H] (atomic-free —
// a global-atomic variant measured 246 ms/step on the 8B bench from
// grid-way contention on H addresses); a small column-sum kernel reduces
// the partials.
#include "common.h"

namespace {

// res/sum_out (optional): fused residual-add — normalizes (x + res) and
// writes the sum for the downstream residual stream (the reference's
// DropoutAddLayerNorm fusion, norm.py:3-30)
template <typename T, int VPT>
__global__ void rmsnorm_fwd_kernel(const T* __restrict__ x,
                                   const T* __restrict__ w,
                                   T* __restrict__ y,
                                   float* __restrict__ invrms,
                                   long n, int H, float eps,
                                   const T* __restrict__ res = nullptr,
                                   T* __restrict__ sum_out = nullptr) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  for (long row = blockIdx.x; row < n; row += gridDim.x) {
    const T* xr = x + row * (long)H;
    T* yr = y + row * (long)H;
    float ss = 0.f;
    float xv[VPT][8];
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        VecIO<T>::load(xv[p], xr + c);
        if (res != nullptr) {
          float rv[8];
          VecIO<T>::load(rv, res + row * (long)H + c);
#pragma unroll
          for (int i = 0; i < 8; ++i) xv[p][i] += rv[i];
          VecIO<T>::store(sum_out + row * (long)H + c, xv[p]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) ss += xv[p][i] * xv[p][i];
      }
    }
    float inv = rsqrtf(block_sum_256(ss, red) / H + eps);
    if (tid == 0) invrms[row] = inv;
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        float wv[8], out[8];
        VecIO<T>::load(wv, w + c);
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = xv[p][i] * inv * wv[i];
        VecIO<T>::store(yr + c, out);
      }
    }
  }
}

template <typename T, int VPT>
__global__ void rmsnorm_bwd_kernel(const T* __restrict__ dy,
                                   const T* __restrict__ x,
                                   const T* __restrict__ w,
                                   const float* __restrict__ invrms,
                                   T* __restrict__ dx,
                                   float* __restrict__ dw_part,  // [grid][H]
                                   long n, int H,
                                   const T* __restrict__ dsum_in = nullptr) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float dw_acc[VPT][8];
#pragma unroll
  for (int p = 0; p < VPT; ++p)
#pragma unroll
    for (int i = 0; i < 8; ++i) dw_acc[p][i] = 0.f;

  float wv[VPT][8];
#pragma unroll
  for (int p = 0; p < VPT; ++p) {
    int c = (tid + p * 256) * 8;
    if (c < H) VecIO<T>::load(wv[p], w + c);
  }

  for (long row = blockIdx.x; row < n; row += gridDim.x) {
    const T* xr = x + row * (long)H;
    const T* dyr = dy + row * (long)H;
    T* dxr = dx + row * (long)H;
    const float inv = invrms[row];
    float xv[VPT][8], dyv[VPT][8];
    float dot = 0.f;
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        VecIO<T>::load(xv[p], xr + c);
        VecIO<T>::load(dyv[p], dyr + c);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          dot += (dyv[p][i] * wv[p][i]) * (xv[p][i] * inv);
      }
    }
    const float c1 = block_sum_256(dot, red) / H;
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        float out[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xhat = xv[p][i] * inv;
          out[i] = inv * (dyv[p][i] * wv[p][i] - xhat * c1);
          dw_acc[p][i] += dyv[p][i] * xhat;
        }
        if (dsum_in != nullptr) {
          float dsv[8];
          VecIO<T>::load(dsv, dsum_in + row * (long)H + c);
#pragma unroll
          for (int i = 0; i < 8; ++i) out[i] += dsv[i];
        }
        VecIO<T>::store(dxr + c, out);
      }
    }
  }
  float* my_part = dw_part + (long)blockIdx.x * H;
#pragma unroll
  for (int p = 0; p < VPT; ++p) {
    int c = (tid + p * 256) * 8;
    if (c < H) VecIO<float>::store(my_part + c, dw_acc[p]);
  }
}

// column-sum of per-block partials: out[c] = sum_g part[g][c], in a fixed
// order so that the result is the same bit for bit on every run.
// A single serial g-loop per column measured 0.5 ms/call at G=2048, so for
// large G the sum runs in two passes: colsum_slices_kernel lets grid.y
// slices of `per` rows each reduce their rows into the slice's first row
// (in place: every element of a slice is read and written by one thread
// only), then colsum_kernel adds those first rows (gstep = per).
__global__ void colsum_slices_kernel(float* __restrict__ part, int G, int H,
                                     int n_out, int per) {
  const int g0 = blockIdx.y * per;
  const int g1 = min(G, g0 + per);
  if (g0 >= g1) return;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
       idx < (long)n_out * H; idx += (long)gridDim.x * blockDim.x) {
    const int o = idx / H;
    const int c = idx - (long)o * H;
    float acc = 0.f;
    float* p = part + (long)o * G * H + c;
    for (int g = g0; g < g1; ++g) acc += p[(long)g * H];
    p[(long)g0 * H] = acc;
  }
}

__global__ void colsum_kernel(const float* __restrict__ part,
                              float* __restrict__ out, int G, int H,
                              int n_out, int gstep) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
       idx < (long)n_out * H; idx += (long)gridDim.x * blockDim.x) {
    const int o = idx / H;
    const int c = idx - (long)o * H;
    float acc = 0.f;
    const float* p = part + (long)o * G * H + c;
    for (int g = 0; g < G; g += gstep) acc += p[(long)g * H];
    out[idx] = acc;
  }
}

// part: [n_out][G][H] (clobbered) -> out: [n_out][H]
static void colsum_launch(float* part, float* out, int G, int H, int n_out,
                          hipStream_t s) {
  const dim3 gx(galv_grid(((long)n_out * H + 255) / 256));
  int gstep = 1;
  if (G > 64) {
    const int gy = 32;
    gstep = (G + gy - 1) / gy;
    hipLaunchKernelGGL(colsum_slices_kernel, dim3(gx.x, gy), dim3(256), 0, s,
                       part, G, H, n_out, gstep);
  }
  hipLaunchKernelGGL(colsum_kernel, gx, dim3(256), 0, s, part, out, G, H,
                     n_out, gstep);
}

template <typename T, int VPT>
__global__ void layernorm_fwd_kernel(const T* __restrict__ x,
                                     const T* __restrict__ w,
                                     const T* __restrict__ b,
                                     T* __restrict__ y,
                                     float* __restrict__ mean_out,
                                     float* __restrict__ invstd_out,
                                     long n, int H, float eps) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  for (long row = blockIdx.x; row < n; row += gridDim.x) {
    const T* xr = x + row * (long)H;
    T* yr = y + row * (long)H;
    float s = 0.f, ss = 0.f;
    float xv[VPT][8];
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        VecIO<T>::load(xv[p], xr + c);
#pragma unroll
        for (int i = 0; i < 8; ++i) s += xv[p][i];
      }
    }
    const float mean = block_sum_256(s, red) / H;
    // centred second pass over the registers: E[x^2] - mean^2 in fp32
    // cancels catastrophically for rows with |mean| >> std (mean 64,
    // std 0.05 lost 10-26 % of the variance and could go negative)
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float dlt = xv[p][i] - mean;
          ss += dlt * dlt;
        }
      }
    }
    const float var = block_sum_256(ss, red) / H;
    const float inv = rsqrtf(var + eps);
    if (tid == 0) { mean_out[row] = mean; invstd_out[row] = inv; }
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        float wv[8], bv[8], out[8];
        VecIO<T>::load(wv, w + c);
        VecIO<T>::load(bv, b + c);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          out[i] = (xv[p][i] - mean) * inv * wv[i] + bv[i];
        VecIO<T>::store(yr + c, out);
      }
    }
  }
}

template <typename T, int VPT>
__global__ void layernorm_bwd_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const T* __restrict__ w,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ invstd,
                                     T* __restrict__ dx,
                                     float* __restrict__ dwdb_part,  // [2][grid][H]
                                     long n, int H) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float dw_acc[VPT][8], db_acc[VPT][8];
#pragma unroll
  for (int p = 0; p < VPT; ++p)
#pragma unroll
    for (int i = 0; i < 8; ++i) { dw_acc[p][i] = 0.f; db_acc[p][i] = 0.f; }

  float wv[VPT][8];
#pragma unroll
  for (int p = 0; p < VPT; ++p) {
    int c = (tid + p * 256) * 8;
    if (c < H) VecIO<T>::load(wv[p], w + c);
  }

  for (long row = blockIdx.x; row < n; row += gridDim.x) {
    const T* xr = x + row * (long)H;
    const T* dyr = dy + row * (long)H;
    T* dxr = dx + row * (long)H;
    const float m = mean[row];
    const float inv = invstd[row];
    float xv[VPT][8], dyv[VPT][8];
    float s1 = 0.f, s2 = 0.f;  // mean(dxhat), mean(dxhat*xhat)
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        VecIO<T>::load(xv[p], xr + c);
        VecIO<T>::load(dyv[p], dyr + c);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float dxhat = dyv[p][i] * wv[p][i];
          s1 += dxhat;
          s2 += dxhat * (xv[p][i] - m) * inv;
        }
      }
    }
    const float c1 = block_sum_256(s1, red) / H;
    const float c2 = block_sum_256(s2, red) / H;
#pragma unroll
    for (int p = 0; p < VPT; ++p) {
      int c = (tid + p * 256) * 8;
      if (c < H) {
        float out[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xhat = (xv[p][i] - m) * inv;
          const float dxhat = dyv[p][i] * wv[p][i];
          out[i] = inv * (dxhat - c1 - xhat * c2);
          dw_acc[p][i] += dyv[p][i] * xhat;
          db_acc[p][i] += dyv[p][i];
        }
        VecIO<T>::store(dxr + c, out);
      }
    }
  }
  float* w_part = dwdb_part + (long)blockIdx.x * H;
  float* b_part = dwdb_part + ((long)gridDim.x + blockIdx.x) * H;
#pragma unroll
  for (int p = 0; p < VPT; ++p) {
    int c = (tid + p * 256) * 8;
    if (c < H) {
      VecIO<float>::store(w_part + c, dw_acc[p]);
      VecIO<float>::store(b_part + c, db_acc[p]);
    }
  }
}

template <template <typename, int> class K>
struct NormDispatch {};

}  // namespace

// ---------------------------------------------------------------------------
// Host launchers (raw pointers; bindings.cpp owns the torch glue).
// ---------------------------------------------------------------------------
#define DISPATCH_VPT(H, FN)                                              \
  do {                                                                   \
    int packs = ((H) + 8 * 256 - 1) / (8 * 256);                         \
    if (packs <= 1)      FN(1);                                          \
    else if (packs <= 2) FN(2);                                          \
    else if (packs <= 4) FN(4);                                          \
    else if (packs <= 8) FN(8);                                          \
  } while (0)

template <typename T>
void rmsnorm_fwd_launch_t(const T* x, const T* w, T* y, float* invrms,
                          long n, int H, float eps, hipStream_t s,
                          const T* res, T* sum_out) {
  int grid = galv_grid(n);
#define RUN(V) hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, V>), dim3(grid), \
                                  dim3(256), 0, s, x, w, y, invrms, n, H, \
                                  eps, res, sum_out)
  DISPATCH_VPT(H, RUN);
#undef RUN
}

int norm_bwd_grid(long n) { return galv_grid(n, 2048); }

template <typename T>
void rmsnorm_bwd_launch_t(const T* dy, const T* x, const T* w,
                          const float* invrms, T* dx, float* dw_part,
                          float* dw, long n, int H, hipStream_t s,
                          const T* dsum_in) {
  int grid = norm_bwd_grid(n);
#define RUN(V) hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, V>), dim3(grid), \
                                  dim3(256), 0, s, dy, x, w, invrms, dx, \
                                  dw_part, n, H, dsum_in)
  DISPATCH_VPT(H, RUN);
#undef RUN
  colsum_launch(dw_part, dw, grid, H, 1, s);
}

template <typename T>
void layernorm_fwd_launch_t(const T* x, const T* w, const T* b, T* y,
                            float* mean, float* invstd, long n, int H,
                            float eps, hipStream_t s) {
  int grid = galv_grid(n);
#define RUN(V) hipLaunchKernelGGL((layernorm_fwd_kernel<T, V>), dim3(grid), \
                                  dim3(256), 0, s, x, w, b, y, mean, invstd, n, H, eps)
  DISPATCH_VPT(H, RUN);
#undef RUN
}

template <typename T>
void layernorm_bwd_launch_t(const T* dy, const T* x, const T* w,
                            const float* mean, const float* invstd, T* dx,
                            float* dwdb_part, float* dwdb, long n, int H,
                            hipStream_t s) {
  int grid = norm_bwd_grid(n);
#define RUN(V) hipLaunchKernelGGL((layernorm_bwd_kernel<T, V>), dim3(grid), \
                                  dim3(256), 0, s, dy, x, w, mean, invstd, dx, dwdb_part, n, H)
  DISPATCH_VPT(H, RUN);
#undef RUN
  colsum_launch(dwdb_part, dwdb, grid, H, 2, s);
}

// explicit instantiations used by bindings.cpp
template void rmsnorm_fwd_launch_t<__bf16>(const __bf16*, const __bf16*, __bf16*, float*, long, int, float, hipStream_t, const __bf16*, __bf16*);
template void rmsnorm_fwd_launch_t<float>(const float*, const float*, float*, float*, long, int, float, hipStream_t, const float*, float*);
template void rmsnorm_bwd_launch_t<__bf16>(const __bf16*, const __bf16*, const __bf16*, const float*, __bf16*, float*, float*, long, int, hipStream_t, const __bf16*);
template void rmsnorm_bwd_launch_t<float>(const float*, const float*, const float*, const float*, float*, float*, float*, long, int, hipStream_t, const float*);
template void layernorm_fwd_launch_t<__bf16>(const __bf16*, const __bf16*, const __bf16*, __bf16*, float*, float*, long, int, float, hipStream_t);
template void layernorm_fwd_launch_t<float>(const float*, const float*, const float*, float*, float*, float*, long, int, float, hipStream_t);
template void layernorm_bwd_launch_t<__bf16>(const __bf16*, const __bf16*, const __bf16*, const float*, const float*, __bf16*, float*, float*, long, int, hipStream_t);
template void layernorm_bwd_launch_t<float>(const float*, const float*, const float*, const float*, const float*, float*, float*, float*, long, int, hipStream_t);
