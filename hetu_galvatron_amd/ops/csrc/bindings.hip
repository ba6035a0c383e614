// Torch bindings for the gfx950 kernel suite (module: _galvatron_hip).
//
// HIP-native throughout (c10::hip stream API, no CUDA-compat shims).
// Python-side dispatch contract: hetu_galvatron_amd/ops/functional.py,
// runtime/tensor_parallel/cross_entropy.py, runtime/optimizer/optimizer.py.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>

#include <hip/hip_runtime.h>

#include <tuple>
#include <vector>

#include "flash_attn_launch.h"

// ---- launcher prototypes (defined in the sibling .hip TUs) ----------------
template <typename T>
void rmsnorm_fwd_launch_t(const T*, const T*, T*, float*, long, int, float, hipStream_t, const T* res = nullptr, T* sum_out = nullptr);
template <typename T>
void rmsnorm_bwd_launch_t(const T*, const T*, const T*, const float*, T*, float*, float*, long, int, hipStream_t, const T* dsum_in = nullptr);
template <typename T>
void layernorm_fwd_launch_t(const T*, const T*, const T*, T*, float*, float*, long, int, float, hipStream_t);
template <typename T>
void layernorm_bwd_launch_t(const T*, const T*, const T*, const float*, const float*, T*, float*, float*, long, int, hipStream_t);
int norm_bwd_grid(long n);
template <typename T>
void swiglu_fwd_launch_t(const T*, T*, long, int, hipStream_t);
template <typename T>
void swiglu_bwd_launch_t(const T*, const T*, T*, long, int, hipStream_t);
template <typename T>
void rope_launch_t(const T*, T*, const float*, const float*, long, int, int, bool, hipStream_t);
template <typename TG>
void grad_accum_launch_t(float*, const TG*, long, hipStream_t);
template <typename TG, typename TO>
void adamw_launch_t(float*, const TG*, float*, float*, TO*, long, int, float, float, float, float, float, float, hipStream_t);
template <typename T>
void ce_max_launch_t(const T*, float*, long, long, hipStream_t);
template <typename T>
void ce_sum_target_launch_t(const T*, const long*, const float*, float*, float*, long, long, long, hipStream_t);
template <typename T>
void ce_bwd_launch_t(T*, const long*, const float*, const float*, const float*, long, long, long, hipStream_t);

void grouped_gemm_launch(const __bf16*, const __bf16*, __bf16*, const void*, int, int, int, long, bool, hipStream_t);
void grouped_gemm_dw_launch(const __bf16*, const __bf16*, float*, const int*, int, int, int, hipStream_t);
#define DECL_MOE(T) \
  void moe_permute_launch_##T(const T*, T*, const long*, long, int, hipStream_t); \
  void moe_permute_bwd_launch_##T(const T*, float*, const long*, long, int, hipStream_t); \
  void moe_unpermute_launch_##T(const T*, const float*, const long*, T*, long, int, int, hipStream_t); \
  void moe_unpermute_bwd_launch_##T(const T*, const T*, const float*, const long*, T*, float*, long, int, hipStream_t);
typedef __bf16 bf16_t;
typedef float f32_t;
DECL_MOE(bf16_t)
DECL_MOE(f32_t)

void rope_qkv_launch(__bf16*, const float*, const float*, long, int, int, int, hipStream_t);
void qkv_grad_finish_launch(__bf16*, const __bf16*, const __bf16*, const float*, const float*, long, int, int, int, hipStream_t);
int multi_sumsq_grid(int);
void multi_sumsq_launch(const long*, int, float*, hipStream_t);
void decode_attn_launch(const __bf16*, const __bf16*, const __bf16*, __bf16*, float*, int, int, int, int, int, int, int, float, const int*, hipStream_t);

namespace {

using at::Tensor;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define CHECK_GPU(x) \
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), #x " must be contiguous on GPU")

const __bf16* bfp(const Tensor& t) {
  return reinterpret_cast<const __bf16*>(t.data_ptr<at::BFloat16>());
}
__bf16* bfp_mut(Tensor& t) {
  return reinterpret_cast<__bf16*>(t.data_ptr<at::BFloat16>());
}

bool is_bf16(const Tensor& t) { return t.scalar_type() == at::kBFloat16; }

// The kernels read bf16 or fp32 and nothing else: any other dtype (fp16,
// fp64, integers) is refused here by name, never reinterpreted.
#define CHECK_IN(t, who)                                                     \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous() &&                        \
                  ((t).scalar_type() == at::kBFloat16 ||                     \
                   (t).scalar_type() == at::kFloat),                         \
              who ": " #t " must be a contiguous bf16 or fp32 GPU tensor, "  \
              "got ", (t).scalar_type(), " on ", (t).device())
// t: same dtype, device and shape as x
#define CHECK_LIKE(t, x, who)                                                \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous() &&                        \
                  (t).scalar_type() == (x).scalar_type() &&                  \
                  (t).device() == (x).device() && (t).sizes() == (x).sizes(), \
              who ": " #t " must be contiguous with " #x "'s dtype, device " \
              "and shape ", (x).sizes(), ", got ", (t).scalar_type(), " ",   \
              (t).sizes())
// t: a per-column vector (norm weight / bias) with x's dtype and H elements
#define CHECK_VEC(t, x, H, who)                                              \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous() &&                        \
                  (t).scalar_type() == (x).scalar_type() &&                  \
                  (t).device() == (x).device() && (t).numel() == (H),        \
              who ": " #t " must be contiguous with " #x "'s dtype and "     \
              "device and ", (H), " elements, got ", (t).scalar_type(), " ", \
              (t).sizes())
// t: a per-row fp32 statistic saved by the forward (n elements)
#define CHECK_STAT(t, x, n, who)                                             \
  TORCH_CHECK((t).is_cuda() && (t).scalar_type() == at::kFloat &&            \
                  (t).device() == (x).device() && (t).numel() == (n),        \
              who ": " #t " must be fp32 on " #x "'s device with ", (n),     \
              " elements, got ", (t).scalar_type(), " ", (t).sizes())
#define CHECK_NORM_H(H, who)                                                 \
  TORCH_CHECK((H) > 0 && (H) % 8 == 0 && (H) <= 16384,                       \
              who ": H must be %8, <=16k")

// ---- norms ----------------------------------------------------------------
std::tuple<Tensor, Tensor> rmsnorm_fwd(const Tensor& x, const Tensor& w,
                                       double eps) {
  CHECK_IN(x, "rmsnorm_fwd");
  TORCH_CHECK(x.dim() >= 1, "rmsnorm_fwd: x must have a last dim");
  const int H = x.size(-1);
  CHECK_NORM_H(H, "rmsnorm");
  const long n = x.numel() / H;
  CHECK_VEC(w, x, H, "rmsnorm_fwd");
  auto y = at::empty_like(x);
  auto invrms = at::empty({n}, x.options().dtype(at::kFloat));
  if (n == 0) {
    auto sz = x.sizes().vec();
    sz.pop_back();
    return {y, invrms.view(sz)};
  }
  if (is_bf16(x))
    rmsnorm_fwd_launch_t<__bf16>(bfp(x), bfp(w), bfp_mut(y),
                                 invrms.data_ptr<float>(), n, H, (float)eps,
                                 cur_stream());
  else
    rmsnorm_fwd_launch_t<float>(x.data_ptr<float>(), w.data_ptr<float>(),
                                y.data_ptr<float>(), invrms.data_ptr<float>(),
                                n, H, (float)eps, cur_stream());
  auto sizes = x.sizes().vec();
  sizes.pop_back();
  return {y, invrms.view(sizes)};
}

std::tuple<Tensor, Tensor> rmsnorm_bwd(const Tensor& dy, const Tensor& x,
                                       const Tensor& w, const Tensor& invrms) {
  CHECK_IN(x, "rmsnorm_bwd");
  TORCH_CHECK(x.dim() >= 1, "rmsnorm_bwd: x must have a last dim");
  const int H = x.size(-1);
  CHECK_NORM_H(H, "rmsnorm");
  const long n = x.numel() / H;
  CHECK_LIKE(dy, x, "rmsnorm_bwd");
  CHECK_VEC(w, x, H, "rmsnorm_bwd");
  CHECK_STAT(invrms, x, n, "rmsnorm_bwd");
  auto dx = at::empty_like(x);
  auto dw = at::zeros({H}, x.options().dtype(at::kFloat));
  if (n == 0) return {dx, dw};
  const int G = norm_bwd_grid(n);
  auto dw_part = at::empty({G, H}, x.options().dtype(at::kFloat));
  auto inv = invrms.contiguous();
  if (is_bf16(x))
    rmsnorm_bwd_launch_t<__bf16>(bfp(dy), bfp(x), bfp(w),
                                 inv.data_ptr<float>(), bfp_mut(dx),
                                 dw_part.data_ptr<float>(),
                                 dw.data_ptr<float>(), n, H, cur_stream());
  else
    rmsnorm_bwd_launch_t<float>(dy.data_ptr<float>(), x.data_ptr<float>(),
                                w.data_ptr<float>(), inv.data_ptr<float>(),
                                dx.data_ptr<float>(), dw_part.data_ptr<float>(),
                                dw.data_ptr<float>(), n, H, cur_stream());
  return {dx, dw};
}

// fused residual-add + rmsnorm: y = rmsnorm(x + res) * w, also returns
// the sum (the downstream residual stream) and invrms
std::tuple<Tensor, Tensor, Tensor> add_rmsnorm_fwd(const Tensor& x,
                                                   const Tensor& res,
                                                   const Tensor& w,
                                                   double eps) {
  CHECK_IN(x, "add_rmsnorm_fwd");
  TORCH_CHECK(is_bf16(x), "add_rmsnorm_fwd: x must be bf16 (bf16 only), got ",
              x.scalar_type());
  TORCH_CHECK(x.dim() >= 1, "add_rmsnorm_fwd: x must have a last dim");
  const int H = x.size(-1);
  CHECK_NORM_H(H, "rmsnorm");
  const long n = x.numel() / H;
  CHECK_LIKE(res, x, "add_rmsnorm_fwd");
  CHECK_VEC(w, x, H, "add_rmsnorm_fwd");
  auto y = at::empty_like(x);
  auto sum = at::empty_like(x);
  auto invrms = at::empty({n}, x.options().dtype(at::kFloat));
  if (n == 0) {
    auto sz = x.sizes().vec();
    sz.pop_back();
    return {y, sum, invrms.view(sz)};
  }
  rmsnorm_fwd_launch_t<__bf16>(bfp(x), bfp(w), bfp_mut(y),
                               invrms.data_ptr<float>(), n, H, (float)eps,
                               cur_stream(), bfp(res), bfp_mut(sum));
  auto sizes = x.sizes().vec();
  sizes.pop_back();
  return {y, sum, invrms.view(sizes)};
}

// backward with the residual-stream grad folded in:
// dx = rmsnorm_bwd(dy wrt sum) + dsum  (dx == dres)
std::tuple<Tensor, Tensor> add_rmsnorm_bwd(const Tensor& dy,
                                           const Tensor& dsum,
                                           const Tensor& sum,
                                           const Tensor& w,
                                           const Tensor& invrms) {
  CHECK_IN(sum, "add_rmsnorm_bwd");
  TORCH_CHECK(is_bf16(sum), "add_rmsnorm_bwd: sum must be bf16 (bf16 only), "
              "got ", sum.scalar_type());
  TORCH_CHECK(sum.dim() >= 1, "add_rmsnorm_bwd: sum must have a last dim");
  const int H = sum.size(-1);
  CHECK_NORM_H(H, "rmsnorm");
  const long n = sum.numel() / H;
  CHECK_LIKE(dy, sum, "add_rmsnorm_bwd");
  CHECK_LIKE(dsum, sum, "add_rmsnorm_bwd");
  CHECK_VEC(w, sum, H, "add_rmsnorm_bwd");
  CHECK_STAT(invrms, sum, n, "add_rmsnorm_bwd");
  auto dx = at::empty_like(sum);
  auto dw = at::zeros({H}, sum.options().dtype(at::kFloat));
  if (n == 0) return {dx, dw};
  const int G = norm_bwd_grid(n);
  auto dw_part = at::empty({G, H}, sum.options().dtype(at::kFloat));
  auto inv = invrms.contiguous();
  rmsnorm_bwd_launch_t<__bf16>(bfp(dy), bfp(sum), bfp(w),
                               inv.data_ptr<float>(), bfp_mut(dx),
                               dw_part.data_ptr<float>(),
                               dw.data_ptr<float>(), n, H, cur_stream(),
                               bfp(dsum));
  return {dx, dw};
}

std::tuple<Tensor, Tensor, Tensor> layernorm_fwd(const Tensor& x,
                                                 const Tensor& w,
                                                 const Tensor& b, double eps) {
  CHECK_IN(x, "layernorm_fwd");
  TORCH_CHECK(x.dim() >= 1, "layernorm_fwd: x must have a last dim");
  const int H = x.size(-1);
  CHECK_NORM_H(H, "layernorm");
  const long n = x.numel() / H;
  CHECK_VEC(w, x, H, "layernorm_fwd");
  CHECK_VEC(b, x, H, "layernorm_fwd");
  auto y = at::empty_like(x);
  auto mean = at::empty({n}, x.options().dtype(at::kFloat));
  auto invstd = at::empty({n}, x.options().dtype(at::kFloat));
  if (n == 0) {
    auto sz = x.sizes().vec();
    sz.pop_back();
    return {y, mean.view(sz), invstd.view(sz)};
  }
  if (is_bf16(x))
    layernorm_fwd_launch_t<__bf16>(bfp(x), bfp(w), bfp(b), bfp_mut(y),
                                   mean.data_ptr<float>(),
                                   invstd.data_ptr<float>(), n, H, (float)eps,
                                   cur_stream());
  else
    layernorm_fwd_launch_t<float>(x.data_ptr<float>(), w.data_ptr<float>(),
                                  b.data_ptr<float>(), y.data_ptr<float>(),
                                  mean.data_ptr<float>(), invstd.data_ptr<float>(),
                                  n, H, (float)eps, cur_stream());
  auto sizes = x.sizes().vec();
  sizes.pop_back();
  return {y, mean.view(sizes), invstd.view(sizes)};
}

std::tuple<Tensor, Tensor, Tensor> layernorm_bwd(const Tensor& dy,
                                                 const Tensor& x,
                                                 const Tensor& w,
                                                 const Tensor& mean,
                                                 const Tensor& invstd) {
  CHECK_IN(x, "layernorm_bwd");
  TORCH_CHECK(x.dim() >= 1, "layernorm_bwd: x must have a last dim");
  const int H = x.size(-1);
  CHECK_NORM_H(H, "layernorm");
  const long n = x.numel() / H;
  CHECK_LIKE(dy, x, "layernorm_bwd");
  CHECK_VEC(w, x, H, "layernorm_bwd");
  CHECK_STAT(mean, x, n, "layernorm_bwd");
  CHECK_STAT(invstd, x, n, "layernorm_bwd");
  auto dx = at::empty_like(x);
  auto dwdb = at::zeros({2, H}, x.options().dtype(at::kFloat));
  if (n == 0) return {dx, dwdb[0], dwdb[1]};
  const int G = norm_bwd_grid(n);
  auto part = at::empty({2, G, H}, x.options().dtype(at::kFloat));
  auto m = mean.contiguous(), r = invstd.contiguous();
  if (is_bf16(x))
    layernorm_bwd_launch_t<__bf16>(bfp(dy), bfp(x), bfp(w),
                                   m.data_ptr<float>(), r.data_ptr<float>(),
                                   bfp_mut(dx), part.data_ptr<float>(),
                                   dwdb.data_ptr<float>(), n, H, cur_stream());
  else
    layernorm_bwd_launch_t<float>(dy.data_ptr<float>(), x.data_ptr<float>(),
                                  w.data_ptr<float>(), m.data_ptr<float>(),
                                  r.data_ptr<float>(), dx.data_ptr<float>(),
                                  part.data_ptr<float>(),
                                  dwdb.data_ptr<float>(), n, H, cur_stream());
  return {dx, dwdb[0], dwdb[1]};
}

// ---- swiglu / rope --------------------------------------------------------
Tensor swiglu_fwd(const Tensor& x) {
  CHECK_IN(x, "swiglu_fwd");
  TORCH_CHECK(x.dim() >= 1, "swiglu_fwd: x must have a last dim");
  const int F2 = x.size(-1);
  TORCH_CHECK(F2 > 0 && F2 % 16 == 0, "swiglu: last dim must be %16");
  const int F = F2 / 2;
  const long rows = x.numel() / F2;
  auto sizes = x.sizes().vec();
  sizes.back() = F;
  auto y = at::empty(sizes, x.options());
  if (rows == 0) return y;
  if (is_bf16(x))
    swiglu_fwd_launch_t<__bf16>(bfp(x), bfp_mut(y), rows, F, cur_stream());
  else
    swiglu_fwd_launch_t<float>(x.data_ptr<float>(), y.data_ptr<float>(),
                               rows, F, cur_stream());
  return y;
}

Tensor swiglu_bwd(const Tensor& dy, const Tensor& x) {
  CHECK_IN(x, "swiglu_bwd");
  TORCH_CHECK(x.dim() >= 1, "swiglu_bwd: x must have a last dim");
  const int F2 = x.size(-1);
  TORCH_CHECK(F2 > 0 && F2 % 16 == 0, "swiglu: last dim must be %16");
  const int F = F2 / 2;
  const long rows = x.numel() / F2;
  auto want = x.sizes().vec();
  want.back() = F;
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() &&
                  dy.scalar_type() == x.scalar_type() &&
                  dy.device() == x.device() && dy.sizes() == at::IntArrayRef(want),
              "swiglu_bwd: dy must be contiguous with x's dtype and device "
              "and shape ", at::IntArrayRef(want), " (x's with the last dim "
              "halved), got ", dy.scalar_type(), " ", dy.sizes());
  auto dx = at::empty_like(x);
  if (rows == 0) return dx;
  if (is_bf16(x))
    swiglu_bwd_launch_t<__bf16>(bfp(dy), bfp(x), bfp_mut(dx), rows, F,
                                cur_stream());
  else
    swiglu_bwd_launch_t<float>(dy.data_ptr<float>(), x.data_ptr<float>(),
                               dx.data_ptr<float>(), rows, F, cur_stream());
  return dx;
}

Tensor rope_fwd(const Tensor& x, const Tensor& cos_t, const Tensor& sin_t,
                bool conj) {
  CHECK_IN(x, "rope_fwd");
  TORCH_CHECK(x.dim() == 4, "rope: x must be [s,b,h,d]");
  const int d = x.size(3);
  TORCH_CHECK(d > 0 && d % 16 == 0, "rope: head dim must be %16");
  const long rows = x.numel() / d;
  const int bh = x.size(1) * x.size(2);
  // the kernel reads table row s_idx for every s_idx < s and d/2 columns
  // of it: a shorter or narrower table would be read out of bounds
  TORCH_CHECK(cos_t.is_cuda() && cos_t.device() == x.device() &&
                  cos_t.is_floating_point() && cos_t.dim() == 2 &&
                  cos_t.size(0) >= x.size(0) && cos_t.size(1) * 2 == d,
              "rope_fwd: cos_t must be a floating [>=s, d/2] = [>=",
              x.size(0), ", ", d / 2, "] table on x's device, got ",
              cos_t.scalar_type(), " ", cos_t.sizes(), " on ",
              cos_t.device());
  TORCH_CHECK(sin_t.is_cuda() && sin_t.device() == x.device() &&
                  sin_t.is_floating_point() &&
                  sin_t.sizes() == cos_t.sizes(),
              "rope_fwd: sin_t must be a floating table on x's device "
              "shaped like cos_t ", cos_t.sizes(), ", got ",
              sin_t.scalar_type(), " ", sin_t.sizes(), " on ",
              sin_t.device());
  auto c = cos_t.contiguous().to(at::kFloat);
  auto s = sin_t.contiguous().to(at::kFloat);
  auto y = at::empty_like(x);
  if (rows == 0) return y;
  if (is_bf16(x))
    rope_launch_t<__bf16>(bfp(x), bfp_mut(y), c.data_ptr<float>(),
                          s.data_ptr<float>(), rows, bh, d, conj,
                          cur_stream());
  else
    rope_launch_t<float>(x.data_ptr<float>(), y.data_ptr<float>(),
                         c.data_ptr<float>(), s.data_ptr<float>(),
                         rows, bh, d, conj, cur_stream());
  return y;
}

// ---- flash attention ------------------------------------------------------
// What the eight flash bindings share.  FlashDims is the geometry of a
// call, read from q/k/v or from a packed linear_qkv buffer.
struct FlashDims {
  int b, sq, skv, hq, hkv, d;
};

// q [b,sq,hq,d], k/v [b,skv,hkv,d] ([s,b,h,d] with sbhd), all checked.
FlashDims flash_dims(const Tensor& q, const Tensor& k, const Tensor& v,
                     bool sbhd, const char* who) {
  CHECK_GPU(q); CHECK_GPU(k); CHECK_GPU(v);
  TORCH_CHECK(is_bf16(q), who, ": q: bf16 only on the native path");
  TORCH_CHECK(q.dim() == 4, who,
              ": q must be [b,s,h,d] (or [s,b,h,d] with sbhd)");
  const int bdim = sbhd ? 1 : 0;
  TORCH_CHECK(is_bf16(k) && k.dim() == 4 && k.size(bdim) == q.size(bdim) &&
              k.size(3) == q.size(3), who,
              ": k must be bf16, 4-D, with q's batch and head dim, got ",
              k.scalar_type(), " ", k.sizes());
  TORCH_CHECK(is_bf16(v) && v.sizes() == k.sizes(), who,
              ": v must be bf16 and shaped like k, got ", v.scalar_type(),
              " ", v.sizes());
  FlashDims g;
  g.b = q.size(bdim); g.sq = q.size(1 - bdim);
  g.hq = q.size(2); g.d = q.size(3);
  g.skv = k.size(1 - bdim); g.hkv = k.size(2);
  TORCH_CHECK(g.d == 64 || g.d == 128, who, ": head dim must be 64|128");
  TORCH_CHECK(g.hkv > 0 && g.hq % g.hkv == 0, who,
              ": GQA needs hq % hkv == 0");
  return g;
}

// Packed-document attention: cu_seqlens [nseg+1] int32 token offsets into
// the batch-major flattened [b*s] stream.  The values are NOT read on the
// host (no sync): the caller validates its host copy (they must tile
// [0, b*s) without straddling a row, with every length <= max_seqlen), so
// every output row is written exactly once and at::empty is correct.
// x: the tensor whose device the table must share.
void check_cu(const Tensor& cu, int64_t max_seqlen, const Tensor& x,
              const FlashDims& g, const char* who) {
  TORCH_CHECK(cu.is_cuda() && cu.is_contiguous() &&
              cu.scalar_type() == at::kInt && cu.dim() == 1 &&
              cu.numel() >= 2 && cu.device() == x.device(), who,
              ": cu_seqlens must be a contiguous 1-D int32 tensor on the "
              "inputs' device with at least 2 entries");
  TORCH_CHECK(max_seqlen >= 1 && max_seqlen <= g.sq, who,
              ": need 1 <= max_seqlen <= s");
  TORCH_CHECK((int64_t)g.b * g.sq < (1LL << 31), who,
              ": b*s must fit int32");
  TORCH_CHECK((cu.numel() - 1) * (int64_t)g.hq <= 65535, who,
              ": nseg*hq exceeds the grid limit (65535)");
}

// Backward inputs: dout and o bf16 shaped like the forward's output, lse
// fp32 [b, hq, sq] on the GPU.  -> lse, contiguous.
Tensor check_bwd(const Tensor& dout, const Tensor& o, const Tensor& lse,
                 at::IntArrayRef out_sizes, const FlashDims& g,
                 const char* who) {
  CHECK_GPU(dout); CHECK_GPU(o);
  TORCH_CHECK(is_bf16(dout) && dout.sizes() == out_sizes, who,
              ": dout/o must be bf16 ", out_sizes, ": dout is ",
              dout.scalar_type(), " ", dout.sizes());
  TORCH_CHECK(is_bf16(o) && o.sizes() == out_sizes, who,
              ": dout/o must be bf16 ", out_sizes, ": o is ", o.scalar_type(),
              " ", o.sizes());
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
              lse.dim() == 3 && lse.size(0) == g.b && lse.size(1) == g.hq &&
              lse.size(2) == g.sq, who,
              ": lse must be fp32 [b, hq, s] on the GPU, got ",
              lse.scalar_type(), " ", lse.sizes(), " on ", lse.device());
  return lse.contiguous();
}

// di = rowsum(dout * o), [b, hq, sq] fp32
Tensor flash_di(const Tensor& dout, const Tensor& o, const FlashDims& g,
                bool sbhd) {
  auto di = at::empty({g.b, g.hq, g.sq}, o.options().dtype(at::kFloat));
  attn_di_launch(bfp(dout), bfp(o), di.data_ptr<float>(), g.b, g.sq, g.hq,
                 g.d, cur_stream(), sbhd);
  return di;
}

// dk_exp / dv_exp carry hq heads: sum each GQA group down to its kv head
Tensor gqa_sum(const Tensor& exp, const FlashDims& g) {
  if (g.hq == g.hkv) return exp;
  return exp.view({exp.size(0), exp.size(1), g.hkv, g.hq / g.hkv, g.d})
      .sum(3);
}

std::tuple<Tensor, Tensor> flash_attn_fwd(
    const Tensor& q, const Tensor& k, const Tensor& v, bool causal,
    double scale, const c10::optional<Tensor>& bias = c10::nullopt,
    bool sbhd = false, int64_t window = 0) {
  TORCH_CHECK(window == 0 || causal,
              "flash_attn: sliding window requires causal");
  const FlashDims g = flash_dims(q, k, v, sbhd, "flash_attn");
  const __bf16* bp = nullptr;
  Tensor bias_c;
  if (bias.has_value()) {
    bias_c = bias->contiguous();
    TORCH_CHECK(is_bf16(bias_c) && bias_c.dim() == 3 &&
                bias_c.size(0) == g.hq && bias_c.size(1) == g.sq &&
                bias_c.size(2) == g.skv,
                "flash_attn: bias must be bf16 [hq, sq, skv]");
    bp = bfp(bias_c);
  }
  auto o = at::empty_like(q);
  auto lse = at::empty({g.b, g.hq, g.sq}, q.options().dtype(at::kFloat));
  flash_fwd_launch(bfp(q), bfp(k), bfp(v), bfp_mut(o),
                   lse.data_ptr<float>(), g.b, g.sq, g.skv, g.hq, g.hkv, g.d,
                   (float)scale, causal, cur_stream(), bp, sbhd,
                   (int)window);
  return {o, lse};
}

std::vector<Tensor> flash_attn_bwd(
    const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v,
    const Tensor& o, const Tensor& lse, bool causal, double scale,
    const c10::optional<Tensor>& bias = c10::nullopt, bool sbhd = false,
    int64_t window = 0) {
  TORCH_CHECK(window == 0 || causal,
              "flash_attn_bwd: sliding window requires causal");
  const FlashDims g = flash_dims(q, k, v, sbhd, "flash_attn_bwd");
  auto lsec = check_bwd(dout, o, lse, q.sizes(), g, "flash_attn_bwd");
  auto di = flash_di(dout, o, g, sbhd);
  auto dq = at::empty_like(q);
  auto dk_exp = sbhd ? at::empty({g.skv, g.b, g.hq, g.d}, k.options())
                     : at::empty({g.b, g.skv, g.hq, g.d}, k.options());
  auto dv_exp = at::empty_like(dk_exp);
  const __bf16* bp = nullptr;
  float* dbp = nullptr;
  Tensor bias_c, dbias;
  if (bias.has_value()) {
    bias_c = bias->contiguous();
    TORCH_CHECK(is_bf16(bias_c) && bias_c.dim() == 3 &&
                bias_c.size(0) == g.hq && bias_c.size(1) == g.sq &&
                bias_c.size(2) == g.skv,
                "flash_attn_bwd: bias must be bf16 [hq, sq, skv]");
    bp = bfp(bias_c);
    dbias = at::zeros({g.hq, g.sq, g.skv}, q.options().dtype(at::kFloat));
    dbp = dbias.data_ptr<float>();
  }
  flash_bwd_launch(bfp(dout), bfp(q), bfp(k), bfp(v),
                   lsec.data_ptr<float>(), di.data_ptr<float>(),
                   bfp_mut(dq), bfp_mut(dk_exp), bfp_mut(dv_exp), g.b, g.sq,
                   g.skv, g.hq, g.hkv, g.d, (float)scale, causal,
                   cur_stream(), bp, dbp, sbhd, (int)window);
  if (bias.has_value())
    return {dq, gqa_sum(dk_exp, g), gqa_sum(dv_exp, g), dbias};
  return {dq, gqa_sum(dk_exp, g), gqa_sum(dv_exp, g)};
}

// self-attention only: k/v share q's b and s
FlashDims varlen_dims(const Tensor& q, const Tensor& k, const Tensor& v,
                      const Tensor& cu, int64_t max_seqlen, bool sbhd,
                      const char* who) {
  const FlashDims g = flash_dims(q, k, v, sbhd, who);
  TORCH_CHECK(g.skv == g.sq, who,
              ": self-attention only (k/v must match q's b, s and d)");
  check_cu(cu, max_seqlen, q, g, who);
  return g;
}

std::tuple<Tensor, Tensor> flash_attn_varlen_fwd(
    const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu,
    int64_t max_seqlen, bool causal, double scale, bool sbhd = false) {
  const FlashDims g =
      varlen_dims(q, k, v, cu, max_seqlen, sbhd, "flash_attn_varlen_fwd");
  auto o = at::empty_like(q);
  auto lse = at::empty({g.b, g.hq, g.sq}, q.options().dtype(at::kFloat));
  flash_varlen_fwd_launch(bfp(q), bfp(k), bfp(v), bfp_mut(o),
                          lse.data_ptr<float>(), cu.data_ptr<int>(),
                          (int)cu.numel() - 1, (int)max_seqlen, g.b, g.sq,
                          g.hq, g.hkv, g.d, (float)scale, causal, sbhd,
                          cur_stream());
  return {o, lse};
}

std::vector<Tensor> flash_attn_varlen_bwd(
    const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v,
    const Tensor& o, const Tensor& lse, const Tensor& cu,
    int64_t max_seqlen, bool causal, double scale, bool sbhd = false) {
  const FlashDims g =
      varlen_dims(q, k, v, cu, max_seqlen, sbhd, "flash_attn_varlen_bwd");
  auto lsec = check_bwd(dout, o, lse, q.sizes(), g, "flash_attn_varlen_bwd");
  auto di = flash_di(dout, o, g, sbhd);
  auto dq = at::empty_like(q);
  auto dk_exp = at::empty_like(q, k.options());
  auto dv_exp = at::empty_like(dk_exp);
  flash_varlen_bwd_launch(bfp(dout), bfp(q), bfp(k), bfp(v),
                          lsec.data_ptr<float>(), di.data_ptr<float>(),
                          bfp_mut(dq), bfp_mut(dk_exp), bfp_mut(dv_exp),
                          cu.data_ptr<int>(), (int)cu.numel() - 1,
                          (int)max_seqlen, g.b, g.sq, g.hq, g.hkv, g.d,
                          (float)scale, causal, sbhd, cur_stream());
  return {dq, gqa_sum(dk_exp, g), gqa_sum(dv_exp, g)};
}

// ---- packed-QKV attention ---------------------------------------------------
// qkv is the linear_qkv output viewed [s, b, G, qpg+2, d] (G local kv
// groups; q heads in slots 0..qpg-1 of a group, k in slot qpg, v in slot
// qpg+1).  The kernels read q, k and v from it in place.
void check_qkv(const Tensor& qkv, const char* who) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && is_bf16(qkv) &&
              qkv.dim() == 5 && qkv.size(3) >= 3, who,
              ": qkv must be a contiguous bf16 GPU tensor [s,b,G,qpg+2,d]");
  const int64_t d = qkv.size(4);
  TORCH_CHECK(d == 64 || d == 128, who, ": head dim must be 64|128");
  TORCH_CHECK(qkv.size(0) >= 1 && qkv.size(1) >= 1 && qkv.size(2) >= 1, who,
              ": empty qkv");
  TORCH_CHECK(qkv.size(1) * qkv.size(2) * qkv.size(3) * d < (1LL << 31),
              who, ": row stride must fit int32");
  TORCH_CHECK(qkv.size(1) * qkv.size(2) * (qkv.size(3) - 2) <= 65535, who,
              ": b*hq exceeds the grid limit (65535)");
}

// cos/sin: [s, d/2], or per-row [s, b, d/2] (packed documents whose
// positions restart; rank 3 selects it, so b == 1 is not ambiguous).
// Returns the number of consecutive kv groups that share one table row:
// b*G for [s, d/2], G for [s, b, d/2].
int check_rope_tables(const Tensor& qkv, const Tensor& cos_t,
                      const Tensor& sin_t, const char* who) {
  const bool per_row = cos_t.dim() == 3;
  TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda() &&
              cos_t.scalar_type() == at::kFloat &&
              sin_t.scalar_type() == at::kFloat && cos_t.is_contiguous() &&
              sin_t.is_contiguous() && (cos_t.dim() == 2 || per_row) &&
              cos_t.sizes() == sin_t.sizes() &&
              cos_t.size(0) == qkv.size(0) &&
              (!per_row || cos_t.size(1) == qkv.size(1)) &&
              cos_t.size(-1) * 2 == qkv.size(4), who,
              ": cos/sin must be contiguous fp32 [s, d/2] or [s, b, d/2] "
              "on the GPU");
  return (int)(per_row ? qkv.size(2) : qkv.size(1) * qkv.size(2));
}

// In-place NEOX RoPE on the q and k slots; v is not touched.
void rope_qkv_(Tensor qkv, const Tensor& cos_t, const Tensor& sin_t) {
  check_qkv(qkv, "rope_qkv_");
  const int per_table_row =
      check_rope_tables(qkv, cos_t, sin_t, "rope_qkv_");
  const long groups = qkv.size(0) * qkv.size(1) * qkv.size(2);
  rope_qkv_launch(bfp_mut(qkv), cos_t.data_ptr<float>(),
                  sin_t.data_ptr<float>(), groups, per_table_row,
                  (int)qkv.size(3) - 2, (int)qkv.size(4), cur_stream());
}

// check_qkv, and with a cu_seqlens table check_cu (see there: the segments
// tile [0, b*s), so every q-slot row of dqkv and every o / lse row is
// written exactly once and at::empty is correct).  hkv = G.
FlashDims qkv_dims(const Tensor& qkv, const Tensor* cu, int64_t max_seqlen,
                   const char* who) {
  check_qkv(qkv, who);
  const int s = qkv.size(0), G = qkv.size(2);
  const FlashDims g{(int)qkv.size(1), s, s, G * ((int)qkv.size(3) - 2), G,
                    (int)qkv.size(4)};
  if (cu != nullptr) check_cu(*cu, max_seqlen, qkv, g, who);
  return g;
}

// -> o [s, b, hq, d], lse [b, hq, s]; cu: the packed-document kernels
std::tuple<Tensor, Tensor> qkv_fwd(const Tensor& qkv, const Tensor* cu,
                                   int64_t max_seqlen, bool causal,
                                   double scale, const char* who) {
  const FlashDims g = qkv_dims(qkv, cu, max_seqlen, who);
  const int qpg = g.hq / g.hkv;
  auto o = at::empty({g.sq, g.b, g.hq, g.d}, qkv.options());
  auto lse = at::empty({g.b, g.hq, g.sq}, qkv.options().dtype(at::kFloat));
  if (cu == nullptr)
    flash_packed_fwd_launch(bfp(qkv), bfp_mut(o), lse.data_ptr<float>(), g.b,
                            g.sq, g.hkv, qpg, g.d, (float)scale, causal,
                            cur_stream());
  else
    flash_packed_varlen_fwd_launch(
        bfp(qkv), bfp_mut(o), lse.data_ptr<float>(), cu->data_ptr<int>(),
        (int)cu->numel() - 1, (int)max_seqlen, g.b, g.sq, g.hkv, qpg, g.d,
        (float)scale, causal, cur_stream());
  return {o, lse};
}

// -> dqkv (q slots = dq before the inverse rotation, k and v slots NOT yet
// written), dk_exp, dv_exp [s, b, hq, d].  qkv_grad_finish_ completes dqkv.
std::vector<Tensor> qkv_bwd(const Tensor& dout, const Tensor& qkv,
                            const Tensor& o, const Tensor& lse,
                            const Tensor* cu, int64_t max_seqlen, bool causal,
                            double scale, const char* who) {
  const FlashDims g = qkv_dims(qkv, cu, max_seqlen, who);
  const int qpg = g.hq / g.hkv;
  auto lsec = check_bwd(dout, o, lse, {g.sq, g.b, g.hq, g.d}, g, who);
  auto di = flash_di(dout, o, g, /*sbhd=*/true);
  // at::empty: the dq kernel writes every q-slot element and
  // qkv_grad_finish_ writes every k- and v-slot element, each exactly once
  auto dqkv = at::empty_like(qkv);
  auto dk_exp = at::empty({g.sq, g.b, g.hq, g.d}, qkv.options());
  auto dv_exp = at::empty_like(dk_exp);
  if (cu == nullptr)
    flash_packed_bwd_launch(bfp(dout), bfp(qkv), lsec.data_ptr<float>(),
                            di.data_ptr<float>(), bfp_mut(dqkv),
                            bfp_mut(dk_exp), bfp_mut(dv_exp), g.b, g.sq,
                            g.hkv, qpg, g.d, (float)scale, causal,
                            cur_stream());
  else
    flash_packed_varlen_bwd_launch(
        bfp(dout), bfp(qkv), lsec.data_ptr<float>(), di.data_ptr<float>(),
        bfp_mut(dqkv), bfp_mut(dk_exp), bfp_mut(dv_exp), cu->data_ptr<int>(),
        (int)cu->numel() - 1, (int)max_seqlen, g.b, g.sq, g.hkv, qpg, g.d,
        (float)scale, causal, cur_stream());
  return {dqkv, dk_exp, dv_exp};
}

std::tuple<Tensor, Tensor> flash_attn_qkv_fwd(const Tensor& qkv, bool causal,
                                              double scale) {
  return qkv_fwd(qkv, nullptr, 0, causal, scale, "flash_attn_qkv_fwd");
}

std::vector<Tensor> flash_attn_qkv_bwd(const Tensor& dout, const Tensor& qkv,
                                       const Tensor& o, const Tensor& lse,
                                       bool causal, double scale) {
  return qkv_bwd(dout, qkv, o, lse, nullptr, 0, causal, scale,
                 "flash_attn_qkv_bwd");
}

std::tuple<Tensor, Tensor> flash_attn_qkv_varlen_fwd(
    const Tensor& qkv, const Tensor& cu, int64_t max_seqlen, bool causal,
    double scale) {
  return qkv_fwd(qkv, &cu, max_seqlen, causal, scale,
                 "flash_attn_qkv_varlen_fwd");
}

std::vector<Tensor> flash_attn_qkv_varlen_bwd(
    const Tensor& dout, const Tensor& qkv, const Tensor& o, const Tensor& lse,
    const Tensor& cu, int64_t max_seqlen, bool causal, double scale) {
  return qkv_bwd(dout, qkv, o, lse, &cu, max_seqlen, causal, scale,
                 "flash_attn_qkv_varlen_bwd");
}

// One pass that turns dqkv into the gradient of the linear_qkv output:
// inverse rotation of the q slots, GQA group sum of dk_exp / dv_exp into the
// k / v slots (k rotated back too).  No cos/sin: no rotary embedding.
void qkv_grad_finish_(Tensor dqkv, const Tensor& dk_exp, const Tensor& dv_exp,
                      const c10::optional<Tensor>& cos_t,
                      const c10::optional<Tensor>& sin_t) {
  check_qkv(dqkv, "qkv_grad_finish_");
  CHECK_GPU(dk_exp); CHECK_GPU(dv_exp);
  const int64_t hq = dqkv.size(2) * (dqkv.size(3) - 2);
  TORCH_CHECK(is_bf16(dk_exp) && dk_exp.dim() == 4 &&
              dk_exp.size(0) == dqkv.size(0) &&
              dk_exp.size(1) == dqkv.size(1) && dk_exp.size(2) == hq &&
              dk_exp.size(3) == dqkv.size(4) && is_bf16(dv_exp) &&
              dv_exp.sizes() == dk_exp.sizes(),
              "qkv_grad_finish_: dk_exp/dv_exp must be bf16 [s, b, hq, d]");
  TORCH_CHECK(cos_t.has_value() == sin_t.has_value(),
              "qkv_grad_finish_: cos and sin go together");
  const float* cp = nullptr;
  const float* sp = nullptr;
  int per_table_row = (int)(dqkv.size(1) * dqkv.size(2));
  if (cos_t.has_value()) {
    per_table_row =
        check_rope_tables(dqkv, *cos_t, *sin_t, "qkv_grad_finish_");
    cp = cos_t->data_ptr<float>();
    sp = sin_t->data_ptr<float>();
  }
  const long groups = dqkv.size(0) * dqkv.size(1) * dqkv.size(2);
  qkv_grad_finish_launch(bfp_mut(dqkv), bfp(dk_exp), bfp(dv_exp), cp, sp,
                         groups, per_table_row, (int)dqkv.size(3) - 2,
                         (int)dqkv.size(4), cur_stream());
}

// Single-token decode attention against a KV cache (serving path).
// q: [b,hq,d]; k_cache/v_cache: [b,max_s,hkv,d]; attends to [0, cur_len).
Tensor decode_attn(const Tensor& q, const Tensor& k_cache,
                   const Tensor& v_cache, int64_t cur_len, double scale,
                   int64_t start = 0) {
  CHECK_GPU(q); CHECK_GPU(k_cache); CHECK_GPU(v_cache);
  TORCH_CHECK(is_bf16(q), "decode_attn: bf16 only");
  TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4, "decode_attn shapes");
  const int b = q.size(0), hq = q.size(1), d = q.size(2);
  const int max_s = k_cache.size(1), hkv = k_cache.size(2);
  TORCH_CHECK(d == 64 || d == 128, "decode_attn: head dim must be 64|128");
  TORCH_CHECK(cur_len >= 1 && cur_len <= max_s, "decode_attn: bad cur_len");
  TORCH_CHECK(start >= 0 && start < cur_len, "decode_attn: bad start");
  // windowed decode (mistral): positions [start, cur_len).  The kernels
  // are unchanged — advancing the cache pointers by start rows shifts
  // every (b, h) address uniformly within its batch row.
  const __bf16* kp = bfp(k_cache) + (long)start * hkv * d;
  const __bf16* vp = bfp(v_cache) + (long)start * hkv * d;
  cur_len -= start;
  auto o = at::empty_like(q);
  // split-KV: fill >=512 workgroups (2/CU) when b*hq alone can't, but keep
  // chunks >=128 positions so the merge stays cheap
  int n_chunks = b * hq >= 256 ? 1 : std::max(1, 512 / (b * hq));
  n_chunks = std::min<int>(n_chunks, (int)((cur_len + 127) / 128));
  // LDS cap: the weight buffer is cur_len/chunk fp32 — keep chunks <= 8192
  n_chunks = std::max<int>(n_chunks, (int)((cur_len + 8191) / 8192));
  Tensor ws;
  float* ws_ptr = nullptr;
  if (n_chunks > 1) {
    ws = at::empty({(long)b * hq * n_chunks * (d + 2)},
                   q.options().dtype(at::kFloat));
    ws_ptr = ws.data_ptr<float>();
  }
  decode_attn_launch(bfp(q), kp, vp, bfp_mut(o), ws_ptr,
                     n_chunks, b, hq, hkv, max_s, (int)cur_len, d,
                     (float)scale, nullptr, cur_stream());
  return o;
}

// hipGraph-capturable variant: the attended length lives in device memory
// (cur_len_dev int32 [1]); launch geometry + LDS are sized for max_len so
// a captured graph replays correctly as the cache grows.
Tensor decode_attn_graph(const Tensor& q, const Tensor& k_cache,
                         const Tensor& v_cache, const Tensor& cur_len_dev,
                         int64_t max_len, double scale) {
  CHECK_GPU(q); CHECK_GPU(cur_len_dev);
  TORCH_CHECK(is_bf16(q) && q.dim() == 3, "decode_attn_graph: bf16 [b,hq,d]");
  TORCH_CHECK(cur_len_dev.scalar_type() == at::kInt, "cur_len_dev: int32");
  const int b = q.size(0), hq = q.size(1), d = q.size(2);
  const int max_s = k_cache.size(1), hkv = k_cache.size(2);
  TORCH_CHECK(d == 64 || d == 128, "decode_attn_graph: head dim 64|128");
  TORCH_CHECK(max_len >= 1 && max_len <= max_s, "bad max_len");
  auto o = at::empty_like(q);
  int n_chunks = b * hq >= 256 ? 1 : std::max(1, 512 / (b * hq));
  n_chunks = std::min<int>(n_chunks, (int)((max_len + 127) / 128));
  n_chunks = std::max<int>(n_chunks, (int)((max_len + 8191) / 8192));
  auto ws = at::empty({(long)b * hq * n_chunks * (d + 2)},
                      q.options().dtype(at::kFloat));
  decode_attn_launch(bfp(q), bfp(k_cache), bfp(v_cache), bfp_mut(o),
                     ws.data_ptr<float>(), n_chunks, b, hq, hkv, max_s,
                     (int)max_len, d, (float)scale,
                     cur_len_dev.data_ptr<int>(), cur_stream());
  return o;
}

Tensor mfma_probe(const Tensor& A, const Tensor& B, bool alt) {
  CHECK_GPU(A); CHECK_GPU(B);
  auto D = at::zeros({32, 32}, A.options().dtype(at::kFloat));
  mfma_probe_launch(bfp(A), bfp(B), D.data_ptr<float>(), alt, cur_stream());
  return D;
}

// ---- vocab-parallel CE ----------------------------------------------------
// logits [n, V] bf16|fp32 with V >= 1; target int64 [n]; per-row stats fp32 [n]
#define CHECK_CE_LOGITS(logits, who)                                        \
  CHECK_IN(logits, who);                                                    \
  TORCH_CHECK((logits).dim() >= 1 && (logits).size(-1) >= 1,                \
              who ": logits must be [n, V] with V >= 1, got ",              \
              (logits).sizes())
#define CHECK_CE_TARGET(target, logits, n, who)                             \
  TORCH_CHECK((target).is_cuda() && (target).scalar_type() == at::kLong &&  \
                  (target).device() == (logits).device() &&                 \
                  (target).numel() == (n),                                  \
              who ": target must be int64 on logits' device with ", (n),    \
              " elements, got ", (target).scalar_type(), " ",               \
              (target).sizes())

Tensor ce_max(const Tensor& logits) {
  CHECK_CE_LOGITS(logits, "ce_max");
  const long V = logits.size(-1);
  const long n = logits.numel() / V;
  auto out = at::empty({n}, logits.options().dtype(at::kFloat));
  if (n == 0) return out;
  if (is_bf16(logits))
    ce_max_launch_t<__bf16>(bfp(logits), out.data_ptr<float>(), n, V,
                            cur_stream());
  else
    ce_max_launch_t<float>(logits.data_ptr<float>(),
                           out.data_ptr<float>(), n, V, cur_stream());
  return out;
}

std::tuple<Tensor, Tensor> ce_sum_target(const Tensor& logits,
                                         const Tensor& target,
                                         const Tensor& gmax,
                                         long vocab_start) {
  CHECK_CE_LOGITS(logits, "ce_sum_target");
  const long V = logits.size(-1);
  const long n = logits.numel() / V;
  CHECK_CE_TARGET(target, logits, n, "ce_sum_target");
  CHECK_STAT(gmax, logits, n, "ce_sum_target");
  auto t = target.contiguous();
  auto g = gmax.contiguous();
  auto sumexp = at::empty({n}, logits.options().dtype(at::kFloat));
  auto tlogit = at::empty({n}, logits.options().dtype(at::kFloat));
  if (n == 0) return {sumexp, tlogit};
  if (is_bf16(logits))
    ce_sum_target_launch_t<__bf16>(bfp(logits), t.data_ptr<long>(),
                                   g.data_ptr<float>(),
                                   sumexp.data_ptr<float>(),
                                   tlogit.data_ptr<float>(), n, V,
                                   vocab_start, cur_stream());
  else
    ce_sum_target_launch_t<float>(logits.data_ptr<float>(),
                                  t.data_ptr<long>(), g.data_ptr<float>(),
                                  sumexp.data_ptr<float>(),
                                  tlogit.data_ptr<float>(), n, V, vocab_start,
                                  cur_stream());
  return {sumexp, tlogit};
}

Tensor ce_bwd(Tensor logits, const Tensor& target, const Tensor& gmax,
              const Tensor& sumexp, const Tensor& grad_out, long vocab_start) {
  CHECK_CE_LOGITS(logits, "ce_bwd");
  const long V = logits.size(-1);
  const long n = logits.numel() / V;
  CHECK_CE_TARGET(target, logits, n, "ce_bwd");
  CHECK_STAT(gmax, logits, n, "ce_bwd");
  CHECK_STAT(sumexp, logits, n, "ce_bwd");
  TORCH_CHECK(grad_out.is_cuda() && grad_out.device() == logits.device() &&
                  grad_out.is_floating_point() && grad_out.numel() == n,
              "ce_bwd: grad_out must be a floating tensor on logits' device "
              "with ", n, " elements, got ", grad_out.scalar_type(), " ",
              grad_out.sizes());
  if (n == 0) return logits;
  auto t = target.contiguous();
  auto g = gmax.contiguous();
  auto se = sumexp.contiguous();
  auto go = grad_out.contiguous().to(at::kFloat);
  if (is_bf16(logits))
    ce_bwd_launch_t<__bf16>(bfp_mut(logits), t.data_ptr<long>(),
                            g.data_ptr<float>(), se.data_ptr<float>(),
                            go.data_ptr<float>(), n, V, vocab_start,
                            cur_stream());
  else
    ce_bwd_launch_t<float>(logits.data_ptr<float>(), t.data_ptr<long>(),
                           g.data_ptr<float>(), se.data_ptr<float>(),
                           go.data_ptr<float>(), n, V, vocab_start,
                           cur_stream());
  return logits;
}

// ---- grad accumulation ----------------------------------------------------
void grad_accum(Tensor flat, const Tensor& grad, long offset) {
  CHECK_GPU(flat); CHECK_GPU(grad);
  TORCH_CHECK(flat.scalar_type() == at::kFloat, "grad_accum: flat must be fp32");
  const long n = grad.numel();
  TORCH_CHECK(offset + n <= flat.numel(), "grad_accum: out of range");
  float* fp = flat.data_ptr<float>() + offset;
  if (is_bf16(grad))
    grad_accum_launch_t<__bf16>(fp, bfp(grad), n, cur_stream());
  else
    grad_accum_launch_t<float>(fp, grad.data_ptr<float>(), n, cur_stream());
}

// ---- MoE permute / unpermute ----------------------------------------------
Tensor moe_permute(const Tensor& x, const Tensor& rows) {
  CHECK_GPU(x); CHECK_GPU(rows);
  const long m = rows.numel();
  const int h = x.size(-1);
  TORCH_CHECK(h % 8 == 0, "moe_permute: h % 8");
  auto y = at::empty({m, (long)h}, x.options());
  if (m == 0) return y;
  if (is_bf16(x))
    moe_permute_launch_bf16_t(bfp(x), bfp_mut(y), rows.data_ptr<long>(), m,
                              h, cur_stream());
  else
    moe_permute_launch_f32_t(x.data_ptr<float>(), y.data_ptr<float>(),
                             rows.data_ptr<long>(), m, h, cur_stream());
  return y;
}

Tensor moe_permute_bwd(const Tensor& dy, const Tensor& rows, long n) {
  CHECK_GPU(dy);
  const long m = rows.numel();
  const int h = dy.size(-1);
  auto acc = at::zeros({n, (long)h}, dy.options().dtype(at::kFloat));
  if (m > 0) {
    if (is_bf16(dy))
      moe_permute_bwd_launch_bf16_t(bfp(dy), acc.data_ptr<float>(),
                                    rows.data_ptr<long>(), m, h,
                                    cur_stream());
    else
      moe_permute_bwd_launch_f32_t(dy.data_ptr<float>(),
                                   acc.data_ptr<float>(),
                                   rows.data_ptr<long>(), m, h,
                                   cur_stream());
  }
  return acc.to(dy.scalar_type());
}

Tensor moe_unpermute(const Tensor& back, const Tensor& probs,
                     const Tensor& inv_order, long n, long k) {
  CHECK_GPU(back);
  const int h = back.size(-1);
  auto out = at::empty({n, (long)h}, back.options());
  if (n == 0) return out;
  auto p = probs.contiguous().to(at::kFloat);
  if (is_bf16(back))
    moe_unpermute_launch_bf16_t(bfp(back), p.data_ptr<float>(),
                                inv_order.data_ptr<long>(), bfp_mut(out), n,
                                (int)k, h, cur_stream());
  else
    moe_unpermute_launch_f32_t(back.data_ptr<float>(), p.data_ptr<float>(),
                               inv_order.data_ptr<long>(),
                               out.data_ptr<float>(), n, (int)k, h,
                               cur_stream());
  return out;
}

std::tuple<Tensor, Tensor> moe_unpermute_bwd(const Tensor& dout,
                                             const Tensor& back,
                                             const Tensor& probs,
                                             const Tensor& t_of) {
  CHECK_GPU(dout); CHECK_GPU(back);
  const long m = back.size(0);
  const int h = back.size(-1);
  auto dback = at::empty_like(back);
  auto dprobs = at::zeros({m}, back.options().dtype(at::kFloat));
  auto p = probs.contiguous().to(at::kFloat);
  if (m > 0) {
    if (is_bf16(back))
      moe_unpermute_bwd_launch_bf16_t(bfp(dout), bfp(back),
                                      p.data_ptr<float>(),
                                      t_of.data_ptr<long>(), bfp_mut(dback),
                                      dprobs.data_ptr<float>(), m, h,
                                      cur_stream());
    else
      moe_unpermute_bwd_launch_f32_t(dout.data_ptr<float>(),
                                     back.data_ptr<float>(),
                                     p.data_ptr<float>(),
                                     t_of.data_ptr<long>(),
                                     dback.data_ptr<float>(),
                                     dprobs.data_ptr<float>(), m, h,
                                     cur_stream());
  }
  return {dback, dprobs};
}

// ---- grouped GEMM (MoE experts) -------------------------------------------
Tensor grouped_gemm(const Tensor& A, const Tensor& W, const Tensor& tiles,
                    long n_out, bool trans_b) {
  CHECK_GPU(A); CHECK_GPU(W); CHECK_GPU(tiles);
  TORCH_CHECK(is_bf16(A) && is_bf16(W), "grouped_gemm: bf16 only");
  const long M = A.size(0), K = A.size(1);
  TORCH_CHECK(K % 32 == 0 && n_out % 128 == 0,
              "grouped_gemm: K%32, N%128 required");
  auto C = at::empty({M, n_out}, A.options());
  if (M > 0)
    grouped_gemm_launch(bfp(A), bfp(W), bfp_mut(C), tiles.data_ptr(),
                        (int)tiles.size(0), (int)K, (int)n_out,
                        W.size(1) * W.size(2), trans_b, cur_stream());
  return C;
}

Tensor grouped_gemm_dw(const Tensor& A, const Tensor& dC,
                       const Tensor& row_off, long E) {
  CHECK_GPU(A); CHECK_GPU(dC); CHECK_GPU(row_off);
  const long K = A.size(1), N = dC.size(1);
  TORCH_CHECK(K % 128 == 0 && N % 128 == 0,
              "grouped_gemm_dw: K%128 and N%128 required");
  auto dW = at::empty({E, K, N}, A.options().dtype(at::kFloat));
  grouped_gemm_dw_launch(bfp(A), bfp(dC), dW.data_ptr<float>(),
                         row_off.data_ptr<int>(), (int)E, (int)K, (int)N,
                         cur_stream());
  return dW;
}

// ---- fused AdamW ----------------------------------------------------------
void fused_adamw(std::vector<Tensor> masters, std::vector<Tensor> grads,
                 std::vector<Tensor> ms, std::vector<Tensor> vs,
                 std::vector<Tensor> outs, long step, double lr, double beta1,
                 double beta2, double eps, double wd, double gscale = 1.0) {
  auto st = cur_stream();
  for (size_t i = 0; i < masters.size(); ++i) {
    auto& m = masters[i];
    const long n = m.numel();
    if (n == 0) continue;
    CHECK_GPU(m);
    TORCH_CHECK(m.scalar_type() == at::kFloat, "adamw: master must be fp32");
    float* mp = m.data_ptr<float>();
    float* ma = ms[i].data_ptr<float>();
    float* va = vs[i].data_ptr<float>();
    const bool g_bf = is_bf16(grads[i]);
    const bool o_bf = is_bf16(outs[i]);
    if (g_bf && o_bf)
      adamw_launch_t<__bf16, __bf16>(mp, bfp(grads[i]), ma, va,
                                     bfp_mut(outs[i]), n, (int)step, lr,
                                     beta1, beta2, eps, wd, (float)gscale, st);
    else if (g_bf && !o_bf)
      adamw_launch_t<__bf16, float>(mp, bfp(grads[i]), ma, va,
                                    outs[i].data_ptr<float>(), n, (int)step,
                                    lr, beta1, beta2, eps, wd, (float)gscale, st);
    else if (!g_bf && o_bf)
      adamw_launch_t<float, __bf16>(mp, grads[i].data_ptr<float>(), ma,
                                    va, bfp_mut(outs[i]), n, (int)step, lr,
                                    beta1, beta2, eps, wd, (float)gscale, st);
    else
      adamw_launch_t<float, float>(mp, grads[i].data_ptr<float>(), ma,
                                   va, outs[i].data_ptr<float>(), n,
                                   (int)step, lr, beta1, beta2, eps, wd, (float)gscale, st);
  }
}

}  // namespace

// ---- multi-tensor grad-norm sum of squares --------------------------------
Tensor multi_sumsq(std::vector<Tensor> grads) {
  TORCH_CHECK(!grads.empty(), "multi_sumsq: empty list");
  auto dev = grads[0].device();
  constexpr long CHUNK = 1 << 20;
  std::vector<long> meta;
  for (auto& g : grads) {
    CHECK_GPU(g);
    TORCH_CHECK(g.scalar_type() == at::kFloat && g.is_contiguous(),
                "multi_sumsq: fp32 contiguous only");
    const long n = g.numel();
    const long base = (long)(intptr_t)g.data_ptr<float>();
    for (long off = 0; off < n; off += CHUNK) {
      meta.push_back(base);
      meta.push_back(off);
      meta.push_back(std::min(CHUNK, n - off));
    }
  }
  auto meta_t = at::from_blob(meta.data(), {(long)meta.size()},
                              at::TensorOptions().dtype(at::kLong))
                    .to(dev, /*non_blocking=*/false);
  const int n_chunks = (int)(meta.size() / 3);
  auto part = at::empty({multi_sumsq_grid(n_chunks)},
                        grads[0].options().dtype(at::kFloat));
  multi_sumsq_launch(meta_t.data_ptr<long>(), n_chunks,
                     part.data_ptr<float>(), cur_stream());
  return part.sum(0, /*keepdim=*/true);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  m.def("add_rmsnorm_bwd", &add_rmsnorm_bwd);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope_fwd", &rope_fwd);
  m.def("flash_attn_fwd", &flash_attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal"), py::arg("scale"), py::arg("bias") = py::none(), py::arg("sbhd") = false, py::arg("window") = 0);
  m.def("flash_attn_bwd", &flash_attn_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"), py::arg("causal"), py::arg("scale"), py::arg("bias") = py::none(), py::arg("sbhd") = false, py::arg("window") = 0);
  m.def("flash_attn_varlen_fwd", &flash_attn_varlen_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("causal"), py::arg("scale"), py::arg("sbhd") = false);
  m.def("flash_attn_varlen_bwd", &flash_attn_varlen_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"), py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("causal"), py::arg("scale"), py::arg("sbhd") = false);
  m.def("rope_qkv_", &rope_qkv_, py::arg("qkv"), py::arg("cos"), py::arg("sin"));
  m.def("flash_attn_qkv_fwd", &flash_attn_qkv_fwd, py::arg("qkv"), py::arg("causal"), py::arg("scale"));
  m.def("flash_attn_qkv_bwd", &flash_attn_qkv_bwd, py::arg("dout"), py::arg("qkv"), py::arg("o"), py::arg("lse"), py::arg("causal"), py::arg("scale"));
  m.def("flash_attn_qkv_varlen_fwd", &flash_attn_qkv_varlen_fwd, py::arg("qkv"), py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("causal"), py::arg("scale"));
  m.def("flash_attn_qkv_varlen_bwd", &flash_attn_qkv_varlen_bwd, py::arg("dout"), py::arg("qkv"), py::arg("o"), py::arg("lse"), py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("causal"), py::arg("scale"));
  m.def("qkv_grad_finish_", &qkv_grad_finish_, py::arg("dqkv"), py::arg("dk_exp"), py::arg("dv_exp"), py::arg("cos") = py::none(), py::arg("sin") = py::none());
  m.def("decode_attn", &decode_attn, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cur_len"), py::arg("scale"), py::arg("start") = 0);
  m.def("decode_attn_graph", &decode_attn_graph);
  m.def("mfma_probe", &mfma_probe);
  m.def("ce_max", &ce_max);
  m.def("ce_sum_target", &ce_sum_target);
  m.def("ce_bwd", &ce_bwd);
  m.def("fused_adamw", &fused_adamw, py::arg("masters"), py::arg("grads"),
        py::arg("ms"), py::arg("vs"), py::arg("outs"), py::arg("step"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wd"), py::arg("gscale") = 1.0);
  m.def("multi_sumsq", &multi_sumsq);
  m.def("grad_accum", &grad_accum);
  m.def("grouped_gemm", &grouped_gemm);
  m.def("moe_permute", &moe_permute);
  m.def("moe_permute_bwd", &moe_permute_bwd);
  m.def("moe_unpermute", &moe_unpermute);
  m.def("moe_unpermute_bwd", &moe_unpermute_bwd);
  m.def("grouped_gemm_dw", &grouped_gemm_dw);
  m.attr("arch") = "gfx950";
}
