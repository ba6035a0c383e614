"""Autograd-wrapped ops dispatching native HIP (GPU) / torch reference (CPU).

Every op here replaces an external CUDA dependency of the reference:
  rms_norm / layer_norm  <- flash_attn.ops.rms_norm / dropout_layer_norm
                            (reference: core/runtime/transformer/norm.py:3-30)
  swiglu / bias-gelu     <- torch.jit fused kernels
                            (reference: transformer/fused_kernels.py:143-226)
  apply_rope             <- flash_attn rotary_emb ext
                            (reference: transformer/fused_kernels.py:227-257)
  flash_attention        <- flash_attn_varlen CUDA
                            (reference: transformer/attention_impl.py:18-108)
  flash_attention_varlen <- the same, with cu_seqlens (packed documents)
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import reference_ops as ref
from ._ext import get_ext, native_available, use_native


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        if use_native(x):
            y, invrms = get_ext(False).rmsnorm_fwd(x, weight, eps)
        else:
            y, invrms = ref.rmsnorm_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, invrms)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, invrms = ctx.saved_tensors
        if use_native(x):
            dx, dw = get_ext(False).rmsnorm_bwd(dy.contiguous(), x, weight, invrms)
        else:
            dx, dw = ref.rmsnorm_bwd(dy, x, weight, invrms)
        return dx, dw.to(weight.dtype), None


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return _RMSNorm.apply(x.contiguous(), weight, eps)


class _AddRMSNorm(torch.autograd.Function):
    """Fused residual-add + RMSNorm: (y, sum) = (rmsnorm(x+res)*w, x+res).
    One kernel each way — removes the standalone residual-add in forward
    AND the grad-join add in backward (the reference fuses the same way
    via flash-attn's DropoutAddLayerNorm, norm.py:3-30)."""

    @staticmethod
    def forward(ctx, x, res, weight, eps):
        y, s, invrms = get_ext(False).add_rmsnorm_fwd(x, res, weight, eps)
        ctx.save_for_backward(s, weight, invrms)
        return y, s

    @staticmethod
    def backward(ctx, dy, dsum):
        s, weight, invrms = ctx.saved_tensors
        dx, dw = get_ext(False).add_rmsnorm_bwd(
            dy.contiguous(), dsum.contiguous(), s, weight, invrms)
        return dx, dx, dw.to(weight.dtype), None


def fused_add_rms_norm(x, res, weight, eps: float = 1e-5):
    """Returns (normed, sum).  Native bf16 path only; callers fall back to
    `rms_norm(x + res)` elsewhere."""
    return _AddRMSNorm.apply(x.contiguous(), res.contiguous(), weight, eps)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        if use_native(x):
            y, mean, invstd = get_ext(False).layernorm_fwd(x, weight, bias, eps)
        else:
            y, mean, invstd = ref.layernorm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, invstd = ctx.saved_tensors
        if use_native(x):
            dx, dw, db = get_ext(False).layernorm_bwd(dy.contiguous(), x, weight, mean, invstd)
        else:
            dx, dw, db = ref.layernorm_bwd(dy, x, weight, mean, invstd)
        return dx, dw.to(weight.dtype), db.to(weight.dtype), None


def layer_norm(x, weight, bias, eps: float = 1e-5) -> torch.Tensor:
    return _LayerNorm.apply(x.contiguous(), weight, bias, eps)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        if use_native(x):
            return get_ext(False).swiglu_fwd(x)
        return ref.swiglu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        if use_native(x):
            return get_ext(False).swiglu_bwd(dy.contiguous(), x)
        return ref.swiglu_bwd(dy, x)


def swiglu(x: torch.Tensor) -> torch.Tensor:
    """x[..., 2F] = [gate, up] -> silu(gate)*up."""
    return _SwiGLU.apply(x.contiguous())


class _RoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin):
        ctx.save_for_backward(cos, sin)
        if use_native(x):
            return get_ext(False).rope_fwd(x, cos, sin, False)
        return ref.rope_apply(x, cos, sin, conj=False)

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        dy = dy.contiguous()
        if use_native(dy):
            return get_ext(False).rope_fwd(dy, cos, sin, True), None, None
        return ref.rope_apply(dy, cos, sin, conj=True), None, None


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [s, b, h, d]; cos/sin: [s, d/2] (NEOX half-rotation)."""
    return _RoPE.apply(x.contiguous(), cos, sin)


class _FlashAttention(torch.autograd.Function):
    """Flash attention with LSE output.

    Layout [b, s, h, d] bf16/fp32; GQA supported (hq multiple of hkv);
    causal masking bottom-right aligned.  Native path: CDNA4 MFMA kernel
    (ops/csrc/flash_attn.hip).
    """

    @staticmethod
    def forward(ctx, q, k, v, causal, softmax_scale, window, sbhd):
        scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(q.shape[-1])
        skv = k.shape[0] if sbhd else k.shape[1]
        # an effective window (window < kv length) routes to the eager
        # reference path (a window argument on the native kernel is a v2
        # item); window >= kv length is a no-op -> native
        eff_window = window if (window is not None and
                                window < skv) else None
        if use_native(q) \
                and q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128) \
                and (eff_window is None or causal):
            o, lse = get_ext(False).flash_attn_fwd(q, k, v, causal, scale,
                                                   None, sbhd,
                                                   eff_window or 0)
        elif sbhd:
            ob, lse = ref.attention_fwd(
                q.permute(1, 0, 2, 3), k.permute(1, 0, 2, 3),
                v.permute(1, 0, 2, 3), causal, scale, window=eff_window)
            o = ob.permute(1, 0, 2, 3).contiguous()
        else:
            o, lse = ref.attention_fwd(q, k, v, causal, scale,
                                       window=eff_window)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        ctx.scale = scale
        ctx.window = eff_window
        ctx.sbhd = sbhd
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        q, k, v, o, lse = ctx.saved_tensors
        do = do.contiguous()
        if use_native(q) \
                and q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128) \
                and (ctx.window is None or ctx.causal):
            dq, dk, dv = get_ext(False).flash_attn_bwd(
                do, q, k, v, o, lse, ctx.causal, ctx.scale, None, ctx.sbhd,
                ctx.window or 0)
        elif ctx.sbhd:
            dq, dk, dv = ref.attention_bwd(
                do.permute(1, 0, 2, 3), q.permute(1, 0, 2, 3),
                k.permute(1, 0, 2, 3), v.permute(1, 0, 2, 3),
                o.permute(1, 0, 2, 3), lse, ctx.causal, ctx.scale,
                window=ctx.window)
            dq = dq.permute(1, 0, 2, 3).contiguous()
            dk = dk.permute(1, 0, 2, 3).contiguous()
            dv = dv.permute(1, 0, 2, 3).contiguous()
        else:
            dq, dk, dv = ref.attention_bwd(do, q, k, v, o, lse, ctx.causal,
                                           ctx.scale, window=ctx.window)
        return dq, dk, dv, None, None, None, None


def flash_attention(q, k, v, causal: bool = True,
                    softmax_scale: Optional[float] = None,
                    return_lse: bool = False, window: Optional[int] = None,
                    sbhd: bool = False):
    """q: [b,s,hq,d]; k,v: [b,s,hkv,d] -> o [b,s,hq,d] (+ lse [b,hq,s]).
    sbhd=True: tensors are [s,b,h,d] (the runtime's native activation
    layout) — saves the permute+contiguous copies around the kernel.
    window: mistral-style sliding window (causal only)."""
    o, lse = _FlashAttention.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                                   causal, softmax_scale, window, sbhd)
    return (o, lse) if return_lse else o


def _varlen_native(q) -> bool:
    return (use_native(q) and q.dtype == torch.bfloat16
            and q.shape[-1] in (64, 128))


class _FlashAttentionVarlen(torch.autograd.Function):
    """Packed-document self-attention (one cu_seqlens for q and kv).
    Native path: the flash_varlen_* kernels of ops/csrc/flash_attn.hip;
    anything else runs the fp32 per-segment reference."""

    @staticmethod
    def forward(ctx, q, k, v, cu, max_seqlen, causal, scale, sbhd):
        if _varlen_native(q):
            o, lse = get_ext(False).flash_attn_varlen_fwd(
                q, k, v, cu, max_seqlen, causal, scale, sbhd)
        else:
            o, lse = ref.attention_varlen_fwd(q, k, v, cu, max_seqlen,
                                              causal, scale, sbhd)
        ctx.save_for_backward(q, k, v, o, lse, cu)
        ctx.max_seqlen = max_seqlen
        ctx.causal = causal
        ctx.scale = scale
        ctx.sbhd = sbhd
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        q, k, v, o, lse, cu = ctx.saved_tensors
        do = do.contiguous()
        if _varlen_native(q):
            dq, dk, dv = get_ext(False).flash_attn_varlen_bwd(
                do, q, k, v, o, lse, cu, ctx.max_seqlen, ctx.causal,
                ctx.scale, ctx.sbhd)
        else:
            dq, dk, dv = ref.attention_varlen_bwd(
                do, q, k, v, o, lse, cu, ctx.max_seqlen, ctx.causal,
                ctx.scale, ctx.sbhd)
        return dq, dk, dv, None, None, None, None, None


def _device_cu_seqlens(cu_seqlens, b, s, max_seqlen, like):
    """A cu_seqlens table ready for the kernels: a CPU one is validated
    against [b, s] and copied asynchronously to like's device; a device one
    is trusted (the caller validated its host copy)."""
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1:
        raise ValueError("cu_seqlens must be a 1-D int32 tensor")
    if not cu_seqlens.is_cuda:
        ref.check_cu_seqlens(cu_seqlens, b, s, max_seqlen)
        if like.is_cuda:
            cu_seqlens = cu_seqlens.to(like.device, non_blocking=True)
    return cu_seqlens.contiguous()


def flash_attention_varlen(q, k, v, cu_seqlens, max_seqlen: int,
                           causal: bool = True,
                           softmax_scale: Optional[float] = None,
                           return_lse: bool = False, sbhd: bool = False):
    """Packed-document flash attention: tokens attend only inside their own
    segment.  q: [b,s,hq,d]; k,v: [b,s,hkv,d] ([s,b,h,d] with sbhd) ->
    o like q (+ lse [b,hq,s]).

    cu_seqlens: int32 [nseg+1] token offsets into the batch-major flattened
    [b*s] stream; the segments tile [0, b*s) and never straddle a batch row
    (padding is just another segment).  max_seqlen bounds the longest
    segment, so nothing is read back from the device.  A CPU cu_seqlens is
    validated here and then copied asynchronously; a device one is trusted
    (the caller validated its host copy).
    """
    b, s = (q.shape[1], q.shape[0]) if sbhd else (q.shape[0], q.shape[1])
    max_seqlen = int(max_seqlen)
    cu_seqlens = _device_cu_seqlens(cu_seqlens, b, s, max_seqlen, q)
    scale = softmax_scale if softmax_scale is not None \
        else 1.0 / math.sqrt(q.shape[-1])
    o, lse = _FlashAttentionVarlen.apply(
        q.contiguous(), k.contiguous(), v.contiguous(), cu_seqlens,
        max_seqlen, causal, scale, sbhd)
    return (o, lse) if return_lse else o


class _FusedQKVAttention(torch.autograd.Function):
    """RoPE + flash attention on the packed linear_qkv output, native only.
    q, k and v are never separated in memory: RoPE rotates the q and k
    slots in place (tables [s, d/2], or per-row [s, b, d/2]), the packed
    flash kernels address the slots directly, and one finishing kernel turns
    dqkv into the gradient of the packed buffer (inverse rotation + GQA
    group sum).  With cu_seqlens the flash_packed_varlen_* kernels
    (ops/csrc/flash_attn_qkv_varlen.hip) run; cu None keeps the dense packed
    kernels (flash_attn_qkv.hip) and their pairing.  elementwise.hip holds
    rope_qkv_kernel and qkv_grad_finish_kernel."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, geom, cu, max_seqlen, causal, scale):
        ext = get_ext(False)
        # qkv is rewritten in place: tell autograd, so that a producer that
        # saved this buffer for its own backward fails loudly instead of
        # reading rotated values.  A dirty input has to be returned.
        ctx.mark_dirty(qkv)
        ctx.set_materialize_grads(False)
        packed = qkv.view(*geom)
        if cos is not None:
            ext.rope_qkv_(packed, cos, sin)
        if cu is None:
            o, lse = ext.flash_attn_qkv_fwd(packed, causal, scale)
        else:
            o, lse = ext.flash_attn_qkv_varlen_fwd(packed, cu, max_seqlen,
                                                   causal, scale)
        # the rotated buffer is what backward needs: nothing else is kept
        ctx.save_for_backward(qkv, o, lse, cos, sin, cu)
        ctx.geom = geom
        ctx.max_seqlen = max_seqlen
        ctx.causal = causal
        ctx.scale = scale
        return o, qkv

    @staticmethod
    def backward(ctx, do, _dbuf):
        if do is None:
            return (None,) * 8
        qkv, o, lse, cos, sin, cu = ctx.saved_tensors
        ext = get_ext(False)
        if cu is None:
            dqkv, dk_exp, dv_exp = ext.flash_attn_qkv_bwd(
                do.contiguous(), qkv.view(*ctx.geom), o, lse, ctx.causal,
                ctx.scale)
        else:
            dqkv, dk_exp, dv_exp = ext.flash_attn_qkv_varlen_bwd(
                do.contiguous(), qkv.view(*ctx.geom), o, lse, cu,
                ctx.max_seqlen, ctx.causal, ctx.scale)
        ext.qkv_grad_finish_(dqkv, dk_exp, dv_exp, cos, sin)
        return (dqkv.view(qkv.shape),) + (None,) * 7


def _qkv_geom(qkv, num_groups, q_per_group, softmax_scale):
    """-> the packed view [s, b, G, qpg+2, d] of qkv and the softmax scale."""
    d = qkv.shape[2:].numel() // (num_groups * (q_per_group + 2))
    scale = softmax_scale if softmax_scale is not None \
        else 1.0 / math.sqrt(d)
    return (qkv.shape[0], qkv.shape[1], num_groups, q_per_group + 2, d), scale


def _fused_qkv_native(qkv, cos, sin, geom, cu_seqlens, max_seqlen, causal,
                      scale):
    if cos is not None:
        cos = cos[:geom[0]].contiguous().float()
        sin = sin[:geom[0]].contiguous().float()
    # the buffer itself goes in, not a view of it: an in-place op on a view
    # would make autograd copy the whole gradient back into the base
    o, _ = _FusedQKVAttention.apply(qkv.contiguous(), cos, sin, geom,
                                    cu_seqlens, max_seqlen, causal, scale)
    return o


def _rope_qk_rows(q, k, cos, sin):
    """apply_rope on q and k with [s, d/2] or per-row [s, b, d/2] tables.
    Per-row: the batch folds into the row axis, [s*b, 1, h, d] with a
    [s*b, d/2] table, as runtime.transformer.rope.apply_rope_qk does."""
    if cos.dim() == 3:
        s, b = q.shape[0], q.shape[1]
        cos, sin = cos.reshape(s * b, -1), sin.reshape(s * b, -1)
        qf = apply_rope(q.reshape(s * b, 1, *q.shape[2:]), cos, sin)
        kf = apply_rope(k.reshape(s * b, 1, *k.shape[2:]), cos, sin)
        return qf.view(q.shape), kf.view(k.shape)
    return apply_rope(q, cos, sin), apply_rope(k, cos, sin)


def _split_qkv(qkv, geom, cos, sin):
    """The composition the native path replaces: slice q, k and v out of
    the packed buffer ([s, b, h, d] each, contiguous) and rotate q and k."""
    s, b, _, slots, d = geom
    qkv = qkv.view(*geom)
    q = qkv[:, :, :, :slots - 2].reshape(s, b, -1, d)
    k = qkv[:, :, :, slots - 2].reshape(s, b, -1, d)
    v = qkv[:, :, :, slots - 1].reshape(s, b, -1, d)
    q, k = q.contiguous(), k.contiguous()
    if cos is not None:
        q, k = _rope_qk_rows(q, k, cos, sin)
    return q, k, v.contiguous()


def fused_qkv_attention_native(qkv, d, cos, window=None) -> bool:
    """True when fused_qkv_attention runs the packed HIP kernels (bf16 on
    the GPU, head dim 64|128, cos None or [s, d/2], no effective window)."""
    return (use_native(qkv) and qkv.dtype == torch.bfloat16
            and d in (64, 128)
            and (cos is None or cos.dim() == 2)
            and (window is None or window >= qkv.shape[0]))


def fused_qkv_attention(qkv, cos, sin, num_groups: int, q_per_group: int,
                        causal: bool = True,
                        softmax_scale: Optional[float] = None,
                        window: Optional[int] = None):
    """Self-attention straight from the linear_qkv output.

    qkv: [s, b, num_groups*(q_per_group+2)*d] (or already viewed
    [s, b, G, qpg+2, d]), interleaved by kv group: q heads in slots
    0..qpg-1, k in slot qpg, v in slot qpg+1.  cos/sin: [s, d/2] NEOX
    tables, or None for no rotary embedding.  Returns o [s, b, G*qpg, d].

    The native path CONSUMES qkv: RoPE rotates it in place (marked dirty
    for autograd), so the caller must not use it afterwards, its producer
    must not have saved it for backward, and it cannot be a leaf that
    requires grad.  Everything else (CPU, fp32, other head dims, per-row
    tables, an effective sliding window) runs the composition of slice,
    apply_rope and flash_attention and leaves qkv alone."""
    geom, scale = _qkv_geom(qkv, num_groups, q_per_group, softmax_scale)
    if fused_qkv_attention_native(qkv, geom[-1], cos, window):
        return _fused_qkv_native(qkv, cos, sin, geom, None, None, causal,
                                 scale)
    if cos is not None and cos.dim() != 2:
        raise ValueError("fused_qkv_attention: cos/sin must be [s, d/2]")
    q, k, v = _split_qkv(qkv, geom, cos, sin)
    return flash_attention(q, k, v, causal=causal,
                           softmax_scale=softmax_scale, window=window,
                           sbhd=True)


def fused_qkv_attention_varlen(qkv, cos, sin, num_groups: int,
                               q_per_group: int, cu_seqlens=None,
                               max_seqlen: Optional[int] = None,
                               causal: bool = True,
                               softmax_scale: Optional[float] = None):
    """fused_qkv_attention for packed documents.

    qkv as in fused_qkv_attention.  cos/sin: None, [s, d/2], or per-row
    [s, b, d/2] (positions that restart per document; rank 3 selects it).
    cu_seqlens/max_seqlen as in flash_attention_varlen: int32 [nseg+1]
    offsets into the batch-major [b*s] stream that tile it without
    straddling a row; a CPU table is validated and copied asynchronously, a
    device table is trusted.  cu_seqlens=None attends over whole rows (the
    reset_position_ids-only case).  Returns o [s, b, G*qpg, d].

    The native path (bf16 on the GPU, head dim 64|128) CONSUMES qkv exactly
    as fused_qkv_attention does.  Everything else runs the composition of
    slice, apply_rope and flash_attention_varlen / flash_attention and
    leaves qkv alone."""
    geom, scale = _qkv_geom(qkv, num_groups, q_per_group, softmax_scale)
    if cos is not None and cos.dim() not in (2, 3):
        raise ValueError("fused_qkv_attention_varlen: cos/sin must be "
                         "[s, d/2] or [s, b, d/2]")
    if cu_seqlens is not None:
        if max_seqlen is None:
            raise ValueError("fused_qkv_attention_varlen: cu_seqlens needs "
                             "max_seqlen")
        max_seqlen = int(max_seqlen)
        cu_seqlens = _device_cu_seqlens(cu_seqlens, geom[1], geom[0],
                                        max_seqlen, qkv)
    if use_native(qkv) and qkv.dtype == torch.bfloat16 \
            and geom[-1] in (64, 128):
        return _fused_qkv_native(qkv, cos, sin, geom, cu_seqlens, max_seqlen,
                                 causal, scale)
    q, k, v = _split_qkv(qkv, geom, cos, sin)
    if cu_seqlens is None:
        return flash_attention(q, k, v, causal=causal,
                               softmax_scale=softmax_scale, sbhd=True)
    return flash_attention_varlen(q, k, v, cu_seqlens, max_seqlen,
                                  causal=causal, softmax_scale=softmax_scale,
                                  sbhd=True)


class _FlashBiasAttention(torch.autograd.Function):
    """Biased flash attention (t5 relative bias [hq, sq, skv]) with grads
    for q/k/v AND the bias (dbias batch-summed, flows back into the bias
    table's construction graph).  Native CDNA4 path when available."""

    @staticmethod
    def forward(ctx, q, k, v, bias, causal, scale):
        o, lse = flash_attention_fwd_only(q, k, v, causal, scale, bias=bias)
        ctx.save_for_backward(q, k, v, o, lse, bias)
        ctx.causal = causal
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, bias = ctx.saved_tensors
        dq, dk, dv, dbias = flash_attention_bwd_only(
            do.contiguous(), q, k, v, o, lse, ctx.causal, ctx.scale,
            bias=bias)
        return dq, dk, dv, dbias.to(bias.dtype), None, None


def flash_bias_attention(q, k, v, bias, causal: bool = True,
                         softmax_scale: Optional[float] = None):
    """q: [b,s,hq,d]; bias [hq, sq, skv] additive pre-softmax scores."""
    scale = softmax_scale if softmax_scale is not None \
        else 1.0 / math.sqrt(q.shape[-1])
    return _FlashBiasAttention.apply(q.contiguous(), k.contiguous(),
                                     v.contiguous(), bias, causal, scale)


def flash_attention_fwd_only(q, k, v, causal=True, softmax_scale=None,
                             bias=None, window=None):
    """No-autograd forward returning (o, lse) — building block for ring CP
    and the generator prefill.  bias [hq, sq, skv] (t5 relative bias) and
    mistral sliding `window` both take the native CDNA4 kernel path."""
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(q.shape[-1])
    eff_window = window if (window is not None and
                            window < k.shape[1]) else None
    if use_native(q) and q.dtype == torch.bfloat16 \
            and q.shape[-1] in (64, 128) \
            and (bias is None or bias.shape[-1] % 4 == 0) \
            and (eff_window is None or (causal and bias is None)):
        bias_n = None if bias is None else bias.to(torch.bfloat16).contiguous()
        return get_ext(False).flash_attn_fwd(q.contiguous(), k.contiguous(),
                                             v.contiguous(), causal, scale,
                                             bias_n, False, eff_window or 0)
    return ref.attention_fwd(q, k, v, causal, scale, bias,
                             window=eff_window)


def flash_attention_bwd_only(do, q, k, v, o, lse, causal=True,
                             softmax_scale=None, bias=None):
    """Without bias: (dq, dk, dv); with bias also dbias (batch-summed,
    fp32 — the native kernel accumulates it atomically in the dK phase)."""
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(q.shape[-1])
    if use_native(q) and q.dtype == torch.bfloat16 \
            and q.shape[-1] in (64, 128) \
            and (bias is None or bias.shape[-1] % 4 == 0):
        bias_n = None if bias is None else bias.to(torch.bfloat16).contiguous()
        out = get_ext(False).flash_attn_bwd(do.contiguous(), q, k, v, o, lse,
                                            causal, scale, bias_n)
        return tuple(out)
    return ref.attention_bwd(do, q, k, v, o, lse, causal, scale, bias)


def _gg_tiles(counts, device):
    """Host-built [n_tiles, 3] int32 (expert, row0, rows) + row_off [E+1]."""
    tiles = []
    off = 0
    row_off = [0]
    for e, m in enumerate(counts):
        m = int(m)
        r = 0
        while r < m:
            tiles.append((e, off + r, min(128, m - r)))
            r += 128
        off += m
        row_off.append(off)
    td = torch.tensor(tiles if tiles else [(0, 0, 0)], dtype=torch.int32)
    ro = torch.tensor(row_off, dtype=torch.int32)
    return td.to(device, non_blocking=True), ro.to(device, non_blocking=True)


class _GroupedGemm(torch.autograd.Function):
    """C_e = A_e @ W[e] over expert-sorted rows (ops/csrc/grouped_gemm.hip).

    Replaces the reference's external grouped_gemm CUDA dep
    (moe/grouped_gemm_util.py). counts is a host list (the MoE dispatcher
    already synchronized it for the all-to-all splits).
    """

    @staticmethod
    def forward(ctx, a, w, counts):
        tiles, row_off = _gg_tiles(counts, a.device)
        c = get_ext(False).grouped_gemm(a, w, tiles, w.shape[2], False)
        ctx.save_for_backward(a, w, tiles, row_off)
        return c

    @staticmethod
    def backward(ctx, dc):
        a, w, tiles, row_off = ctx.saved_tensors
        dc = dc.contiguous()
        ext = get_ext(False)
        # dA = dC @ W^T ; dW = A^T dC
        da = ext.grouped_gemm(dc, w, tiles, w.shape[1], True)
        dw = ext.grouped_gemm_dw(a, dc, row_off, w.shape[0])
        return da, dw.to(w.dtype), None


def grouped_gemm(a: torch.Tensor, w: torch.Tensor, counts) -> torch.Tensor:
    """a [M, K] bf16 expert-sorted; w [E, K, N]; counts: per-expert rows."""
    return _GroupedGemm.apply(a.contiguous(), w, counts)


def grouped_gemm_available(a, w) -> bool:
    """fwd needs K%32, N%128; backward dW needs K%128 and N%128; dA needs
    the reverse — so both dims of every W must be multiples of 128."""
    return (a.is_cuda and a.dtype == torch.bfloat16
            and w.shape[1] % 128 == 0 and w.shape[2] % 128 == 0
            and use_native(a))


class _MoEPermute(torch.autograd.Function):
    """Expert-sorted row gather (ops/csrc/moe_permute.hip); backward
    scatter-adds repeated source rows through an fp32 accumulator."""

    @staticmethod
    def forward(ctx, x, rows):
        ctx.save_for_backward(rows)
        ctx.n = x.shape[0]
        return get_ext(False).moe_permute(x, rows)

    @staticmethod
    def backward(ctx, dy):
        (rows,) = ctx.saved_tensors
        return get_ext(False).moe_permute_bwd(dy.contiguous(), rows,
                                              ctx.n), None


def moe_permute(x: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    if x.is_cuda and native_available() and x.shape[-1] % 8 == 0 \
            and x.dtype in (torch.bfloat16, torch.float32):
        return _MoEPermute.apply(x.contiguous(), rows.contiguous())
    return x[rows]


class _MoEUnpermute(torch.autograd.Function):
    """Probability-weighted top-k merge back to token order."""

    @staticmethod
    def forward(ctx, back, probs, order, n, k):
        inv = torch.argsort(order)
        t_of = torch.div(order, k, rounding_mode="floor")
        ctx.save_for_backward(back, probs, t_of)
        return get_ext(False).moe_unpermute(back, probs, inv, n, k)

    @staticmethod
    def backward(ctx, dout):
        back, probs, t_of = ctx.saved_tensors
        dback, dprobs = get_ext(False).moe_unpermute_bwd(
            dout.contiguous(), back, probs, t_of)
        return dback, dprobs.to(probs.dtype), None, None, None


def moe_unpermute(back: torch.Tensor, probs: torch.Tensor,
                  order: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """back [m,h] expert-sorted outputs; probs [m] sorted routing weights;
    order: argsort of the flat (token*k) expert assignment."""
    if back.is_cuda and native_available() and back.shape[-1] % 8 == 0 \
            and back.dtype in (torch.bfloat16, torch.float32):
        return _MoEUnpermute.apply(back.contiguous(), probs.contiguous(),
                                   order.contiguous(), n, k)
    h = back.shape[-1]
    out = back.new_zeros(n * k, h)
    out[order] = back * probs.unsqueeze(-1).to(back.dtype)
    return out.reshape(n, k, h).sum(1)


@torch.no_grad()
def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, cur_len: int,
                     softmax_scale=None, window=None) -> torch.Tensor:
    """Single-token decode attention against a KV cache (serving path).

    q: [b, hq, d]; k_cache/v_cache: [b, max_s, hkv, d]; attends to
    positions [0, cur_len), or the last `window` of them (mistral
    sliding-window decode).  Native CDNA4 kernel on GPU bf16
    (memory-bound KV streaming, decode_attn_kernel in elementwise.hip);
    plain torch reference elsewhere.  Reference role: the optional
    flash-decode path (nvidia_chunked_flash_attn, attention.py:398-514).
    """
    scale = softmax_scale if softmax_scale is not None \
        else q.shape[-1] ** -0.5
    start = max(0, cur_len - window) if window else 0
    if q.is_cuda and native_available() and q.dtype == torch.bfloat16 \
            and q.shape[-1] in (64, 128):
        return get_ext().decode_attn(q.contiguous(), k_cache, v_cache,
                                     int(cur_len), float(scale), int(start))
    return _decode_attention_torch(q, k_cache, v_cache, cur_len, scale, start)


def _decode_attention_torch(q, k_cache, v_cache, cur_len, scale, start):
    b, hq, d = q.shape
    hkv = k_cache.shape[2]
    k = k_cache[:, start:cur_len].float()
    v = v_cache[:, start:cur_len].float()
    if hq != hkv:
        rep = hq // hkv
        k = k.repeat_interleave(rep, dim=2)
        v = v.repeat_interleave(rep, dim=2)
    att = torch.einsum("bhd,bshd->bhs", q.float(), k) * scale
    w = att.softmax(-1)
    o = torch.einsum("bhs,bshd->bhd", w, v)
    return o.to(q.dtype)


@torch.no_grad()
def decode_attention_batched(q: torch.Tensor, k_cache: torch.Tensor,
                             v_cache: torch.Tensor, lengths: torch.Tensor,
                             slots: torch.Tensor = None, max_len: int = None,
                             softmax_scale=None, window=None,
                             k_scale: torch.Tensor = None,
                             v_scale: torch.Tensor = None,
                             page_table: torch.Tensor = None) -> torch.Tensor:
    """Decode attention for a batch of rows with their own lengths and cache
    rows (continuous-batching serving).

    q: [n, hq, d]; k_cache/v_cache: [S, max_s, hkv, d]; lengths: int32 [n],
    the attended length of each row, newest token included; slots: int32
    [n], the cache row of each q row (None: row i uses cache row i, n == S).
    Row i attends to [0, lengths[i]) or the last `window` of them.  max_len
    (None: max_s) bounds every length and sizes the launch.

    Native CDNA4 kernel on GPU bf16 with d in (64, 128) and hq/hkv <= 16
    (decode_attn_batched.hip): one launch for the whole batch, each K/V row
    read once per GQA group, lengths and slots read on the device — no host
    read-back, so a captured graph replays after they change in place; a
    length above max_len is clamped, a row with length <= 0 or a slot
    outside [0, S) gives zeros.  Elsewhere a loop over rows through the torch
    arithmetic of `decode_attention` (reads lengths and slots on the host).

    float8_e4m3fn caches (format tag DbE4m3 of decode_body.h) hold real =
    stored * scale[h] with k_scale / v_scale fp32 [hkv] (None: ones); q and
    the result stay bf16.  The scales are ignored for caches of any other dtype.

    page_table: int32 [S, max_pages] on the device makes the caches pools
    [P, page, hkv, d] of either dtype (addressing tag DbPaged), page a power
    of two >= 32: slots[i] is a row of the table and position p of row i is
    pool[page_table[slots[i], p // page], p % page].  max_len (None:
    max_pages * page) must lie within the table.  A table entry outside
    [0, P) contributes nothing: its positions are skipped and a row without
    a valid attended page gives zeros.  The table is read on the device, so
    it too may change in place under a captured graph; the torch path reads
    it on the host and gathers each row's pages.
    """
    n, hq, d = q.shape
    S, max_s, hkv = k_cache.shape[:3]
    scale = softmax_scale if softmax_scale is not None else d ** -0.5
    if page_table is not None:
        S, max_s = page_table.shape[0], page_table.shape[1] * max_s
    max_len = max_s if max_len is None else int(max_len)
    if slots is None:
        assert n == S, "slots=None needs one q row per cache row"
        slots = torch.arange(n, dtype=torch.int32, device=q.device)
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if q.is_cuda and native_available() and q.dtype == torch.bfloat16 \
            and d in (64, 128) and hq // hkv <= 16:
        if page_table is not None:
            if fp8:
                return get_ext().decode_attn_paged_fp8(
                    q.contiguous(), k_cache, v_cache, k_scale, v_scale,
                    page_table, lengths, slots, max_len, float(scale),
                    int(window or 0), 0)
            return get_ext().decode_attn_paged(
                q.contiguous(), k_cache, v_cache, page_table, lengths, slots,
                max_len, float(scale), int(window or 0), 0)
        if fp8:
            return get_ext().decode_attn_batched_fp8(
                q.contiguous(), k_cache, v_cache, k_scale, v_scale, lengths,
                slots, max_len, float(scale), int(window or 0), 0)
        return get_ext().decode_attn_batched(
            q.contiguous(), k_cache, v_cache, lengths, slots, max_len,
            float(scale), int(window or 0), 0)
    if page_table is not None:
        return _decode_attention_paged_torch(
            q, k_cache, v_cache, page_table, lengths, slots, max_len, scale,
            window, k_scale, v_scale)
    if fp8:
        return _decode_attention_batched_fp8_torch(
            q, k_cache, v_cache, lengths, slots, max_len, scale, window,
            k_scale, v_scale)
    return _decode_attention_batched_torch(q, k_cache, v_cache, lengths,
                                           slots, max_len, scale, window)


@torch.no_grad()
def decode_attention_multi(q: torch.Tensor, k_cache: torch.Tensor,
                           v_cache: torch.Tensor, lengths: torch.Tensor,
                           q_lens: torch.Tensor, slots: torch.Tensor,
                           window=None, max_len: int = None,
                           softmax_scale=None, n_chunks: int = None,
                           k_scale: torch.Tensor = None,
                           v_scale: torch.Tensor = None,
                           page_table: torch.Tensor = None) -> torch.Tensor:
    """Decode attention of up to T consecutive new tokens per row against
    that row's cache, causal inside the block (speculative verification,
    chunked decode, chunked prefill).

    q: [n, T, hq, d], any T >= 1; caches, pools, scales,
    slots, page_table, window and max_len as in `decode_attention_batched`.
    lengths: int32 [n], the row's cached length with the new tokens included
    (the caller has written them); q_lens: int32 [n] in [0, T], how many of
    the T tokens are real.  Token t < q_lens[i] sits at pos = lengths[i] -
    q_lens[i] + t and attends to [max(0, pos + 1 - window), pos] of cache row
    (table row) slots[i].  o[i, t] is zeros for t >= q_lens[i] and for a row
    with lengths[i] outside (0, max_len], q_lens[i] outside [0, T] or above
    the length, or a slot outside [0, S).

    Native CDNA4 kernels on GPU bf16 with d in (64, 128) and hq/hkv <= 16,
    for every T.  T <= 16 (decode_attn_multi.hip): the T * hq/hkv (token,
    head) columns of a kv head share one pass over its K and V rows, 32
    columns per workgroup, weights as three bf16 terms (the decode element
    rule).  T > 16 (decode_attn_prefill.hip): the flash-forward shape, 128
    columns per workgroup over 64-key K/V tiles staged once in LDS (e4m3
    dequantised while staging); the weights enter the second product as one
    bf16 term, a relative 2^-9 each, which is the accuracy of
    `flash_attention_fwd_only` and not that of the decode kernels.  Nothing
    is read back, so a captured graph replays after lengths, q_lens, slots,
    the table and the caches change in place.  n_chunks (None: chosen)
    forces the split-KV chunk count.  Elsewhere a loop over (row, token)
    through the torch arithmetic of `decode_attention` at cur = pos + 1.
    """
    n, T, hq, d = q.shape
    S, max_s, hkv = k_cache.shape[:3]
    scale = softmax_scale if softmax_scale is not None else d ** -0.5
    if page_table is not None:
        S, max_s = page_table.shape[0], page_table.shape[1] * max_s
    max_len = max_s if max_len is None else int(max_len)
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if q.is_cuda and native_available() and q.dtype == torch.bfloat16 \
            and d in (64, 128) and hq // hkv <= 16:
        ext = get_ext()
        tail = (lengths, q_lens, slots, max_len, float(scale),
                int(window or 0), int(n_chunks or 0))
        sc = (k_scale, v_scale) if fp8 else ()
        name = "decode_attn_multi" if T <= 16 else "decode_attn_prefill"
        if page_table is not None:
            f = getattr(ext, name + ("_paged_fp8" if fp8 else "_paged"))
            return f(q.contiguous(), k_cache, v_cache, *sc, page_table, *tail)
        f = getattr(ext, name + ("_fp8" if fp8 else ""))
        return f(q.contiguous(), k_cache, v_cache, *sc, *tail)
    return _decode_attention_multi_torch(
        q, k_cache, v_cache, lengths, q_lens, slots, S, max_len, scale,
        window, k_scale, v_scale, page_table)


def _decode_attention_multi_torch(q, k_cache, v_cache, lengths, q_lens, slots,
                                  S, max_len, scale, window, k_scale, v_scale,
                                  page_table):
    """Each (row, token) through `_decode_attention_torch` at cur = pos + 1
    on the row's positions [0, cur): e4m3 rows dequantised, pages gathered,
    positions of invalid pages left out."""
    n, T = q.shape[:2]
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    ks = k_scale.float()[:, None] if fp8 and k_scale is not None else None
    vs = v_scale.float()[:, None] if fp8 and v_scale is not None else None
    P, page = k_cache.shape[:2]
    out = torch.zeros_like(q)
    for i, (L, ql, s) in enumerate(zip(lengths.tolist(), q_lens.tolist(),
                                       slots.tolist())):
        if not (0 < L <= max_len and 0 <= ql <= T and ql <= L
                and 0 <= s < S):
            continue
        for t in range(ql):
            cur = L - ql + t + 1
            start = max(0, cur - window) if window else 0
            if page_table is not None:
                pos = torch.arange(start, cur, device=q.device)
                ids = page_table[s].to(q.device)[pos // page]
                keep = (ids >= 0) & (ids < P)
                if not bool(keep.any()):
                    continue
                ids, off = ids[keep].long(), (pos % page)[keep]
                k, v = k_cache[ids, off][None], v_cache[ids, off][None]
            else:
                k, v = k_cache[s:s + 1, start:cur], v_cache[s:s + 1, start:cur]
            if fp8:
                k, v = k.float(), v.float()
                k = k if ks is None else k * ks
                v = v if vs is None else v * vs
            out[i, t] = _decode_attention_torch(
                q[i, t][None], k, v, k.shape[1], scale, 0)[0]
    return out


def _decode_attention_paged_torch(q, k_pool, v_pool, page_table, lengths,
                                  slots, max_len, scale, window, k_scale=None,
                                  v_scale=None):
    """`decode_attention_batched` on a paged cache in torch: each row's valid
    pages gathered into a contiguous row, positions of invalid pages left
    out, then the contiguous torch path on that one row."""
    P, page = k_pool.shape[:2]
    S = page_table.shape[0]
    table = page_table.tolist()
    fp8 = k_pool.dtype == torch.float8_e4m3fn
    one = torch.ones(1, dtype=torch.int32, device=q.device)
    out = torch.zeros_like(q)
    for i, (cur, s) in enumerate(zip(lengths.tolist(), slots.tolist())):
        cur = min(cur, max_len)
        if cur <= 0 or not 0 <= s < S:
            continue
        start = max(0, cur - window) if window else 0
        pos = torch.arange(start, cur, device=q.device)
        ids = torch.tensor(table[s], device=q.device)[pos // page]
        keep = (ids >= 0) & (ids < P)
        if not bool(keep.any()):
            continue
        ids, off = ids[keep], (pos % page)[keep]
        k_row, v_row = k_pool[ids, off][None], v_pool[ids, off][None]
        L = k_row.shape[1]
        f = _decode_attention_batched_fp8_torch if fp8 \
            else _decode_attention_batched_torch
        extra = (k_scale, v_scale) if fp8 else ()
        out[i:i + 1] = f(q[i:i + 1], k_row, v_row, L * one, 0 * one, L,
                         scale, None, *extra)
    return out


def _decode_attention_batched_torch(q, k_cache, v_cache, lengths, slots,
                                    max_len, scale, window):
    S = k_cache.shape[0]
    out = torch.zeros_like(q)
    for i, (cur, s) in enumerate(zip(lengths.tolist(), slots.tolist())):
        cur = min(cur, max_len)
        if cur <= 0 or not 0 <= s < S:
            continue
        start = max(0, cur - window) if window else 0
        out[i:i + 1] = _decode_attention_torch(
            q[i:i + 1], k_cache[s:s + 1], v_cache[s:s + 1], cur, scale,
            start)
    return out


def _decode_attention_batched_fp8_torch(q, k_cache, v_cache, lengths, slots,
                                        max_len, scale, window, k_scale=None,
                                        v_scale=None):
    """`decode_attention_batched` on e4m3 caches in torch: the row loop on
    each row's window, dequantised to fp32 (exact)."""
    S = k_cache.shape[0]
    ks = 1.0 if k_scale is None else k_scale.float()[:, None]
    vs = 1.0 if v_scale is None else v_scale.float()[:, None]
    out = torch.zeros_like(q)
    for i, (cur, s) in enumerate(zip(lengths.tolist(), slots.tolist())):
        cur = min(cur, max_len)
        if cur <= 0 or not 0 <= s < S:
            continue
        start = max(0, cur - window) if window else 0
        out[i:i + 1] = _decode_attention_torch(
            q[i:i + 1], k_cache[s:s + 1, start:cur].float() * ks,
            v_cache[s:s + 1, start:cur].float() * vs, cur - start, scale, 0)
    return out


@torch.no_grad()
def kv_cache_append(k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, slots: torch.Tensor,
                    positions: torch.Tensor, k_scale: torch.Tensor = None,
                    v_scale: torch.Tensor = None) -> None:
    """Write new K/V rows into the serving caches:
    cache[slots[i], positions[i]] = k[i] (v likewise).

    k, v: [n, hkv, d] (any row and head stride, e.g. views of the packed qkv
    output); caches [S, max_s, hkv, d]; slots, positions: int32 [n] on the
    caches' device.  A row whose slot is outside [0, S) or whose position is
    outside [0, max_s) is skipped.  float8_e4m3fn caches store
    e4m3_rne(clamp(x / scale[h], -448, 448)) with k_scale / v_scale fp32
    [hkv] (None: ones): one native launch for both tensors on the GPU
    (kv_append_fp8_kernel in decode_attn_fp8.hip), torch elsewhere.  Caches
    of any other dtype get a plain indexed copy in torch.
    """
    if k_cache.dtype == torch.float8_e4m3fn and k.is_cuda \
            and native_available() and k.dtype == torch.bfloat16 \
            and k.shape[-1] in (64, 128):
        get_ext().kv_append_fp8(k, v, k_cache, v_cache, slots, positions,
                                k_scale, v_scale)
        return
    _kv_cache_append_torch(k, v, k_cache, v_cache, slots, positions, k_scale,
                           v_scale)


def _kv_cache_append_torch(k, v, k_cache, v_cache, slots, positions,
                           k_scale=None, v_scale=None):
    S, max_s = k_cache.shape[:2]
    keep = (slots >= 0) & (slots < S) & (positions >= 0) & (positions < max_s)
    sl, ps = slots[keep].long(), positions[keep].long()
    for x, cache, scale in ((k, k_cache, k_scale), (v, v_cache, v_scale)):
        x = x[keep]
        if cache.dtype == torch.float8_e4m3fn:
            x = x.float()
            if scale is not None:
                x = x / scale.float()[:, None]
            x = x.clamp(-448.0, 448.0)
        cache[sl, ps] = x.to(cache.dtype)


@torch.no_grad()
def rope_kv_append(qkv: torch.Tensor, num_groups: int, q_per_group: int,
                   cos: Optional[torch.Tensor], sin: Optional[torch.Tensor],
                   lengths: torch.Tensor, q_lens: torch.Tensor,
                   slots: torch.Tensor, k_cache: torch.Tensor,
                   v_cache: torch.Tensor, k_scale: torch.Tensor = None,
                   v_scale: torch.Tensor = None,
                   page_table: torch.Tensor = None,
                   interleaved: bool = False) -> torch.Tensor:
    """The decode prologue: per-row RoPE of q and k and the cache write of k
    and v for the new tokens of a serving step, from the packed qkv linear
    output.  Returns q [n, T, G*qpg, D], ready for `decode_attention_multi`
    (or, T = 1, `decode_attention_batched` on q[:, 0]).

    qkv: the `linear_qkv` output of n*T token rows, contiguous, viewed as
    [n, T, G, qpg+2, D] (G = num_groups, qpg = q_per_group): slots 0..qpg-1
    of a group are its q heads, slot qpg is k and slot qpg+1 is v, the layout
    of `fused_qkv_attention`.  It is not modified.  lengths, q_lens, slots:
    the int32 [n] device tensors of `decode_attention_multi`, lengths with the
    new tokens counted.  cos, sin: fp32 [rows, D/2] position tables (None:
    no rotation).  Caches, scales and page_table as in
    `decode_attention_batched`, hkv = G; scales as in `kv_cache_append`.

    Token t of row i sits at p = lengths[i] - q_lens[i] + t.  It is live when
    t < q_lens[i], slots[i] is inside the caches (the table) and
    0 <= p < min(rows, capacity), capacity = max_s or max_pages * page.  A
    live token gets its q heads rotated at p and its rotated k and its v
    stored at position p of its cache row, or of its page; when that page id
    is outside [0, P) nothing is stored.  Any other token gets a zero q row
    and stores nothing.  The rotation is fp32 with every product and sum
    rounded on its own, then rounded to the input dtype: pairs (j, j + D/2),
    or (2j, 2j + 1) when interleaved.  e4m3 caches store what
    `kv_cache_append` stores for the rotated k and for v.

    Native CDNA4 kernel on GPU bf16 with D in (64, 128)
    (decode_prologue.hip): one launch, positions, cache rows and page ids
    read on the device, nothing read back.  Elsewhere the same arithmetic in
    torch, bit for bit.
    """
    D = k_cache.shape[-1]
    if qkv.is_cuda and native_available() and qkv.dtype == torch.bfloat16 \
            and D in (64, 128) \
            and k_cache.dtype in (torch.bfloat16, torch.float8_e4m3fn):
        return get_ext().rope_kv_append(
            qkv, num_groups, q_per_group, cos, sin, lengths, q_lens, slots,
            k_cache, v_cache, k_scale, v_scale, page_table, interleaved)
    return _rope_kv_append_torch(
        qkv, num_groups, q_per_group, cos, sin, lengths, q_lens, slots,
        k_cache, v_cache, k_scale, v_scale, page_table, interleaved)


def _rope_pairs_torch(x, c, s, interleaved):
    """x [..., D] rotated by c, s (broadcastable to [..., D/2]) in fp32, each
    product and sum rounded on its own, rounded back to x's dtype."""
    d2 = x.shape[-1] // 2
    if interleaved:
        x1, x2 = x[..., 0::2].float(), x[..., 1::2].float()
        y = torch.empty_like(x, dtype=torch.float32)
        y[..., 0::2] = x1 * c - x2 * s
        y[..., 1::2] = x2 * c + x1 * s
        return y.to(x.dtype)
    x1, x2 = x[..., :d2].float(), x[..., d2:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)


def _rope_kv_append_torch(qkv, G, qpg, cos, sin, lengths, q_lens, slots,
                          k_cache, v_cache, k_scale, v_scale, page_table,
                          interleaved):
    n, D = lengths.shape[0], k_cache.shape[-1]
    x = qkv.reshape(n, -1, G, qpg + 2, D)
    T = x.shape[1]
    if page_table is None:
        S, cap = k_cache.shape[:2]
    else:
        S, cap = page_table.shape[0], page_table.shape[1] * k_cache.shape[1]
    lim = cap if cos is None else min(cap, cos.shape[0])
    t = torch.arange(T, device=qkv.device)
    sl = slots.long()[:, None].expand(n, T)
    pos = (lengths.long() - q_lens.long())[:, None] + t
    live = (t < q_lens[:, None]) & (sl >= 0) & (sl < S) & (pos >= 0) \
        & (pos < lim)
    q, k, v = x[..., :qpg, :], x[..., qpg, :], x[..., qpg + 1, :]
    if cos is not None:
        p = pos.clamp(0, lim - 1)
        c, s = cos[p].float(), sin[p].float()            # [n, T, D/2]
        q = _rope_pairs_torch(q, c[:, :, None, None], s[:, :, None, None],
                              interleaved)
        k = _rope_pairs_torch(k, c[:, :, None], s[:, :, None], interleaved)
    q = torch.where(live[:, :, None, None, None], q, torch.zeros_like(q))
    sl, pos, k, v = sl[live], pos[live], k[live], v[live]
    if page_table is not None:
        lg = k_cache.shape[1].bit_length() - 1
        sl = page_table.to(sl.device)[sl, pos >> lg].long()
        pos = pos & (k_cache.shape[1] - 1)
    _kv_cache_append_torch(k, v, k_cache, v_cache, sl, pos, k_scale, v_scale)
    return q.reshape(n, T, G * qpg, D)
