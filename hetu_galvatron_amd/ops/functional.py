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
