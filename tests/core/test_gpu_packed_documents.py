"""Packed documents on the GPU: the runtime path over the native kernels
(varlen flash attention in sbhd layout, per-row RoPE through the existing
rope kernel)."""
import copy

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref
from hetu_galvatron_amd.runtime.dataloader import build_batch_context
from tests.core.test_packed_documents import (
    EOD, PACKED, SPLIT, _cfg, _logits, _two_doc_tokens)

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def test_per_row_rope_runs_the_hip_kernel():
    """cos/sin [s, b, d/2]: x viewed as [s*b, 1, h, d] with a [s*b, d/2]
    table goes through rope_kernel unchanged; fwd and bwd vs the fp32
    batched reference at the dense rope test's bf16 tolerance (2e-2)."""
    from hetu_galvatron_amd.runtime.transformer.rope import apply_rope_qk
    torch.manual_seed(21)
    s, b, hq, hkv, d = 96, 3, 4, 2, 128
    # positions restart at different places in every row
    pos = torch.stack([torch.cat([torch.arange(c), torch.arange(s - c)])
                       for c in (1, 37, 96)], dim=1).to(dev())  # [s, b]
    cos_t, sin_t = ref.rope_freqs(s, d, device=dev())
    cos, sin = cos_t[pos].contiguous(), sin_t[pos].contiguous()
    q = torch.randn(s, b, hq, d, device=dev()).bfloat16().requires_grad_(True)
    k = (torch.randn(s, b, hkv, d, device=dev()) * 0.7).bfloat16() \
        .requires_grad_(True)
    wq, wk = torch.randn_like(q), torch.randn_like(k)
    yq, yk = apply_rope_qk(q, k, cos, sin)
    assert yq.shape == q.shape and yk.shape == k.shape
    (yq.float() * wq.float()).sum().add((yk.float() * wk.float()).sum()) \
        .backward()
    q32 = q.detach().float().requires_grad_(True)
    k32 = k.detach().float().requires_grad_(True)
    rq = ref.rope_apply_neox_batched(q32, cos, sin)
    rk = ref.rope_apply_neox_batched(k32, cos, sin)
    (rq * wq.float()).sum().add((rk * wk.float()).sum()).backward()
    for name, a, b_ in (("q", yq, rq), ("k", yk, rk),
                        ("dq", q.grad, q32.grad), ("dk", k.grad, k32.grad)):
        err = (a.float() - b_).abs().max().item()
        lim = 2e-2 + 2e-2 * b_.abs().max().item()
        assert err <= lim, f"per-row rope {name}: {err:.3e} > {lim:.3e}"


def _gpu_model(cfg):
    from hetu_galvatron_amd.runtime import GalvatronModel
    torch.manual_seed(0)
    return GalvatronModel(cfg, device=dev())


def test_document_isolation_bf16_native():
    """tiny llama, bf16, native kernels: rewriting document A must leave
    document B's logits alone.  Every op besides attention works row by row
    and the varlen kernel never reads across a boundary, so the expected
    difference is zero; the bound leaves room for two bf16 ulps of a
    logit below 2 (2 * 2^-7) in case a GEMM reduces in a different order."""
    cfg = _cfg("tiny-llama", PACKED, {"parallel": {"mixed_precision": "bf16"}})
    model = _gpu_model(cfg).eval()
    t1 = _two_doc_tokens(1)
    t2 = t1.clone()
    t2[:, :SPLIT - 1] = _two_doc_tokens(2)[:, :SPLIT - 1]
    on = dict(eod_token=EOD, reset_attention_mask=True,
              reset_position_ids=True)
    l1 = _logits(model, build_batch_context(t1, dev(), **on))
    l2 = _logits(model, build_batch_context(t2, dev(), **on))
    assert torch.isfinite(l1).all() and l1.abs().max() < 2.0
    assert (l1[:SPLIT] - l2[:SPLIT]).abs().max() > 1e-3, "doc A did change"
    leak = (l1[SPLIT:] - l2[SPLIT:]).abs().max().item()
    assert leak <= 2 * 2 ** -7, f"document B saw document A: {leak:.3e}"


def test_packed_training_step_bf16_native():
    from hetu_galvatron_amd.runtime import get_train_iterator
    data = dict(PACKED, synthetic_mean_doc_length=16)
    cfg = _cfg("tiny-llama", data, {"parallel": {"mixed_precision": "bf16"}})
    model = _gpu_model(cfg)
    ctx = next(get_train_iterator(cfg, dev()))
    assert ctx["position_ids"].is_cuda and "doc_boundaries" in ctx
    stats = model.forward_backward(copy.copy(ctx), chunks=2)
    assert stats.loss == stats.loss and 0 < stats.loss < 20
    for blk in model.stage_model.blocks:
        if blk.flat is not None and blk.flat.flat_grad is not None:
            assert torch.isfinite(blk.flat.flat_grad).all()
