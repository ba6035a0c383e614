"""Packed documents take ops.fused_qkv_attention_varlen in SelfAttention:
the module on a packed batch and the whole tiny llama with
reset_attention_mask + reset_position_ids, fused dispatch on against off."""
import copy

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref
from tests.core.test_packed_documents import PACKED, _cfg

pytestmark = pytest.mark.gpu

S, B = 320, 2
CU = [0, 1, 65, 320, 577, 640]  # row 0: 1/64/255, row 1: 257/63
MAXLEN = 257
GQA = {"num_attention_heads": 4, "num_key_value_heads": 2}


def dev():
    return torch.device("cuda:0")


class Spy:
    """Counts _FusedQKVAttention.forward calls while active."""

    def __enter__(self):
        from hetu_galvatron_amd.ops import functional
        self.calls = []
        self.fn = functional._FusedQKVAttention
        self.orig = orig = self.fn.forward

        def spy(ctx, *a):
            self.calls.append(a[3] is not None)  # with cu_seqlens?
            return orig(ctx, *a)

        self.fn.forward = staticmethod(spy)
        return self

    def __exit__(self, *exc):
        self.fn.forward = staticmethod(self.orig)


def test_self_attention_packed_batch_matches_unfused():
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.runtime.transformer.attention import SelfAttention
    cfg = load_config(base={
        "model": dict(GQA, model_name="tiny-llama"),
        "parallel": {"mixed_precision": "bf16"}})
    torch.manual_seed(7)
    att = SelfAttention(cfg.model, None, None, None,
                        dtype=torch.bfloat16).to(dev())
    assert att.q_per_group == 2 and att.head_dim == 64
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.randn(S, B, cfg.model.hidden_size, generator=g) \
        .to(dev()).bfloat16()
    dy = torch.randn(S, B, cfg.model.hidden_size, generator=g) \
        .to(dev()).bfloat16()
    pos = torch.empty(B * S, dtype=torch.long)
    for lo, hi in zip(CU[:-1], CU[1:]):
        pos[lo:hi] = torch.arange(hi - lo)
    pos = pos.view(B, S).t().contiguous().to(dev())
    cos_t, sin_t = ref.rope_freqs(S, att.head_dim, device=dev())
    cos, sin = cos_t[pos].contiguous(), sin_t[pos].contiguous()
    cu = torch.tensor(CU, dtype=torch.int32, device=dev())

    out, calls = {}, {}
    for fused in (True, False):
        att.fused_qkv = fused
        att.zero_grad()
        with Spy() as spy:
            y = att(x, cos, sin, cu_seqlens=cu, max_seqlen=MAXLEN)
        y.backward(dy)
        calls[fused] = spy.calls
        out[fused] = (y.detach(), att.linear_qkv.weight.grad.clone())
    assert calls[True] == [True], "the new op runs once when switched on"
    assert calls[False] == [], "and not at all when switched off"
    assert torch.isfinite(out[True][0].float()).all()
    assert torch.equal(out[True][0], out[False][0]), \
        "layer output, fused vs not"
    a, b_ = out[True][1].float(), out[False][1].float()
    err = (a - b_).abs().max().item()
    lim = 6e-2 + 3e-2 * b_.abs().max().item()
    print(f"linear_qkv weight grad: max|err|={err:.4e} bound={lim:.4e}")
    assert err <= lim, f"linear_qkv weight grad: {err:.4e} > {lim:.4e}"


def test_whole_model_packed_step_matches_unfused():
    """One forward_backward of the tiny llama on packed documents.  Every
    layer output is bit-equal with the dispatch on and off (the test above),
    so the loss is expected to be equal, and is required to be."""
    from hetu_galvatron_amd.runtime import GalvatronModel, get_train_iterator
    from hetu_galvatron_amd.runtime.transformer.attention import SelfAttention
    data = dict(PACKED, synthetic_mean_doc_length=16)
    cfg = _cfg("tiny-llama", data, {"parallel": {"mixed_precision": "bf16"},
                                    "model": GQA})
    torch.manual_seed(0)
    model = GalvatronModel(cfg, device=dev())
    atts = [m for blk in model.stage_model.blocks for m in blk.modules()
            if isinstance(m, SelfAttention)]
    assert atts and all(a.head_dim == 64 and a.fused_qkv for a in atts)
    ctx = next(get_train_iterator(cfg, dev()))
    assert "position_ids" in ctx and "doc_boundaries" in ctx

    with Spy() as spy:
        stats = model.forward_backward(copy.copy(ctx), chunks=2)
    # (a multiple: activation recomputation would run a forward twice)
    assert len(spy.calls) >= 2 * len(atts) and all(spy.calls) \
        and len(spy.calls) % (2 * len(atts)) == 0, \
        "every layer of every microbatch takes the new op, with cu_seqlens"
    assert stats.loss == stats.loss and 0 < stats.loss < 20
    for blk in model.stage_model.blocks:
        if blk.flat is not None and blk.flat.flat_grad is not None:
            assert torch.isfinite(blk.flat.flat_grad).all()

    for a in atts:
        a.fused_qkv = False
    with Spy() as spy:
        unfused = model.forward_backward(copy.copy(ctx), chunks=2)
    assert spy.calls == []
    assert stats.loss == unfused.loss, \
        f"loss {stats.loss!r} vs {unfused.loss!r} with the dispatch off"
