"""ops.fused_qkv_attention_varlen off the native path (CPU, fp32): the
fallback is the composition of slice, apply_rope_qk and
flash_attention_varlen / flash_attention that SelfAttention runs for packed
documents with the fused dispatch off, so the op and one forward and
backward of the layer are bit-identical either way."""
import pytest
import torch

from hetu_galvatron_amd.config import load_config
from hetu_galvatron_amd.ops import (flash_attention, flash_attention_varlen,
                                    fused_qkv_attention_varlen)
from hetu_galvatron_amd.ops import reference_ops as ref
from hetu_galvatron_amd.runtime.transformer.attention import SelfAttention
from hetu_galvatron_amd.runtime.transformer.rope import apply_rope_qk

S, B, G, QPG, D = 24, 2, 2, 2, 16
CU = [0, 1, 8, 24, 37, 37, 48]  # row 0: 1/7/16, row 1: 13/empty/11
MAXLEN = 16


def _tables(kind, s=S, b=B, d=D, cu=CU):
    """None, [s, d/2], or [s, b, d/2] with positions restarting per segment."""
    if kind == "none":
        return None, None
    cos, sin = ref.rope_freqs(s, d)
    if kind == "plain":
        return cos, sin
    pos = torch.empty(b * s, dtype=torch.long)
    for lo, hi in zip(cu[:-1], cu[1:]):
        pos[lo:hi] = torch.arange(hi - lo)
    pos = pos.view(b, s).t()  # [s, b]
    return cos[pos].contiguous(), sin[pos].contiguous()


def _composition(qkv, cos, sin, cu, causal):
    x = qkv.clone().requires_grad_(True)
    p = x.view(S, B, G, QPG + 2, D)
    q = p[:, :, :, :QPG].reshape(S, B, -1, D)
    k = p[:, :, :, QPG].reshape(S, B, -1, D)
    v = p[:, :, :, QPG + 1].reshape(S, B, -1, D)
    q, k = apply_rope_qk(q.contiguous(), k.contiguous(), cos, sin)
    if cu is None:
        o = flash_attention(q, k, v.contiguous(), causal=causal, sbhd=True)
    else:
        o = flash_attention_varlen(q, k, v.contiguous(), cu, MAXLEN,
                                   causal=causal, sbhd=True)
    return o, x


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("packed", [True, False], ids=["cu", "nocu"])
@pytest.mark.parametrize("kind", ["none", "plain", "rows"])
def test_fallback_equals_composition_bitwise(kind, packed, causal):
    g = torch.Generator().manual_seed(21)
    qkv = torch.randn(S, B, G * (QPG + 2) * D, generator=g)
    do = torch.randn(S, B, G * QPG, D, generator=g)
    cos, sin = _tables(kind)
    cu = torch.tensor(CU, dtype=torch.int32) if packed else None
    o_c, x_c = _composition(qkv, cos, sin, cu, causal)
    o_c.backward(do)

    x = qkv.clone().requires_grad_(True)
    keep = x.detach().clone()
    o = fused_qkv_attention_varlen(x, cos, sin, G, QPG, cu_seqlens=cu,
                                   max_seqlen=MAXLEN if packed else None,
                                   causal=causal)
    assert o.shape == (S, B, G * QPG, D)
    assert torch.equal(x.detach(), keep), "the fallback changed its input"
    o.backward(do)
    assert torch.equal(o.detach(), o_c.detach()), "o differs"
    assert torch.equal(x.grad, x_c.grad), "qkv.grad differs"
    if packed and kind == "rows":
        # the segments matter: the unsegmented result is another one
        o_d, _ = _composition(qkv, cos, sin, None, causal)
        assert not torch.equal(o.detach(), o_d.detach())


@pytest.mark.parametrize("cu", [
    [0, 8, 24, 40],          # does not reach b*s
    [0, 8, 30, 48],          # [8, 30) straddles row 0 / row 1
    [1, 24, 48],             # does not start at 0
    [0, 24, 20, 48],         # decreases
], ids=["short", "straddle", "start", "decrease"])
def test_bad_host_cu_seqlens_raise(cu):
    qkv = torch.randn(S, B, G * (QPG + 2) * D)
    with pytest.raises(ValueError):
        fused_qkv_attention_varlen(
            qkv, None, None, G, QPG,
            cu_seqlens=torch.tensor(cu, dtype=torch.int32), max_seqlen=S)


def test_cu_seqlens_argument_checks():
    qkv = torch.randn(S, B, G * (QPG + 2) * D)
    good = torch.tensor(CU, dtype=torch.int32)
    with pytest.raises(ValueError, match="int32"):
        fused_qkv_attention_varlen(qkv, None, None, G, QPG,
                                   cu_seqlens=good.long(), max_seqlen=MAXLEN)
    with pytest.raises(ValueError, match="1-D"):
        fused_qkv_attention_varlen(qkv, None, None, G, QPG,
                                   cu_seqlens=good[None], max_seqlen=MAXLEN)
    with pytest.raises(ValueError, match="max_seqlen"):
        fused_qkv_attention_varlen(qkv, None, None, G, QPG, cu_seqlens=good,
                                   max_seqlen=MAXLEN - 1)
    cos, sin = ref.rope_freqs(S, D)
    with pytest.raises(ValueError, match="cos/sin"):
        fused_qkv_attention_varlen(qkv, cos[None, None], sin[None, None], G,
                                   QPG)


def _attention(extra=None):
    model = {"model_name": "tiny-llama", "num_attention_heads": 4,
             "num_key_value_heads": 2}
    model.update(extra or {})
    cfg = load_config(base={"model": model,
                            "parallel": {"mixed_precision": "fp32"}})
    torch.manual_seed(3)
    return cfg, SelfAttention(cfg.model, None, None, None,
                              dtype=torch.float32)


def _run(att, x, dy, cos, sin, cu, maxlen, fused):
    att.fused_qkv = fused
    att.zero_grad()
    xi = x.clone().requires_grad_(True)
    y = att(xi, cos, sin, cu_seqlens=cu, max_seqlen=maxlen)
    y.backward(dy)
    return [y.detach(), xi.grad] + [p.grad.clone() for p in att.parameters()]


@pytest.mark.parametrize("packed", [True, False], ids=["cu", "rows-only"])
def test_self_attention_packed_batch_bitwise(packed):
    cfg, att = _attention()
    g = torch.Generator().manual_seed(22)
    x = torch.randn(S, B, cfg.model.hidden_size, generator=g)
    dy = torch.randn(S, B, cfg.model.hidden_size, generator=g)
    cos, sin = _tables("rows", d=att.head_dim)
    cu = torch.tensor(CU, dtype=torch.int32) if packed else None
    maxlen = MAXLEN if packed else None
    want = _run(att, x, dy, cos, sin, cu, maxlen, fused=False)
    got = _run(att, x, dy, cos, sin, cu, maxlen, fused=True)
    assert len(got) == len(want) >= 4
    for i, (a, w) in enumerate(zip(got, want)):
        assert torch.equal(a, w), f"tensor {i} differs with the fused dispatch"


def test_self_attention_takes_the_new_op(monkeypatch):
    """The packed batch goes through ops.fused_qkv_attention_varlen exactly
    when the fused dispatch is on."""
    from hetu_galvatron_amd.runtime.transformer import attention as mod
    cfg, att = _attention()
    calls = []
    orig = mod.fused_qkv_attention_varlen

    def spy(*a, **kw):
        calls.append(kw.get("cu_seqlens") is not None)
        return orig(*a, **kw)

    monkeypatch.setattr(mod, "fused_qkv_attention_varlen", spy)
    x = torch.randn(S, B, cfg.model.hidden_size)
    cos, sin = _tables("rows", d=att.head_dim)
    cu = torch.tensor(CU, dtype=torch.int32)
    att(x, cos, sin, cu_seqlens=cu, max_seqlen=MAXLEN)
    att(x, cos, sin)
    assert calls == [True, False]
    att.fused_qkv = False
    att(x, cos, sin, cu_seqlens=cu, max_seqlen=MAXLEN)
    assert len(calls) == 2


def test_cu_seqlens_with_sliding_window_still_refused():
    cfg, att = _attention({"sliding_window": 5})
    x = torch.randn(S, B, cfg.model.hidden_size)
    cos, sin = _tables("rows", d=att.head_dim)
    cu = torch.tensor(CU, dtype=torch.int32)
    for fused in (True, False):
        att.fused_qkv = fused
        with pytest.raises(RuntimeError, match="packed-document"):
            att(x, cos, sin, cu_seqlens=cu, max_seqlen=MAXLEN)
