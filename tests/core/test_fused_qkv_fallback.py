"""ops.fused_qkv_attention off the native path (CPU, fp32): the fallback is
the composition of slice, apply_rope and flash_attention that SelfAttention
ran before the fused op existed, so one forward and backward of the layer
is bit-identical with the fused dispatch on and off."""
import pytest
import torch

from hetu_galvatron_amd.config import load_config
from hetu_galvatron_amd.ops import fused_qkv_attention
from hetu_galvatron_amd.ops import reference_ops as ref
from hetu_galvatron_amd.runtime.transformer.attention import SelfAttention


def _attention(model_name, extra=None):
    model = {"model_name": model_name}
    model.update(extra or {})
    cfg = load_config(base={"model": model,
                            "parallel": {"mixed_precision": "fp32"}})
    torch.manual_seed(3)
    return cfg, SelfAttention(cfg.model, None, None, None,
                              dtype=torch.float32)


def _run(att, x, dy, cos, sin, fused):
    att.fused_qkv = fused
    att.zero_grad()
    xi = x.clone().requires_grad_(True)
    y = att(xi, cos, sin)
    y.backward(dy)
    return [y.detach(), xi.grad] + [p.grad.clone() for p in att.parameters()]


@pytest.mark.parametrize("model_name,extra,rope", [
    ("tiny-llama", {"num_attention_heads": 4, "num_key_value_heads": 2},
     True),
    ("tiny-llama", None, True),
    ("tiny-llama", {"sliding_window": 5}, True),
    ("tiny-gpt", None, False),
], ids=["gqa", "mha", "window", "norope"])
def test_fallback_equals_composition_bitwise(model_name, extra, rope):
    cfg, att = _attention(model_name, extra)
    s, b = 24, 2
    g = torch.Generator().manual_seed(11)
    x = torch.randn(s, b, cfg.model.hidden_size, generator=g)
    dy = torch.randn(s, b, cfg.model.hidden_size, generator=g)
    cos, sin = ref.rope_freqs(s, att.head_dim) if rope else (None, None)
    want = _run(att, x, dy, cos, sin, fused=False)
    got = _run(att, x, dy, cos, sin, fused=True)
    assert len(got) == len(want) >= 4
    for i, (a, w) in enumerate(zip(got, want)):
        assert torch.equal(a, w), f"tensor {i} differs with the fused dispatch"


def test_fallback_leaves_its_input_alone():
    s, b, G, qpg, d = 8, 1, 2, 2, 16
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(s, b, G * (qpg + 2) * d, generator=g)
    keep = qkv.clone()
    cos, sin = ref.rope_freqs(s, d)
    o = fused_qkv_attention(qkv, cos, sin, G, qpg)
    assert o.shape == (s, b, G * qpg, d)
    assert torch.equal(qkv, keep)
    with pytest.raises(ValueError, match="cos/sin"):
        fused_qkv_attention(qkv, cos[:, None].expand(s, b, d // 2),
                            sin[:, None].expand(s, b, d // 2), G, qpg)
