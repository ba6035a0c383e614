"""ops.fused_qkv_attention: RoPE + flash attention on the packed linear_qkv
buffer [s, b, G, qpg+2, d], against today's composition (slice, apply_rope,
flash_attention) on the same inputs and the same dout.

Two shapes:
  SMALL  s=320, b=2, G=2: one full 256-row q block plus a 64-row tail, so
         the partial-tile path and the batch stride are hit.  b*hq is far
         below the launchers' pairing threshold, so every block runs alone
         (pass 0 only).
  PAIRED s=576, b=2, hq=64, causal: three q blocks (256, 256, 64-row tail)
         and ceil(3/2) * b * hq = 256 workgroups, exactly the threshold at
         which the launchers switch to complementary-pair scheduling.  Block
         0 then also runs its partner, block 2 (the tail), in a second pass;
         block 1 is its own partner and stops after the first.  This is the
         path the flagship takes: the forward's inlined two-pass loop and
         the second call sites of dq and dkv.

o, lse, the v slot of the rotated buffer and the q slots of dqkv must be
bit-identical to the composition (same block bodies, same tile order, same
RoPE arithmetic).  The k and v slots of dqkv may differ from it only in the
fp32 order of the GQA group sum, so they use the dense flash tests'
assert_close formula and tolerances, against the composition and against an
fp32 reference_ops oracle.
"""
import math

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref

pytestmark = pytest.mark.gpu

SMALL = (320, 2, 2)  # s, b, G

PARAMS = [(d, qpg, causal, rope)
          for d in (64, 128) for qpg in (1, 4)
          for causal in (True, False) for rope in (True, False)]
IDS = [f"d{d}-qpg{qpg}-{'causal' if c else 'full'}-{'rope' if r else 'norope'}"
       for d, qpg, c, r in PARAMS]

PAIRED_S, PAIRED_B, PAIRED_HQ = 576, 2, 64
PAIRED_PARAMS = [(d, qpg) for d in (64, 128) for qpg in (1, 4)]
PAIRED_IDS = [f"d{d}-qpg{qpg}" for d, qpg in PAIRED_PARAMS]


def is_paired(s, b, hq, causal):
    """The launchers' rule (flash_packed_fwd_launch_d / _bwd_launch_d)."""
    nqb = (s + 255) // 256
    return causal and ((nqb + 1) // 2) * b * hq >= 256


def dev():
    return torch.device("cuda:0")


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def assert_close(a, b, atol, rtol=2e-2, what=""):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs().max().item()
    denom = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * denom, \
        f"{what}: max|err|={err:.4e} vs atol={atol} rtol*max={rtol * denom:.4e}"


def assert_equal(a, b, what):
    if not torch.equal(a, b):
        diff = (a.float() - b.float()).abs()
        raise AssertionError(
            f"{what}: {int((diff > 0).sum())} of {diff.numel()} elements "
            f"differ, max|diff|={diff.max().item():.4e}")


_INPUTS = {}


def inputs(shape, d, qpg):
    """qkv with q, k and v drawn at different scales (a slot mix-up cannot
    pass), dout, and the NEOX tables; one draw per (shape, d, qpg)."""
    key = (shape, d, qpg)
    if key not in _INPUTS:
        S, B, G = shape
        g = torch.Generator(device="cpu").manual_seed(4000 + d + qpg + S)
        qkv = torch.randn(S, B, G, qpg + 2, d, generator=g)
        qkv[:, :, :, qpg] *= 0.7
        qkv[:, :, :, qpg + 1] *= 1.3
        do = torch.randn(S, B, G * qpg, d, generator=g) * 0.9
        cos, sin = ref.rope_freqs(S, d, device=dev())
        _INPUTS[key] = (qkv.to(dev()).bfloat16(), do.to(dev()).bfloat16(),
                        cos, sin)
    return _INPUTS[key]


def split(x, qpg):
    S, B, d = x.shape[0], x.shape[1], x.shape[-1]
    return (x[:, :, :, :qpg].reshape(S, B, -1, d),
            x[:, :, :, qpg].reshape(S, B, -1, d),
            x[:, :, :, qpg + 1].reshape(S, B, -1, d))


def composition(shape, d, qpg, causal, rope):
    """Today's native path: slice, apply_rope, flash_attention(sbhd)."""
    from hetu_galvatron_amd.ops import apply_rope, flash_attention
    qkv, do, cos, sin = inputs(shape, d, qpg)
    x = qkv.clone().requires_grad_(True)
    q, k, v = split(x, qpg)
    q, k = q.contiguous(), k.contiguous()
    if rope:
        q, k = apply_rope(q, cos, sin), apply_rope(k, cos, sin)
    o, lse = flash_attention(q, k, v.contiguous(), causal=causal,
                             return_lse=True, sbhd=True)
    o.backward(do)
    return o.detach(), lse.detach(), x.grad, q.detach(), k.detach()


_REF = {}


def reference(shape, d, qpg, causal, rope):
    """fp32 reference_ops oracle for dqkv, through autograd; computed once
    per case and never modified."""
    key = (shape, d, qpg, causal, rope)
    if key not in _REF:
        qkv, do, cos, sin = inputs(shape, d, qpg)
        x = qkv.float().requires_grad_(True)
        q, k, v = split(x, qpg)
        if rope:
            q, k = ref.rope_apply(q, cos, sin), ref.rope_apply(k, cos, sin)
        o, _ = ref.attention_fwd(q.permute(1, 0, 2, 3), k.permute(1, 0, 2, 3),
                                 v.permute(1, 0, 2, 3), causal,
                                 1.0 / math.sqrt(d))
        o.permute(1, 0, 2, 3).backward(do.float())
        _REF[key] = x.grad
    return _REF[key]


def check_against_composition(shape, d, qpg, causal, rope):
    from hetu_galvatron_amd.ops import fused_qkv_attention
    S, B, G = shape
    qkv, do, cos, sin = inputs(shape, d, qpg)
    o_c, lse_c, dqkv_c, q_rot, k_rot = composition(shape, d, qpg, causal,
                                                   rope)

    x = qkv.clone().requires_grad_(True)
    buf = x.clone()  # the op consumes its input: not a leaf
    o = fused_qkv_attention(buf, cos if rope else None,
                            sin if rope else None, G, qpg, causal=causal)
    assert o.shape == (S, B, G * qpg, d)
    assert_equal(o.detach(), o_c, "o vs composition")
    # buf now holds the rotated buffer
    buf = buf.detach()
    qf, kf, vf = split(buf, qpg)
    assert_equal(vf, split(qkv, qpg)[2], "v slot after the op vs input")
    assert_equal(qf, q_rot, "rotated q vs composition")
    assert_equal(kf, k_rot, "rotated k vs composition")
    o2, lse = ext().flash_attn_qkv_fwd(buf, causal, 1.0 / math.sqrt(d))
    assert_equal(o2, o_c, "packed forward binding o vs composition")
    assert_equal(lse, lse_c, "lse vs composition")

    o.backward(do)
    dqkv = x.grad
    assert dqkv.shape == qkv.shape
    assert torch.isfinite(dqkv.float()).all(), "non-finite values in dqkv"
    dq, dk, dv = split(dqkv, qpg)
    dq_c, dk_c, dv_c = split(dqkv_c, qpg)
    dq_r, dk_r, dv_r = split(reference(shape, d, qpg, causal, rope), qpg)
    assert_equal(dq, dq_c, "dqkv q slots vs composition")
    assert_close(dq, dq_r, 6e-2, rtol=3e-2, what="dq vs reference")
    for name, a, c, r in (("dk", dk, dk_c, dk_r), ("dv", dv, dv_c, dv_r)):
        err_c = (a.float() - c.float()).abs().max().item()
        err_r = (a.float() - r).abs().max().item()
        print(f"{name}: max|fused-composition|={err_c:.4e} "
              f"max|fused-reference|={err_r:.4e} max|ref|={r.abs().max():.4e}")
        assert_close(a, c, 6e-2, rtol=3e-2, what=f"{name} vs composition")
        assert_close(a, r, 6e-2, rtol=3e-2, what=f"{name} vs reference")


@pytest.mark.parametrize("d,qpg,causal,rope", PARAMS, ids=IDS)
def test_fused_qkv_matches_composition(d, qpg, causal, rope):
    assert not is_paired(SMALL[0], SMALL[1], SMALL[2] * qpg, causal)
    check_against_composition(SMALL, d, qpg, causal, rope)


@pytest.mark.parametrize("d,qpg", PAIRED_PARAMS, ids=PAIRED_IDS)
def test_fused_qkv_paired_causal(d, qpg):
    """Complementary-pair scheduling: both passes of the forward loop, the
    partner index, the self-partnered middle block and the second call
    sites of dq and dkv."""
    assert is_paired(PAIRED_S, PAIRED_B, PAIRED_HQ, True)
    shape = (PAIRED_S, PAIRED_B, PAIRED_HQ // qpg)
    check_against_composition(shape, d, qpg, True, True)


def test_fused_qkv_binding_checks():
    qkv, do, cos, sin = inputs(SMALL, 64, 4)
    with pytest.raises(RuntimeError, match="qkv must be"):
        ext().flash_attn_qkv_fwd(qkv.float(), True, 0.125)
    with pytest.raises(RuntimeError, match="qkv must be"):
        ext().flash_attn_qkv_fwd(qkv[:, :, :, :2].contiguous(), True, 0.125)
    with pytest.raises(RuntimeError, match="head dim"):
        ext().flash_attn_qkv_fwd(qkv[..., :32].contiguous(), True, 0.125)
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().rope_qkv_(qkv.clone(), cos[:-1].contiguous(),
                        sin[:-1].contiguous())
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().rope_qkv_(qkv.clone(), cos.double(), sin.double())


def test_self_attention_dispatch_matches_unfused():
    """SelfAttention on the plain local path takes the fused op (at a shape
    that pairs); output and the linear_qkv weight gradient against the same
    module with the fused path switched off."""
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.ops import functional
    from hetu_galvatron_amd.runtime.transformer.attention import SelfAttention
    cfg = load_config(base={
        "model": {"model_name": "tiny-llama", "num_attention_heads": 4,
                  "num_key_value_heads": 2},
        "parallel": {"mixed_precision": "bf16"}})
    torch.manual_seed(7)
    att = SelfAttention(cfg.model, None, None, None,
                        dtype=torch.bfloat16).to(dev())
    assert att.q_per_group == 2 and att.head_dim == 64
    S, B = PAIRED_S, 32  # 4 heads: 2 * 32 * 4 = 256 workgroups, paired
    assert is_paired(S, B, att.heads_local, att.causal)
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.randn(S, B, cfg.model.hidden_size, generator=g) \
        .to(dev()).bfloat16()
    dy = torch.randn(S, B, cfg.model.hidden_size, generator=g) \
        .to(dev()).bfloat16()
    cos, sin = ref.rope_freqs(S, att.head_dim, device=dev())

    calls = []
    orig = functional._FusedQKVAttention.forward

    def spy(ctx, *a):
        calls.append(1)
        return orig(ctx, *a)

    out = {}
    for fused in (True, False):
        att.fused_qkv = fused
        att.zero_grad()
        functional._FusedQKVAttention.forward = staticmethod(spy)
        try:
            y = att(x, cos, sin)
        finally:
            functional._FusedQKVAttention.forward = staticmethod(orig)
        y.backward(dy)
        out[fused] = (y.detach(), att.linear_qkv.weight.grad.clone())
    assert len(calls) == 1, "the fused op ran exactly when switched on"
    assert_equal(out[True][0], out[False][0], "layer output, fused vs not")
    assert_close(out[True][1], out[False][1], 6e-2, rtol=3e-2,
                 what="linear_qkv weight grad")
