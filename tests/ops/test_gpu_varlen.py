"""Packed-document (cu_seqlens) flash attention kernels on the GPU.

Shape b=2, s=1024.  Row 0 packs seven segments whose lengths hit every
path of the 256-row work mapping and whose start offsets are odd, row 1 is
one full-length segment:

    length  start  exercises
         1      0  single token
        31      1  below one wave's 32 rows
        64     32  exactly one KV tile
        65     96  a tail of 1
       256    161  exactly one q block
       257    417  a second q block with 1 row
       350    674  two blocks with a partial tail

The oracle is ops/reference_ops.attention_varlen_fwd/bwd (checked on the CPU
against an independent block-diagonal mask in test_varlen_reference.py);
tolerances and the assert_close formula are the dense flash tests'.
"""
import math

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref

pytestmark = pytest.mark.gpu

B, S = 2, 1024
LENS0 = [1, 31, 64, 65, 256, 257, 350]
CU = [0, 1, 32, 96, 161, 417, 674, 1024, 2048]
MAXLEN = 1024
POISON = (96, 161)  # the 65-token segment

PARAMS = [(d, hq, hkv, causal, sbhd)
          for d in (64, 128) for hq, hkv in ((8, 8), (8, 2))
          for causal in (True, False) for sbhd in (False, True)]
IDS = [f"d{d}-h{hq}_{hkv}-{'causal' if c else 'full'}-"
       f"{'sbhd' if l else 'bshd'}" for d, hq, hkv, c, l in PARAMS]


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def dev():
    return torch.device("cuda:0")


def assert_close(a, b, atol, rtol=2e-2, what=""):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs().max().item()
    denom = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * denom, \
        f"{what}: max|err|={err:.4e} vs atol={atol} rtol*max={rtol * denom:.4e}"


def lay(t, sbhd):
    """[b,s,h,d] data -> the layout under test."""
    return t.permute(1, 0, 2, 3).contiguous() if sbhd else t


def tokens(t, sbhd):
    """layout under test -> token-major [b*s, ...] view for row selection."""
    if sbhd:
        t = t.permute(1, 0, 2, 3)
    return t.reshape(B * S, *t.shape[2:])


def cu_dev(cu=CU):
    return torch.tensor(cu, dtype=torch.int32, device=dev())


_INPUTS = {}


def inputs(d, hq, hkv, sbhd):
    """q/k/v/dout drawn with different scales (a q<->k or k<->v mix-up
    cannot pass); one draw per (d, heads), shared by both layouts."""
    key = (d, hq, hkv)
    if key not in _INPUTS:
        g = torch.Generator(device="cpu").manual_seed(1000 + d + hkv)
        q = torch.randn(B, S, hq, d, generator=g)
        k = torch.randn(B, S, hkv, d, generator=g) * 0.7
        v = torch.randn(B, S, hkv, d, generator=g) * 1.3
        do = torch.randn(B, S, hq, d, generator=g) * 0.9
        _INPUTS[key] = tuple(t.to(dev()).bfloat16() for t in (q, k, v, do))
    return tuple(lay(t, sbhd) for t in _INPUTS[key])


_REF = {}


def reference(d, hq, hkv, causal):
    """fp32 oracle (bshd), computed once per case and never modified."""
    key = (d, hq, hkv, causal)
    if key not in _REF:
        q, k, v, do = (t.float() for t in inputs(d, hq, hkv, False))
        scale = 1.0 / math.sqrt(d)
        o, lse = ref.attention_varlen_fwd(q, k, v, CU, MAXLEN, causal, scale)
        dq, dk, dv = ref.attention_varlen_bwd(do, q, k, v, o, lse, CU,
                                              MAXLEN, causal, scale)
        _REF[key] = (o, lse, dq, dk, dv)
    return _REF[key]


def run_native(q, k, v, do, cu, maxlen, causal, sbhd):
    scale = 1.0 / math.sqrt(q.shape[-1])
    o, lse = ext().flash_attn_varlen_fwd(q, k, v, cu, maxlen, causal, scale,
                                         sbhd)
    dq, dk, dv = ext().flash_attn_varlen_bwd(do, q, k, v, o, lse, cu, maxlen,
                                             causal, scale, sbhd)
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("d,hq,hkv,causal,sbhd", PARAMS, ids=IDS)
def test_varlen_numerics(d, hq, hkv, causal, sbhd):
    q, k, v, do = inputs(d, hq, hkv, sbhd)
    o, lse, dq, dk, dv = run_native(q, k, v, do, cu_dev(), MAXLEN, causal,
                                    sbhd)
    o_r, lse_r, dq_r, dk_r, dv_r = reference(d, hq, hkv, causal)
    assert o.shape == q.shape and lse.shape == (B, hq, S)
    assert dk.shape == k.shape and dv.shape == v.shape
    assert_close(o, lay(o_r, sbhd), 3e-2, what="varlen o")
    assert_close(lse, lse_r, 2e-2, what="varlen lse")
    assert_close(dq, lay(dq_r, sbhd), 6e-2, rtol=3e-2, what="varlen dq")
    assert_close(dk, lay(dk_r, sbhd), 6e-2, rtol=3e-2, what="varlen dk")
    assert_close(dv, lay(dv_r, sbhd), 6e-2, rtol=3e-2, what="varlen dv")


@pytest.mark.parametrize("d,hq,hkv,causal,sbhd", PARAMS, ids=IDS)
def test_varlen_one_segment_per_row_equals_dense(d, hq, hkv, causal, sbhd):
    """Same block bodies, same tile order -> bit-identical to the dense
    kernels when every row is one segment."""
    q, k, v, do = inputs(d, hq, hkv, sbhd)
    scale = 1.0 / math.sqrt(d)
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=dev())
    o_d, lse_d = ext().flash_attn_fwd(q, k, v, causal, scale, None, sbhd)
    o, lse = ext().flash_attn_varlen_fwd(q, k, v, cu, S, causal, scale, sbhd)
    assert torch.equal(o, o_d), "o differs from the dense kernel"
    assert torch.equal(lse, lse_d), "lse differs from the dense kernel"
    g_d = ext().flash_attn_bwd(do, q, k, v, o_d, lse_d, causal, scale, None,
                               sbhd)
    g = ext().flash_attn_varlen_bwd(do, q, k, v, o_d, lse_d, cu, S, causal,
                                    scale, sbhd)
    for name, a, b_ in zip(("dq", "dk", "dv"), g, g_d):
        assert torch.equal(a, b_), f"{name} differs from the dense kernel"


@pytest.mark.parametrize("d,hq,hkv,causal,sbhd", PARAMS, ids=IDS)
def test_varlen_isolation_nan_poison(d, hq, hkv, causal, sbhd):
    """NaN in one segment's q/k/v/dout must not reach any other segment: a
    masked-but-loaded NaN enters the MFMA as 0*NaN, so any out-of-segment
    read shows up."""
    q, k, v, do = inputs(d, hq, hkv, sbhd)
    clean = run_native(q, k, v, do, cu_dev(), MAXLEN, causal, sbhd)
    lo, hi = POISON
    poisoned = [t.clone() for t in (q, k, v, do)]
    for t in poisoned:
        if sbhd:
            t[lo:hi, 0] = float("nan")
        else:
            t[0, lo:hi] = float("nan")
    dirty = run_native(*poisoned, cu_dev(), MAXLEN, causal, sbhd)
    keep = torch.ones(B * S, dtype=torch.bool, device=dev())
    keep[lo:hi] = False
    for name, a, b_ in zip(("o", "lse", "dq", "dk", "dv"), dirty, clean):
        if name == "lse":  # [b, hq, s] -> token-major [b*s, hq]
            a, b_ = (t.permute(0, 2, 1).reshape(B * S, -1) for t in (a, b_))
        else:
            a, b_ = tokens(a, sbhd), tokens(b_, sbhd)
        assert torch.isfinite(a[keep].float()).all(), \
            f"{name}: NaN leaked out of the poisoned segment"
        assert torch.equal(a[keep], b_[keep]), \
            f"{name}: other segments changed when one was poisoned"


@pytest.mark.parametrize("d,hq,hkv,causal,sbhd", PARAMS, ids=IDS)
def test_varlen_empty_segment(d, hq, hkv, causal, sbhd):
    q, k, v, do = inputs(d, hq, hkv, sbhd)
    cu_dup = [0, 0, 1, 32, 32, 96, 161, 417, 674, 1024, 1024, 2048, 2048]
    a = run_native(q, k, v, do, cu_dev(), MAXLEN, causal, sbhd)
    b_ = run_native(q, k, v, do, cu_dev(cu_dup), MAXLEN, causal, sbhd)
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), a, b_):
        assert torch.equal(x, y), f"{name} changed with empty segments"


@pytest.mark.parametrize("d,hq,hkv,causal,sbhd", PARAMS, ids=IDS)
def test_varlen_autograd_matches_bindings(d, hq, hkv, causal, sbhd):
    from hetu_galvatron_amd.ops import flash_attention_varlen
    q, k, v, do = inputs(d, hq, hkv, sbhd)
    want = run_native(q, k, v, do, cu_dev(), MAXLEN, causal, sbhd)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    # host cu_seqlens: validated, then copied asynchronously
    o, lse = flash_attention_varlen(
        qa, ka, va, torch.tensor(CU, dtype=torch.int32), MAXLEN,
        causal=causal, return_lse=True, sbhd=sbhd)
    o.backward(do)
    got = (o, lse, qa.grad, ka.grad, va.grad)
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), got, want):
        assert torch.equal(x.detach(), y), f"{name}: autograd vs bindings"


def test_varlen_binding_checks():
    q, k, v, do = inputs(64, 8, 2, False)
    scale = 0.125
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        ext().flash_attn_varlen_fwd(q, k, v, cu_dev().long(), MAXLEN, True,
                                    scale)
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        ext().flash_attn_varlen_fwd(q, k, v, cu_dev().cpu(), MAXLEN, True,
                                    scale)
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        ext().flash_attn_varlen_fwd(q, k, v, cu_dev()[:1], MAXLEN, True,
                                    scale)
    for bad in (0, S + 1):
        with pytest.raises(RuntimeError, match="max_seqlen"):
            ext().flash_attn_varlen_fwd(q, k, v, cu_dev(), bad, True, scale)
    with pytest.raises(RuntimeError, match="bf16"):
        ext().flash_attn_varlen_fwd(q.float(), k.float(), v.float(),
                                    cu_dev(), MAXLEN, True, scale)
