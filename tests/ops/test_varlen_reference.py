"""Packed-document (cu_seqlens) attention: the fp32 reference ops.

attention_varlen_fwd/bwd are the CPU execution path of
flash_attention_varlen AND the oracle of the GPU kernel tests, so they are
checked here against an independently built block-diagonal mask.
"""
import math

import pytest
import torch

from hetu_galvatron_amd.ops import flash_attention_varlen
from hetu_galvatron_amd.ops import reference_ops as ref

B, S, HQ, HKV, D = 2, 24, 4, 2, 8
# row 0: 1 + 6 + 9 + 8, row 1: 24 (offsets into the flattened [B*S] stream)
CU = [0, 1, 7, 16, 24, 48]
MAXLEN = 24


def _qkv(seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, HQ, D, generator=g)
    k = torch.randn(B, S, HKV, D, generator=g) * 0.7
    v = torch.randn(B, S, HKV, D, generator=g) * 1.3
    return q, k, v


def _masked_attention(q, k, v, cu, causal):
    """Plain softmax attention over the whole row under a block-diagonal
    (x causal) mask built from a per-token document id — no per-segment
    slicing anywhere."""
    b, s, hq, d = q.shape
    doc = torch.zeros(b * s, dtype=torch.long)
    for i, (lo, hi) in enumerate(zip(cu[:-1], cu[1:])):
        doc[lo:hi] = i
    doc = doc.view(b, s)
    allowed = doc[:, :, None] == doc[:, None, :]          # [b, s, s]
    if causal:
        allowed = allowed & torch.tril(torch.ones(s, s, dtype=torch.bool))
    rep = hq // k.shape[2]
    kx = k.repeat_interleave(rep, dim=2)
    vx = v.repeat_interleave(rep, dim=2)
    sc = torch.einsum("bihd,bjhd->bhij", q, kx) / math.sqrt(d)
    sc = sc.masked_fill(~allowed[:, None], float("-inf"))
    lse = torch.logsumexp(sc, -1)
    o = torch.einsum("bhij,bjhd->bihd", sc.softmax(-1), vx)
    return o, lse


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("sbhd", [False, True])
def test_fwd_matches_block_diagonal_mask(causal, sbhd):
    q, k, v = _qkv()
    o_ref, lse_ref = _masked_attention(q, k, v, CU, causal)
    args = [t.permute(1, 0, 2, 3).contiguous() if sbhd else t
            for t in (q, k, v)]
    o, lse = ref.attention_varlen_fwd(*args, CU, MAXLEN, causal, sbhd=sbhd)
    if sbhd:
        o = o.permute(1, 0, 2, 3)
    assert o.shape == q.shape and lse.shape == (B, HQ, S)
    assert (o - o_ref).abs().max() < 1e-5
    assert (lse - lse_ref).abs().max() < 1e-5


@pytest.mark.parametrize("causal", [True, False])
def test_one_segment_per_row_is_dense(causal):
    q, k, v = _qkv(1)
    cu = [0, S, 2 * S]
    o, lse = ref.attention_varlen_fwd(q, k, v, cu, S, causal)
    o_d, lse_d = ref.attention_fwd(q, k, v, causal)
    assert torch.equal(o, o_d) and torch.equal(lse, lse_d)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("sbhd", [False, True])
def test_bwd_matches_autograd_of_masked_attention(causal, sbhd):
    q, k, v = _qkv(2)
    do = torch.randn(B, S, HQ, D, generator=torch.Generator().manual_seed(9))
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = _masked_attention(qa, ka, va, CU, causal)
    gq, gk, gv = torch.autograd.grad(o_ref, (qa, ka, va), do)

    def lay(t):
        return t.permute(1, 0, 2, 3).contiguous() if sbhd else t
    o, lse = ref.attention_varlen_fwd(lay(q), lay(k), lay(v), CU, MAXLEN,
                                      causal, sbhd=sbhd)
    dq, dk, dv = ref.attention_varlen_bwd(lay(do), lay(q), lay(k), lay(v), o,
                                          lse, CU, MAXLEN, causal, sbhd=sbhd)
    for got, want in ((dq, gq), (dk, gk), (dv, gv)):
        assert got.shape == lay(want).shape
        assert (got - lay(want)).abs().max() < 1e-4


def test_empty_segment_is_accepted():
    q, k, v = _qkv(3)
    cu_dup = [0, 1, 7, 7, 16, 24, 24, 48]
    o, lse = ref.attention_varlen_fwd(q, k, v, CU, MAXLEN)
    o2, lse2 = ref.attention_varlen_fwd(q, k, v, cu_dup, MAXLEN)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    do = torch.ones_like(o)
    g = ref.attention_varlen_bwd(do, q, k, v, o, lse, CU, MAXLEN)
    g2 = ref.attention_varlen_bwd(do, q, k, v, o, lse, cu_dup, MAXLEN)
    for a, b in zip(g, g2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cu,maxlen,what", [
    ([0, 7, 24, 40], 24, "end at"),            # gap: does not reach b*s
    ([1, 7, 24, 48], 24, "start at 0"),        # gap at the front
    ([0, 16, 7, 24, 48], 24, "decreases"),
    ([0, 7, 30, 48], 24, "straddles"),         # [7, 30) crosses row 0 -> 1
    ([0, 48], 24, "straddles"),
    ([0, 1, 7, 16, 24, 48], 23, "max_seqlen"),  # row 1 is 24 long
    ([0, 24, 48], 0, "max_seqlen"),
    ([0, 24, 48], 25, "max_seqlen"),
])
def test_validation_errors(cu, maxlen, what):
    q, k, v = _qkv()
    with pytest.raises(ValueError, match=what):
        ref.attention_varlen_fwd(q, k, v, cu, maxlen)
    with pytest.raises(ValueError, match=what):
        flash_attention_varlen(q, k, v, torch.tensor(cu, dtype=torch.int32),
                               maxlen)


def test_autograd_function_on_cpu_uses_reference():
    q, k, v = _qkv(4)
    cu = torch.tensor(CU, dtype=torch.int32)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    o, lse = flash_attention_varlen(qa, ka, va, cu, MAXLEN, return_lse=True)
    o_ref, lse_ref = ref.attention_varlen_fwd(q, k, v, CU, MAXLEN)
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    do = torch.randn(o.shape, generator=torch.Generator().manual_seed(5))
    o.backward(do)
    want = ref.attention_varlen_bwd(do, q, k, v, o_ref, lse_ref, CU, MAXLEN)
    for got, w in zip((qa.grad, ka.grad, va.grad), want):
        assert torch.equal(got, w)
    with pytest.raises(ValueError, match="int32"):
        flash_attention_varlen(q, k, v, torch.tensor(CU), MAXLEN)
