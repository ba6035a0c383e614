"""ops.fused_qkv_attention_varlen: packed documents on the packed linear_qkv
buffer [s, b, G, qpg+2, d], against today's composition (slice,
apply_rope_qk, flash_attention_varlen(sbhd=True)) on the same inputs and the
same dout.

Shape and segments are those of test_gpu_varlen.py: b=2, s=1024, row 0 packs

    length  start  exercises
         1      0  single token
        31      1  below one wave's 32 rows
        64     32  exactly one KV tile
        65     96  a tail of 1
       256    161  exactly one q block
       257    417  a second q block with 1 row
       350    674  two blocks with a partial tail

and row 1 is one full-length segment.  Per-row tables are cos_t[pos] with
pos the token index minus its segment's start.

o, lse, the rotated q and k slots, the untouched v slot and the q slots of
dqkv must be bit-identical to the composition (same block bodies, same tile
order, same RoPE arithmetic).  The k and v slots of dqkv may differ from it
only in the fp32 order of the GQA group sum, so they use the dense flash
tests' assert_close formula and tolerances, against the composition and
against an fp32 reference_ops oracle (per-segment attention_fwd through
autograd).
"""
import math

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref

pytestmark = pytest.mark.gpu

B, S, G = 2, 1024, 2
CU = [0, 1, 32, 96, 161, 417, 674, 1024, 2048]
MAXLEN = 1024
POISON = (96, 161)  # the 65-token segment
# repeated entries (empty segments) at the start, inside and at the end
CU_DUP = [0, 0, 1, 32, 32, 96, 161, 417, 674, 1024, 1024, 2048, 2048]
# row 1 ends in a 48-token padding segment
CU_PAD = [0, 1, 32, 96, 161, 417, 674, 1024, 2000, 2048]

ROPES = ("none", "plain", "rows")
PARAMS = [(d, qpg, causal, rope)
          for d in (64, 128) for qpg in (1, 4)
          for causal in (True, False) for rope in ROPES]
IDS = [f"d{d}-qpg{qpg}-{'causal' if c else 'full'}-{r}"
       for d, qpg, c, r in PARAMS]
DQC = [(d, qpg, causal) for d in (64, 128) for qpg in (1, 4)
       for causal in (True, False)]
DQC_IDS = [f"d{d}-qpg{qpg}-{'causal' if c else 'full'}" for d, qpg, c in DQC]

# the PAIRED shape of test_gpu_fused_qkv.py, two documents per row
PAIRED_S, PAIRED_B, PAIRED_HQ = 576, 2, 64
PAIRED_CU = [0, 100, 576, 876, 1152]
PAIRED_PARAMS = [(d, qpg) for d in (64, 128) for qpg in (1, 4)]
PAIRED_IDS = [f"d{d}-qpg{qpg}" for d, qpg in PAIRED_PARAMS]


def dev():
    return torch.device("cuda:0")


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def cu_dev(cu):
    return torch.tensor(cu, dtype=torch.int32, device=dev())


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


def positions(s, b, cu):
    """[s, b] token index minus the start of its segment."""
    pos = torch.empty(b * s, dtype=torch.long)
    for lo, hi in zip(cu[:-1], cu[1:]):
        pos[lo:hi] = torch.arange(hi - lo)
    return pos.view(b, s).t().contiguous().to(dev())


_INPUTS = {}


def inputs(shape, d, qpg):
    """qkv with q, k and v drawn at different scales (a slot mix-up cannot
    pass), dout, and the [s, d/2] NEOX tables; one draw per case."""
    key = (shape, d, qpg)
    if key not in _INPUTS:
        s, b, g_ = shape
        g = torch.Generator(device="cpu").manual_seed(5000 + d + qpg + s)
        qkv = torch.randn(s, b, g_, qpg + 2, d, generator=g)
        qkv[:, :, :, qpg] *= 0.7
        qkv[:, :, :, qpg + 1] *= 1.3
        do = torch.randn(s, b, g_ * qpg, d, generator=g) * 0.9
        cos, sin = ref.rope_freqs(s, d, device=dev())
        _INPUTS[key] = (qkv.to(dev()).bfloat16(), do.to(dev()).bfloat16(),
                        cos, sin)
    return _INPUTS[key]


def tables(shape, d, qpg, rope, cu):
    qkv, do, cos, sin = inputs(shape, d, qpg)
    if rope == "none":
        return None, None
    if rope == "plain":
        return cos, sin
    pos = positions(shape[0], shape[1], cu)
    return cos[pos].contiguous(), sin[pos].contiguous()


def split(x, qpg):
    s, b, d = x.shape[0], x.shape[1], x.shape[-1]
    return (x[:, :, :, :qpg].reshape(s, b, -1, d),
            x[:, :, :, qpg].reshape(s, b, -1, d),
            x[:, :, :, qpg + 1].reshape(s, b, -1, d))


def tokens(t):
    """[s, b, ...] -> token-major [b*s, ...] for row selection."""
    return t.transpose(0, 1).reshape(t.shape[0] * t.shape[1], *t.shape[2:])


_COMP = {}


def composition(shape, cu, d, qpg, causal, rope, attend=True):
    """Today's native path: slice, apply_rope_qk, flash_attention_varlen
    (attend=False: whole rows, flash_attention; cu then only shapes the
    per-row tables).  Computed once per case and never modified."""
    key = (shape, tuple(cu), d, qpg, causal, rope, attend)
    if key not in _COMP:
        from hetu_galvatron_amd.ops import (flash_attention,
                                            flash_attention_varlen)
        from hetu_galvatron_amd.runtime.transformer.rope import apply_rope_qk
        qkv, do, _, _ = inputs(shape, d, qpg)
        cos, sin = tables(shape, d, qpg, rope, cu)
        x = qkv.clone().requires_grad_(True)
        q, k, v = split(x, qpg)
        q, k = apply_rope_qk(q.contiguous(), k.contiguous(), cos, sin)
        if attend:
            o, lse = flash_attention_varlen(
                q, k, v.contiguous(), cu_dev(cu), MAXLEN if shape[0] == S
                else shape[0], causal=causal, return_lse=True, sbhd=True)
        else:
            o, lse = flash_attention(q, k, v.contiguous(), causal=causal,
                                     return_lse=True, sbhd=True)
        o.backward(do)
        _COMP[key] = (o.detach(), lse.detach(), x.grad, q.detach(),
                      k.detach())
    return _COMP[key]


_REF = {}


def reference(shape, cu, d, qpg, causal, rope, attend=True):
    """fp32 reference_ops oracle for dqkv through autograd: per-row rotation
    by rope_apply on the folded [s*b, 1, h, d] rows, attention_fwd on each
    segment's rows.  Computed once per case and never modified."""
    key = (shape, tuple(cu), d, qpg, causal, rope, attend)
    if key not in _REF:
        s, b, _ = shape
        qkv, do, _, _ = inputs(shape, d, qpg)
        cos, sin = tables(shape, d, qpg, rope, cu)
        x = qkv.float().requires_grad_(True)
        q, k, v = split(x, qpg)
        if cos is not None and cos.dim() == 3:
            c2, s2 = cos.reshape(s * b, -1), sin.reshape(s * b, -1)
            q = ref.rope_apply(q.reshape(s * b, 1, -1, d), c2, s2).view(q.shape)
            k = ref.rope_apply(k.reshape(s * b, 1, -1, d), c2, s2).view(k.shape)
        elif cos is not None:
            q, k = ref.rope_apply(q, cos, sin), ref.rope_apply(k, cos, sin)
        qt, kt, vt = tokens(q), tokens(k), tokens(v)
        segs = cu if attend else list(range(0, b * s + 1, s))
        outs = [ref.attention_fwd(qt[lo:hi][None], kt[lo:hi][None],
                                  vt[lo:hi][None], causal,
                                  1.0 / math.sqrt(d))[0][0]
                for lo, hi in zip(segs[:-1], segs[1:]) if hi > lo]
        o = torch.cat(outs).view(b, s, -1, d).transpose(0, 1)
        o.backward(do.float())
        _REF[key] = x.grad
    return _REF[key]


def run_op(shape, cu, d, qpg, causal, rope, attend=True, qkv=None,
           host_cu=False):
    """The op under test -> (o, rotated buffer, dqkv)."""
    from hetu_galvatron_amd.ops import fused_qkv_attention_varlen
    s, b, g_ = shape
    base, do, _, _ = inputs(shape, d, qpg)
    cos, sin = tables(shape, d, qpg, rope, cu)
    x = (base if qkv is None else qkv).clone().requires_grad_(True)
    buf = x.clone()  # the op consumes its input: not a leaf
    cut = None
    if attend:
        cut = torch.tensor(cu, dtype=torch.int32) if host_cu else cu_dev(cu)
    o = fused_qkv_attention_varlen(
        buf, cos, sin, g_, qpg, cu_seqlens=cut,
        max_seqlen=(MAXLEN if s == S else s) if attend else None,
        causal=causal)
    assert o.shape == (s, b, g_ * qpg, d)
    o.backward(do)
    return o.detach(), buf.detach(), x.grad


def check_against_composition(shape, cu, d, qpg, causal, rope, attend=True):
    s = shape[0]
    qkv, do, _, _ = inputs(shape, d, qpg)
    o_c, lse_c, dqkv_c, q_rot, k_rot = composition(shape, cu, d, qpg, causal,
                                                   rope, attend)
    o, buf, dqkv = run_op(shape, cu, d, qpg, causal, rope, attend)
    assert_equal(o, o_c, "o vs composition")
    qf, kf, vf = split(buf, qpg)
    assert_equal(vf, split(qkv, qpg)[2], "v slot after the op vs input")
    assert_equal(qf, q_rot, "rotated q vs composition")
    assert_equal(kf, k_rot, "rotated k vs composition")
    scale = 1.0 / math.sqrt(d)
    if attend:
        o2, lse = ext().flash_attn_qkv_varlen_fwd(
            buf, cu_dev(cu), MAXLEN if s == S else s, causal, scale)
    else:
        o2, lse = ext().flash_attn_qkv_fwd(buf, causal, scale)
    assert_equal(o2, o_c, "raw forward binding o vs composition")
    assert_equal(lse, lse_c, "lse vs composition")

    assert dqkv.shape == qkv.shape
    assert torch.isfinite(dqkv.float()).all(), "non-finite values in dqkv"
    dq, dk, dv = split(dqkv, qpg)
    dq_c, dk_c, dv_c = split(dqkv_c, qpg)
    dq_r, dk_r, dv_r = split(reference(shape, cu, d, qpg, causal, rope,
                                       attend), qpg)
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
def test_matches_composition(d, qpg, causal, rope):
    check_against_composition((S, B, G), CU, d, qpg, causal, rope)


@pytest.mark.parametrize("d,qpg,causal", DQC, ids=DQC_IDS)
def test_one_segment_per_row_equals_fused_qkv_attention(d, qpg, causal):
    """Same block bodies, same tile order -> bit-identical to the dense
    packed kernels (unpaired at this shape) when every row is one segment."""
    from hetu_galvatron_amd.ops import fused_qkv_attention
    shape = (S, B, G)
    qkv, do, cos, sin = inputs(shape, d, qpg)
    o, _, dqkv = run_op(shape, [0, S, 2 * S], d, qpg, causal, "plain")
    x = qkv.clone().requires_grad_(True)
    o_f = fused_qkv_attention(x.clone(), cos, sin, G, qpg, causal=causal)
    o_f.backward(do)
    assert_equal(o, o_f.detach(), "o vs fused_qkv_attention")
    assert_equal(dqkv, x.grad, "dqkv vs fused_qkv_attention")


@pytest.mark.parametrize("d", (64, 128))
def test_per_row_tables_matter(d):
    """Row 0 restarts its positions at every boundary, so past the first one
    its rotated k differs from the plain-table rotation; row 1 is one
    segment from position 0, so there the two agree."""
    shape, qpg = (S, B, G), 4
    _, rows, _ = run_op(shape, CU, d, qpg, True, "rows")
    _, plain, _ = run_op(shape, CU, d, qpg, True, "plain")
    for slot, name in ((0, "q"), (qpg, "k")):
        a, b_ = rows[:, :, :, slot], plain[:, :, :, slot]
        assert_equal(a[:, 1], b_[:, 1], f"rotated {name}, row 1")
        assert_equal(a[:CU[1], 0], b_[:CU[1], 0],
                     f"rotated {name}, row 0 before the first boundary")
        differ = (a[CU[1]:, 0] != b_[CU[1]:, 0]).flatten(1).any(1)
        assert differ.all(), \
            f"rotated {name}: {int((~differ).sum())} row-0 tokens past the " \
            "first boundary ignore the per-row table"
    assert_equal(rows[:, :, :, qpg + 1], plain[:, :, :, qpg + 1], "v slot")


@pytest.mark.parametrize("d,qpg,causal", DQC, ids=DQC_IDS)
def test_isolation_nan_poison(d, qpg, causal):
    """NaN in one segment's q, k and v slots must not reach any other
    segment: a masked-but-loaded NaN enters the MFMA as 0*NaN, so any
    out-of-segment read shows up."""
    shape = (S, B, G)
    qkv, _, _, _ = inputs(shape, d, qpg)
    o_c, _, dqkv_c = run_op(shape, CU, d, qpg, causal, "rows")
    lo, hi = POISON
    bad = qkv.clone()
    bad[lo:hi, 0] = float("nan")
    o_p, _, dqkv_p = run_op(shape, CU, d, qpg, causal, "rows", qkv=bad)
    keep = torch.ones(B * S, dtype=torch.bool, device=dev())
    keep[lo:hi] = False
    for name, a, b_ in (("o", o_p, o_c), ("dqkv", dqkv_p, dqkv_c)):
        a, b_ = tokens(a)[keep], tokens(b_)[keep]
        assert torch.isfinite(a.float()).all(), \
            f"{name}: NaN leaked out of the poisoned segment"
        assert_equal(a, b_, f"{name} of the other segments")
    assert torch.isnan(tokens(o_p)[lo:hi].float()).all()


@pytest.mark.parametrize("d,qpg,causal", DQC, ids=DQC_IDS)
def test_empty_segments(d, qpg, causal):
    """Repeated cu entries change nothing; a trailing padding segment is a
    segment like any other."""
    shape = (S, B, G)
    a = run_op(shape, CU, d, qpg, causal, "plain")
    b_ = run_op(shape, CU_DUP, d, qpg, causal, "plain", host_cu=True)
    for name, x, y in zip(("o", "rotated qkv", "dqkv"), a, b_):
        assert_equal(y, x, f"{name} with empty segments")
    check_against_composition(shape, CU_PAD, d, qpg, causal, "rows")


@pytest.mark.parametrize("d,qpg", PAIRED_PARAMS, ids=PAIRED_IDS)
def test_rows_only_at_a_pairing_shape(d, qpg):
    """cu_seqlens=None with per-row tables: the dense packed kernels with
    complementary-pair scheduling (see test_gpu_fused_qkv.py), per-row RoPE;
    against apply_rope_qk per-row + flash_attention."""
    nqb = (PAIRED_S + 255) // 256
    assert ((nqb + 1) // 2) * PAIRED_B * PAIRED_HQ >= 256
    shape = (PAIRED_S, PAIRED_B, PAIRED_HQ // qpg)
    check_against_composition(shape, PAIRED_CU, d, qpg, True, "rows",
                              attend=False)


@pytest.mark.parametrize("d,qpg,causal", DQC, ids=DQC_IDS)
def test_autograd_matches_bindings(d, qpg, causal):
    shape = (S, B, G)
    qkv, do, _, _ = inputs(shape, d, qpg)
    cos, sin = tables(shape, d, qpg, "rows", CU)
    scale = 1.0 / math.sqrt(d)
    buf = qkv.clone()
    ext().rope_qkv_(buf, cos, sin)
    o, lse = ext().flash_attn_qkv_varlen_fwd(buf, cu_dev(CU), MAXLEN, causal,
                                             scale)
    dqkv, dk_exp, dv_exp = ext().flash_attn_qkv_varlen_bwd(
        do, buf, o, lse, cu_dev(CU), MAXLEN, causal, scale)
    ext().qkv_grad_finish_(dqkv, dk_exp, dv_exp, cos, sin)
    # host cu_seqlens: validated, then copied asynchronously
    got = run_op(shape, CU, d, qpg, causal, "rows", host_cu=True)
    for name, x, y in zip(("o", "rotated qkv", "dqkv"), got,
                          (o, buf, dqkv)):
        assert_equal(x, y, f"{name}: autograd vs bindings")


def test_binding_checks():
    shape = (S, B, G)
    qkv, do, cos, sin = inputs(shape, 64, 4)
    cu = cu_dev(CU)
    scale = 0.125
    fwd = ext().flash_attn_qkv_varlen_fwd
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        fwd(qkv, cu.long(), MAXLEN, True, scale)
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        fwd(qkv, cu[None], MAXLEN, True, scale)
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        fwd(qkv, cu.cpu(), MAXLEN, True, scale)
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        fwd(qkv, cu[:1], MAXLEN, True, scale)
    for bad in (0, S + 1):
        with pytest.raises(RuntimeError, match="max_seqlen"):
            fwd(qkv, cu, bad, True, scale)
    with pytest.raises(RuntimeError, match="qkv must be"):
        fwd(qkv.float(), cu, MAXLEN, True, scale)
    o, lse = fwd(qkv, cu, MAXLEN, True, scale)
    bwd = ext().flash_attn_qkv_varlen_bwd
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        bwd(do, qkv, o, lse, cu.long(), MAXLEN, True, scale)
    with pytest.raises(RuntimeError, match="max_seqlen"):
        bwd(do, qkv, o, lse, cu, 0, True, scale)
    with pytest.raises(RuntimeError, match="dout/o"):
        bwd(do[:-1], qkv, o, lse, cu, MAXLEN, True, scale)
    # per-row tables: rank 3 with qkv's b; the old checks keep raising
    rows_c, rows_s = tables(shape, 64, 4, "rows", CU)
    wrong_c = torch.cat([rows_c, rows_c[:, :1]], 1).contiguous()  # b + 1
    wrong_s = torch.cat([rows_s, rows_s[:, :1]], 1).contiguous()
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().rope_qkv_(qkv.clone(), wrong_c, wrong_s)
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().rope_qkv_(qkv.clone(), rows_c[:, :1].contiguous(),
                        rows_s[:, :1].contiguous())
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().rope_qkv_(qkv.clone(), rows_c, sin)  # mismatched cos / sin
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().rope_qkv_(qkv.clone(), rows_c[:-1].contiguous(),
                        rows_s[:-1].contiguous())
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().rope_qkv_(qkv.clone(), rows_c.double(), rows_s.double())
    dk_exp = torch.zeros_like(do)
    with pytest.raises(RuntimeError, match="cos/sin"):
        ext().qkv_grad_finish_(qkv.clone(), dk_exp, dk_exp, wrong_c, wrong_s)
