"""Flash attention with one LDS image per operand tile (transposed reads).

The block bodies of ops/csrc/flash_attn.hip stage V, K and Q / dO once, by
rows, into a swizzled LDS image and feed the second product of each body
from ds_read_b64_tr_b16 reads of that image.  What can go wrong is an
operand map (a swapped chunk, a wrong row of a 4 x 16 block) or a tail
(the zeroed rows of the last tile), so:

1. exact operand-map checks: with q = k one-hot rows P is the identity
   after bf16 rounding, so o == v and dv == dout bit for bit, through the
   dense, varlen and packed-QKV kernels;
2. tails and seams against the fp32 reference over whole tensors, with the
   tolerances of test_flash_fwd / test_flash_bwd (tests/ops/
   test_gpu_kernels.py);
3. the bitwise equalities between the four modules at one tail shape;
4. SHA-256 digests of every output of the cases of 2 against the record
   that tools/flash_golden.py wrote with the build that still staged a
   second, transposed image from global memory
   (tests/ops/flash_golden_parent.json; flash_golden_bias_tail.json for
   the one case where that build was wrong, see GOLDEN_BIAS_TAIL).
"""
import importlib.util
import json
import math
import os

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))


def _load_golden_tool():
    spec = importlib.util.spec_from_file_location(
        "flash_golden", os.path.join(_ROOT, "tools", "flash_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


golden = _load_golden_tool()
CASE_INDEX = {name: i for i, (name, _) in enumerate(golden.CASES)}
CASE_BY_NAME = dict(golden.CASES)


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def dev():
    return torch.device("cuda:0")


def assert_close(a, b, atol, rtol=2e-2, what=""):
    """test_gpu_kernels.assert_close over the whole tensors.  Rows that see
    no key (causal with sq > skv) have lse = -inf on both sides: the
    infinities must coincide and the bound is taken over the finite rest."""
    a = a.float().cpu()
    b = b.float().cpu()
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    inf = torch.isinf(b)
    assert torch.equal(inf, torch.isinf(a)) and \
        torch.equal(a[inf], b[inf]), f"{what}: infinities differ"
    a, b = a[~inf], b[~inf]
    if a.numel() == 0:
        return
    err = (a - b).abs().max().item()
    denom = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * denom, \
        f"{what}: max|err|={err:.4e} vs atol={atol} rtol*max={rtol * denom:.4e}"


# ---------------------------------------------------------------------------
# 1. exact operand-map checks
# ---------------------------------------------------------------------------
B, HQ, HKV = 2, 4, 1


def identity_inputs(d, s, sbhd):
    """q = k = 32 * one-hot rows (scores 1024/sqrt(d) on the diagonal, 0
    elsewhere), v and dout random bf16."""
    g = torch.Generator().manual_seed(7000 + 10 * d + s)
    eye = 32.0 * torch.eye(s, d)                       # [s, d], s <= d
    q = eye[None, :, None, :].expand(B, s, HQ, d)
    k = eye[None, :, None, :].expand(B, s, HKV, d)
    v = torch.randn(B, s, HKV, d, generator=g)
    dout = torch.randn(B, s, HQ, d, generator=g)
    out = [t.bfloat16().contiguous() for t in (q, k, v, dout)]
    if sbhd:
        out = [t.permute(1, 0, 2, 3).contiguous() for t in out]
    return [t.to(dev()) for t in out]


def check_identity(o, lse, dv, v, dout, d, what):
    assert torch.equal(o, v.expand_as(o)), f"{what}: o != v"
    # the binding sums the per-q-head dv over the GQA group with this very
    # reduction, so a per-head dv equal to dout gives exactly this
    want = dout.view(*dout.shape[:2], HKV, HQ // HKV, d).sum(3)
    assert torch.equal(dv, want), f"{what}: dv != group sum of dout"
    diag = 1024.0 / math.sqrt(d)
    rel = ((lse - diag).abs().max() / diag).item()
    assert rel <= 1e-5, f"{what}: lse off the diagonal score by {rel:.3e}"


@pytest.mark.parametrize("sbhd", [False, True])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("s_is", ["1", "33", "D"])
@pytest.mark.parametrize("d", [64, 128])
def test_identity_dense_and_varlen(d, s_is, causal, sbhd):
    s = d if s_is == "D" else int(s_is)
    q, k, v, dout = identity_inputs(d, s, sbhd)
    scale = 1.0 / math.sqrt(d)
    o, lse = ext().flash_attn_fwd(q, k, v, causal, scale, None, sbhd)
    dq, dk, dv = ext().flash_attn_bwd(dout, q, k, v, o, lse, causal, scale,
                                      None, sbhd)
    check_identity(o, lse, dv, v, dout, d, "dense")
    cu = torch.tensor([0, s, 2 * s], dtype=torch.int32, device=dev())
    o2, lse2 = ext().flash_attn_varlen_fwd(q, k, v, cu, s, causal, scale,
                                           sbhd)
    dq2, dk2, dv2 = ext().flash_attn_varlen_bwd(dout, q, k, v, o2, lse2, cu,
                                                s, causal, scale, sbhd)
    check_identity(o2, lse2, dv2, v, dout, d, "varlen")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("s_is", ["1", "33", "D"])
@pytest.mark.parametrize("d", [64, 128])
def test_identity_packed_qkv(d, s_is, causal):
    from hetu_galvatron_amd.ops import fused_qkv_attention
    s = d if s_is == "D" else int(s_is)
    q, k, v, dout = identity_inputs(d, s, True)        # [s, b, h, d]
    qpg = HQ // HKV
    packed = torch.cat([q, k, v], dim=2).view(s, B, HKV, qpg + 2, d)
    scale = 1.0 / math.sqrt(d)
    o, lse = ext().flash_attn_qkv_fwd(packed, causal, scale)
    dqkv, dk_exp, dv_exp = ext().flash_attn_qkv_bwd(dout, packed, o, lse,
                                                    causal, scale)
    assert torch.equal(o, v.expand_as(o)), "packed: o != v"
    assert torch.equal(dv_exp, dout), "packed: per-q-head dv != dout"
    diag = 1024.0 / math.sqrt(d)
    assert ((lse - diag).abs().max() / diag).item() <= 1e-5

    # through the op, without RoPE, all heads of the group sharing dout:
    # the v slot of the gradient is qpg * dout
    x = packed.clone().requires_grad_(True)
    shared = dout[:, :, :1].expand(s, B, HQ, d).contiguous()
    of = fused_qkv_attention(x.clone(), None, None, HKV, qpg, causal=causal)
    assert torch.equal(of.detach(), o), "op forward vs binding"
    of.backward(shared)
    dv_slot = x.grad[:, :, :, qpg + 1]
    assert_close(dv_slot, qpg * shared[:, :, :1].float(), 6e-2, rtol=3e-2,
                 what="v slot of dqkv vs qpg * dout")


# ---------------------------------------------------------------------------
# 2. tails and seams against the fp32 reference / 4. the parent's digests
# ---------------------------------------------------------------------------
_RUNS = {}


def run(name):
    """Native forward + backward of a case, once; shared by 2 and 4."""
    if name not in _RUNS:
        _RUNS[name] = golden.run_case(ext(), CASE_BY_NAME[name],
                                      CASE_INDEX[name], dev())
    return _RUNS[name]


def bshd(t, c):
    return t.permute(1, 0, 2, 3) if c["sbhd"] else t


@pytest.mark.parametrize("name", list(CASE_BY_NAME))
def test_tails_vs_reference(name):
    c = CASE_BY_NAME[name]
    inp, out = run(name)
    q, k, v, dout = (bshd(inp[n], c).float() for n in ("q", "k", "v", "dout"))
    bias = inp["bias"].float() if inp["bias"] is not None else None
    scale = 1.0 / math.sqrt(c["d"])
    window = c.get("window")
    o_r, lse_r = ref.attention_fwd(q, k, v, c["causal"], scale, bias, window)
    grads = ref.attention_bwd(dout, q, k, v, o_r, lse_r, c["causal"], scale,
                              bias, window)
    assert_close(bshd(out["o"], c), o_r, 3e-2, what=f"{name} o")
    assert_close(out["lse"], lse_r, 2e-2, what=f"{name} lse")
    for key, r in zip(("dq", "dk", "dv"), grads):
        assert_close(bshd(out[key], c), r, 6e-2, rtol=3e-2,
                     what=f"{name} {key}")
    if bias is not None:
        assert_close(out["dbias"], grads[3], 6e-2, rtol=3e-2,
                     what=f"{name} dbias")


def _record(fname):
    with open(os.path.join(_HERE, fname)) as f:
        return json.load(f)


GOLDEN = _record("flash_golden_parent.json")
# The biased tail case found a fault of the recorded build itself:
# load_bias16 clamped a quad of bias values that reached past the row end to
# a 4-aligned start, so with skv % 4 != 0 the last skv % 4 keys of a row got
# the bias of earlier keys (that build misses the fp32 reference there by
# max|err| 0.417 on o against a bound of 0.061).  The fix changes the bits
# of exactly the biased cases with skv % 4 != 0; for those the record is
# the one written by the recorded build with that fix alone applied to it.
# Nobody can regenerate that second record from a commit of the repository,
# so for these cases the check that counts is test_tails_vs_reference; the
# digests only say that the transposed-read change left them alone too.
GOLDEN_BIAS_TAIL = _record("flash_golden_bias_tail.json")


def test_golden_records_cover_every_case():
    assert sorted(GOLDEN) == sorted(CASE_BY_NAME)
    assert sorted(GOLDEN_BIAS_TAIL) == sorted(
        n for n, c in CASE_BY_NAME.items()
        if c.get("bias") and c["skv"] % 4 != 0)
    for name, rec in GOLDEN_BIAS_TAIL.items():
        assert sorted(rec) == sorted(GOLDEN[name])


@pytest.mark.parametrize("name", list(CASE_BY_NAME))
def test_outputs_match_parent_digests(name):
    _, out = run(name)
    want = GOLDEN_BIAS_TAIL.get(name, GOLDEN[name])
    got = {key: golden.digest(val) for key, val in out.items()
           if key != "dbias"}
    diff = [key for key in got if got[key] != want[key]]
    assert not diff and sorted(got) == sorted(want), \
        f"{name}: {diff} differ from the recorded build bit for bit"


# ---------------------------------------------------------------------------
# 3. bitwise equalities between the modules at a tail shape
# ---------------------------------------------------------------------------
def test_modules_agree_bitwise_at_a_tail():
    from hetu_galvatron_amd.ops import fused_qkv_attention
    s, b, d, hq, hkv = 257, 2, 128, 4, 1
    qpg = hq // hkv
    g = torch.Generator().manual_seed(99)
    packed = torch.randn(s, b, hkv, qpg + 2, d, generator=g).bfloat16()
    dout = torch.randn(s, b, hq, d, generator=g).bfloat16().to(dev())
    packed = packed.to(dev())
    q = packed[:, :, :, :qpg].reshape(s, b, hq, d).contiguous()
    k = packed[:, :, :, qpg].reshape(s, b, hkv, d).contiguous()
    v = packed[:, :, :, qpg + 1].reshape(s, b, hkv, d).contiguous()
    scale = 1.0 / math.sqrt(d)

    o, lse = ext().flash_attn_fwd(q, k, v, True, scale, None, True)
    dq, dk, dv = ext().flash_attn_bwd(dout, q, k, v, o, lse, True, scale,
                                      None, True)

    # one segment per row in varlen == dense
    cu = torch.tensor([0, s, 2 * s], dtype=torch.int32, device=dev())
    o_v, lse_v = ext().flash_attn_varlen_fwd(q, k, v, cu, s, True, scale,
                                             True)
    got = ext().flash_attn_varlen_bwd(dout, q, k, v, o_v, lse_v, cu, s, True,
                                      scale, True)
    for what, a, w in (("o", o_v, o), ("lse", lse_v, lse), ("dq", got[0], dq),
                       ("dk", got[1], dk), ("dv", got[2], dv)):
        assert torch.equal(a, w), f"varlen {what} != dense"

    # the packed op == the composition on o, lse and the q slots
    x = packed.clone().requires_grad_(True)
    o_p = fused_qkv_attention(x.clone(), None, None, hkv, qpg, causal=True)
    _, lse_p = ext().flash_attn_qkv_fwd(packed, True, scale)
    o_p.backward(dout)
    assert torch.equal(o_p.detach(), o), "packed o != composition"
    assert torch.equal(lse_p, lse), "packed lse != composition"
    assert torch.equal(x.grad[:, :, :, :qpg].reshape(s, b, hq, d), dq), \
        "packed q slots of dqkv != composition dq"
