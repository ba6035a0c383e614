"""Input checks of the flash-attention bindings: the dense pair refuses what
it used to read out of bounds, naming the argument, and nothing valid is shut
out (cross lengths, sbhd, a non-contiguous lse through all four backwards).
Smallest shapes that still form a launch: b 1, sq 64, hq 2, hkv 1, d 64."""
import os

import pytest
import torch

from hetu_galvatron_amd.ops._ext import get_ext

pytestmark = pytest.mark.gpu

B, S, HQ, HKV, D = 1, 64, 2, 1, 64
SCALE = 0.125


def ext():
    return get_ext(False)


def rand(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16().cuda()


@pytest.fixture(scope="module")
def dense():
    q, k, v = rand(B, S, HQ, D), rand(B, S, HKV, D, seed=1), \
        rand(B, S, HKV, D, seed=2)
    do = rand(B, S, HQ, D, seed=3)
    o, lse = ext().flash_attn_fwd(q, k, v, True, SCALE)
    return q, k, v, do, o, lse


@pytest.mark.parametrize("case, name", [
    ("k_head_dim", "k must"), ("k_fp32", "k must"), ("v_shape", "v must"),
    ("k_batch", "k must")])
def test_fwd_rejects(dense, case, name):
    q, k, v = dense[:3]
    if case == "k_head_dim":
        k = rand(B, S, HKV, 128)
    elif case == "k_fp32":
        k = k.float()
    elif case == "v_shape":
        v = rand(B, S + 32, HKV, D)
    else:
        k, v = rand(B + 1, S, HKV, D), rand(B + 1, S, HKV, D)
    with pytest.raises(RuntimeError, match=name):
        ext().flash_attn_fwd(q, k, v, True, SCALE)
    with pytest.raises(RuntimeError, match=name):
        ext().flash_attn_bwd(dense[3], q, k, v, dense[4], dense[5], True,
                             SCALE)


@pytest.mark.parametrize("case, name", [
    ("dout_short", "dout is"), ("o_fp32", "o is"), ("lse_swapped", "lse must"),
    ("lse_bf16", "lse must"), ("lse_cpu", "lse must")])
def test_bwd_rejects(dense, case, name):
    q, k, v, do, o, lse = dense
    if case == "dout_short":
        do = do[:, :-1].contiguous()
    elif case == "o_fp32":
        o = o.float()
    elif case == "lse_swapped":
        lse = lse.transpose(1, 2).contiguous()
    elif case == "lse_bf16":
        lse = lse.bfloat16()
    else:
        lse = lse.cpu()
    with pytest.raises(RuntimeError, match=name):
        ext().flash_attn_bwd(do, q, k, v, o, lse, True, SCALE)


def recorded(name):
    """o, lse, dq, dk, dv of the same call as the bindings returned them
    before they gained their checks (tests/golden/flash_bindings_head.pt;
    bf16 stored as int16 bit patterns)."""
    path = os.path.join(os.path.dirname(__file__), os.pardir, "golden",
                        "flash_bindings_head.pt")
    gold = torch.load(path, weights_only=True)
    out = [gold[f"{name}.{n}"] for n in ("o", "lse", "dq", "dk", "dv")]
    return [t.view(torch.bfloat16) if t.dtype == torch.int16 else t
            for t in out]


@pytest.mark.parametrize("name, skv, causal, sbhd", [
    ("cross", 96, False, False),   # skv 96 against sq 64, non-causal
    ("sbhd", S, True, True)])
def test_still_accepted_and_unchanged(name, skv, causal, sbhd):
    q, do = rand(B, S, HQ, D), rand(B, S, HQ, D, seed=3)
    k, v = rand(B, skv, HKV, D, seed=1), rand(B, skv, HKV, D, seed=2)
    if sbhd:
        q, k, v, do = (x.transpose(0, 1).contiguous() for x in (q, k, v, do))
    o, lse = ext().flash_attn_fwd(q, k, v, causal, SCALE, None, sbhd)
    dq, dk, dv = ext().flash_attn_bwd(do, q, k, v, o, lse, causal, SCALE,
                                      None, sbhd)
    for got, want, what in zip((o, lse, dq, dk, dv), recorded(name),
                               ("o", "lse", "dq", "dk", "dv")):
        assert torch.equal(got.cpu(), want), f"{name}: {what} changed"


def strided(lse):
    """lse as a non-contiguous view of a transposed allocation"""
    out = lse.transpose(1, 2).contiguous().transpose(1, 2)
    assert not out.is_contiguous() and torch.equal(out, lse)
    return out


def test_noncontiguous_lse_through_all_backwards(dense):
    q, k, v, do, o, lse = dense
    cu = torch.tensor([0, 40, 64], dtype=torch.int32).cuda()
    runs = [lambda l: ext().flash_attn_bwd(do, q, k, v, o, l, True, SCALE)]
    ov, lsev = ext().flash_attn_varlen_fwd(q, k, v, cu, 40, True, SCALE)
    runs.append(lambda l, ov=ov: ext().flash_attn_varlen_bwd(
        do, q, k, v, ov, l, cu, 40, True, SCALE))
    qkv = rand(S, B, HKV, HQ // HKV + 2, D, seed=4)
    dop = rand(S, B, HQ, D, seed=5)
    op, lsep = ext().flash_attn_qkv_fwd(qkv, True, SCALE)
    runs.append(lambda l: ext().flash_attn_qkv_bwd(dop, qkv, op, l, True,
                                                   SCALE))
    opv, lsepv = ext().flash_attn_qkv_varlen_fwd(qkv, cu, 40, True, SCALE)
    runs.append(lambda l: ext().flash_attn_qkv_varlen_bwd(
        dop, qkv, opv, l, cu, 40, True, SCALE))
    for run, l in zip(runs, (lse, lsev, lsep, lsepv)):
        want = run(l.contiguous())
        got = run(strided(l))
        # the packed backwards leave the k and v slots of dqkv to
        # qkv_grad_finish_: compare what they write
        for g, w in zip(got, want):
            if g.dim() == 5:
                g, w = g[:, :, :, :-2], w[:, :, :, :-2]
            assert torch.equal(g, w)
