"""The torch paths of `decode_attention_batched` on e4m3 caches and of
`kv_cache_append` (CPU): the oracle and the byte comparison of
test_gpu_decode_fp8.py at two small shapes; bf16 caches are served as before."""
import pytest
import torch

from hetu_galvatron_amd.ops import (decode_attention, decode_attention_batched,
                                    kv_cache_append)

from .test_gpu_decode_fp8 import Case, append_case


@pytest.mark.parametrize("d,hq,hkv,window,scaled", [(64, 4, 2, 0, True),
                                                    (128, 8, 1, 37, False)])
def test_attention_torch_path(d, hq, hkv, window, scaled):
    c = Case(d, hq, hkv, 4, 300, (1, 129, 0, 300, 400), (3, 0, 1, 2, 1),
             window, 300, scaled)
    q, k8, v8, ks, vs, lengths, slots = c.tensors("cpu")
    o = decode_attention_batched(q, k8, v8, lengths, slots, max_len=300,
                                 window=window, k_scale=ks, v_scale=vs)
    c.check(o, f"torch path d={d} window={window}")


@pytest.mark.parametrize("n,hkv,d", [(5, 2, 64), (300, 8, 128)])
def test_append_torch_path(n, hkv, d):
    args, want = append_case(n, hkv, d, "cpu")
    kv_cache_append(*args)
    for got, ref in zip(args[2:4], want):
        assert torch.equal(got.view(torch.uint8), ref)


def test_bf16_caches_as_before():
    g = torch.Generator().manual_seed(3)
    lengths, slots = [1, 40, 0, 50], [3, 0, 1, 2]
    q = torch.randn(4, 4, 16, generator=g)
    kc, vc = torch.randn(2, 5, 40, 2, 16, generator=g).unbind(0)
    i32 = torch.int32
    o = decode_attention_batched(q, kc, vc, torch.tensor(lengths, dtype=i32),
                                 torch.tensor(slots, dtype=i32), max_len=33)
    for i, (L, s) in enumerate(zip(lengths, slots)):
        want = decode_attention(q[i:i + 1], kc[s:s + 1], vc[s:s + 1],
                                min(L, 33)) if L else torch.zeros(1, 4, 16)
        assert torch.equal(o[i:i + 1], want), i
    k, v = torch.randn(2, 3, 2, 16, generator=g).unbind(0)
    kv_cache_append(k, v, kc, vc, torch.tensor([4, 0, 9], dtype=i32),
                    torch.tensor([39, 7, 1], dtype=i32))
    assert torch.equal(kc[4, 39], k[0]) and torch.equal(vc[0, 7], v[1])
