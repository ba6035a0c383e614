"""`decode_attention_batched(page_table=...)` off the native path (the CPU):
bit for bit the torch path on each row's pages gathered into a contiguous
cache."""
import pytest
import torch

from hetu_galvatron_amd.ops import decode_attention_batched

F8 = torch.float8_e4m3fn


@pytest.mark.parametrize("window", [None, 37])
@pytest.mark.parametrize("dtype", [torch.float32, F8])
def test_paged_fallback_equals_gathered(dtype, window):
    g = torch.Generator().manual_seed(7)
    page, max_pages, hq, hkv, d = 32, 4, 4, 2, 16
    lengths = [1, 128, 70, 0, 150]           # an empty and a clamped row
    slots = [3, 0, 4, 1, 2]
    S, P = 5, 5 * max_pages + 3
    q = torch.randn(len(lengths), hq, d, generator=g)
    kp = torch.randn(P, page, hkv, d, generator=g).to(dtype)
    vp = torch.randn(P, page, hkv, d, generator=g).to(dtype)
    table = torch.randperm(P, generator=g)[:S * max_pages] \
        .reshape(S, max_pages).int()
    scales = {}
    if dtype == F8:
        scales = dict(k_scale=torch.tensor([0.5, 1.7]),
                      v_scale=torch.tensor([1.3, 0.6]))
    i32 = dict(dtype=torch.int32)
    args = (torch.tensor(lengths, **i32), torch.tensor(slots, **i32))
    kw = dict(max_len=100, window=window, **scales)
    got = decode_attention_batched(q, kp, vp, *args, page_table=table, **kw)
    # cache row s = the pages of table row s, in order
    kc = kp[table.long()].reshape(S, max_pages * page, hkv, d)
    vc = vp[table.long()].reshape(S, max_pages * page, hkv, d)
    want = decode_attention_batched(q, kc, vc, *args, **kw)
    assert torch.equal(got, want)
    assert not got[3].any() and got[4].abs().sum() > 0
