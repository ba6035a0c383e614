"""The four `decode_attn_multi*` kernels through `decode_attention_multi`
against the fp64 decode oracle per (row, token), under the element rule of
kernel_oracle.py: NaN in every cache position no token attends to and in the
q rows past q_lens, poisoned outputs and workspace."""
import functools

import pytest
import torch

from hetu_galvatron_amd.ops._ext import get_ext

from . import kernel_oracle as ko
from .test_decode_multi_fallback import BF16, Case
from .test_gpu_decode_batched import chunks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_LEN = 1280
FP8 = pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])


def split(n, d, hq, hkv, T, page, window, forced):
    """(n_chunks, chunk) as the binding forms them: one workgroup per 16
    columns, or per 32 where a kv head has more than 16."""
    cols = T * (hq // hkv)
    groups = -(-cols // (32 if cols > 16 else 16))
    span = min(MAX_LEN, window + T - 1 + (31 if page else 0)) if window \
        else MAX_LEN
    return chunks(n, hkv * groups, span, forced)


def run(c, n_chunks, tensors=None):
    n, T, hq, hkv, d = c.dims
    nc = split(n, d, hq, hkv, T, c.page, c.window, n_chunks)[0]
    ko.poison(DEV, ((n, T, hq, d), BF16),
              ((n * T * hq * nc * (d + 2),), torch.float32))
    return c.run(DEV, n_chunks, tensors)


case = functools.lru_cache(maxsize=2)(Case)


@pytest.mark.parametrize("n_chunks", [1, 3, 0])
@pytest.mark.parametrize("window", [0, 2, 37])
@pytest.mark.parametrize("hq,hkv,T", [(4, 4, 1), (8, 2, 5), (8, 2, 9),
                                      (16, 1, 3), (6, 2, 6)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [None, 32, 128])
@FP8
def test_ragged_rows(fp8, page, d, hq, hkv, T, window, n_chunks):
    nc, chunk = split(9, d, hq, hkv, T, page, window, n_chunks)
    rows = ((T, T), (33, min(T, 3)), (129, T), ((page or 32) + 1, T),
            (2 * chunk + 1, T),         # past max_len with one chunk: zeros
            (MAX_LEN, T), (50, 0), (200, 1), (0, 1))
    c = case(fp8, page, d, hq, hkv, T, window, rows, MAX_LEN)
    c.check(run(c, n_chunks), f"multi fp8={fp8} page={page} d={d} "
            f"h={hq}/{hkv} T={T} w={window} chunks={nc}x{chunk}")


@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("page", [None, 64])
@FP8
def test_one_token_is_the_existing_kernel(fp8, page, n_chunks):
    rows = ((1, 1), (33, 1), (700, 1), (0, 1), (MAX_LEN, 1))
    c = Case(fp8, page, 128, 8, 2, 1, 37 if page else 0, rows, MAX_LEN)
    t = c.tensors(DEV)
    ext = get_ext(False)
    name = ("_paged" if page else "") + ("_fp8" if fp8 else "")
    old = getattr(ext, ("decode_attn_paged" if page else "decode_attn_batched")
                  + ("_fp8" if fp8 else ""))
    sc = (t["k_scale"], t["v_scale"]) if fp8 else ()
    tb = (t["page_table"],) if page else ()
    tail = (c.max_len, c.scale, c.window, n_chunks)
    want = old(t["q"][:, 0].contiguous(), t["k_cache"], t["v_cache"], *sc,
               *tb, t["lengths"], t["slots"], *tail)
    got = getattr(ext, "decode_attn_multi" + name)(
        t["q"], t["k_cache"], t["v_cache"], *sc, *tb, t["lengths"],
        t["q_lens"], t["slots"], *tail)
    assert torch.equal(got[:, 0], want)


@FP8
def test_invalid_pages_are_skipped(fp8):
    c = Case(fp8, 32, 128, 8, 2, 5, 0,
             ((20, 5), (300, 5), (200, 4), (333, 5)), 512,
             holes={0: 0, 2: 1, 3: 2})
    assert c.ref[0] == [None] * 5 and c.ref[1][0] is not None
    for n_chunks in (1, 2):
        c.check(run(c, n_chunks), f"holes n_chunks={n_chunks}")


@FP8
def test_graph_replay(fp8):
    """One captured call; lengths, q_lens, table and pools then change in
    place."""
    a = Case(fp8, 64, 128, 8, 2, 5, 0, ((300, 5), (5, 5), (1000, 2)), MAX_LEN,
             pool=45)
    b = Case(fp8, 64, 128, 8, 2, 5, 0, ((129, 1), (777, 4), (2, 0)), MAX_LEN,
             seed=1, pool=45)
    t = a.tensors(DEV)
    run(a, None, t)                          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = a.run(DEV, None, t)
    for c in (a, b, a):
        for k, src in c.tensors(DEV).items():
            t[k].copy_(src)
        o.fill_(float("nan"))
        graph.replay()
        c.check(o, f"graph replay lengths {c.lengths}")


BAD = {  # name -> (refusal, change of the binding's arguments)
    "q_lens_int64": ("q_lens must", lambda a: a.update(
        q_lens=a["q_lens"].long())),
    "q_lens_cpu": ("q_lens must", lambda a: a.update(
        q_lens=a["q_lens"].cpu())),
    "T_17": ("q must", lambda a: a.update(
        q=torch.zeros(3, 17, 8, 64, dtype=BF16, device=DEV))),
    "q_3d": ("q must", lambda a: a.update(q=a["q"][:, 0].contiguous()))}


@pytest.mark.parametrize("bad", list(BAD))
@FP8
def test_binding_refuses(fp8, bad):
    c = case(fp8, 64, 64, 8, 2, 5, 0, ((0, 1), (300, 5), (700, 2)), MAX_LEN)
    t = c.tensors(DEV)
    BAD[bad][1](t)
    ext = get_ext(False)
    f = ext.decode_attn_multi_paged_fp8 if fp8 else ext.decode_attn_multi_paged
    sc = (t["k_scale"], t["v_scale"]) if fp8 else ()
    with pytest.raises(RuntimeError, match=BAD[bad][0]):
        f(t["q"], t["k_cache"], t["v_cache"], *sc, t["page_table"],
          t["lengths"], t["q_lens"], t["slots"], c.max_len, c.scale, 0, 0)
    c.check(run(c, None), "after a refusal")
