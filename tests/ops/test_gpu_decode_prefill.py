"""The four `decode_attn_prefill*` kernels (T > 16 tokens of a row against its
cache) against the fp64 decode oracle per (row, token): NaN in every cache
position no token attends to and in the q rows past q_lens, poisoned outputs
and workspace.

Bound.  The weights enter the second product as one bf16 term, a relative
2^-9 each, and decode_scale >= sum_p w_p (|v| + |o|) bounds numerator plus
normaliser; a factor 2 covers the fp32 terms the decode rule already allows:
|got - round_bf16(oracle)| <= ulp_bf16(|oracle|) + 2^-8 * decode_scale."""
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


def binding(c, stem="decode_attn_prefill"):
    return getattr(get_ext(False), stem + ("_paged" if c.page else "")
                   + ("_fp8" if c.fp8 else ""))


def call(c, n_chunks, t=None, f=None):
    """Through the binding itself, after poisoning what it allocates."""
    n, T, hq, hkv, d = c.dims
    span = min(c.max_len, c.window + T - 1 + (31 if c.page else 0)) \
        if c.window else c.max_len
    nc = chunks(n, hkv * -(-T * (hq // hkv) // 128), span, n_chunks)[0]
    ko.poison(DEV, ((n, T, hq, d), BF16),
              ((n * T * hq * nc * (d + 2),), torch.float32))
    t = t or c.tensors(DEV)
    sc = (t["k_scale"], t["v_scale"]) if c.fp8 else ()
    tb = (t["page_table"],) if c.page else ()
    return (f or binding(c))(
        t["q"], t["k_cache"], t["v_cache"], *sc, *tb, t["lengths"],
        t["q_lens"], t["slots"], c.max_len, c.scale, c.window, n_chunks)


def check(c, o, what):
    got = o.cpu()
    for i, row in enumerate(c.ref):
        for t, ref in enumerate(row):
            w = f"{what} row {i} (len {c.lengths[i]}) token {t}"
            if ref is None:
                assert not got[i, t].any(), f"{w}: not zeros"
            else:
                ko.assert_elem(got[i, t][None], ref[0], ref[1] * 2 ** 12, w)


case = functools.lru_cache(maxsize=2)(Case)


@pytest.mark.parametrize("n_chunks", [1, 3, 0])
@pytest.mark.parametrize("window", [0, 2, 37])
@pytest.mark.parametrize("hq,hkv,T", [(4, 4, 17), (8, 2, 40), (6, 2, 70),
                                      (16, 1, 33)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("page", [None, 32, 128])
@FP8
def test_ragged_rows(fp8, page, d, hq, hkv, T, window, n_chunks):
    pg = (page or 32) + 1
    rows = ((T, T), (33, min(T, 33)), (129, T), (pg, min(T, pg)),
            (MAX_LEN, T), (700, 1), (50, 0), (0, 1), (MAX_LEN + 1, T))
    c = case(fp8, page, d, hq, hkv, T, window, rows, MAX_LEN)
    check(c, call(c, n_chunks), f"prefill fp8={fp8} page={page} d={d} "
          f"h={hq}/{hkv} T={T} w={window} n_chunks={n_chunks}")


@FP8
def test_invalid_pages_are_skipped(fp8):
    c = Case(fp8, 32, 128, 8, 2, 40, 0,
             ((20, 20), (300, 40), (200, 33), (333, 40)), 512,
             holes={0: 0, 1: 8, 2: 1, 3: 2})
    assert c.ref[0] == [None] * 40 and c.ref[1][0] is not None
    for n_chunks in (1, 2):
        check(c, call(c, n_chunks), f"holes n_chunks={n_chunks}")


@FP8
def test_dispatch(fp8):
    """T > 16 goes to the prefill bindings, T <= 16 stays where it was."""
    for T, stem in ((17, "decode_attn_prefill"), (16, "decode_attn_multi")):
        c = Case(fp8, 64, 64, 8, 2, T, 37, ((300, T), (T, T), (90, 3)), 512)
        t = c.tensors(DEV)
        assert torch.equal(c.run(DEV, None, t),
                           call(c, 0, t, binding(c, stem)))


@FP8
def test_graph_replay(fp8):
    """One captured call; lengths, q_lens, table and pools then change in
    place."""
    a = Case(fp8, 64, 128, 8, 2, 40, 0, ((300, 40), (40, 40), (1000, 2)),
             MAX_LEN, pool=45)
    b = Case(fp8, 64, 128, 8, 2, 40, 0, ((129, 1), (777, 33), (2, 0)),
             MAX_LEN, seed=1, pool=45)
    t = a.tensors(DEV)
    a.run(DEV, None, t)                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = a.run(DEV, None, t)
    for c in (a, b, a):
        for k, src in c.tensors(DEV).items():
            t[k].copy_(src)
        o.fill_(float("nan"))
        graph.replay()
        check(c, o, f"graph replay lengths {c.lengths}")


BAD = {  # name -> (refusal, change of the binding's arguments)
    "q_lens_int64": ("q_lens must", lambda a: a.update(
        q_lens=a["q_lens"].long())),
    "q_lens_cpu": ("q_lens must", lambda a: a.update(
        q_lens=a["q_lens"].cpu())),
    "q_3d": ("q must", lambda a: a.update(q=a["q"][:, 0].contiguous()))}


@pytest.mark.parametrize("bad", list(BAD))
@FP8
def test_binding_refuses(fp8, bad):
    c = case(fp8, 64, 64, 8, 2, 20, 0, ((0, 1), (300, 20), (700, 2)), MAX_LEN)
    t = c.tensors(DEV)
    BAD[bad][1](t)
    with pytest.raises(RuntimeError, match=BAD[bad][0]):
        call(c, 0, t)
