"""Decode attention and the grad-norm sum of squares at their edges.

`decode_attn` / `decode_attn_graph` (the single-block, split and merge
kernels) against the fp64 oracle under the element rule of kernel_oracle.py,
on inputs with a peaked softmax whose heavy positions sit where a kernel can
lose one: the window's ends, both sides of every chunk boundary, the
256-thread stripe and the V slices.  Cache rows outside [start, cur) hold
NaN, `o` and the split workspace are allocated over NaN-poisoned memory.
`multi_sumsq` against the fp64 sum under the accumulation rule, on lists
with planted large values in every tail, at every 2^20 chunk boundary and
past the 2048-block grid cap, as views at odd element offsets.
test_kernel_oracle.py shows on the CPU, on the same inputs, that the fp32
reference passes these rules and that every planted mutant misses them.
"""
import os

import pytest
import torch

from . import kernel_oracle as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
BF16 = torch.bfloat16
NAN = float("nan")


def _ids(v):
    return str(v).replace("torch.", "").replace(" ", "")


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


# ---------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------
def caches(c, clean=False):
    """The case's caches on the GPU, NaN outside [start, cur)."""
    kc, vc = c.kc.clone(), c.vc.clone()
    if not clean:
        for t in (kc, vc):
            t[:, :c.start] = NAN
            t[:, c.cur:] = NAN
    return kc.to(DEV), vc.to(DEV)


def run(c, q, kc, vc, cur32=None):
    """One call over poisoned output and workspace memory."""
    specs = [((c.b, c.hq, c.d), BF16)]
    if c.nc > 1 or c.max_len:
        specs.append(((c.b * c.hq * c.nc * (c.d + 2),), F32))
    ko.poison(DEV, *specs)
    if c.max_len:
        return ext().decode_attn_graph(q, kc, vc, cur32, c.max_len, c.scale)
    return ext().decode_attn(q, kc, vc, c.cur, c.scale, c.start)


def check(o, o64, sc, what):
    ko.assert_finite(o, what=what)
    got = o.cpu()
    want = o64.to(BF16)
    differ = int((got != want).sum())
    one_ulp = int(((got.view(torch.int16).int()
                    - want.view(torch.int16).int()).abs() == 1).sum())
    r = ko.assert_elem(got, o64, sc, what)
    print(f"[decode] {what}: bound used {r:.3g}; {differ} of {got.numel()} "
          f"elements differ from the rounded oracle, {one_ulp} by one ulp")


def run_case(c, clean=False):
    q = c.q.to(DEV)
    kc, vc = caches(c, clean)
    cur32 = torch.tensor([c.cur], dtype=torch.int32, device=DEV) \
        if c.max_len else None
    return run(c, q, kc, vc, cur32)


@pytest.mark.parametrize(
    "b,hq,hkv,d,max_s,n,start",
    ko.decode_params(ko.DECODE_SINGLE + ko.DECODE_SPLIT + ko.DECODE_LDS),
    ids=_ids)
def test_decode_attn(b, hq, hkv, d, max_s, n, start):
    c = ko.decode_case(b, hq, hkv, d, max_s, n, start)
    check(run_case(c), c.o, c.sc, f"decode {c.tag}")


@pytest.mark.parametrize("b,hq,hkv,d,max_s,n", ko.decode_graph_params(),
                         ids=_ids)
def test_decode_attn_graph(b, hq, hkv, d, max_s, n):
    c = ko.decode_case(b, hq, hkv, d, max_s, n,
                       max_len=ko.DECODE_GRAPH_MAX_LEN)
    o = run_case(c)
    check(o, c.o, c.sc, f"decode graph {c.tag}")
    if n == ko.DECODE_GRAPH_MAX_LEN:
        # the host-length binding forms the same 16 chunks of 128
        assert ko.decode_chunks(b, hq, n) == (c.nc, c.chunk)
        kc, vc = caches(c)
        assert torch.equal(
            o, ext().decode_attn(c.q.to(DEV), kc, vc, n, c.scale))


@pytest.mark.parametrize("d", ko.DECODE_DIMS)
def test_decode_attn_graph_length_advanced_in_place(d):
    b, hq, hkv, max_s, _ = ko.DECODE_GRAPH[0]
    c = ko.decode_case(b, hq, hkv, d, max_s, 2047,
                       max_len=ko.DECODE_GRAPH_MAX_LEN)
    q = c.q.to(DEV)
    kc, vc = caches(c)
    cur32 = torch.tensor([2046], dtype=torch.int32, device=DEV)
    first = run(c, q, kc, vc, cur32)
    o64, aux = ko.decode_attn(c.q, c.kc, c.vc, 2046, c.scale)
    sc = ko.decode_scale(c.q, c.kc, c.vc, 2046, c.scale, 0, o64, aux)
    check(first, o64, sc, f"decode graph d={d} cur=2046")
    cur32.add_(1)
    check(run(c, q, kc, vc, cur32), c.o, c.sc,
          f"decode graph d={d} cur=2046+1")


@pytest.mark.parametrize("key,max_len", [
    ((8, 32, 2, 64, 512, 300, 37), None),           # single block
    ((1, 4, 2, 128, 1280, 1025, 37), None),         # 9 chunks
    ((1, 4, 2, 64, 2048, 17), ko.DECODE_GRAPH_MAX_LEN)], ids=_ids)
def test_decode_reads_nothing_outside_the_window(key, max_len):
    """NaN in every cache row outside [start, cur) changes no bit (a
    0 * NaN would)."""
    c = ko.decode_case(*key, max_len=max_len)
    clean = run_case(c, clean=True)
    assert torch.equal(run_case(c), clean)
    check(clean, c.o, c.sc, f"decode clean {c.tag}")


@pytest.mark.parametrize("d", ko.DECODE_DIMS)
def test_decode_extreme_scores(d):
    """Scores spanning +-60, and one head whose scores are all below -100."""
    b, hq, hkv, max_s, n = ko.DECODE_EXTREME
    c = ko.decode_case(b, hq, hkv, d, max_s, n, extreme=True)
    check(run_case(c), c.o, c.sc, f"decode extreme {c.tag}")


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_generate_through_split_and_merge(graphed):
    """The tiny llama with a 260-token prompt: decode runs 3 chunks (4 under
    the graph, max_seq 512) through the split and merge kernels; every new
    token is a near-argmax of a full-prefix recompute."""
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.runtime import GalvatronModel
    from hetu_galvatron_amd.runtime.inference import (GalvatronGenerator,
                                                      KVCache)
    cfg = load_config(base={
        "model": {"model_name": "tiny-llama"},
        "train": {"global_train_batch_size": 2, "train_iters": 1},
    })
    torch.manual_seed(0)
    model = GalvatronModel(cfg)
    P, NEW, S = 260, 4, 512
    gen = GalvatronGenerator(model, max_batch=2, max_seq=S)
    assert ko.decode_chunks(2, cfg.model.num_attention_heads, P + 1)[0] == 3
    ids = torch.randint(0, cfg.model.vocab_size, (2, P), device="cuda")
    if graphed:
        out = gen.generate_graphed(ids, max_new_tokens=NEW, warmup_steps=1)
    else:
        out = gen.generate(ids, max_new_tokens=NEW, temperature=0.0)
    assert out.shape == (2, P + NEW)
    for i in range(NEW):
        cache = KVCache(len(gen.layers), 2, S, cfg.model.kv_heads,
                        cfg.model.head_dim, ids.device)
        logits = gen._forward_tokens(out[:, :P + i], cache)
        got = logits.gather(1, out[:, P + i:P + i + 1])
        gap = float((logits.max(-1, keepdim=True).values - got).max())
        print(f"[generate] graphed={graphed} token {i}: gap {gap:.3g}")
        assert gap < 0.05, i


# ---- bindings ---------------------------------------------------------------
BIND = (1, 4, 2, 64, 1280, 129, 0)           # 2 chunks; graph: 10 chunks


def _bind_case(graph):
    return ko.decode_case(*BIND[:6], max_len=BIND[4]) if graph \
        else ko.decode_case(*BIND)


def _call(graph, q, kc, vc, cur=None, start=0, cur32=None, max_len=None):
    c = _bind_case(graph)
    if graph:
        if cur32 is None:
            cur32 = torch.tensor([c.cur], dtype=torch.int32, device=DEV)
        return ext().decode_attn_graph(q, kc, vc, cur32,
                                       max_len or c.max_len, c.scale)
    return ext().decode_attn(q, kc, vc, cur or c.cur, c.scale, start)


def _still_right(graph):
    """After a refused call a valid one returns the oracle's answer."""
    c = _bind_case(graph)
    check(run_case(c), c.o, c.sc, f"decode after a refusal {c.tag}")


@pytest.mark.parametrize("graph", [False, True],
                         ids=["decode_attn", "decode_attn_graph"])
@pytest.mark.parametrize("case,name", [
    ("k_fp32", "k_cache must"), ("v_shape", "v_cache must"),
    ("v_fp32", "v_cache must"), ("v_cpu", "v_cache must"),
    ("k_strided", "k_cache must"), ("v_strided", "v_cache must"),
    ("head_dim", "k_cache must"), ("batch", "k_cache must"),
    ("gqa", "hq % hkv"), ("q_strided", "q must")])
def test_decode_bindings_refuse(case, name, graph):
    c = _bind_case(graph)
    q = c.q.to(DEV)
    kc, vc = caches(c)
    b, max_s, hkv, d = kc.shape
    if case == "k_fp32":
        kc = kc.float()
    elif case == "v_shape":
        vc = vc[:, :max_s // 2].contiguous()
    elif case == "v_fp32":
        vc = vc.float()
    elif case == "v_cpu":
        vc = vc.cpu()
    elif case == "k_strided":
        big = torch.zeros(b, max_s, 2 * hkv, d, dtype=BF16, device=DEV)
        kc = big[:, :, ::2]
    elif case == "v_strided":
        big = torch.zeros(b, max_s, 2 * hkv, d, dtype=BF16, device=DEV)
        vc = big[:, :, ::2]
    elif case == "head_dim":
        kc = torch.zeros(b, max_s, hkv, 2 * d, dtype=BF16, device=DEV)
        vc = torch.zeros_like(kc)
    elif case == "batch":
        kc = torch.zeros(b + 1, max_s, hkv, d, dtype=BF16, device=DEV)
        vc = torch.zeros_like(kc)
    elif case == "gqa":
        kc = torch.zeros(b, max_s, 3, d, dtype=BF16, device=DEV)
        vc = torch.zeros_like(kc)
    else:
        q = torch.zeros(b, 2 * c.hq, d, dtype=BF16, device=DEV)[:, ::2]
    with pytest.raises(RuntimeError, match=name):
        _call(graph, q, kc, vc)
    _still_right(graph)


@pytest.mark.parametrize("case,name", [
    ("cur32_int64", "cur_len_dev must"), ("cur32_cpu", "cur_len_dev must"),
    ("max_len_0", "max_len must"), ("max_len_past", "max_len must")])
def test_decode_attn_graph_refuses(case, name):
    c = _bind_case(True)
    q = c.q.to(DEV)
    kc, vc = caches(c)
    cur32 = torch.tensor([c.cur], dtype=torch.int32, device=DEV)
    max_len = c.max_len
    if case == "cur32_int64":
        cur32 = cur32.long()
    elif case == "cur32_cpu":
        cur32 = cur32.cpu()
    elif case == "max_len_0":
        max_len = 0
    else:
        max_len = c.max_s + 1
    with pytest.raises(RuntimeError, match=name):
        ext().decode_attn_graph(q, kc, vc, cur32, max_len, c.scale)
    _still_right(True)


@pytest.mark.parametrize("cur,start,name", [
    (0, 0, "cur_len must"), (1281, 0, "cur_len must"),
    (129, 129, "start must"), (129, 200, "start must"),
    (129, -1, "start must")])
def test_decode_attn_refuses_lengths(cur, start, name):
    c = _bind_case(False)
    kc, vc = caches(c)
    with pytest.raises(RuntimeError, match=name):
        ext().decode_attn(c.q.to(DEV), kc, vc, cur, c.scale, start)
    _still_right(False)


GOLDEN = [("single", (8, 32, 2, 64, 512, 300, 37), None),
          ("split", (1, 4, 2, 128, 1280, 1025, 37), None),
          ("graph", (1, 4, 2, 64, 2048, 2047), ko.DECODE_GRAPH_MAX_LEN)]


def input_digest(c):
    """Sum of the inputs' bit patterns: the recorded outputs belong to
    these inputs only."""
    return sum(int(t.view(torch.int16).long().sum())
               for t in (c.q, c.kc, c.vc))


@pytest.mark.parametrize("name,key,max_len", GOLDEN,
                         ids=[g[0] for g in GOLDEN])
def test_valid_calls_unchanged_by_the_checks(name, key, max_len):
    """o bit for bit what the bindings returned before they gained their
    checks (tests/golden/decode_bindings_head.pt; bf16 stored as int16)."""
    gold = torch.load(os.path.join(os.path.dirname(__file__), os.pardir,
                                   "golden", "decode_bindings_head.pt"),
                      weights_only=True)
    c = ko.decode_case(*key, max_len=max_len)
    assert int(gold[f"{name}.inputs"]) == input_digest(c), \
        "the generated inputs differ from the recorded ones"
    o = run_case(c)
    assert torch.equal(o.cpu(), gold[f"{name}.o"].view(BF16)), name


# ---------------------------------------------------------------------------
# multi_sumsq
# ---------------------------------------------------------------------------
_LISTS = ko.sumsq_lists()


def sumsq_grid(spans):
    C = ko.SUMSQ_CHUNK
    chunks = sum(-(-n // C) for _, n in spans)
    return max(1, min(4 * chunks, ko.SUMSQ_GRID))


def run_sumsq(flat_d, spans):
    views = ko.sumsq_views(flat_d, spans)
    ko.poison(DEV, ((sumsq_grid(spans),), F32), ((1,), F32))
    got = ext().multi_sumsq(views)
    assert got.shape == (1,) and got.dtype == F32
    return got


@pytest.mark.parametrize("name,sizes,off", _LISTS,
                         ids=[c[0] for c in _LISTS])
def test_multi_sumsq(name, sizes, off):
    flat, spans = ko.sumsq_inputs(sizes, off)
    xs = ko.sumsq_views(flat, spans)
    o64, r32 = ko.sumsq(xs), ko.sumsq_ref32(xs)
    flat_d = flat.to(DEV)
    assert all(v.data_ptr() % 16 == (4 * off) % 16
               for v in ko.sumsq_views(flat_d, spans) if v.numel())
    got = run_sumsq(flat_d, spans)
    ko.assert_finite(got, what=f"sumsq {name}")
    err = float((ko.f64(got) - o64).abs())
    e_ref = float((ko.f64(r32) - o64).abs())
    print(f"[sumsq] {name}: kernel error {err:.3g}, E_ref {e_ref:.3g}, "
          f"half ulp {2.0 ** -24 * float(o64):.3g}")
    ko.assert_accum(got.cpu(), r32, o64, f"sumsq {name}")
    if not sum(sizes):
        assert float(got) == 0.0


@pytest.mark.parametrize("bad,where", [(float("inf"), "tail"),
                                       (NAN, "body")])
def test_multi_sumsq_non_finite_shows(bad, where):
    """One inf in a tail element gives inf, one NaN in a body element NaN
    (what the fp16 loss scaler's overflow check reads)."""
    sizes = [5, ko.SUMSQ_CHUNK + 7, 3]
    flat, spans = ko.sumsq_inputs(sizes, 1)
    start, n = spans[1]
    flat[start + (n - 1 if where == "tail" else 4 * 1000 + 1)] = bad
    got = float(run_sumsq(flat.to(DEV), spans))
    assert got == bad or (bad != bad and got != got), got


def test_multi_sumsq_same_bits_every_call():
    flat, spans = ko.sumsq_inputs(ko.SUMSQ_MANY, 3)
    flat_d = flat.to(DEV)
    first = run_sumsq(flat_d, spans).clone()
    for _ in range(2):
        assert torch.equal(run_sumsq(flat_d, spans), first)


def test_multi_sumsq_refuses():
    x = torch.ones(64, device=DEV)
    e = ext()
    with pytest.raises(RuntimeError, match="fp32 contiguous"):
        e.multi_sumsq([x, x.bfloat16()])
    with pytest.raises(RuntimeError, match="contiguous"):
        e.multi_sumsq([x[::2]])
    with pytest.raises(RuntimeError, match="empty list"):
        e.multi_sumsq([])
    with pytest.raises(RuntimeError, match="GPU"):
        e.multi_sumsq([x.cpu()])
    assert float(e.multi_sumsq([x])) == 64.0
