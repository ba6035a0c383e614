"""`decode_attn_paged` / `decode_attn_paged_fp8` against the fp64 decode oracle
on each row's pages gathered on the CPU, under the element rule of
kernel_oracle.py.  Page ids come from a shuffled pool about twice the need;
NaN (bf16) or the NaN byte (e4m3) in every pool position no row attends to;
a heavy key at each row's first and last position; poisoned outputs."""
import functools
import math

import pytest
import torch

from hetu_galvatron_amd.ops._ext import get_ext

from . import kernel_oracle as ko
from .test_gpu_decode_batched import chunks
from .test_gpu_decode_fp8 import NAN_BYTE, quantise

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn


def span_of(window, max_len):
    """What the binding splits: a windowed row's tiles start on the 32-key
    grid, up to 31 positions before its window."""
    return min(max_len, window + 31) if window else max_len


class Case:
    """Inputs, and per row the oracle (o64, scale) or None for an empty row.
    `holes`: {row: page index} whose table entry becomes -1 (even rows) or
    P (odd rows) and whose positions the oracle leaves out."""

    def __init__(self, fp8, d, hq, hkv, page, lengths, window, max_len,
                 holes=None, seed=0, pool=None):
        g = torch.Generator().manual_seed(1000 * page + d + hq + seed)
        n, rep, self.scale = len(lengths), hq // hkv, d ** -0.5
        self.fp8, self.window, self.max_len = fp8, window, max_len
        self.lengths, self.dims = list(lengths), (n, hq, hkv, d)
        mp = max_len // page
        P = pool or 2 * sum(-(-min(L, max_len) // page) for L in lengths) + 1
        perm = torch.randperm(P, generator=g).tolist()
        h = torch.arange(hkv, dtype=torch.float32)
        self.ks = 0.37 + 0.21 * h if fp8 else None
        self.vs = 1.9 - 0.13 * h if fp8 else None
        ks, vs = (torch.ones(hkv) if s is None else s
                  for s in (self.ks, self.vs))
        q = torch.randn(n, hkv, 1, d, generator=g) \
            + 0.5 * torch.randn(n, hkv, rep, d, generator=g)
        self.q = q.reshape(n, hq, d).bfloat16()
        kr = torch.randn(P, page, hkv, d, generator=g)
        vr = torch.randn(P, page, hkv, d, generator=g)
        self.table = torch.full((n, mp), -1, dtype=torch.int32)
        live = torch.zeros(P, page, dtype=torch.bool)
        rows = []                            # per row: (pool pages, offsets)
        for i, L in enumerate(lengths):
            L = min(L, max_len)
            if L <= 0:
                rows.append(None)
                continue
            ids = torch.tensor([perm.pop() for _ in range(-(-L // page))])
            self.table[i, :len(ids)] = ids
            st = max(0, L - window) if window else 0
            pos = torch.arange(st, L)
            pg, off = ids[pos // page], pos % page
            qg = self.q[i].float().reshape(hkv, rep, d)
            u = qg.mean(1)
            u = u / u.norm(dim=-1, keepdim=True)
            align = (qg * u[:, None]).sum(-1).mean(-1)
            for j, t in ((0, 1.5), (-1, 2.0)):          # the heavy keys
                gain = (math.log(L - st) + t) / (self.scale * align)
                assert bool((gain.abs() < 448 * ks).all()), "key saturates"
                kr[pg[j], off[j]] = gain[:, None] * u
                vr[pg[j], off[j]] = (1 + 2 * torch.rand(hkv, d, generator=g)) \
                    * (1 - 2 * (int(pos[j]) % 2))
            live[pg, off] = True
            keep = pos // page != holes.get(i, -1) if holes else pos >= 0
            rows.append((pg[keep], off[keep]) if keep.any() else None)
        if fp8:
            self.kp, self.vp = quantise(kr, ks), quantise(vr, vs)
            self.kp.view(torch.uint8)[~live] = NAN_BYTE
            self.vp.view(torch.uint8)[~live] = NAN_BYTE
        else:
            self.kp, self.vp = kr.bfloat16(), vr.bfloat16()
            self.kp[~live] = float("nan")
            self.vp[~live] = float("nan")
        for i, pi in (holes or {}).items():
            self.table[i, pi] = -1 if i % 2 == 0 else P
        self.ref = []
        for i, r in enumerate(rows):
            if r is None:
                self.ref.append(None)
                continue
            k = self.kp[r[0], r[1]][None]
            v = self.vp[r[0], r[1]][None]
            if fp8:
                k = k.double() * ks.double()[:, None]
                v = v.double() * vs.double()[:, None]
            a = (self.q[i:i + 1], k, v, k.shape[1], self.scale, 0)
            o64, aux = ko.decode_attn(*a)
            self.ref.append((o64, ko.decode_scale(*a, o64, aux)))

    def tensors(self):
        """q, pools, [scales,] table, lengths, slots on the device."""
        i32 = dict(dtype=torch.int32, device=DEV)
        sc = [self.ks.to(DEV), self.vs.to(DEV)] if self.fp8 else []
        n = len(self.lengths)
        return (self.q.to(DEV), self.kp.to(DEV), self.vp.to(DEV), *sc,
                self.table.to(DEV), torch.tensor(self.lengths, **i32),
                torch.arange(n, **i32))

    def run(self, n_chunks, tensors=None):
        n, hq, hkv, d = self.dims
        nc = chunks(n, hkv, span_of(self.window, self.max_len), n_chunks)[0]
        ko.poison(DEV, ((n, hq, d), BF16), ((n * hq * nc * (d + 2),),
                                            torch.float32))
        ext = get_ext(False)
        f = ext.decode_attn_paged_fp8 if self.fp8 else ext.decode_attn_paged
        return f(*(tensors or self.tensors()), self.max_len, self.scale,
                 self.window, n_chunks)

    def check(self, o, what):
        got = o.cpu()
        for i, ref in enumerate(self.ref):
            if ref is None:
                assert not got[i].any(), f"{what}: empty row {i} is not zero"
            else:
                ko.assert_elem(got[i:i + 1], ref[0], ref[1],
                               f"{what} row {i} len {self.lengths[i]}")


case = functools.lru_cache(maxsize=4)(Case)


@pytest.mark.parametrize("window", [0, 37])
@pytest.mark.parametrize("n_chunks", [1, 3, 0])
@pytest.mark.parametrize("page", [32, 128])
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2), (16, 1)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_ragged_lengths(fp8, d, hq, hkv, page, n_chunks, window):
    max_len = 1280
    nc, chunk = chunks(6, hkv, span_of(window, max_len), n_chunks)
    lengths = (1, page - 1, page, page + 1, 2 * chunk + 1, max_len)
    c = case(fp8, d, hq, hkv, page, lengths, window, max_len)
    c.check(c.run(n_chunks), f"paged fp8={fp8} d={d} h={hq}/{hkv} "
                             f"page={page} w={window} chunks={nc}x{chunk}")


@pytest.mark.parametrize("page", [32, 256])
@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_bit_identical_to_contiguous(fp8, d, n_chunks, page):
    """The same storage as a cache [S, max_s] and as a pool of its pages."""
    S, max_s, hq, hkv = 3, 768, 8, 2
    g = torch.Generator().manual_seed(d + page)
    q = torch.randn(S, hq, d, generator=g).bfloat16().to(DEV)
    kc, vc = (torch.randn(S, max_s, hkv, d, generator=g) for _ in "kv")
    i32 = dict(dtype=torch.int32, device=DEV)
    lengths = torch.tensor([max_s, 301, 33], **i32)
    slots = torch.tensor([2, 0, 1], **i32)
    table = torch.arange(S * max_s // page, **i32).reshape(S, -1)
    ext, tail = get_ext(False), (lengths, slots, max_s, d ** -0.5, 0, n_chunks)
    if fp8:
        sc = [torch.tensor([0.37, 0.58], device=DEV),
              torch.tensor([1.9, 1.77], device=DEV)]
        kc, vc = kc.to(F8).to(DEV), vc.to(F8).to(DEV)
        want = ext.decode_attn_batched_fp8(q, kc, vc, *sc, *tail)
        got = ext.decode_attn_paged_fp8(
            q, kc.view(-1, page, hkv, d), vc.view(-1, page, hkv, d), *sc,
            table, *tail)
    else:
        kc, vc = kc.bfloat16().to(DEV), vc.bfloat16().to(DEV)
        want = ext.decode_attn_batched(q, kc, vc, *tail)
        got = ext.decode_attn_paged(q, kc.view(-1, page, hkv, d),
                                    vc.view(-1, page, hkv, d), table, *tail)
    assert torch.equal(got, want)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_invalid_pages_are_skipped(fp8):
    """Row 2's page 1 is -1, row 3's page 2 is P: those positions drop out
    of the oracle; the rows beside them are untouched; row 0's only page is
    invalid, so it is zeros."""
    c = Case(fp8, 128, 8, 2, 32, (20, 300, 200, 333), 0, 512,
             holes={0: 0, 2: 1, 3: 2})
    assert c.ref[0] is None and c.ref[1] is not None
    for n_chunks in (1, 2):
        c.check(c.run(n_chunks), f"holes n_chunks={n_chunks}")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_graph_replay(fp8):
    """One captured call; lengths, table and pools then change in place."""
    a = Case(fp8, 128, 8, 2, 64, (300, 5, 1000), 0, 1280, pool=45)
    b = Case(fp8, 128, 8, 2, 64, (129, 777, 2), 0, 1280, seed=1, pool=45)
    t = a.tensors()
    a.run(0, t)                              # warm-up outside the capture
    torch.cuda.synchronize()
    ext = get_ext(False)
    f = ext.decode_attn_paged_fp8 if fp8 else ext.decode_attn_paged
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = f(*t, a.max_len, a.scale, 0, 0)
    for c in (a, b, a):
        for dst, src in zip(t, c.tensors()):
            dst.copy_(src)
        o.fill_(float("nan"))
        graph.replay()
        c.check(o, f"graph replay lengths {c.lengths}")
        assert torch.equal(o, c.run(0, t))


BAD = {  # name -> (refusal, change of the binding's arguments)
    "table_int64": ("page_table must", lambda a: a.update(
        table=a["table"].long())),
    "table_cpu": ("page_table must", lambda a: a.update(
        table=a["table"].cpu())),
    "page_48": ("page ", lambda a: a.update(
        kp=a["kp"][:, :48].contiguous(), vp=a["vp"][:, :48].contiguous())),
    "max_len_past": ("max_len must", lambda a: a.update(max_len=1281)),
    "slots_n_plus_1": ("slots must", lambda a: a.update(
        slots=torch.zeros(4, dtype=torch.int32, device=DEV)))}


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_binding_refuses(fp8, bad):
    c = case(fp8, 64, 8, 2, 64, (0, 300, 700), 0, 1280)
    names = ("q", "kp", "vp") + (("ks", "vs") if fp8 else ()) \
        + ("table", "lengths", "slots")
    a = dict(zip(names, c.tensors()), max_len=c.max_len)
    BAD[bad][1](a)
    ext = get_ext(False)
    f = ext.decode_attn_paged_fp8 if fp8 else ext.decode_attn_paged
    with pytest.raises(RuntimeError, match=BAD[bad][0]):
        f(*a.values(), c.scale, 0, 0)
    c.check(c.run(0), "after a refusal")
