"""`decode_attn_batched` against the fp64 decode oracle, row by row, under
the element rule of kernel_oracle.py.  NaN in every cache position outside a
row's [start, len) and in unused cache rows; a heavy key at each row's first
and last position; `o` and the workspace over NaN-poisoned memory.  Not
exercised: a slot outside [0, S)."""
import functools
import math

import pytest
import torch

from hetu_galvatron_amd.ops._ext import get_ext

from . import kernel_oracle as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
NAN = float("nan")
TILE = 128                                   # key tile of the kernel


def chunks(n, hkv, span, forced):
    """(n_chunks, chunk) as the binding forms them for the longest window."""
    nc = forced or min(max(1, 512 // (n * hkv)), -(-span // 256))
    nc = min(nc, -(-span // TILE))
    chunk = -(-(-(-span // nc)) // TILE) * TILE
    return -(-span // chunk), chunk


class Case:
    """Inputs, and per row the oracle (o64, scale) or None for an empty row.
    `lengths` are the device values; a row attends to min(length, max_len)."""

    def __init__(self, d, hq, hkv, S, max_s, lengths, slots, window, max_len):
        g = torch.Generator().manual_seed(len(lengths) * 1000 + d + hq)
        n, rep, self.scale = len(lengths), hq // hkv, d ** -0.5
        q = torch.randn(n, hkv, 1, d, generator=g) \
            + 0.5 * torch.randn(n, hkv, rep, d, generator=g)
        self.q = q.reshape(n, hq, d).bfloat16()
        self.kc = torch.randn(S, max_s, hkv, d, generator=g).bfloat16()
        self.vc = torch.randn(S, max_s, hkv, d, generator=g).bfloat16()
        self.lengths, self.slots = list(lengths), list(slots)
        self.window, self.max_len, self.dims = window, max_len, (n, hq, hkv, d)
        live = torch.zeros(S, max_s, dtype=torch.bool)
        spans = []
        for i, (L, s) in enumerate(zip(lengths, slots)):
            L = min(L, max_len)
            if L <= 0:
                spans.append(None)
                continue
            st = max(0, L - window) if window else 0
            qg = self.q[i].float().reshape(hkv, rep, d)
            u = qg.mean(1)
            u = u / u.norm(dim=-1, keepdim=True)
            align = (qg * u[:, None]).sum(-1).mean(-1)
            for p, t in ((st, 1.5), (L - 1, 2.0)):      # the heavy keys
                gain = (math.log(L - st) + t) / (self.scale * align)
                self.kc[s, p] = (gain[:, None] * u).bfloat16()
                self.vc[s, p] = (1 + 2 * torch.rand(hkv, d, generator=g)) \
                    .bfloat16() * (1 - 2 * (p % 2))
            live[s, st:L] = True
            spans.append((st, L))
        self.kc[~live] = NAN
        self.vc[~live] = NAN
        self.ref = []
        for i, sp in enumerate(spans):
            if sp is None:
                self.ref.append(None)
                continue
            s = slots[i]
            a = (self.q[i:i + 1], self.kc[s:s + 1], self.vc[s:s + 1], sp[1],
                 self.scale, sp[0])
            o64, aux = ko.decode_attn(*a)
            self.ref.append((o64, ko.decode_scale(*a, o64, aux)))

    def tensors(self):
        i32 = dict(dtype=torch.int32, device=DEV)
        return (self.q.to(DEV), self.kc.to(DEV), self.vc.to(DEV),
                torch.tensor(self.lengths, **i32),
                torch.tensor(self.slots, **i32))

    def run(self, n_chunks, tensors=None):
        n, hq, hkv, d = self.dims
        span = min(self.max_len, self.window or self.max_len)
        nc = chunks(n, hkv, span, n_chunks)[0]
        ko.poison(DEV, ((n, hq, d), BF16), ((n * hq * nc * (d + 2),),
                                            torch.float32))
        return get_ext(False).decode_attn_batched(
            *(tensors or self.tensors()), self.max_len, self.scale,
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
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2), (16, 1)])
@pytest.mark.parametrize("d", [64, 128])
def test_ragged_lengths(d, hq, hkv, n_chunks, window):
    max_s = 1280
    nc, chunk = chunks(6, hkv, window or max_s, n_chunks)
    lengths = (1, TILE - 1, TILE, TILE + 1, 2 * chunk + 1, max_s)
    c = case(d, hq, hkv, 8, max_s, lengths, (5, 0, 7, 2, 3, 6), window, max_s)
    c.check(c.run(n_chunks), f"ragged d={d} h={hq}/{hkv} w={window} "
                             f"chunks={nc}x{chunk}")


@pytest.mark.parametrize("n_chunks", [0, 1, 2])
@pytest.mark.parametrize("key", [
    # 8200 positions: 33 chunks, 2, or one (LDS does not grow with length)
    (128, 4, 1, 2, 8320, (8200, 3), (1, 0), 0, 8200),
    # length 0 gives zeros; a device length of 700 with max_len 520 is the
    # result for 520 (positions from 520 on hold NaN, inside the cache)
    (128, 8, 2, 3, 1280, (0, 300, 700), (1, 2, 0), 0, 520)],
    ids=["long", "empty-clamped"])
def test_long_empty_and_clamped_rows(key, n_chunks):
    c = case(*key)
    c.check(c.run(n_chunks), f"lengths {key[5]} n_chunks={n_chunks}")


def test_graph_replay():
    """One captured call; lengths, slots and caches then change in place."""
    a = case(128, 8, 2, 4, 1280, (300, 5, 1000), (2, 0, 3), 0, 1280)
    b = case(128, 8, 2, 4, 1280, (129, 777, 2), (1, 3, 0), 0, 1280)
    assert torch.equal(a.q, b.q)
    t = a.tensors()
    a.run(0, t)                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = get_ext(False).decode_attn_batched(*t, a.max_len, a.scale, 0, 0)
    for c in (a, b, a):
        for dst, src in zip(t, c.tensors()):
            dst.copy_(src)
        o.fill_(NAN)
        graph.replay()
        c.check(o, f"graph replay lengths {c.lengths}")
        assert torch.equal(o, c.run(0, t))


def test_agrees_with_decode_attn():
    """Uniform lengths, identity slots: both kernels meet the same oracle."""
    c = ko.decode_case(8, 32, 2, 64, 512, 300, 37)
    q, kc, vc = c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    new = get_ext(False).decode_attn_batched(
        q, kc, vc, torch.full((8,), c.cur, **i32), torch.arange(8, **i32),
        c.max_s, c.scale, c.n, 0)
    old = get_ext(False).decode_attn(q, kc, vc, c.cur, c.scale, c.start)
    ko.assert_elem(new.cpu(), c.o, c.sc, f"batched {c.tag}")
    ko.assert_elem(old.cpu(), c.o, c.sc, f"decode_attn {c.tag}")


BAD = {  # name -> (refusal, change of (q, kc, vc, lengths, slots, max_len))
    "lengths_int64": ("lengths must", lambda a: a.update(
        lengths=a["lengths"].long())),
    "lengths_cpu": ("lengths must", lambda a: a.update(
        lengths=a["lengths"].cpu())),
    "slots_n_plus_1": ("slots must", lambda a: a.update(
        slots=torch.zeros(4, dtype=torch.int32, device=DEV))),
    "max_len_past": ("max_len must", lambda a: a.update(max_len=1281)),
    "qpg_32": ("qpg", lambda a: a.update(
        q=torch.zeros(3, 64, 64, dtype=BF16, device=DEV))),
    "cache_fp32": ("k_cache must", lambda a: a.update(
        kc=a["kc"].float(), vc=a["vc"].float()))}


@pytest.mark.parametrize("bad", list(BAD))
def test_binding_refuses(bad):
    c = case(64, 8, 2, 3, 1280, (0, 300, 700), (1, 2, 0), 0, 520)
    a = dict(zip(("q", "kc", "vc", "lengths", "slots"), c.tensors()),
             max_len=c.max_len)
    BAD[bad][1](a)
    with pytest.raises(RuntimeError, match=BAD[bad][0]):
        get_ext(False).decode_attn_batched(*a.values(), c.scale, 0, 0)
    c.check(c.run(0), "after a refusal")
