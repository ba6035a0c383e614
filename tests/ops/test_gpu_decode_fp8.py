"""`decode_attn_batched_fp8` against the fp64 decode oracle on stored *
scale, row by row, under the element rule of kernel_oracle.py (the stored
bytes are the inputs); the NaN byte outside every row's [start, len), heavy
keys at its ends, poisoned outputs.  `kv_append_fp8`: the caches, as bytes,
against torch's divide, clamp and cast."""
import functools
import math

import pytest
import torch

from hetu_galvatron_amd.ops._ext import get_ext

from . import kernel_oracle as ko
from .test_gpu_decode_batched import TILE, chunks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
NAN_BYTE, SENTINEL = 0x7F, 0xA5


def quantise(x, scale):
    """x [..., hkv, d] -> e4m3, the reference arithmetic of the append."""
    return (x.float() / scale[:, None]).clamp(-448, 448).to(F8)


class Case:
    """Inputs, and per row the oracle (o64, scale) or None for an empty row.
    The caches are quantised first; the oracle sees stored * scale."""

    def __init__(self, d, hq, hkv, S, max_s, lengths, slots, window, max_len,
                 scaled=True):
        g = torch.Generator().manual_seed(len(lengths) * 1000 + d + hq)
        n, rep, self.scale = len(lengths), hq // hkv, d ** -0.5
        h = torch.arange(hkv, dtype=torch.float32)
        self.ks = 0.37 + 0.21 * h if scaled else None
        self.vs = 1.9 - 0.13 * h if scaled else None
        ks, vs = (torch.ones(hkv) if s is None else s
                  for s in (self.ks, self.vs))
        q = torch.randn(n, hkv, 1, d, generator=g) \
            + 0.5 * torch.randn(n, hkv, rep, d, generator=g)
        self.q = q.reshape(n, hq, d).bfloat16()
        kr = torch.randn(S, max_s, hkv, d, generator=g)
        vr = torch.randn(S, max_s, hkv, d, generator=g)
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
                assert bool((gain.abs() < 448 * ks).all()), "key saturates"
                kr[s, p] = gain[:, None] * u
                vr[s, p] = (1 + 2 * torch.rand(hkv, d, generator=g)) \
                    * (1 - 2 * (p % 2))
            live[s, st:L] = True
            spans.append((st, L))
        self.k8, self.v8 = quantise(kr, ks), quantise(vr, vs)
        self.k8.view(torch.uint8)[~live] = NAN_BYTE
        self.v8.view(torch.uint8)[~live] = NAN_BYTE
        k64 = self.k8.double() * ks.double()[:, None]
        v64 = self.v8.double() * vs.double()[:, None]
        self.ref = []
        for i, sp in enumerate(spans):
            if sp is None:
                self.ref.append(None)
                continue
            s = slots[i]
            a = (self.q[i:i + 1], k64[s:s + 1], v64[s:s + 1], sp[1],
                 self.scale, sp[0])
            o64, aux = ko.decode_attn(*a)
            self.ref.append((o64, ko.decode_scale(*a, o64, aux)))

    def tensors(self, dev=DEV):
        """q, k8, v8, k_scale, v_scale, lengths, slots on `dev`."""
        i32 = dict(dtype=torch.int32, device=dev)
        sc = [None if s is None else s.to(dev) for s in (self.ks, self.vs)]
        return (self.q.to(dev), self.k8.to(dev), self.v8.to(dev), *sc,
                torch.tensor(self.lengths, **i32),
                torch.tensor(self.slots, **i32))

    def run(self, n_chunks, tensors=None):
        n, hq, hkv, d = self.dims
        span = min(self.max_len, self.window or self.max_len)
        nc = chunks(n, hkv, span, n_chunks)[0]
        ko.poison(DEV, ((n, hq, d), BF16), ((n * hq * nc * (d + 2),),
                                            torch.float32))
        return get_ext(False).decode_attn_batched_fp8(
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

RAGGED = [(d, hq, hkv, nc, w, True) for d in (64, 128)
          for hq, hkv in ((4, 4), (8, 2), (16, 1)) for nc in (1, 3, 0)
          for w in (0, 37)] + [(128, 8, 2, 0, 0, False), (64, 8, 2, 3, 37, False)]


@pytest.mark.parametrize("d,hq,hkv,n_chunks,window,scaled", RAGGED)
def test_ragged_lengths(d, hq, hkv, n_chunks, window, scaled):
    max_s = 1280
    nc, chunk = chunks(6, hkv, window or max_s, n_chunks)
    lengths = (1, TILE - 1, TILE, TILE + 1, 2 * chunk + 1, max_s)
    c = case(d, hq, hkv, 8, max_s, lengths, (5, 0, 7, 2, 3, 6), window, max_s,
             scaled)
    c.check(c.run(n_chunks), f"ragged d={d} h={hq}/{hkv} w={window} "
                             f"chunks={nc}x{chunk} scaled={scaled}")


@pytest.mark.parametrize("n_chunks", [0, 1, 2])
@pytest.mark.parametrize("key", [
    (128, 4, 1, 2, 8320, (8200, 3), (1, 0), 0, 8200),
    (128, 8, 2, 3, 1280, (0, 300, 700), (1, 2, 0), 0, 520)],
    ids=["long", "empty-clamped"])
def test_long_empty_and_clamped_rows(key, n_chunks):
    c = case(*key)
    c.check(c.run(n_chunks), f"lengths {key[5]} n_chunks={n_chunks}")


@pytest.mark.parametrize("length,first", [(200, 160), (190, 158)],
                         ids=["full-step", "last-step"])
@pytest.mark.parametrize("d", [64, 128])
def test_one_hot_weight_returns_the_stored_v_row(d, length, first):
    """Row i's q is 64 e_i and key first + i is 64 e_i (stored), every other
    key zero: the score gap is 4096 scale k_scale >= 134 > 126 ln 2, every
    other weight underflows to 0 and o is bf16(v_scale * stored V row)."""
    hq, hkv, n = 8, 2, min(32, length - first)
    g = torch.Generator().manual_seed(d + first)
    ks = torch.tensor([0.37, 0.58])
    vs = torch.tensor([1.9, 1.77])
    assert 4096 * d ** -0.5 * float(ks.min()) > 126 * math.log(2)
    k = torch.zeros(1, 256, hkv, d)
    k[0, first + torch.arange(n), :, torch.arange(n)] = 64.0
    vbytes = torch.randint(0, 256, (1, 256, hkv, d), generator=g,
                           dtype=torch.uint8)
    vbytes[vbytes & 0x7F == NAN_BYTE] = 0x3A
    v8 = vbytes.view(F8)
    q = torch.zeros(n, hq, d)
    q[torch.arange(n), :, torch.arange(n)] = 64.0
    i32 = dict(dtype=torch.int32, device=DEV)
    o = get_ext(False).decode_attn_batched_fp8(
        q.bfloat16().to(DEV), k.to(F8).to(DEV), v8.to(DEV), ks.to(DEV),
        vs.to(DEV), torch.full((n,), length, **i32), torch.zeros(n, **i32),
        256, d ** -0.5, 0, 0)
    want = (v8[0, first:first + n].float() * vs[:, None]).bfloat16()
    assert torch.equal(o.cpu(), want.repeat_interleave(hq // hkv, dim=1))


def test_graph_replay():
    """One captured call; lengths, slots and caches then change in place."""
    a = case(128, 8, 2, 4, 1280, (300, 5, 1000), (2, 0, 3), 0, 1280)
    b = case(128, 8, 2, 4, 1280, (129, 777, 2), (1, 3, 0), 0, 1280)
    t = a.tensors()
    a.run(0, t)                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = get_ext(False).decode_attn_batched_fp8(*t, a.max_len, a.scale,
                                                   0, 0)
    for c in (a, b, a):
        for dst, src in zip(t, c.tensors()):
            dst.copy_(src)
        o.fill_(float("nan"))
        graph.replay()
        c.check(o, f"graph replay lengths {c.lengths}")
        assert torch.equal(o, c.run(0, t))


def append_case(n, hkv, d, dev, S=4, max_s=128, qpg=2):
    """The binding's arguments (k, v: views of a packed buffer; sentinel
    caches) and the caches it must leave.  Every other element is a special
    value times its head's scale: +-0, +-448 and beyond, every midpoint of
    adjacent e4m3 codes (2^-10 included).  k_scale is a power of two (exact
    quotients); v_scale is not (the division's rounding)."""
    g = torch.Generator().manual_seed(n * 100 + hkv * 10 + d)
    codes = torch.arange(0, 127, dtype=torch.uint8).view(F8).float()
    sp = torch.cat([codes, (codes[:-1] + codes[1:]) / 2,
                    torch.tensor([464.0, 480.0, 1e4])])
    sp = torch.cat([sp, -sp])
    ks = 2.0 ** (torch.arange(hkv) % 3 - 1).float()
    vs = 0.37 + 0.21 * torch.arange(hkv).float()
    buf = torch.randn(n, hkv, qpg + 2, d, generator=g) * 40
    idx = torch.arange(n * hkv * d).reshape(n, hkv, d)
    for j, s in ((qpg, ks), (qpg + 1, vs)):
        special = sp[(idx // 2 + j) % len(sp)] * s[:, None]
        buf[:, :, j] = torch.where(idx % 2 == 0, special, buf[:, :, j])
    buf = buf.bfloat16()
    k, v = buf[:, :, qpg], buf[:, :, qpg + 1]
    perm = torch.randperm(S * max_s, generator=g)[:n]
    slots, pos = (perm // max_s).int(), (perm % max_s).int()
    if n >= 5:                               # rows the kernel must skip
        slots[0], slots[1], pos[2] = -1, S, max_s
    keep = (slots >= 0) & (slots < S) & (pos < max_s)
    want = []
    for x, s in ((k, ks), (v, vs)):
        c = torch.full((S, max_s, hkv, d), SENTINEL, dtype=torch.uint8)
        c[slots[keep].long(), pos[keep].long()] = \
            quantise(x[keep], s).view(torch.uint8)
        want.append(c)
    buf = buf.to(dev)
    caches = [torch.full((S, max_s, hkv, d), SENTINEL, dtype=torch.uint8,
                         device=dev).view(F8) for _ in range(2)]
    args = (buf[:, :, qpg], buf[:, :, qpg + 1], *caches, slots.to(dev),
            pos.to(dev), ks.to(dev), vs.to(dev))
    return args, want


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("hkv", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 5, 300])
def test_append_bytes(n, hkv, d):
    args, want = append_case(n, hkv, d, DEV)
    get_ext(False).kv_append_fp8(*args)
    for got, ref, name in zip(args[2:4], want, "kv"):
        diff = (got.view(torch.uint8).cpu() != ref).nonzero()
        assert not len(diff), f"{name}_cache differs at {diff[:4].tolist()}"


BAD = {  # name -> (refusal, change of the binding's tensor arguments)
    "cache_bf16": ("k_cache must", lambda a: a.update(
        kc=a["kc"].to(BF16), vc=a["vc"].to(BF16))),
    "scale_shape": ("k_scale must", lambda a: a.update(
        ks=torch.ones(3, device=DEV))),
    "scale_fp64": ("v_scale must", lambda a: a.update(vs=a["vs"].double())),
    "scale_cpu": ("k_scale must", lambda a: a.update(ks=a["ks"].cpu())),
    "lengths_int64": ("lengths must", lambda a: a.update(
        lengths=a["lengths"].long())),
    "qpg_32": ("qpg", lambda a: a.update(
        q=torch.zeros(3, 64, 64, dtype=BF16, device=DEV)))}


@pytest.mark.parametrize("bad", list(BAD))
def test_binding_refuses(bad):
    c = case(64, 8, 2, 3, 1280, (0, 300, 700), (1, 2, 0), 0, 520)
    a = dict(zip(("q", "kc", "vc", "ks", "vs", "lengths", "slots"),
                 c.tensors()))
    BAD[bad][1](a)
    with pytest.raises(RuntimeError, match=BAD[bad][0]):
        get_ext(False).decode_attn_batched_fp8(*a.values(), c.max_len,
                                               c.scale, 0, 0)
    with pytest.raises(RuntimeError, match="k_cache must"):
        get_ext(False).decode_attn_batched(
            c.q.to(DEV), c.k8.to(DEV), c.v8.to(DEV), a["slots"], a["slots"],
            c.max_len, c.scale, 0, 0)
