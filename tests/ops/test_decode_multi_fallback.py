"""`decode_attention_multi` off the native path (the CPU) against the fp64
decode oracle on each token's attended positions, under the element rule of
kernel_oracle.py.  `Case` also serves the GPU tests of the native kernels."""
import pytest
import torch

from hetu_galvatron_amd.ops import decode_attention_multi

from . import kernel_oracle as ko

BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
NAN_BYTE = 0x7F


class Case:
    """rows: (length, q_len[, slot]) per q row; page None: contiguous caches.
    NaN (the NaN byte for e4m3) in every cache or pool position that no token
    attends to and in every q row t >= q_len.  `holes`: {row: page index}
    whose table entry becomes -1 (even rows) or P (odd rows).  ref[i][t] is
    the oracle (o64, scale), or None where o[i, t] must be zeros."""

    def __init__(self, fp8, page, d, hq, hkv, T, window, rows, max_len,
                 holes=None, seed=0, pool=None):
        g = torch.Generator().manual_seed(1000 * T + d + hq + seed)
        n, self.scale, holes = len(rows), d ** -0.5, holes or {}
        self.fp8, self.page, self.window, self.max_len = fp8, page, window, \
            max_len
        self.dims = (n, T, hq, hkv, d)
        self.lengths = [r[0] for r in rows]
        self.q_lens = [r[1] for r in rows]
        self.slots = [r[2] if len(r) > 2 else n - 1 - i
                      for i, r in enumerate(rows)]
        h = torch.arange(hkv, dtype=torch.float32)
        self.ks = 0.37 + 0.21 * h if fp8 else None
        self.vs = 1.9 - 0.13 * h if fp8 else None
        self.q = torch.randn(n, T, hq, d, generator=g).bfloat16()
        ok = [0 < L <= max_len and 0 <= ql <= min(T, L) and 0 <= s < n
              for L, ql, s in zip(self.lengths, self.q_lens, self.slots)]
        for i in range(n):
            self.q[i, self.q_lens[i] if ok[i] else 0:] = float("nan")
        lo = lambda pos: max(0, pos + 1 - window) if window else 0
        if page:
            need = sum(-(-L // page) for L, v in zip(self.lengths, ok) if v)
            P = pool or 2 * need + 1
            perm = torch.randperm(P, generator=g).tolist()
            self.table = torch.full((n, max_len // page), -1,
                                    dtype=torch.int32)
            shape = (P, page, hkv, d)
        else:
            shape = (n, max_len, hkv, d)
        kr, vr = (torch.full(shape, float("nan")) for _ in "kv")
        where = []                       # per row: storage index of lo0 .. L-1
        for i, (L, ql, s) in enumerate(zip(self.lengths, self.q_lens,
                                           self.slots)):
            if not ok[i] or ql == 0:
                where.append(None)
                continue
            pos = torch.arange(lo(L - ql), L)
            if page:
                ids = torch.tensor([perm.pop() for _ in range(-(-L // page))])
                self.table[s, :len(ids)] = ids.int()
                idx = (ids[pos // page], pos % page)
            else:
                idx = (torch.full_like(pos, s), pos)
            kr[idx] = torch.randn(len(pos), hkv, d, generator=g)
            vr[idx] = torch.randn(len(pos), hkv, d, generator=g)
            where.append((pos, idx))
        if fp8:
            dead = kr[:, :, 0, 0].isnan()
            self.kc = (kr.nan_to_num(0.) / self.ks[:, None]).to(F8)
            self.vc = (vr.nan_to_num(0.) / self.vs[:, None]).to(F8)
            self.kc.view(torch.uint8)[dead] = NAN_BYTE
            self.vc.view(torch.uint8)[dead] = NAN_BYTE
        else:
            self.kc, self.vc = kr.bfloat16(), vr.bfloat16()
        for i, pi in holes.items():
            self.table[self.slots[i], pi] = -1 if i % 2 == 0 else P
        self.ref = []
        for i, w in enumerate(where):
            self.ref.append([None] * T)
            if w is None:
                continue
            pos, idx = w
            k, v = self.kc[idx].double(), self.vc[idx].double()
            if fp8:
                k = k * self.ks.double()[:, None]
                v = v * self.vs.double()[:, None]
            for t in range(self.q_lens[i]):
                p = self.lengths[i] - self.q_lens[i] + t
                keep = (pos >= lo(p)) & (pos <= p)
                if i in holes:
                    keep &= pos // page != holes[i]
                if not keep.any():
                    continue
                a = (self.q[i, t][None], k[keep][None], v[keep][None],
                     int(keep.sum()), self.scale, 0)
                o64, aux = ko.decode_attn(*a)
                self.ref[i][t] = (o64, ko.decode_scale(*a, o64, aux))

    def tensors(self, dev):
        i32 = dict(dtype=torch.int32, device=dev)
        kw = dict(q=self.q.to(dev), k_cache=self.kc.to(dev),
                  v_cache=self.vc.to(dev),
                  lengths=torch.tensor(self.lengths, **i32),
                  q_lens=torch.tensor(self.q_lens, **i32),
                  slots=torch.tensor(self.slots, **i32))
        if self.fp8:
            kw.update(k_scale=self.ks.to(dev), v_scale=self.vs.to(dev))
        if self.page:
            kw.update(page_table=self.table.to(dev))
        return kw

    def run(self, dev, n_chunks=None, tensors=None):
        return decode_attention_multi(
            **(tensors or self.tensors(dev)), window=self.window,
            max_len=self.max_len, softmax_scale=self.scale,
            n_chunks=n_chunks)

    def check(self, o, what):
        got = o.cpu()
        for i, row in enumerate(self.ref):
            for t, ref in enumerate(row):
                w = f"{what} row {i} (len {self.lengths[i]}) token {t}"
                if ref is None:
                    assert not got[i, t].any(), f"{w}: not zeros"
                else:
                    ko.assert_elem(got[i, t][None], ref[0], ref[1], w)


@pytest.mark.parametrize("window", [0, 2, 37])
@pytest.mark.parametrize("hq,hkv,T", [(4, 4, 1), (8, 2, 5), (6, 2, 6)])
@pytest.mark.parametrize("page", [None, 32])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_fallback_against_oracle(fp8, page, hq, hkv, T, window):
    rows = [(T, T), (33, min(T, 3)), (129, T), (50, 0), (90, 1), (0, 1),
            (161, T), (77, T, 99), (40, T + 1)]
    c = Case(fp8, page, 64, hq, hkv, T, window, rows, 160)
    assert c.ref[2][T - 1] is not None and c.ref[6][0] is None  # 161 > max_len
    c.check(c.run("cpu"), f"fallback fp8={fp8} page={page} h={hq}/{hkv} "
                          f"T={T} w={window}")


def test_fallback_skips_invalid_pages():
    c = Case(True, 32, 64, 8, 2, 5, 0, [(20, 5), (100, 5), (70, 3)], 128,
             holes={0: 0, 1: 1})
    assert c.ref[0] == [None] * 5 and c.ref[1][4] is not None
    c.check(c.run("cpu"), "fallback holes")
