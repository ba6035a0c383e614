#!/usr/bin/env python
"""Record SHA-256 digests of the batched decode kernels' raw outputs.

    python tools/decode_golden.py --parent <commit> \
        > tests/ops/decode_golden_parent.json

Inputs are built on the CPU from fixed seeds; the four decode bindings
(decode_attn_batched, _batched_fp8, _paged, _paged_fp8) and kv_append_fp8 run
on the GPU and the raw bytes of what they write are hashed.  The committed
record was written by the build named inside it, the last one with two chunk
bodies and three merge kernels; tests/ops/test_gpu_decode_golden.py recomputes
the digests, so "the fold left every bit alone" stays checkable after that
build is gone.

One batch of 12 rows serves every attention case: lengths 0, 1, the edges of
a 32-key step and of a 128-key tile, 200, max_len, one above max_len
(clamped) and one row whose slot is outside [0, S); the slots are a
permutation.  The pools are the pages of the contiguous cache, shuffled.  In
the paged cases the max_len row has one page id outside the pool (-1 or P) in
the middle of what it attends to, and the 200 row has nothing but such ids.
"""
import argparse
import functools
import hashlib
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_S = 1280
LENGTHS = (0, 1, 31, 32, 33, 127, 128, 129, 200, MAX_S, MAX_S + 220, 64)
SLOTS = (7, 2, 9, 0, 11, 4, 1, 10, 3, 6, 8, 5)      # row 11: replaced below
N = S = len(LENGTHS)
ROW_FULL, ROW_HOLES, ROW_BAD_SLOT = 9, 8, 11
HEADS = ((4, 4), (8, 2), (16, 1))
FORMATS = ("bf16", "e4m3", "e4m3-noscale")
LAYOUTS = (0, 32, 128)                               # 0: contiguous, else page
F8 = torch.float8_e4m3fn


def attn_cases():
    out = []
    for d, (hq, hkv), fmt, page, nc, w in itertools.product(
            (64, 128), HEADS, FORMATS, LAYOUTS, (1, 3, 0), (0, 37)):
        c = dict(d=d, hq=hq, hkv=hkv, fmt=fmt, page=page, n_chunks=nc,
                 window=w)
        name = "attn-d%d-h%dx%d-%s-%s-c%d-w%d" % (
            d, hq, hkv, fmt, "page%d" % page if page else "contig", nc, w)
        out.append((name, c))
    return out


def append_cases():
    out = []
    for d, hkv, n, scales in itertools.product((64, 128), (1, 8),
                                               (1, 5, 300), (True, False)):
        c = dict(d=d, hkv=hkv, n=n, scales=scales)
        name = "append-d%d-h%d-n%d-%s" % (d, hkv, n,
                                          "scales" if scales else "noscale")
        out.append((name, c))
    return out


ATTN_CASES = attn_cases()
APPEND_CASES = append_cases()


def scales_of(hkv):
    h = torch.arange(hkv, dtype=torch.float32)
    return 0.37 + 0.21 * h, 1.9 - 0.13 * h


@functools.lru_cache(maxsize=2)
def base_inputs(d, hq, hkv, device):
    """q and the contiguous caches of both dtypes, on the device."""
    g = torch.Generator().manual_seed(4000 + 10 * d + hq)
    q = torch.randn(N, hq, d, generator=g).bfloat16()
    k = torch.randn(S, MAX_S, hkv, d, generator=g)
    v = torch.randn(S, MAX_S, hkv, d, generator=g)
    return dict(q=q.to(device),
                bf16=(k.bfloat16().to(device), v.bfloat16().to(device)),
                e4m3=(k.to(F8).to(device), v.to(F8).to(device)))


@functools.lru_cache(maxsize=4)
def page_table(page, window):
    """(table [S, MAX_S / page] int32, pool index of every cache page): a
    seeded shuffle, then the out-of-pool ids of ROW_HOLES and ROW_FULL."""
    mp = MAX_S // page
    g = torch.Generator().manual_seed(77 + page)
    perm = torch.randperm(S * mp, generator=g)
    table = perm.to(torch.int32).reshape(S, mp).clone()
    table[SLOTS[ROW_HOLES], 0::2] = -1
    table[SLOTS[ROW_HOLES], 1::2] = S * mp
    # a position the full row attends to with and without the window
    hole = (MAX_S - 36 if window else MAX_S // 2) // page
    table[SLOTS[ROW_FULL], hole] = S * mp if window else -1
    return table, perm


@functools.lru_cache(maxsize=2)
def pools(d, hq, hkv, fp8, page, device):
    """The contiguous caches as pools [P, page, hkv, d]: cache page j is pool
    page perm[j].  Gathered as bytes."""
    perm = page_table(page, 0)[1]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(len(perm))
    inv = inv.to(device)
    out = []
    for t in base_inputs(d, hq, hkv, device)["e4m3" if fp8 else "bf16"]:
        raw = t.view(torch.uint8).view(len(perm), -1)[inv]
        out.append(raw.view(t.dtype).view(-1, page, hkv, d))
    return tuple(out)


def run_attn(ext, c, device):
    """The case's o [N, hq, d] from its binding."""
    d, hq, hkv, page = c["d"], c["hq"], c["hkv"], c["page"]
    inp = base_inputs(d, hq, hkv, device)
    fp8 = c["fmt"] != "bf16"
    kc, vc = inp["e4m3" if fp8 else "bf16"]
    i32 = dict(dtype=torch.int32, device=device)
    slots = list(SLOTS)
    slots[ROW_BAD_SLOT] = S if c["n_chunks"] == 1 else -1
    if page:
        kc, vc = pools(d, hq, hkv, fp8, page, device)
        table = page_table(page, c["window"])[0]
    args = [inp["q"], kc, vc]
    if fp8:
        args += [s.to(device) for s in scales_of(hkv)] \
            if c["fmt"] == "e4m3" else [None, None]
    if page:
        args.append(table.to(device))
    args += [torch.tensor(LENGTHS, **i32), torch.tensor(slots, **i32), MAX_S,
             d ** -0.5, c["window"], c["n_chunks"]]
    name = "decode_attn_" + ("paged" if page else "batched") \
        + ("_fp8" if fp8 else "")
    return getattr(ext, name)(*args)


def run_append(ext, c, device):
    """The two caches after one append of strided k and v views, some values
    past the e4m3 range; with n > 1, row n // 2 has a position outside the
    cache and is skipped."""
    d, hkv, n = c["d"], c["hkv"], c["n"]
    cs, cmax = 4, 96
    g = torch.Generator().manual_seed(9000 + d + 10 * hkv + n)
    kv = (60.0 * torch.randn(n, hkv, 2, d + 8, generator=g)).bfloat16()
    kv = kv.to(device)
    k, v = kv[:, :, 0, :d], kv[:, :, 1, :d]
    idx = torch.arange(n)
    pos = idx // cs
    if n > 1:
        pos[n // 2] = cmax
    i32 = dict(dtype=torch.int32, device=device)
    kc = torch.zeros(cs, cmax, hkv, d, dtype=torch.uint8, device=device)
    vc = torch.zeros_like(kc)
    sc = [s.to(device) for s in scales_of(hkv)] if c["scales"] \
        else [None, None]
    ext.kv_append_fp8(k, v, kc.view(F8), vc.view(F8),
                      (idx % cs).to(**i32), pos.to(**i32), *sc)
    return torch.cat([kc, vc])


def digest(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True,
                    help="hash of the commit whose build is being recorded")
    a = ap.parse_args()
    from hetu_galvatron_amd.ops._ext import get_ext
    ext = get_ext(False)
    device = torch.device("cuda:0")
    digests = {}
    for name, c in ATTN_CASES:
        digests[name] = digest(run_attn(ext, c, device))
    for name, c in APPEND_CASES:
        digests[name] = digest(run_append(ext, c, device))
    json.dump(dict(parent=a.parent, digests=digests), sys.stdout, indent=0,
              sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
