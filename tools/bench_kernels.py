#!/usr/bin/env python3
"""Standalone per-kernel microbenchmarks (GPU box).

python tools/bench_kernels.py [flash|varlen|qkv|qkv-varlen|decode-batched|decode-paged|decode-multi|decode-prefill|decode-prologue|norms|elementwise|adam|all] [--iters N]

Prints per-kernel wall time + achieved TF/s (compute) or GB/s (memory).
Used with rocprofv3 PMC runs to drive the guide's diagnostic loop.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def timeit(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_flash(iters):
    e = ext()
    # bench-shape slice: one microbatch of the llama-3-8b bench
    b, s, hq, hkv, d = 1, 4096, 32, 8, 128
    q = torch.randn(b, s, hq, d, device="cuda").bfloat16()
    k = torch.randn(b, s, hkv, d, device="cuda").bfloat16()
    v = torch.randn(b, s, hkv, d, device="cuda").bfloat16()
    scale = 1.0 / math.sqrt(d)
    t = timeit(lambda: e.flash_attn_fwd(q, k, v, True, scale), iters)
    flops = 4 * b * hq * (s * s / 2) * d  # QK^T + PV, causal
    print(f"flash_fwd  b{b} s{s} hq{hq} d{d}: {t*1e3:8.2f} ms  "
          f"{flops/t/1e12:7.1f} TF/s")
    o, lse = e.flash_attn_fwd(q, k, v, True, scale)
    do = torch.randn_like(o)
    t = timeit(lambda: e.flash_attn_bwd(do, q, k, v, o, lse, True, scale),
               iters)
    print(f"flash_bwd  b{b} s{s} hq{hq} d{d}: {t*1e3:8.2f} ms  "
          f"{2.5*flops/t/1e12:7.1f} TF/s")


def median_of_windows(fn, iters, repeats, warmup=20):
    """Warm up, then time `repeats` windows of `iters` calls each (every
    window ends in a device synchronize).  Returns (median, min, max) of the
    per-call time — the spread is the run-to-run noise of this process."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = sorted(timeit(fn, iters, warmup=0) for _ in range(repeats))
    return ts[len(ts) // 2], ts[0], ts[-1]


def bench_varlen(iters, repeats=9, dense_only=False):
    """Packed-document flash attention vs the dense kernels, bench-shape
    slice b1 s4096 h32/8 d128 causal bf16, fwd and bwd:
      dense            flash_attn_fwd/bwd (complementary-pair scheduling)
      varlen 1x4096    one segment: same work, no pairing
      varlen 16x256    the same tokens packed as 16 documents
    Times are medians over `repeats` windows with [min, max].  dense_only
    skips the varlen rows (to time another build of the extension that
    predates them with the same code)."""
    e = ext()
    b, s, hq, hkv, d = 1, 4096, 32, 8, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(b, s, hq, d, device="cuda", generator=g).bfloat16()
    k = torch.randn(b, s, hkv, d, device="cuda", generator=g).bfloat16()
    v = torch.randn(b, s, hkv, d, device="cuda", generator=g).bfloat16()
    do = torch.randn(b, s, hq, d, device="cuda", generator=g).bfloat16()
    scale = 1.0 / math.sqrt(d)

    def row(name, fwd, bwd, pairs):
        # pairs: causal (q, key) pairs actually attended, per head
        flops = 4 * b * hq * pairs * d
        tf, lo, hi = median_of_windows(fwd, iters, repeats)
        print(f"{name:16s} fwd {tf*1e3:7.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]"
              f"  {flops/tf/1e12:6.1f} TF/s")
        tb, lo, hi = median_of_windows(bwd, iters, repeats)
        print(f"{name:16s} bwd {tb*1e3:7.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]"
              f"  {2.5*flops/tb/1e12:6.1f} TF/s")

    o, lse = e.flash_attn_fwd(q, k, v, True, scale)
    row("dense", lambda: e.flash_attn_fwd(q, k, v, True, scale),
        lambda: e.flash_attn_bwd(do, q, k, v, o, lse, True, scale),
        s * (s + 1) / 2)
    if dense_only:
        return
    for nseg in (1, 16):
        L = s // nseg
        cu = torch.arange(0, s + 1, L, dtype=torch.int32, device="cuda")
        ov, lsev = e.flash_attn_varlen_fwd(q, k, v, cu, L, True, scale)
        if nseg == 1:
            assert torch.equal(ov, o) and torch.equal(lsev, lse), \
                "varlen with one segment must reproduce the dense kernel"
        row(f"varlen {nseg}x{L}",
            lambda: e.flash_attn_varlen_fwd(q, k, v, cu, L, True, scale),
            lambda: e.flash_attn_varlen_bwd(do, q, k, v, ov, lsev, cu, L,
                                            True, scale),
            nseg * L * (L + 1) / 2)


def bench_qkv(iters, repeats=9):
    """linear_qkv output -> attention output, forward + backward, one
    layer-microbatch of the llama-3-8b bench (b4 s4096 h32/8 d128 causal
    bf16, packed buffer [s, b, 8, 6, 128]):
      composition   slice q/k/v, apply_rope x2, flash_attention(sbhd) and
                    autograd's backward of all of it
      fused         ops.fused_qkv_attention (in-place packed RoPE, packed
                    flash kernels, one finishing kernel)
    The fused op consumes its input (rotated in place, so not a leaf): both
    rows start from a fresh x.clone(), which stands for the producer and
    costs both the same."""
    from hetu_galvatron_amd.ops import (apply_rope, flash_attention,
                                        fused_qkv_attention)
    from hetu_galvatron_amd.ops.reference_ops import rope_freqs
    s, b, G, qpg, d = 4096, 4, 8, 4, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(s, b, G, qpg + 2, d, device="cuda",
                    generator=g).bfloat16().requires_grad_(True)
    do = torch.randn(s, b, G * qpg, d, device="cuda", generator=g).bfloat16()
    cos, sin = rope_freqs(s, d, device="cuda")

    def composition():
        xc = x.clone()
        q = xc[:, :, :, :qpg].reshape(s, b, -1, d)
        k = xc[:, :, :, qpg].reshape(s, b, -1, d)
        v = xc[:, :, :, qpg + 1].reshape(s, b, -1, d)
        q = apply_rope(q.contiguous(), cos, sin)
        k = apply_rope(k.contiguous(), cos, sin)
        return flash_attention(q, k, v.contiguous(), causal=True, sbhd=True)

    def fused():
        return fused_qkv_attention(x.clone(), cos, sin, G, qpg, causal=True)

    def fwd_bwd(fn):
        def run():
            x.grad = None
            fn().backward(do)
        return run

    for name, fn in (("composition", composition), ("fused", fused)):
        with torch.no_grad():
            tf, lo, hi = median_of_windows(fn, iters, repeats)
        print(f"qkv {name:12s} fwd     {tf*1e3:7.3f} ms "
              f"[{lo*1e3:.3f}, {hi*1e3:.3f}]")
        tb, lo, hi = median_of_windows(fwd_bwd(fn), iters, repeats)
        print(f"qkv {name:12s} fwd+bwd {tb*1e3:7.3f} ms "
              f"[{lo*1e3:.3f}, {hi*1e3:.3f}]")


def bench_qkv_varlen(iters, repeats=9, composition_only=False):
    """bench_qkv for packed documents: linear_qkv output -> attention output
    with cu_seqlens and per-row [s, b, d/2] RoPE tables, b4 s4096 G8 qpg4
    d128 causal bf16, every row of the batch segmented the same way:
      1x4096   one document per row (the unpaired varlen cost on both sides)
      16x256   sixteen documents per row
      mixed    2048 + 1024 + 512 + 256 + 255 + 1
      composition   slice q/k/v, apply_rope_qk per-row,
                    flash_attention_varlen(sbhd) and autograd's backward
      fused         ops.fused_qkv_attention_varlen
    Both rows start from a fresh x.clone(), as in bench_qkv.
    composition_only skips the fused row (to time another build of the
    extension that predates the op with the same code)."""
    from hetu_galvatron_amd.ops import flash_attention_varlen
    from hetu_galvatron_amd.ops.reference_ops import rope_freqs
    from hetu_galvatron_amd.runtime.transformer.rope import apply_rope_qk
    s, b, G, qpg, d = 4096, 4, 8, 4, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(s, b, G, qpg + 2, d, device="cuda",
                    generator=g).bfloat16().requires_grad_(True)
    do = torch.randn(s, b, G * qpg, d, device="cuda", generator=g).bfloat16()
    cos_t, sin_t = rope_freqs(s, d, device="cuda")

    def fwd_bwd(fn):
        def run():
            x.grad = None
            fn().backward(do)
        return run

    for label, lens in (("1x4096", [4096]), ("16x256", [256] * 16),
                        ("mixed", [2048, 1024, 512, 256, 255, 1])):
        assert sum(lens) == s
        offs = [0]
        for _ in range(b):
            for n in lens:
                offs.append(offs[-1] + n)
        cu = torch.tensor(offs, dtype=torch.int32, device="cuda")
        maxlen = max(lens)
        pos = torch.cat([torch.arange(n) for n in lens]).cuda()
        cos = cos_t[pos][:, None].expand(s, b, d // 2).contiguous()
        sin = sin_t[pos][:, None].expand(s, b, d // 2).contiguous()

        def composition():
            xc = x.clone()
            q = xc[:, :, :, :qpg].reshape(s, b, -1, d)
            k = xc[:, :, :, qpg].reshape(s, b, -1, d)
            v = xc[:, :, :, qpg + 1].reshape(s, b, -1, d)
            q, k = apply_rope_qk(q.contiguous(), k.contiguous(), cos, sin)
            return flash_attention_varlen(q, k, v.contiguous(), cu, maxlen,
                                          causal=True, sbhd=True)

        def fused():
            from hetu_galvatron_amd.ops import fused_qkv_attention_varlen
            return fused_qkv_attention_varlen(
                x.clone(), cos, sin, G, qpg, cu_seqlens=cu,
                max_seqlen=maxlen, causal=True)

        rows = [("composition", composition)]
        if not composition_only:
            rows.append(("fused", fused))
            with torch.no_grad():
                assert torch.equal(fused(), composition()), \
                    "the fused op must reproduce the composition"
        for name, fn in rows:
            with torch.no_grad():
                tf, lo, hi = median_of_windows(fn, iters, repeats)
            print(f"qkv-varlen {label:7s} {name:12s} fwd     {tf*1e3:7.3f} ms"
                  f" [{lo*1e3:.3f}, {hi*1e3:.3f}]")
            tb, lo, hi = median_of_windows(fwd_bwd(fn), iters, repeats)
            print(f"qkv-varlen {label:7s} {name:12s} fwd+bwd {tb*1e3:7.3f} ms"
                  f" [{lo*1e3:.3f}, {hi*1e3:.3f}]")


def bench_decode_batched(iters, repeats=9, loop_only=False):
    """One ops.decode_attention_batched call vs the loop of per-slot
    ops.decode_attention calls it replaces in the serving engine, and vs
    decode_attn at b = n (uniform lengths only): h32/8 d128 bf16, n slots of
    a [n, 4096, 8, 128] cache, lengths uniform 4096 or a geometric ladder
    from 1 to 4096.  GB/s counts each attended K and V row once.
    loop_only times only the loop and decode_attn (to time another build of
    the extension that predates the batched op with the same code)."""
    from hetu_galvatron_amd import ops
    hq, hkv, d, max_s = 32, 8, 128, 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (8, 32):
        q = torch.randn(n, hq, d, device="cuda", generator=g).bfloat16()
        kc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        vc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        slots = torch.arange(n, dtype=torch.int32, device="cuda")
        ladder = [max(1, round(max_s ** (i / (n - 1)))) for i in range(n)]
        for label, lens in (("uniform", [max_s] * n), ("mixed", ladder)):
            lengths = torch.tensor(lens, dtype=torch.int32, device="cuda")
            gb = 2 * sum(lens) * hkv * d * 2 / 1e9

            def loop():
                return [ops.decode_attention(q[i:i + 1], kc[i:i + 1],
                                             vc[i:i + 1], L)
                        for i, L in enumerate(lens)]

            def batched():
                return ops.decode_attention_batched(q, kc, vc, lengths, slots,
                                                    max_len=max(lens))

            rows = [("loop", loop)]
            if label == "uniform":
                rows.append(("decode_attn", lambda: ops.decode_attention(
                    q, kc, vc, max_s)))
            if not loop_only:
                rows.append(("batched", batched))
            for name, fn in rows:
                t, lo, hi = median_of_windows(fn, iters, repeats)
                print(f"decode-batched n{n:<2d} {label:7s} {name:11s} "
                      f"{t*1e6:8.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]  "
                      f"{gb/t:6.0f} GB/s")


def bench_decode_batched_fp8(iters, repeats=9):
    """ops.decode_attention_batched on e4m3 caches beside the same call on
    bf16 caches, and ops.kv_cache_append (n = 32 rows, one launch) beside the
    two index_put calls it replaces: the cases, method and GB/s (attended
    bytes: one per element here, two for bf16) of bench_decode_batched."""
    from hetu_galvatron_amd import ops
    hq, hkv, d, max_s = 32, 8, 128, 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (8, 32):
        q = torch.randn(n, hq, d, device="cuda", generator=g).bfloat16()
        kc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        vc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        ks = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        vs = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        k8 = (kc.float() / ks[:, None]).to(torch.float8_e4m3fn)
        v8 = (vc.float() / vs[:, None]).to(torch.float8_e4m3fn)
        slots = torch.arange(n, dtype=torch.int32, device="cuda")
        ladder = [max(1, round(max_s ** (i / (n - 1)))) for i in range(n)]
        for label, lens in (("uniform", [max_s] * n), ("mixed", ladder)):
            lengths = torch.tensor(lens, dtype=torch.int32, device="cuda")
            rows = [("bf16", 2, lambda: ops.decode_attention_batched(
                        q, kc, vc, lengths, slots, max_len=max(lens))),
                    ("fp8", 1, lambda: ops.decode_attention_batched(
                        q, k8, v8, lengths, slots, max_len=max(lens),
                        k_scale=ks, v_scale=vs))]
            for name, width, fn in rows:
                gb = 2 * sum(lens) * hkv * d * width / 1e9
                t, lo, hi = median_of_windows(fn, iters, repeats)
                print(f"decode-batched-fp8 n{n:<2d} {label:7s} {name:5s} "
                      f"{t*1e6:8.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]  "
                      f"{gb/t:6.0f} GB/s")
    n = 32
    x = torch.randn(n, hkv, 6, d, device="cuda", generator=g).bfloat16()
    k, v = x[:, :, 4], x[:, :, 5]            # views, as the engine's
    pos = torch.randint(0, max_s, (n,), device="cuda", generator=g)

    def index_put():
        kc[slots.long(), pos] = k
        vc[slots.long(), pos] = v

    pos32 = pos.int()
    for name, fn in (("index_put x2 (bf16)", index_put),
                     ("kv_cache_append", lambda: ops.kv_cache_append(
                         k, v, k8, v8, slots, pos32, ks, vs))):
        t, lo, hi = median_of_windows(fn, iters, repeats)
        print(f"kv-append n{n} {name:20s} {t*1e6:8.1f} us "
              f"[{lo*1e6:.1f}, {hi*1e6:.1f}]")


def bench_decode_paged(iters, repeats=9, contiguous_only=False):
    """ops.decode_attention_batched on paged pools (pages of 32 and 128, ids
    shuffled over the pool) beside the same call on the contiguous caches
    holding the same rows, bf16 and e4m3: the cases, method and GB/s of
    bench_decode_batched.  contiguous_only times only the contiguous rows (to
    time a build of the extension that predates paging with the same code)."""
    from hetu_galvatron_amd import ops
    hq, hkv, d, max_s = 32, 8, 128, 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (8, 32):
        q = torch.randn(n, hq, d, device="cuda", generator=g).bfloat16()
        kc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        vc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        ks = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        vs = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        k8 = (kc.float() / ks[:, None]).to(torch.float8_e4m3fn)
        v8 = (vc.float() / vs[:, None]).to(torch.float8_e4m3fn)
        slots = torch.arange(n, dtype=torch.int32, device="cuda")
        ladder = [max(1, round(max_s ** (i / (n - 1)))) for i in range(n)]
        pools = {}
        for page in () if contiguous_only else (32, 128):
            P = n * max_s // page
            perm = torch.randperm(P, device="cuda", generator=g)
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(P, device="cuda")
            # pool page perm[j] holds page j of the caches' storage order
            pools[page] = (perm.int().reshape(n, -1),) + tuple(
                c.view(P, page, hkv, d)[inv].contiguous()
                for c in (kc, vc, k8, v8))
        for label, lens in (("uniform", [max_s] * n), ("mixed", ladder)):
            lengths = torch.tensor(lens, dtype=torch.int32, device="cuda")
            for name, width, k, v, sc in (
                    ("bf16", 2, 1, 2, {}),
                    ("fp8", 1, 3, 4, dict(k_scale=ks, v_scale=vs))):
                gb = 2 * sum(lens) * hkv * d * width / 1e9
                caches = (None, kc, vc, k8, v8)
                rows = [("contiguous", lambda: ops.decode_attention_batched(
                    q, caches[k], caches[v], lengths, slots,
                    max_len=max(lens), **sc))]
                for page, pl in pools.items():
                    rows.append((f"page {page}", lambda pl=pl:
                                 ops.decode_attention_batched(
                                     q, pl[k], pl[v], lengths, slots,
                                     max_len=max(lens), page_table=pl[0],
                                     **sc)))
                ref = rows[0][1]()
                for what, fn in rows:
                    assert torch.equal(fn(), ref), "paged != contiguous"
                    t, lo, hi = median_of_windows(fn, iters, repeats)
                    print(f"decode-paged n{n:<2d} {label:7s} {name:4s} "
                          f"{what:10s} {t*1e6:8.1f} us "
                          f"[{lo*1e6:.1f}, {hi*1e6:.1f}]  {gb/t:6.0f} GB/s")


def bench_decode_multi(iters, repeats=9, expanded_only=False):
    """ops.decode_attention_multi (T new tokens per row in one pass over the
    row's K/V) beside what the one-token kernel does with the same work:
    decode_attention_batched on the n*T expanded rows (q reshaped, lengths =
    pos + 1, the slot repeated).  h32/8 d128, n in (8, 32), uniform 4096 and
    the mixed ladder, T in (1, 2, 4, 8), bf16 and e4m3, contiguous and page
    32.  expanded_only times only the expanded rows (to time a build of the
    extension that predates the multi-token kernels with the same code)."""
    from hetu_galvatron_amd import ops
    hq, hkv, d, max_s, page = 32, 8, 128, 4096, 32
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (8, 32):
        kc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        vc = torch.randn(n, max_s, hkv, d, device="cuda",
                         generator=g).bfloat16()
        ks = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        vs = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        k8 = (kc.float() / ks[:, None]).to(torch.float8_e4m3fn)
        v8 = (vc.float() / vs[:, None]).to(torch.float8_e4m3fn)
        slots = torch.arange(n, dtype=torch.int32, device="cuda")
        ladder = [max(1, round(max_s ** (i / (n - 1)))) for i in range(n)]
        P = n * max_s // page
        perm = torch.randperm(P, device="cuda", generator=g)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(P, device="cuda")
        table = perm.int().reshape(n, -1)
        pool = [c.view(P, page, hkv, d)[inv].contiguous()
                for c in (kc, vc, k8, v8)]
        for T in (1, 2, 4, 8):
            q = torch.randn(n, T, hq, d, device="cuda", generator=g).bfloat16()
            q_lens = torch.full((n,), T, dtype=torch.int32, device="cuda")
            steps = torch.arange(T, dtype=torch.int32, device="cuda")
            for label, lens in (("uniform", [max_s] * n),
                                ("mixed", [max(x, T) for x in ladder])):
                lengths = torch.tensor(lens, dtype=torch.int32, device="cuda")
                # the expanded rows: token t of row i attends to pos + 1 keys
                lens_x = (lengths[:, None] - T + 1 + steps).reshape(-1)
                slots_x = slots.repeat_interleave(T)
                qx = q.reshape(n * T, hq, d)
                for name, k, v, sc in (
                        ("bf16", 0, 1, {}),
                        ("fp8", 2, 3, dict(k_scale=ks, v_scale=vs))):
                    for what, kk, vv, tb in (
                            ("contiguous", (kc, vc, k8, v8)[k],
                             (kc, vc, k8, v8)[v], {}),
                            ("page 32", pool[k], pool[v],
                             dict(page_table=table))):
                        kw = dict(max_len=max(lens), **sc, **tb)
                        rows = [("expanded", lambda: (
                            ops.decode_attention_batched(
                                qx, kk, vv, lens_x, slots_x, **kw)))]
                        if not expanded_only:
                            rows.append(("multi", lambda: (
                                ops.decode_attention_multi(
                                    q, kk, vv, lengths, q_lens, slots,
                                    **kw))))
                            err = (rows[1][1]().reshape(qx.shape).float()
                                   - rows[0][1]().float()).abs().max()
                            assert float(err) < 0.05, "multi != expanded"
                        for how, fn in rows:
                            t, lo, hi = median_of_windows(fn, iters, repeats)
                            print(f"decode-multi n{n:<2d} T{T} {label:7s} "
                                  f"{name:4s} {what:10s} {how:8s} "
                                  f"{t*1e6:8.1f} us "
                                  f"[{lo*1e6:.1f}, {hi*1e6:.1f}]")


def bench_decode_prefill(iters, repeats=9, baseline_only=False):
    """ops.decode_attention_multi at T in (64, 256, 1024) new tokens per row
    against a cache of 4096 (the prefill kernels) beside what the engine did
    for the same work without them: flash_attention_fwd_only on a gathered
    bf16 contiguous copy of the row's K/V, the copy (gather, dequantisation)
    included.  h32/8 d128, n in (1, 8), bf16 and e4m3, contiguous and page
    32.  baseline_only times only the copy + flash rows (to time a build of
    the extension that predates the prefill kernels with the same code)."""
    from hetu_galvatron_amd import ops
    hq, hkv, d, L, page = 32, 8, 128, 4096, 32
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (1, 8):
        kc, vc = (torch.randn(n, L, hkv, d, device="cuda",
                              generator=g).bfloat16() for _ in "kv")
        ks = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        vs = 0.5 + torch.rand(hkv, device="cuda", generator=g)
        k8 = (kc.float() / ks[:, None]).to(torch.float8_e4m3fn)
        v8 = (vc.float() / vs[:, None]).to(torch.float8_e4m3fn)
        slots = torch.arange(n, dtype=torch.int32, device="cuda")
        lengths = torch.full((n,), L, dtype=torch.int32, device="cuda")
        P = n * L // page
        perm = torch.randperm(P, device="cuda", generator=g)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(P, device="cuda")
        table = perm.int().reshape(n, -1)
        pool = [c.view(P, page, hkv, d)[inv].contiguous()
                for c in (kc, vc, k8, v8)]
        for T in (64, 256, 1024):
            q = torch.randn(n, T, hq, d, device="cuda", generator=g).bfloat16()
            q_lens = torch.full((n,), T, dtype=torch.int32, device="cuda")
            for name, k, sc in (("bf16", 0, None), ("fp8", 2, (ks, vs))):
                for what, kk, vv, tb in (
                        ("contiguous", (kc, vc, k8, v8)[k],
                         (kc, vc, k8, v8)[k + 1], None),
                        ("page 32", pool[k], pool[k + 1], table)):
                    def copy(c, s):
                        if tb is not None:       # gather the rows' pages
                            c = c[tb.long()].reshape(n, L, hkv, d)
                        if sc is not None:       # dequantise
                            return (c.float() * s[:, None]).bfloat16()
                        return c.clone() if tb is None else c

                    def flash():
                        return ops.flash_attention_fwd_only(
                            q, copy(kk, sc and sc[0]), copy(vv, sc and sc[1]),
                            causal=True, softmax_scale=d ** -0.5)[0]

                    def prefill():
                        kw = {} if sc is None else dict(k_scale=sc[0],
                                                        v_scale=sc[1])
                        return ops.decode_attention_multi(
                            q, kk, vv, lengths, q_lens, slots, max_len=L,
                            page_table=tb, **kw)

                    rows = [("copy+flash", flash)]
                    if not baseline_only:
                        rows.append(("prefill", prefill))
                        err = (prefill().float() - flash().float()).abs().max()
                        assert float(err) < 0.05, "prefill != flash"
                    for how, fn in rows:
                        t, lo, hi = median_of_windows(fn, iters, repeats)
                        print(f"decode-prefill n{n} T{T:<4d} {name:4s} "
                              f"{what:10s} {how:10s} {t*1e6:8.1f} us "
                              f"[{lo*1e6:.1f}, {hi*1e6:.1f}]")


def bench_decode_prologue(iters, repeats=9, composition_only=False):
    """One ops.rope_kv_append call beside the composition it replaces in the
    serving engine: the split of the packed qkv, the cos/sin gathers,
    `_rope_rows` on q and k and the cache write (two index_put calls for a
    bf16 contiguous cache, the row gather and `kv_cache_append` for an e4m3
    cache with pages of 32; the write indices are built outside the timing).
    h32/8 d128, n rows of T tokens at mixed lengths.  composition_only skips
    the op (a build without it)."""
    from types import SimpleNamespace
    from hetu_galvatron_amd import ops
    from hetu_galvatron_amd.runtime.inference import GalvatronGenerator
    from hetu_galvatron_amd.runtime.serving import _rope_rows
    G, qpg, d, max_s, page = 8, 4, 128, 4096, 32
    attn = SimpleNamespace(num_groups_local=G, q_per_group=qpg, head_dim=d)
    g = torch.Generator(device="cuda").manual_seed(0)
    ang = torch.arange(max_s, device="cuda")[:, None] * 10000.0 ** (
        -torch.arange(0, d, 2, device="cuda") / d)[None]
    cos_t, sin_t = ang.cos(), ang.sin()
    for n in (1, 8, 32):
        for T in (1, 4):
            qkv = torch.randn(1, n * T, G * (qpg + 2) * d, device="cuda",
                              generator=g).bfloat16()
            base = torch.randint(1, max_s - T, (n,), device="cuda",
                                 generator=g)
            pos = (base[:, None] + torch.arange(T, device="cuda")).reshape(-1)
            slots = torch.arange(n, device="cuda")
            slot32 = slots.int()
            q_lens = torch.full((n,), T, dtype=torch.int32, device="cuda")
            lengths = base.int() + q_lens
            real_t = torch.arange(n * T, device="cuda")
            table = torch.randperm(n * max_s // page, device="cuda",
                                   generator=g).int().reshape(n, -1)
            for name, fp8 in (("bf16 contiguous", False),
                              ("e4m3 page32", True)):
                if fp8:
                    shape, dtype = (n * max_s // page, page, G, d), \
                        torch.float8_e4m3fn
                    wr_t = table[slots.repeat_interleave(T), pos // page]
                    wr_pos = (pos % page).int()
                    kw = {"page_table": table}
                else:
                    shape, dtype = (n, max_s, G, d), torch.bfloat16
                    wr_t, wr_pos, kw = slots.repeat_interleave(T), pos, {}
                kc = torch.zeros(shape, device="cuda").to(dtype)
                vc = torch.zeros(shape, device="cuda").to(dtype)

                def composition():
                    q, k, v = GalvatronGenerator._split_qkv(attn, qkv)
                    q = _rope_rows(q, cos_t[pos], sin_t[pos])
                    k = _rope_rows(k, cos_t[pos], sin_t[pos])
                    if fp8:
                        ops.kv_cache_append(k[0][real_t], v[0][real_t], kc,
                                            vc, wr_t, wr_pos)
                    else:
                        kc[wr_t, wr_pos] = k[0][real_t]
                        vc[wr_t, wr_pos] = v[0][real_t]
                    return q

                rows = [("composition", composition)]
                if not composition_only:
                    rows.append(("rope_kv_append", lambda: ops.rope_kv_append(
                        qkv, G, qpg, cos_t, sin_t, lengths, q_lens, slot32,
                        kc, vc, **kw)))
                for label, fn in rows:
                    t, lo, hi = median_of_windows(fn, iters, repeats)
                    print(f"decode-prologue n{n:<2d} T{T} {name:15s} "
                          f"{label:14s} {t*1e6:8.1f} us "
                          f"[{lo*1e6:.1f}, {hi*1e6:.1f}]")


def bench_norms(iters):
    e = ext()
    n, H = 4096, 4096
    x = torch.randn(n, H, device="cuda").bfloat16()
    w = torch.randn(H, device="cuda").bfloat16()
    t = timeit(lambda: e.rmsnorm_fwd(x, w, 1e-5), iters)
    gb = 2 * n * H * 2 / 1e9
    print(f"rmsnorm_fwd [{n}x{H}]: {t*1e6:8.1f} us  {gb/t:7.0f} GB/s")
    y, inv = e.rmsnorm_fwd(x, w, 1e-5)
    dy = torch.randn_like(x)
    t = timeit(lambda: e.rmsnorm_bwd(dy, x, w, inv), iters)
    gb = 3 * n * H * 2 / 1e9
    print(f"rmsnorm_bwd [{n}x{H}]: {t*1e6:8.1f} us  {gb/t:7.0f} GB/s")


def bench_elementwise(iters):
    e = ext()
    n, F = 4096, 14336
    x = torch.randn(n, 2 * F, device="cuda").bfloat16()
    t = timeit(lambda: e.swiglu_fwd(x), iters)
    gb = 3 * n * F * 2 / 1e9
    print(f"swiglu_fwd [{n}x2x{F}]: {t*1e6:8.1f} us  {gb/t:7.0f} GB/s")
    s, bb, h, d = 4096, 1, 32, 128
    xr = torch.randn(s, bb, h, d, device="cuda").bfloat16()
    cos = torch.randn(s, d // 2, device="cuda").float()
    sin = torch.randn(s, d // 2, device="cuda").float()
    t = timeit(lambda: e.rope_fwd(xr, cos, sin, False), iters)
    gb = 2 * s * bb * h * d * 2 / 1e9
    print(f"rope_fwd [{s}x{bb}x{h}x{d}]: {t*1e6:8.1f} us  {gb/t:7.0f} GB/s")


def bench_adam(iters):
    e = ext()
    n = 500_000_000
    master = torch.randn(n, device="cuda").float()
    g = torch.randn(n, device="cuda").bfloat16()
    m = torch.zeros(n, device="cuda").float()
    v = torch.zeros(n, device="cuda").float()
    out = torch.zeros(n, device="cuda").bfloat16()
    t = timeit(lambda: e.fused_adamw([master], [g], [m], [v], [out], 2,
                                     1e-4, 0.9, 0.95, 1e-8, 0.01), iters)
    gb = n * (4 * 3 * 2 + 2 + 2) / 1e9  # m/v/master rw, g read, out write
    print(f"fused_adamw [{n/1e6:.0f}M]: {t*1e3:8.2f} ms  {gb/t:7.0f} GB/s")
    flat = torch.zeros(n, device="cuda").float()
    t = timeit(lambda: e.grad_accum(flat, g, 0), iters)
    gb = n * (4 * 2 + 2) / 1e9
    print(f"grad_accum [{n/1e6:.0f}M]: {t*1e3:8.2f} ms  {gb/t:7.0f} GB/s")


def bench_bias(iters):
    """t5-3b attention layer shapes: native biased flash vs the eager fp32
    path it replaces (VERDICT r1 #5 done-criterion: >=5x)."""
    import torch.autograd as ag
    from hetu_galvatron_amd.ops import flash_bias_attention
    from hetu_galvatron_amd.runtime.transformer.attention_impl import (
        eager_bias_attention)
    b, s, h, d = 4, 512, 32, 128
    q = torch.randn(b, s, h, d, device="cuda", requires_grad=True).bfloat16()
    k = torch.randn(b, s, h, d, device="cuda").bfloat16()
    v = torch.randn(b, s, h, d, device="cuda").bfloat16()
    bias = torch.randn(h, s, s, device="cuda").bfloat16().requires_grad_(True)
    scale = 1.0

    def run(fn):
        o = fn()
        o.float().sum().backward()

    qn = q.detach().requires_grad_(True)
    t_native = timeit(lambda: run(lambda: flash_bias_attention(
        qn, k, v, bias, True, scale)), iters)
    t_eager = timeit(lambda: run(lambda: eager_bias_attention(
        qn, k, v, bias, True, scale)), iters)
    print(f"bias_attn t5-3b layer b{b} s{s} h{h} d{d} fwd+bwd: "
          f"native {t_native*1e3:7.2f} ms  eager {t_eager*1e3:7.2f} ms  "
          f"speedup {t_eager/t_native:5.1f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9,
                    help="timed windows per row (varlen and qkv entries)")
    ap.add_argument("--dense-only", action="store_true",
                    help="varlen entry: time only the dense kernels")
    ap.add_argument("--loop-only", action="store_true",
                    help="decode-batched entry: skip the batched op")
    ap.add_argument("--contiguous-only", action="store_true",
                    help="decode-paged entry: skip the paged pools")
    ap.add_argument("--expanded-only", action="store_true",
                    help="decode-multi entry: time only the expanded rows")
    ap.add_argument("--baseline-only", action="store_true",
                    help="decode-prefill entry: time only copy + flash")
    ap.add_argument("--composition-only", action="store_true",
                    help="qkv-varlen and decode-prologue entries: time only "
                         "the composition")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    fns = {"flash": bench_flash, "norms": bench_norms,
           "elementwise": bench_elementwise, "adam": bench_adam,
           "bias": bench_bias,
           "varlen": lambda it: bench_varlen(it, args.repeats,
                                             args.dense_only),
           "qkv": lambda it: bench_qkv(it, args.repeats),
           "decode-batched": lambda it: bench_decode_batched(
               it, args.repeats, args.loop_only),
           "decode-batched-fp8": lambda it: bench_decode_batched_fp8(
               it, args.repeats),
           "decode-paged": lambda it: bench_decode_paged(
               it, args.repeats, args.contiguous_only),
           "decode-multi": lambda it: bench_decode_multi(
               it, args.repeats, args.expanded_only),
           "decode-prefill": lambda it: bench_decode_prefill(
               it, args.repeats, args.baseline_only),
           "qkv-varlen": lambda it: bench_qkv_varlen(
               it, args.repeats, args.composition_only),
           "decode-prologue": lambda it: bench_decode_prologue(
               it, args.repeats, args.composition_only)}
    if args.what == "all":
        for f in fns.values():
            f(args.iters)
    else:
        fns[args.what](args.iters)


if __name__ == "__main__":
    main()
