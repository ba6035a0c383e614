#!/usr/bin/env python3
"""Standalone per-kernel microbenchmarks (GPU box).

python tools/bench_kernels.py [flash|varlen|qkv|qkv-varlen|norms|elementwise|adam|all] [--iters N]

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
    ap.add_argument("--composition-only", action="store_true",
                    help="qkv-varlen entry: time only the composition")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    fns = {"flash": bench_flash, "norms": bench_norms,
           "elementwise": bench_elementwise, "adam": bench_adam,
           "bias": bench_bias,
           "varlen": lambda it: bench_varlen(it, args.repeats,
                                             args.dense_only),
           "qkv": lambda it: bench_qkv(it, args.repeats),
           "qkv-varlen": lambda it: bench_qkv_varlen(
               it, args.repeats, args.composition_only)}
    if args.what == "all":
        for f in fns.values():
            f(args.iters)
    else:
        fns[args.what](args.iters)


if __name__ == "__main__":
    main()
