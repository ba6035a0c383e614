#!/usr/bin/env python
"""Cases for the flash-attention softmax / mask paths, and their digests.

    python tools/flash_valu_cases.py > tests/ops/flash_golden_valu_parent.json

The block bodies take different instruction paths by what a tile holds: rows
that have seen no key yet, a running max that does or does not move, tiles
(and, in dkv, 32-row halves) with and without a masked key.  CASES builds inputs that
steer each of those paths, run() takes a case through one of the five entry
points (dense bshd / sbhd, varlen, packed QKV, packed QKV varlen), and main()
records the SHA-256 digests of every output, as tools/flash_golden.py does
for its own list.  tests/ops/test_gpu_flash_valu.py recomputes them.

The committed record was written by the build before the softmax VALU work
(exp2f() and a select per element, two scalar bf16 conversions per word, the
O rescale on every tile, the dq mask tested per element), so that the claim of
bit-identical outputs stays checkable after that build is gone.  The cases
of the "underflow" group are not recorded: there the two builds may differ
(a P or an alpha below 2^-126 is a denormal in the one and 0 in the other).
"""
import importlib.util
import json
import math
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))


def _load_golden_tool():
    spec = importlib.util.spec_from_file_location(
        "flash_golden", os.path.join(_HERE, "flash_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


golden = _load_golden_tool()
digest = golden.digest

BATCH, HQ, HKV = golden.BATCH, 4, 2
ENTRIES = ("bshd", "sbhd", "varlen", "packed", "packed-varlen")


def _cases():
    out = []

    def add(group, inputs="randn", **kw):
        c = dict(group=group, inputs=inputs, hq=HQ, hkv=HKV, sbhd=False, **kw)
        out.append(c)

    for d in (64, 128):
        # 1. dead rows: bottom-right aligned causal with sq > skv, rows
        # 0 .. sq-skv-1 see no key; with a window the first tiles of the
        # later rows lie wholly below it as well
        for sq, skv in ((96, 40), (300, 257)):
            add("dead", d=d, sq=sq, skv=skv, causal=True)
        add("dead", d=d, sq=300, skv=257, causal=True, window=40)
        for causal in (False, True):
            # 2. one or two keys dominate by more than 126 in log2 units
            add("underflow", "underflow", d=d, sq=257, skv=257, causal=causal)
            # 3. how the running max moves over the four forward tiles
            for kind in ("rise", "first", "onerow"):
                add("rescale", kind, d=d, sq=256, skv=256, causal=causal)
            # 4. tiles and halves with and without a masked key
            for s in (32, 33, 63, 64, 65, 257):
                add("mask", d=d, sq=s, skv=s, causal=causal)
            for sq, skv in ((65, 129), (129, 65)):
                add("mask", d=d, sq=sq, skv=skv, causal=causal)
        # the window's lower edge and the row end (key 100) fall inside a
        # 32-key wave tile; likewise the diagonal and the row end with bias
        add("mask", d=d, sq=100, skv=100, causal=True, window=45)
        add("mask", d=d, sq=70, skv=100, causal=True, bias=True)
    return [(case_name(c), c) for c in out]


def case_name(c):
    n = "%s-d%d-%s-q%d-k%d" % (c["group"], c["d"],
                               "causal" if c["causal"] else "full",
                               c["sq"], c["skv"])
    if c["inputs"] != "randn":
        n += "-" + c["inputs"]
    if c.get("bias"):
        n += "-bias"
    if c.get("window"):
        n += "-w%d" % c["window"]
    return n


CASES = _cases()
CASE_BY_NAME = dict(CASES)
CASE_INDEX = {name: i for i, (name, _) in enumerate(CASES)}


def admits(c, entry):
    """Dense takes everything; the other entry points are self-attention
    (sq == skv) without bias or window."""
    if entry in ("bshd", "sbhd"):
        return True
    return c["sq"] == c["skv"] and not c.get("bias") and not c.get("window")


def runs():
    """Every (case name, entry point) the case list gives rise to."""
    return [(name, e) for name, c in CASES for e in ENTRIES if admits(c, e)]


def run_key(name, entry):
    return "%s|%s" % (name, entry)


def recorded(name):
    return CASE_BY_NAME[name]["group"] != "underflow"


# ---------------------------------------------------------------------------
# inputs, [b, s, h, d] bf16 on the CPU
# ---------------------------------------------------------------------------
_SEED_SHIFT = 2000   # keeps the random cases off the seeds of flash_golden


def make_inputs(c, index):
    """q, k, v, dout, bias|None in bshd layout."""
    if c["inputs"] == "randn":
        return golden.make_inputs(c, _SEED_SHIFT + index)
    g = torch.Generator().manual_seed(4000 + index)
    d, sq, skv = c["d"], c["sq"], c["skv"]
    scale = 1.0 / math.sqrt(d)

    def rnd(s, h, std):
        return std * torch.randn(BATCH, s, h, d, generator=g)

    v, dout = rnd(skv, HKV, 1.0), rnd(sq, HQ, 1.0)
    kind = c["inputs"]
    if kind == "underflow":
        # q = a_i e0 + noise, two keys (tiles 1 and 3 of the forward) with
        # 8 e0, every other key 0 e0: those two score a_i * 8 * scale above
        # the rest.  a_i alternates between a large value (the gap is
        # hundreds of log2 units: exp2 of it is 0 in either build) and one
        # whose gap lies between 126 and 149 (a denormal from exp2f(), 0
        # from the bare instruction).  Tile 0 holds ordinary scores, so the
        # running max jumps by the whole gap in tile 1 and alpha underflows.
        big, small = (256.0, 94.0) if d == 64 else (512.0, 128.0)
        log2e = 1.4426950408889634
        assert big * 8 * scale * log2e > 300
        assert 126 < small * 8 * scale * log2e < 149
        q, k = rnd(sq, HQ, 0.5), rnd(skv, HKV, 0.5)
        q[..., 0] = torch.where(torch.arange(sq) % 2 == 0, big, small)[
            None, :, None]
        k[..., 0] = 0.0
        k[:, 70, :, 0] = 8.0
        k[:, 200, :, 0] = 8.0
    else:
        # scores are a_i * b_j * scale on e0 (+ e1 for "onerow") plus noise
        # of about 0.01 from the other dimensions
        q, k = rnd(sq, HQ, 0.1), rnd(skv, HKV, 0.1)
        q[..., :2] = 0.0
        k[..., :2] = 0.0
        q[..., 0] = 4.0
        if kind == "rise":
            # keys ordered by score: every row's max rises in every tile
            k[..., 0] = (torch.arange(skv) / 32.0)[None, :, None] / \
                (8 * scale)
        else:
            # key 0 (score 3) holds every row's max from the first tile on.
            # No higher: with P(key 0) near 1 in every row, dk of key 0 sums
            # the rounding of o to bf16 (through di) coherently over all
            # rows and leaves the reference tolerance, in any build.
            k[:, 0, :, 0] = 6.0 / (8 * scale)
            if kind == "onerow":
                # ... except for row 200 (wave 6), which key 150 (tile 2)
                # tops with score 6 through e1; no other row has an e1
                # component
                q[:, 200, :, 1] = 8.0
                k[:, 150, :, 1] = 6.0 / (8 * scale)
    return tuple(t.bfloat16() for t in (q, k, v, dout)) + (None,)


# ---------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------
def run(ext, name, entry, device):
    """Native forward + backward of a case through one entry point.

    Every entry point gets the same values, so one reference serves a case.
    Returns (inputs, outputs): inputs q, k, v, dout in bshd layout and bias;
    outputs o, dq, dk, dv in bshd layout too (views of what the kernels
    wrote, so their digests are those of the raw bytes in a fixed order),
    lse [b, hq, s], and dbias for the biased case.  The packed entry points
    return dk and dv per q head, [b, s, hq, d]: sum_group() reduces them."""
    c = CASE_BY_NAME[name]
    index = CASE_INDEX[name]
    assert admits(c, entry)
    scale = 1.0 / math.sqrt(c["d"])
    causal, window = c["causal"], c.get("window", 0)
    if entry == "bshd" and c["inputs"] == "randn":
        return golden.run_case(ext, c, _SEED_SHIFT + index, device)

    q, k, v, dout, bias = (t.to(device) if t is not None else None
                           for t in make_inputs(c, index))
    inp = dict(q=q, k=k, v=v, dout=dout, bias=bias)
    s, b, d = c["sq"], BATCH, c["d"]
    sb = [t.permute(1, 0, 2, 3).contiguous() for t in (q, k, v, dout)]
    cu = torch.tensor([0, s, 2 * s], dtype=torch.int32, device=device)

    def back(t):
        return t.permute(1, 0, 2, 3)

    if entry == "bshd":
        o, lse = ext.flash_attn_fwd(q, k, v, causal, scale, bias, False,
                                    window)
        res = ext.flash_attn_bwd(dout, q, k, v, o, lse, causal, scale, bias,
                                 False, window)
        out = dict(o=o, lse=lse, dq=res[0], dk=res[1], dv=res[2])
    elif entry == "sbhd":
        o, lse = ext.flash_attn_fwd(sb[0], sb[1], sb[2], causal, scale, bias,
                                    True, window)
        res = ext.flash_attn_bwd(sb[3], sb[0], sb[1], sb[2], o, lse, causal,
                                 scale, bias, True, window)
        out = dict(o=back(o), lse=lse, dq=back(res[0]), dk=back(res[1]),
                   dv=back(res[2]))
    elif entry == "varlen":
        o, lse = ext.flash_attn_varlen_fwd(q, k, v, cu, s, causal, scale)
        res = ext.flash_attn_varlen_bwd(dout, q, k, v, o, lse, cu, s, causal,
                                        scale)
        out = dict(o=o, lse=lse, dq=res[0], dk=res[1], dv=res[2])
    else:
        qpg = HQ // HKV
        qkv = torch.cat([sb[0].view(s, b, HKV, qpg, d),
                         sb[1].view(s, b, HKV, 1, d),
                         sb[2].view(s, b, HKV, 1, d)], dim=3).contiguous()
        if entry == "packed":
            o, lse = ext.flash_attn_qkv_fwd(qkv, causal, scale)
            res = ext.flash_attn_qkv_bwd(sb[3], qkv, o, lse, causal, scale)
        else:
            o, lse = ext.flash_attn_qkv_varlen_fwd(qkv, cu, s, causal, scale)
            res = ext.flash_attn_qkv_varlen_bwd(sb[3], qkv, o, lse, cu, s,
                                                causal, scale)
        dq = res[0][:, :, :, :qpg].reshape(s, b, HQ, d)
        out = dict(o=back(o), lse=lse, dq=back(dq), dk=back(res[1]),
                   dv=back(res[2]))
    if bias is not None:
        out["dbias"] = res[3]
    return inp, out


def sum_group(t):
    """[b, s, hq, d] per-q-head dk / dv -> fp32 [b, s, hkv, d]."""
    b, s, _, d = t.shape
    return t.float().view(b, s, HKV, HQ // HKV, d).sum(3)


def digests(out):
    # dbias is summed with fp32 atomics over the batch: its bits depend on
    # the order the hardware retires them, so it is not recorded
    return {key: digest(val) for key, val in out.items() if key != "dbias"}


def main():
    from hetu_galvatron_amd.ops._ext import get_ext
    ext = get_ext(False)
    device = torch.device("cuda:0")
    record = {}
    for name, entry in runs():
        if recorded(name):
            _, out = run(ext, name, entry, device)
            record[run_key(name, entry)] = digests(out)
    json.dump(record, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
