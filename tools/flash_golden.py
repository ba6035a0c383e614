#!/usr/bin/env python
"""Record SHA-256 digests of the flash-attention kernels' raw outputs.

    python tools/flash_golden.py > tests/ops/flash_golden_parent.json

For every tail/seam case of CASES, inputs are built on the CPU from a fixed
seed, the native forward and backward run on the GPU, and the raw bytes of
o, lse, dq, dk, dv (and dbias of the biased case) are hashed.  The committed
record was written by the build that still staged transposed operand images
from global memory; tests/ops/test_gpu_flash_tr.py recomputes the digests,
so the claim that the transposed-LDS-read kernels are bit-identical stays
checkable after that build is gone.
"""
import hashlib
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _cases():
    """(name, dict) for every case of the tail/seam list."""
    out = []
    for d in (64, 128):
        for hq, hkv in ((4, 4), (4, 1)):
            for sbhd in (False, True):
                for causal in (False, True):
                    for s in (1, 31, 33, 63, 65, 257):
                        out.append(dict(d=d, hq=hq, hkv=hkv, sbhd=sbhd,
                                        causal=causal, sq=s, skv=s))
                    # cross lengths: causal ones have off = skv - sq != 0
                    for sq, skv in ((128, 200), (200, 128)):
                        out.append(dict(d=d, hq=hq, hkv=hkv, sbhd=sbhd,
                                        causal=causal, sq=sq, skv=skv))
    out.append(dict(d=64, hq=4, hkv=4, sbhd=False, causal=False, sq=65,
                    skv=129, bias=True))
    out.append(dict(d=128, hq=4, hkv=1, sbhd=False, causal=True, sq=257,
                    skv=257, window=40))
    return [(case_name(c), c) for c in out]


def case_name(c):
    n = "d%d-h%dx%d-%s-%s-q%d-k%d" % (
        c["d"], c["hq"], c["hkv"], "sbhd" if c["sbhd"] else "bshd",
        "causal" if c["causal"] else "full", c["sq"], c["skv"])
    if c.get("bias"):
        n += "-bias"
    if c.get("window"):
        n += "-w%d" % c["window"]
    return n


CASES = _cases()
BATCH = 2


def make_inputs(c, index):
    """Seeded CPU inputs in the case's layout: q, k, v, dout, bias|None."""
    g = torch.Generator().manual_seed(1000 + index)
    d, hq, hkv, sq, skv = c["d"], c["hq"], c["hkv"], c["sq"], c["skv"]

    def mk(s, h):
        shape = (s, BATCH, h, d) if c["sbhd"] else (BATCH, s, h, d)
        return torch.randn(shape, generator=g).bfloat16()

    q, k, v, dout = mk(sq, hq), mk(skv, hkv), mk(skv, hkv), mk(sq, hq)
    bias = None
    if c.get("bias"):
        bias = torch.randn(hq, sq, skv, generator=g).bfloat16()
    return q, k, v, dout, bias


def run_case(ext, c, index, device):
    """Native forward + backward; dict of output tensors (on the device)."""
    q, k, v, dout, bias = (t.to(device) if t is not None else None
                           for t in make_inputs(c, index))
    scale = 1.0 / math.sqrt(c["d"])
    window = c.get("window", 0)
    o, lse = ext.flash_attn_fwd(q, k, v, c["causal"], scale, bias, c["sbhd"],
                                window)
    res = ext.flash_attn_bwd(dout, q, k, v, o, lse, c["causal"], scale, bias,
                             c["sbhd"], window)
    out = dict(o=o, lse=lse, dq=res[0], dk=res[1], dv=res[2])
    if bias is not None:
        out["dbias"] = res[3]
    return dict(q=q, k=k, v=v, dout=dout, bias=bias), out


def digest(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    from hetu_galvatron_amd.ops._ext import get_ext
    ext = get_ext(False)
    device = torch.device("cuda:0")
    record = {}
    for index, (name, c) in enumerate(CASES):
        _, out = run_case(ext, c, index, device)
        # dbias is summed with fp32 atomics over the batch: its bits depend
        # on the order the hardware retires them, so it is not recorded
        record[name] = {key: digest(val) for key, val in out.items()
                        if key != "dbias"}
    json.dump(record, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
