"""The decode prologue kernel (decode_prologue.hip) against the op's torch
path, bit for bit, on q and on the whole sentinel-filled caches: the edge
shape of test_rope_kv_append_fallback.py (q heads that fill no power of two,
a page crossing, an invalid page, slots outside the table, the last position)
and one case at the flagship geometry."""
import pytest
import torch

from hetu_galvatron_amd.ops import functional as F

from .test_rope_kv_append_fallback import EDGE, FLAGSHIP, KINDS, make_case

pytestmark = pytest.mark.gpu

CASES = [(D, fp8, paged, il, 4, EDGE, True) for D in (64, 128)
         for fp8, paged in KINDS for il in (False, True)]
CASES += [(64, False, False, False, 4, EDGE, False),      # cos=None
          (128, True, False, False, 3, EDGE, True),       # slot 3 outside
          (64, False, True, True, 3, EDGE, True),
          (128, True, True, False, 4, FLAGSHIP, True)]


@pytest.mark.parametrize("D,fp8,paged,il,S,shape,rotate", CASES)
def test_native_equals_fallback(D, fp8, paged, il, S, shape, rotate):
    assert F.native_available()
    out = []
    for f in (F.rope_kv_append, F._rope_kv_append_torch):
        args, kw, _ = make_case(D, fp8, paged, S, shape, "cuda")
        if not rotate:
            args[3] = args[4] = None
        kw = {"k_scale": None, "v_scale": None, "page_table": None, **kw}
        q = f(*args, **kw, interleaved=il)
        out.append([q] + [kw[c].view(torch.uint8)
                          for c in ("k_cache", "v_cache")])
    torch.cuda.synchronize()
    for name, got, want in zip("qkv", *out):
        assert torch.equal(got, want), name
