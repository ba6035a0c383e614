"""test_serving_fused_prologue.py on the GPU in bf16, where the fused engine
runs the decode prologue kernel and the unfused one `_rope_rows`, indexed
copies and `kv_cache_append`: identical tokens and caches, and the chunked
prefill criterion of test_gpu_serving_prefill_chunk.py."""
import pytest

from .test_serving_fused_prologue import (IDS, KINDS, check_chunked,
                                          check_decode, make_model)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
@pytest.mark.parametrize("spec", [0, 3])
def test_fused_decode_generates_the_unfused_tokens(spec, kw):
    check_decode(make_model(fp32=False)[0], spec, kw)


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_fused_chunked_prefill(kw):
    check_chunked(*make_model(fp32=False), kw)
