"""ContinuousBatchingEngine(prefill_chunk=32) on the CPU (fp32, torch paths):
the tokens of the unchunked engine, for prompts of one chunk and of four."""
import pytest
import torch

from hetu_galvatron_amd.runtime.serving import ContinuousBatchingEngine

from .test_serving_speculative import VOCAB, make_model, run_schedule


def long_prompt(model, **kw):
    """A 100-token prompt: three chunks of 32 and a tail of 4."""
    eng = ContinuousBatchingEngine(model, max_slots=2, max_seq=128,
                                   batched_attention=True, **kw)
    g = torch.Generator().manual_seed(7)
    p = torch.randint(0, VOCAB, (100,), generator=g).to(eng.gen._dev)
    rid = eng.add_request(p, 10)
    while eng.n_active:
        eng.step()
    return eng.outputs[rid]


@pytest.mark.parametrize("window", [None, 8])
@pytest.mark.parametrize("page_size", [None, 32])
def test_chunked_prefill_generates_the_unchunked_tokens(page_size, window):
    model = make_model(window)
    kw = dict(page_size=page_size, kv_cache_dtype=None)
    assert run_schedule(model, prefill_chunk=32, **kw)[0] == \
        run_schedule(model, **kw)[0]
    assert long_prompt(model, prefill_chunk=32, **kw) == \
        long_prompt(model, **kw)


def test_prefill_chunk_needs_batched_attention():
    with pytest.raises(ValueError, match="batched_attention"):
        ContinuousBatchingEngine(make_model(), max_slots=2, max_seq=64,
                                 prefill_chunk=32)
