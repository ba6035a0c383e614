"""ContinuousBatchingEngine(page_size=32) on the GPU, bf16 and fp8 caches:
the schedule of test_serving_paged.py gives the tokens of the contiguous
engine with the same cache dtype (without a window the paged kernels return
the contiguous kernels' bits)."""
import pytest
import torch

from .test_serving_paged import NUM_PAGES, PAGE, run_schedule

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kv_cache_dtype", [None, "fp8"])
def test_paged_engine_generates_the_contiguous_tokens(kv_cache_dtype):
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.runtime import GalvatronModel
    cfg = load_config(base={
        "model": {"model_name": "tiny-llama"},
        "train": {"global_train_batch_size": 2, "train_iters": 1}})
    torch.manual_seed(0)
    model = GalvatronModel(cfg)
    vocab = cfg.model.vocab_size
    want = run_schedule(model, vocab, kv_cache_dtype=kv_cache_dtype)
    got = run_schedule(model, vocab, kv_cache_dtype=kv_cache_dtype,
                       page_size=PAGE, num_pages=NUM_PAGES)
    assert got == want
