"""ContinuousBatchingEngine(prefill_chunk=64, page_size=32), the scenario of
test_gpu_serving_fp8.py: the 260-token prompt is four 64-token chunks on the
prefill kernels and a 4-token tail on the multi-token ones.  Run with the
torch forms of `decode_attention_multi` and `kv_cache_append` (the reference)
and native: largest gap to the argmax of a bf16 recompute."""
import pytest
import torch

from .test_gpu_serving_fp8 import _largest_gap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kv_cache_dtype", [None, "fp8"])
def test_engine_chunked_prefill(kv_cache_dtype, monkeypatch):
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.ops import functional as F
    from hetu_galvatron_amd.runtime import GalvatronModel, serving
    cfg = load_config(base={
        "model": {"model_name": "tiny-llama"},
        "train": {"global_train_batch_size": 2, "train_iters": 1}})
    torch.manual_seed(0)
    model = GalvatronModel(cfg)
    S = 512

    def engine():
        return serving.ContinuousBatchingEngine(
            model, max_slots=3, max_seq=S, batched_attention=True,
            kv_cache_dtype=kv_cache_dtype, page_size=32, prefill_chunk=64)

    def attend(q, kc, vc, lengths, q_lens, slots, window=None, max_len=None,
               softmax_scale=None, k_scale=None, v_scale=None,
               page_table=None):
        return F._decode_attention_multi_torch(
            q, kc, vc, lengths, q_lens, slots, page_table.shape[0], max_len,
            softmax_scale, window, k_scale, v_scale, page_table)

    with monkeypatch.context() as mp:
        mp.setattr(serving, "decode_attention_multi", attend)
        mp.setattr(serving, "kv_cache_append", F._kv_cache_append_torch)
        ref = _largest_gap(engine(), cfg, S)
    got = _largest_gap(engine(), cfg, S)
    print(f"[engine chunked prefill] cache={kv_cache_dtype}: largest gap "
          f"torch paths {ref:.4g}, native {got:.4g}")
    assert got <= max(2 * ref, 0.05)
