"""ContinuousBatchingEngine(speculative_tokens=3) on a paged cache, run with
the torch paths of the cache ops (the reference) and native: largest gap to
the argmax of a full bf16 recompute, the method and bound of
test_gpu_serving_fp8.py.  Drafts are the plain engine's recorded continuation
with every third proposal's second token wrong, so some are accepted and some
rejected."""
import pytest
import torch

from .test_gpu_serving_fp8 import _largest_gap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kv_cache_dtype", [None, "fp8"])
def test_speculative_engine_native(kv_cache_dtype, monkeypatch):
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.ops import functional as F
    from hetu_galvatron_amd.runtime import GalvatronModel, serving
    cfg = load_config(base={
        "model": {"model_name": "tiny-llama"},
        "train": {"global_train_batch_size": 2, "train_iters": 1}})
    torch.manual_seed(0)
    model = GalvatronModel(cfg)
    S = 512

    def engine(**kw):
        return serving.ContinuousBatchingEngine(
            model, max_slots=3, max_seq=S, batched_attention=True,
            kv_cache_dtype=kv_cache_dtype, page_size=32, **kw)

    plain = engine()
    _largest_gap(plain, cfg, S)
    # the prompts of _largest_gap, in request order, with the plain tokens
    record = [torch.randint(
        0, cfg.model.vocab_size, (n,), device="cuda",
        generator=torch.Generator("cuda").manual_seed(n)).tolist()
        + plain.outputs[rid] for rid, n in enumerate((5, 260, 9))]
    calls = [0]

    def draft_fn(history, k):
        full = next((f for f in record if f[:len(history)] == history), [])
        d = full[len(history):len(history) + k]
        if calls[0] % 3 == 0 and len(d) > 1:     # the first, the fourth, ..
            d[1] = (d[1] + 1) % cfg.model.vocab_size
        calls[0] += 1
        return d

    spec = dict(speculative_tokens=3, draft_fn=draft_fn)

    def attend(q, kc, vc, lengths, q_lens, slots, window=None, max_len=None,
               softmax_scale=None, k_scale=None, v_scale=None,
               page_table=None):
        return F._decode_attention_multi_torch(
            q, kc, vc, lengths, q_lens, slots, page_table.shape[0], max_len,
            softmax_scale, window, k_scale, v_scale, page_table)

    with monkeypatch.context() as mp:
        mp.setattr(serving, "decode_attention_multi", attend)
        mp.setattr(serving, "kv_cache_append", F._kv_cache_append_torch)
        ref = _largest_gap(engine(**spec), cfg, S)
    eng = engine(**spec)
    got = _largest_gap(eng, cfg, S)
    drafted, accepted = (sum(x.values()) for x in (eng.drafted, eng.accepted))
    print(f"[engine speculative] cache={kv_cache_dtype}: largest gap torch "
          f"paths {ref:.4g}, native {got:.4g}; {accepted} of {drafted} drafts "
          f"accepted")
    assert drafted > accepted > 0
    assert got <= max(2 * ref, 0.05)
