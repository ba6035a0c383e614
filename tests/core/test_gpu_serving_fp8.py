"""ContinuousBatchingEngine(kv_cache_dtype="fp8"), the scenario of
test_gpu_serving_batched.py, run with the torch paths of the two cache ops
(the reference) and native: largest gap to the argmax of a bf16 recompute."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _largest_gap(eng, cfg, S):
    from hetu_galvatron_amd.runtime.inference import KVCache
    prompts = [torch.randint(0, cfg.model.vocab_size, (n,), device="cuda",
                             generator=torch.Generator("cuda").manual_seed(n))
               for n in (5, 260, 9)]
    rids = [eng.add_request(prompts[0], 6), eng.add_request(prompts[1], 4)]
    eng.step()
    rids.append(eng.add_request(prompts[2], 3))
    while eng.n_active:
        eng.step()
    worst = 0.0
    for p, rid in zip(prompts, rids):
        seq = torch.cat([p, torch.tensor(eng.outputs[rid], device="cuda")])
        for i in range(p.shape[0], seq.shape[0]):
            cache = KVCache(len(eng.gen.layers), 1, S, cfg.model.kv_heads,
                            cfg.model.head_dim, seq.device)
            logits = eng.gen._forward_tokens(seq[None, :i], cache)
            worst = max(worst, float(logits.max() - logits[0, seq[i]]))
    return worst


@pytest.mark.parametrize("window", [None, 8])
def test_engine_fp8_cache(window, monkeypatch):
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.ops import functional as F
    from hetu_galvatron_amd.runtime import GalvatronModel, serving
    model_cfg = {"model_name": "tiny-llama"}
    if window:
        model_cfg["sliding_window"] = window
    cfg = load_config(base={
        "model": model_cfg,
        "train": {"global_train_batch_size": 2, "train_iters": 1}})
    torch.manual_seed(0)
    model = GalvatronModel(cfg)
    S = 512

    def engine(**kw):
        return serving.ContinuousBatchingEngine(model, max_slots=3, max_seq=S,
                                                kv_cache_dtype="fp8", **kw)

    with pytest.raises(ValueError, match="batched_attention"):
        engine(batched_attention=False)

    def attend(q, kc, vc, lengths, slots, max_len, softmax_scale, **kw):
        return F._decode_attention_batched_fp8_torch(
            q, kc, vc, lengths, slots, max_len, softmax_scale, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(serving, "decode_attention_batched", attend)
        mp.setattr(serving, "kv_cache_append", F._kv_cache_append_torch)
        ref = _largest_gap(engine(batched_attention=True), cfg, S)
    eng = engine(batched_attention=True)
    assert eng.cache.k[0].dtype == torch.float8_e4m3fn
    got = _largest_gap(eng, cfg, S)
    print(f"[engine fp8] window={window}: largest gap torch paths {ref:.4g}, "
          f"native {got:.4g}")
    assert got <= max(2 * ref, 0.05)
