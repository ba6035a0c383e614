"""ContinuousBatchingEngine(speculative_tokens=3) on the CPU (fp32, torch
paths): the greedy tokens of the plain batched engine in fewer steps, with
drafts that are partly right."""
import pytest
import torch

from hetu_galvatron_amd.runtime.serving import (ContinuousBatchingEngine,
                                                ngram_draft)

VOCAB = 512


def make_model(window=None):
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.runtime import GalvatronModel
    model_cfg = {"model_name": "tiny-llama"}
    if window:
        model_cfg["sliding_window"] = window
    cfg = load_config(base={
        "model": model_cfg, "parallel": {"mixed_precision": "fp32"},
        "train": {"global_train_batch_size": 2, "train_iters": 1,
                  "distributed_backend": "gloo"}})
    torch.manual_seed(0)
    return GalvatronModel(cfg)


def run_schedule(model, **kw):
    """30 + 12 crosses a page boundary while decoding; a third request joins
    after the first step.  -> (prompt + tokens per request, steps, engine)"""
    eng = ContinuousBatchingEngine(model, max_slots=3, max_seq=128,
                                   batched_attention=True, **kw)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).to(eng.gen._dev)
               for n in (30, 9, 5)]
    rids = [eng.add_request(prompts[0], 12), eng.add_request(prompts[1], 10)]
    out = eng.step()
    rids.append(eng.add_request(prompts[2], 8))
    steps = 1
    while eng.n_active:
        out = eng.step()
        steps += 1
    return [p.tolist() + eng.outputs[r] for p, r in zip(prompts, rids)], \
        steps, eng


@pytest.mark.parametrize("window", [None, 8])
@pytest.mark.parametrize("kv_cache_dtype", [None, "fp8"])
@pytest.mark.parametrize("page_size", [None, 32])
def test_speculative_engine_generates_the_plain_tokens(page_size,
                                                       kv_cache_dtype, window):
    model = make_model(window)
    kw = dict(page_size=page_size, kv_cache_dtype=kv_cache_dtype)
    want, plain_steps, _ = run_schedule(model, **kw)
    calls = [0]

    def draft_fn(history, k):
        """The recorded continuation; every third proposal's second token
        is wrong."""
        full = next(f for f in want if f[:len(history)] == history)
        d = full[len(history):len(history) + k]
        calls[0] += 1
        if calls[0] % 3 == 0 and len(d) > 1:
            d[1] = (d[1] + 1) % VOCAB
        return d

    got, steps, eng = run_schedule(model, speculative_tokens=3,
                                   draft_fn=draft_fn, **kw)
    assert got == want
    assert steps < plain_steps
    assert all(a >= 1 for a in eng.accepted.values()), eng.accepted
    assert sum(eng.accepted.values()) < sum(eng.drafted.values())


def test_ngram_draft():
    assert ngram_draft([1, 2, 3, 4, 1, 2, 9, 1, 2], 3) == [9, 1, 2]
    assert ngram_draft([1, 2, 3, 4, 1, 2, 9, 1, 2], 1) == [9]
    assert ngram_draft([7, 1, 2, 5, 1, 2], 4) == [5, 1, 2]
    assert ngram_draft([1, 2, 3, 4], 3) == [] and ngram_draft([1, 2], 3) == []


def test_speculative_needs_batched_attention():
    with pytest.raises(ValueError, match="batched_attention"):
        ContinuousBatchingEngine(make_model(), max_slots=2, max_seq=64,
                                 speculative_tokens=2)
