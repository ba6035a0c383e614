"""ContinuousBatchingEngine(fused_prologue=True) against the same engine
without it (fp32 here, so `rope_kv_append` takes its torch path): the same
tokens and caches in plain and speculative decode, and a chunked prefill that
is as close to a recompute as the unfused one."""
import pytest
import torch

from hetu_galvatron_amd.runtime.inference import KVCache
from hetu_galvatron_amd.runtime.serving import ContinuousBatchingEngine

KINDS = [dict(), dict(kv_cache_dtype="fp8", page_size=32)]
IDS = ["bf16-contiguous", "fp8-paged"]


def make_model(fp32=True):
    from hetu_galvatron_amd.config import load_config
    from hetu_galvatron_amd.runtime import GalvatronModel
    base = {"model": {"model_name": "tiny-llama"},
            "train": {"global_train_batch_size": 2, "train_iters": 1}}
    if fp32:
        base["parallel"] = {"mixed_precision": "fp32"}
        base["train"]["distributed_backend"] = "gloo"
    cfg = load_config(base=base)
    torch.manual_seed(0)
    return GalvatronModel(cfg), cfg


def decode_run(model, fused, spec, **kw):
    """12 steps of two requests whose 30-token prompts repeat themselves; the
    model soon loops on them, so `ngram_draft` proposes.
    -> (the steps' tokens, the cache tensors)"""
    eng = ContinuousBatchingEngine(model, max_slots=3, max_seq=128,
                                   batched_attention=True,
                                   speculative_tokens=spec,
                                   fused_prologue=fused, **kw)
    for c in eng.cache.k + eng.cache.v:
        c.view(torch.uint8).zero_()
    for seed in (17, 23):
        a = torch.randint(0, 512, (13,),
                          generator=torch.Generator().manual_seed(seed))
        eng.add_request(torch.cat([a, a, a[:4]]).to(eng.gen._dev), 30)
    toks = [eng.step() for _ in range(12)]
    assert not spec or sum(eng.drafted.values()) > 0
    return toks, [c.view(torch.uint8) for c in eng.cache.k + eng.cache.v]


def check_decode(model, spec, kw):
    want, want_caches = decode_run(model, False, spec, **kw)
    got, caches = decode_run(model, True, spec, **kw)
    assert got == want
    assert all(torch.equal(a, b) for a, b in zip(caches, want_caches))


def chunk_gap(model, cfg, fused, **kw):
    """A 70-token prompt in chunks of 32, 32 and 6, then 6 tokens: the largest
    gap of an emitted token to the argmax of a recompute."""
    eng = ContinuousBatchingEngine(model, max_slots=2, max_seq=128,
                                   batched_attention=True, prefill_chunk=32,
                                   fused_prologue=fused, **kw)
    dev = eng.gen._dev
    p = torch.randint(0, 512, (70,),
                      generator=torch.Generator().manual_seed(70)).to(dev)
    rid = eng.add_request(p, 6)
    while eng.n_active:
        eng.step()
    seq = torch.cat([p, torch.tensor(eng.outputs[rid], device=dev)])
    worst = 0.0
    for i in range(70, seq.shape[0]):
        cache = KVCache(len(eng.gen.layers), 1, 128, cfg.model.kv_heads,
                        cfg.model.head_dim, dev,
                        dtype=next(eng.gen.embedding.parameters()).dtype)
        logits = eng.gen._forward_tokens(seq[None, :i], cache)
        worst = max(worst, float(logits.max() - logits[0, seq[i]]))
    return worst


def check_chunked(model, cfg, kw):
    ref = chunk_gap(model, cfg, False, **kw)
    got = chunk_gap(model, cfg, True, **kw)
    print(f"[fused chunked prefill] {kw}: largest gap unfused {ref:.4g}, "
          f"fused {got:.4g}")
    assert got <= max(2 * ref, 0.05)


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
@pytest.mark.parametrize("spec", [0, 3])
def test_fused_decode_generates_the_unfused_tokens(spec, kw):
    check_decode(make_model()[0], spec, kw)


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_fused_chunked_prefill(kw):
    check_chunked(*make_model(), kw)


def test_fused_prologue_needs_batched_attention():
    with pytest.raises(ValueError, match="batched_attention"):
        ContinuousBatchingEngine(make_model()[0], max_slots=2, max_seq=64,
                                 fused_prologue=True)
