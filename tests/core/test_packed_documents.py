"""Packed documents through the training path: data.reset_attention_mask /
data.reset_position_ids (document boundaries -> cu_seqlens -> varlen
attention; per-document positions).  CPU, fp32 reference attention path.
"""
import copy

import pytest
import torch

from hetu_galvatron_amd.config import HybridParallelPlan, load_config
from hetu_galvatron_amd.runtime.dataloader import (
    SyntheticCausalLMDataset, build_batch_context, packed_cu_seqlens)
from hetu_galvatron_amd.runtime.pipeline.engine import chunk_batch

EOD = 5
CPU = torch.device("cpu")


# ---------------------------------------------------------------------------
# batch context
# ---------------------------------------------------------------------------
def _rows():
    """[B=5, S+1=9] hand-written token rows (last column only feeds labels)."""
    E = EOD
    return torch.tensor([
        [E, 7, 8, 9, 7, 8, 9, 7, 7],   # EOD at position 0
        [7, 8, 9, 7, 8, 9, 7, E, 7],   # EOD at position S-1
        [7, 8, E, E, 9, 7, 8, 9, 7],   # two adjacent EODs
        [7, 8, 9, 7, 8, 9, 7, 8, 7],   # no EOD at all
        [7, E, 8, 9, 7, E, 8, 9, E],   # two documents + an EOD label only
    ])


BOUNDS = [[0, 1, 8], [0, 8], [0, 3, 4, 8], [0, 8], [0, 2, 6, 8]]
POSITIONS = [[0, 0, 1, 2, 3, 4, 5, 6],
             [0, 1, 2, 3, 4, 5, 6, 7],
             [0, 1, 2, 0, 0, 1, 2, 3],
             [0, 1, 2, 3, 4, 5, 6, 7],
             [0, 1, 0, 1, 2, 3, 0, 1]]


def test_boundaries_and_positions_literal():
    ctx = build_batch_context(_rows(), CPU, eod_token=EOD,
                              reset_attention_mask=True,
                              reset_position_ids=True)
    assert ctx["doc_boundaries"] == BOUNDS
    assert ctx["position_ids"].tolist() == POSITIONS
    assert ctx["position_ids"].dtype == torch.long


def test_each_flag_adds_only_its_key():
    base = build_batch_context(_rows(), CPU, eod_token=EOD)
    assert set(base) == {"input_ids", "labels", "batch_size", "seq_len"}
    a = build_batch_context(_rows(), CPU, eod_token=EOD,
                            reset_attention_mask=True)
    assert set(a) - set(base) == {"doc_boundaries"}
    p = build_batch_context(_rows(), CPU, eod_token=EOD,
                            reset_position_ids=True)
    assert set(p) - set(base) == {"position_ids"}
    for k in base:
        same = torch.equal(base[k], a[k]) if torch.is_tensor(base[k]) \
            else base[k] == a[k]
        assert same
    with pytest.raises(AssertionError, match="eod_token_id"):
        build_batch_context(_rows(), CPU, reset_attention_mask=True)


def test_chunk_batch_and_rows_helper():
    ctx = build_batch_context(_rows(), CPU, eod_token=EOD,
                              reset_attention_mask=True,
                              reset_position_ids=True)
    # whole batch
    cu, mx = packed_cu_seqlens(ctx, 0, 5, CPU)
    assert cu.dtype == torch.int32
    assert cu.tolist() == [0, 1, 8, 16, 19, 20, 24, 32, 34, 38, 40]
    assert mx == 8
    # a dp slice: offsets restart at the slice's first row
    cu, mx = packed_cu_seqlens(ctx, 2, 3, CPU)
    assert cu.tolist() == [0, 3, 4, 8] and mx == 4
    cu, mx = packed_cu_seqlens(ctx, 4, 5, CPU)
    assert cu.tolist() == [0, 2, 6, 8] and mx == 4
    # memoized: the same tensor object comes back
    assert packed_cu_seqlens(ctx, 4, 5, CPU)[0] is cu
    # uneven microbatches: 5 rows over 2 chunks -> 3 + 2
    mbs = chunk_batch(ctx, 2, dp=1)
    assert [m["batch_size"] for m in mbs] == [3, 2]
    assert mbs[0]["doc_boundaries"] == BOUNDS[:3]
    assert mbs[1]["doc_boundaries"] == BOUNDS[3:]
    assert mbs[0]["position_ids"].tolist() == POSITIONS[:3]
    assert mbs[1]["position_ids"].tolist() == POSITIONS[3:]
    cu, mx = packed_cu_seqlens(mbs[1], 0, 2, CPU)
    assert cu.tolist() == [0, 8, 10, 14, 16] and mx == 8
    cu, mx = packed_cu_seqlens(mbs[1], 1, 2, CPU)
    assert cu.tolist() == [0, 2, 6, 8] and mx == 4
    # each microbatch memoizes on its own
    assert mbs[0]["_cu_seqlens_cache"] is not mbs[1]["_cu_seqlens_cache"]
    # dp=2 microbatches stay multiples of dp
    ctx4 = build_batch_context(_rows()[:4], CPU, eod_token=EOD,
                               reset_attention_mask=True)
    mbs = chunk_batch(ctx4, 2, dp=2)
    assert [m["doc_boundaries"] for m in mbs] == [BOUNDS[:2], BOUNDS[2:4]]
    assert packed_cu_seqlens(mbs[1], 1, 2, CPU)[0].tolist() == [0, 8]


def test_ctx_unchanged_through_chunk_batch_when_off():
    ctx = build_batch_context(_rows(), CPU, eod_token=EOD)
    for m in chunk_batch(ctx, 2):
        assert "doc_boundaries" not in m and "position_ids" not in m
        assert "_cu_seqlens_cache" not in m


def test_synthetic_dataset_documents():
    off = SyntheticCausalLMDataset(512, 128, seed=3)
    on = SyntheticCausalLMDataset(512, 128, seed=3, eod_token=EOD,
                                  mean_doc_length=16)
    a, b = off[7], on[7]
    assert torch.equal(on[7], b), "deterministic"
    changed = a != b
    assert changed.any() and (b[changed] == EOD).all(), \
        "only EODs are written over the unchanged stream"
    n_docs = int((b == EOD).sum())
    assert 3 <= n_docs <= 40
    assert torch.equal(
        SyntheticCausalLMDataset(512, 128, seed=3, eod_token=EOD)[7], a)


# ---------------------------------------------------------------------------
# tiny model (fp32, 1 process)
# ---------------------------------------------------------------------------
S = 128
SPLIT = 50          # document A = [0, 50) (EOD at 49), document B = [50, 128)
PACKED = {"eod_token_id": EOD, "reset_attention_mask": True,
          "reset_position_ids": True}


def _cfg(model_name="tiny-llama", data=None, extra=None):
    base = {
        "model": {"model_name": model_name},
        "train": {"global_train_batch_size": 4, "train_iters": 3,
                  "lr": 1e-3, "lr_decay_style": "constant",
                  "distributed_backend": "gloo"},
        "parallel": {"mixed_precision": "fp32"},
        "data": dict(data or {}),
    }
    for k, v in (extra or {}).items():
        base.setdefault(k, {}).update(v)
    return load_config(base=base)


def _model(cfg):
    from hetu_galvatron_amd.runtime import GalvatronModel
    torch.manual_seed(0)
    return GalvatronModel(cfg).eval()


def _two_doc_tokens(seed):
    """[2, S+1] tokens without accidental EODs, one EOD at SPLIT-1."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(EOD + 1, 512, (2, S + 1), generator=g)
    t[:, SPLIT - 1] = EOD
    return t


@torch.no_grad()
def _logits(model, ctx):
    """[S, b, V] logits: all blocks but the loss head, then its linear."""
    ctx = dict(ctx)
    ctx["global_batch"] = ctx["batch_size"]
    blocks = model.stage_model.blocks
    h = None
    for blk in blocks[:-1]:
        h = blk(h, ctx)
    head = blocks[-1]
    assert head.kind == "lm_head"
    if head.flat is not None:
        head.flat.gather_params()
    return head.inner.lm_head(h).float()


def _packed_ctx(tokens, **flags):
    return build_batch_context(tokens, CPU, eod_token=EOD, **flags)


@pytest.mark.parametrize("model_name", ["tiny-llama", "tiny-gpt"])
def test_document_isolation(model_name):
    model = _model(_cfg(model_name, PACKED))
    t1 = _two_doc_tokens(1)
    t2 = t1.clone()
    t2[:, :SPLIT - 1] = _two_doc_tokens(2)[:, :SPLIT - 1]  # rewrite doc A
    assert not torch.equal(t1, t2)
    on = dict(reset_attention_mask=True, reset_position_ids=True)
    l1 = _logits(model, _packed_ctx(t1, **on))
    l2 = _logits(model, _packed_ctx(t2, **on))
    assert (l1[:SPLIT] - l2[:SPLIT]).abs().max() > 1e-3, "doc A did change"
    assert (l1[SPLIT:] - l2[SPLIT:]).abs().max() < 1e-6, \
        "document B saw document A"
    # the same batch WITHOUT the flags leaks A into B (dense causal)
    d1 = _logits(model, _packed_ctx(t1))
    d2 = _logits(model, _packed_ctx(t2))
    assert (d1[SPLIT:] - d2[SPLIT:]).abs().max() > 1e-3


@pytest.mark.parametrize("model_name", ["tiny-llama", "tiny-gpt"])
def test_document_equals_running_it_alone(model_name):
    model = _model(_cfg(model_name, PACKED))
    t = _two_doc_tokens(3)
    packed = _logits(model, _packed_ctx(t, reset_attention_mask=True,
                                        reset_position_ids=True))
    alone = _logits(model, build_batch_context(t[:, SPLIT:], CPU))
    assert alone.shape[0] == S - SPLIT
    assert (packed[SPLIT:] - alone).abs().max() < 1e-5
    if model_name == "tiny-gpt":
        # absolute (learned) positions: attention isolation alone is not
        # enough, the positions have to restart too (RoPE is relative, so
        # llama does not show this)
        mask_only = _logits(model, _packed_ctx(t, reset_attention_mask=True))
        assert (mask_only[SPLIT:] - alone).abs().max() > 1e-4


def _flat_grads(model):
    return [blk.flat.flat_grad.clone() for blk in model.stage_model.blocks
            if blk.flat is not None and blk.flat.flat_grad is not None]


def test_microbatching_keeps_gradients():
    from hetu_galvatron_amd.runtime import get_train_iterator
    data = dict(PACKED, synthetic_mean_doc_length=16)
    cfg = _cfg("tiny-llama", data)
    ctx = next(get_train_iterator(cfg, CPU))
    assert len(ctx["doc_boundaries"]) == 4
    assert max(len(b) for b in ctx["doc_boundaries"]) > 3
    grads = []
    for chunks in (1, 2):
        model = _model(cfg).train()
        stats = model.forward_backward(copy.copy(ctx), chunks=chunks)
        assert stats.loss == stats.loss
        grads.append(_flat_grads(model))
    assert len(grads[0]) == len(grads[1]) > 0
    for a, b in zip(*grads):
        assert a.abs().max() > 0
        assert (a - b).abs().max() < 1e-5


def test_three_steps_train():
    from hetu_galvatron_amd.runtime import (
        get_optimizer_and_param_scheduler, get_train_iterator)
    data = dict(PACKED, synthetic_mean_doc_length=16)
    cfg = _cfg("tiny-llama", data)
    model = _model(cfg).train()
    opt, sched = get_optimizer_and_param_scheduler(model.stage_model, cfg)
    ctx = next(get_train_iterator(cfg, CPU))  # one batch, memorized
    losses = []
    for _ in range(3):
        opt.zero_grad()
        stats = model.forward_backward(copy.copy(ctx), chunks=2)
        opt.step()
        sched.step()
        losses.append(stats.loss)
    assert all(l == l and l < float("inf") for l in losses), losses
    assert losses[0] > losses[1] > losses[2], losses


# ---------------------------------------------------------------------------
# distributed (gloo, world 2) vs the 1-process run
# ---------------------------------------------------------------------------
DIST_EXTRA = {"data": dict(PACKED, synthetic_mean_doc_length=16)}


def _dist_case(plan):
    from tests.core.test_parallel_correctness import (
        TOL, _dist_worker, get_baseline_with)
    from tests.utils import run_distributed
    base_losses, state_path = get_baseline_with(DIST_EXTRA)
    res = run_distributed(_dist_worker, world_size=2,
                          args=(plan.to_config_dict(), state_path,
                                DIST_EXTRA))
    for r, losses in enumerate(res):
        for s, (a, b) in enumerate(zip(losses, base_losses)):
            assert abs(a - b) < TOL, f"rank {r} step {s}: {a:.4f} vs {b:.4f}"


@pytest.mark.distributed
def test_dp2_packed_documents():
    _dist_case(HybridParallelPlan.uniform(2, 2, dp_type="ddp", global_bsz=4))


@pytest.mark.distributed
def test_tp2_packed_documents():
    _dist_case(HybridParallelPlan.uniform(2, 2, tp=2, vtp=2, global_bsz=4))


# ---------------------------------------------------------------------------
# config
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["reset_attention_mask",
                                  "reset_position_ids"])
@pytest.mark.parametrize("extra,what", [
    ({"parallel": {"global_cp_deg": 2}}, "cp > 1"),
    ({"parallel": {"use_ulysses": True}}, "Ulysses"),
    ({"model": {"sliding_window": 64}}, "sliding_window"),
    ({"model": {"attention_dropout": 0.1}}, "attention_dropout"),
    ({"model": {"model_type": "t5"}}, "t5"),
])
def test_forbidden_combinations_raise(flag, extra, what):
    data = {"eod_token_id": EOD, flag: True}
    _cfg("tiny-llama", data)  # fine on its own
    with pytest.raises(ValueError, match=what):
        _cfg("tiny-llama", data, extra)


def test_flags_need_eod_token():
    with pytest.raises(ValueError, match="eod_token_id"):
        _cfg("tiny-llama", {"reset_attention_mask": True})
    with pytest.raises(ValueError, match="eod_token_id"):
        _cfg("tiny-llama", {"reset_position_ids": True})
    with pytest.raises(ValueError, match="eod_token_id"):
        _cfg("tiny-llama", {"synthetic_mean_doc_length": 16})


@pytest.mark.parametrize("plan", [
    HybridParallelPlan.uniform(2, 2, cp=2, global_bsz=4),
    HybridParallelPlan.uniform(2, 2, tp=2, use_sp=True, global_bsz=4),
])
def test_plan_with_cp_or_ulysses_is_refused_at_model_build(plan):
    from hetu_galvatron_amd.runtime import GalvatronModel
    with pytest.raises(ValueError, match="cp > 1 or Ulysses"):
        GalvatronModel(_cfg("tiny-llama", PACKED), plan)


def test_attention_refuses_cu_seqlens_off_the_local_path():
    """A layer that cannot isolate documents must not run dense instead."""
    from hetu_galvatron_amd.runtime.transformer.attention import SelfAttention
    cfg = _cfg("tiny-llama", extra={"model": {"sliding_window": 16}})
    att = SelfAttention(cfg.model, None, None, None, dtype=torch.float32)
    x = torch.randn(8, 1, cfg.model.hidden_size)
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="packed-document"):
        att(x, None, None, cu_seqlens=cu, max_seqlen=5)
