"""Data pipeline: synthetic causal-LM batches (+ batch-context assembly).

Reference: galvatron/core/runtime/dataloader.py:36-567 (FakeCausalLMDataset,
get_batch, loss averaging).  The megatron mmap dataset stack hooks in via
data.dataset="megatron" (see datasets/).

Design note: every rank materializes the FULL global batch of token ids
(ids are ~2 bytes/token of int64 -> negligible vs activations) and each
layer module slices batch/sequence by its own layout — this is what makes
per-layer dp/tp/cp degrees composable without a per-layer dataloader.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional

import torch

from ..config import GalvatronConfig


class SyntheticCausalLMDataset(torch.utils.data.Dataset):
    """Deterministic synthetic token stream (same on every rank for a given
    seed + index; reference: dataloader.py:36 FakeCausalLMDataset)."""

    def __init__(self, vocab_size: int, seq_length: int, size: int = 1024,
                 seed: int = 1234, eod_token: Optional[int] = None,
                 mean_doc_length: int = 0):
        self.vocab_size = vocab_size
        self.seq_length = seq_length
        self.size = size
        self.seed = seed
        # packed-document mode: an EOD closes a document every
        # uniform[1, 2*mean-1] tokens (off by default: stream unchanged)
        self.eod_token = eod_token
        self.mean_doc_length = int(mean_doc_length or 0)
        if self.mean_doc_length:
            assert eod_token is not None, \
                "mean_doc_length needs an eod_token"

    def __len__(self) -> int:
        return self.size

    def __getitem__(self, idx: int) -> torch.Tensor:
        g = torch.Generator()
        g.manual_seed(self.seed * 100003 + idx)
        tokens = torch.randint(0, self.vocab_size, (self.seq_length + 1,),
                               generator=g)
        if self.mean_doc_length:
            n = self.seq_length + 1
            lens = torch.randint(1, 2 * self.mean_doc_length, (n,),
                                 generator=g)
            ends = torch.cumsum(lens, 0) - 1  # last token of each document
            tokens[ends[ends < n]] = self.eod_token
        return tokens


def document_boundaries(input_ids: torch.Tensor, eod_token: int
                        ) -> List[List[int]]:
    """Per-row document boundaries of input_ids [B, S], on the host.

    A document ends AFTER each position holding eod_token (the EOD belongs
    to the document it closes; the next one starts at i+1).  Each row's
    list starts at 0, ends at S and is strictly increasing."""
    ids = input_ids.cpu()
    S = ids.shape[1]
    out = []
    for row in ids:
        ends = (torch.nonzero(row == eod_token).flatten() + 1).tolist()
        out.append([0] + [e for e in ends if e < S] + [S])
    return out


def positions_from_boundaries(bounds: List[List[int]], S: int
                              ) -> torch.Tensor:
    """position_ids [B, S] (host int64) restarting at 0 at every boundary."""
    ar = torch.arange(S)
    pos = torch.empty(len(bounds), S, dtype=torch.long)
    for r, bd in enumerate(bounds):
        start = torch.zeros(S, dtype=torch.long)
        start[torch.tensor(bd[:-1])] = torch.tensor(bd[:-1])
        pos[r] = ar - torch.cummax(start, 0).values
    return pos


def packed_cu_seqlens(ctx: Dict, lo: int, hi: int, device
                      ) -> tuple:
    """(cu_seqlens int32 on `device`, max_seqlen) for batch rows [lo, hi)
    of a packed-document ctx (ctx["doc_boundaries"], host lists).

    cu_seqlens are token offsets into the batch-major flattened
    [(hi-lo)*S] stream of just those rows — what a layer hands to
    flash_attention_varlen for its dp slice.  Built on the host and
    memoized in the (microbatch) ctx, so all layers share one async
    host-to-device copy and nothing is ever read back from the device."""
    cache = ctx.setdefault("_cu_seqlens_cache", {})
    key = (lo, hi, str(device))
    hit = cache.get(key)
    if hit is None:
        S = ctx["seq_len"]
        cu, longest = [0], 1
        for r, bd in enumerate(ctx["doc_boundaries"][lo:hi]):
            assert bd[0] == 0 and bd[-1] == S, "bad document boundaries"
            cu.extend(r * S + e for e in bd[1:])
            longest = max(longest, max(b - a for a, b in zip(bd, bd[1:])))
        t = torch.tensor(cu, dtype=torch.int32)
        if torch.device(device).type == "cuda":
            t = t.pin_memory().to(device, non_blocking=True)
        hit = cache[key] = (t, longest)
    return hit


def build_batch_context(tokens: torch.Tensor, device,
                        eod_token: int = None,
                        eod_mask_loss: bool = False,
                        reset_attention_mask: bool = False,
                        reset_position_ids: bool = False) -> Dict:
    """tokens: [B, S+1] -> ctx with input_ids/labels [B, S].
    eod_mask_loss (reference dataloader get_batch loss_mask): zero the
    loss on end-of-document labels; loss_denom is the GLOBAL unmasked
    token count (identical on every rank -> grads normalize exactly).

    Packed documents (reference get_ltor_masks_and_position_ids), both
    derived from input_ids on the HOST before the device copy:
    reset_attention_mask adds "doc_boundaries" (per-row boundary lists,
    kept on the CPU; the layers turn them into cu_seqlens), and
    reset_position_ids adds "position_ids" [B, S] restarting at 0 after
    each EOD.  Without the flags the ctx has no extra keys."""
    packed = {}
    if reset_attention_mask or reset_position_ids:
        assert eod_token is not None, \
            "reset_attention_mask / reset_position_ids need data.eod_token_id"
        bounds = document_boundaries(tokens[:, :-1], eod_token)
        if reset_attention_mask:
            packed["doc_boundaries"] = bounds
        if reset_position_ids:
            packed["position_ids"] = positions_from_boundaries(
                bounds, tokens.shape[1] - 1).to(device)
    tokens = tokens.to(device)
    ctx = {
        "input_ids": tokens[:, :-1].contiguous(),
        "labels": tokens[:, 1:].contiguous(),
        "batch_size": tokens.shape[0],
        "seq_len": tokens.shape[1] - 1,
    }
    if eod_mask_loss:
        assert eod_token is not None, "eod_mask_loss needs data.eod_token_id"
        mask = (ctx["labels"] != eod_token).to(torch.float32)
        ctx["loss_mask"] = mask
        ctx["loss_denom"] = float(mask.sum())
    ctx.update(packed)
    return ctx


def build_enc_dec_batch_context(enc_ids: torch.Tensor,
                                dec_tokens: torch.Tensor, device) -> Dict:
    """t5: enc_ids [B, S_enc]; dec_tokens [B, S_dec+1]."""
    ctx = build_batch_context(dec_tokens, device)
    ctx["enc_input_ids"] = enc_ids.to(device).contiguous()
    ctx["enc_seq_len"] = enc_ids.shape[1]
    return ctx


def split_range(n: int, split: str, which: str) -> tuple:
    """[lo, hi) index range of the train/valid/test partition under the
    reference's weight string (data.split, e.g. "969,30,1")."""
    w = [float(x) for x in split.split(",")]
    while len(w) < 3:
        w.append(0.0)
    tot = sum(w) or 1.0
    n_train = int(n * w[0] / tot)
    n_valid = int(n * w[1] / tot)
    lo, hi = {"train": (0, n_train),
              "valid": (n_train, n_train + n_valid),
              "test": (n_train + n_valid, n)}[which]
    if hi <= lo:  # degenerate split: fall back to the whole set
        return 0, n
    return lo, hi


def get_train_iterator(cfg: GalvatronConfig, device,
                       global_batch: Optional[int] = None,
                       split: str = "train") -> Iterator[Dict]:
    """Yield batch contexts of the global batch size, cycling the dataset
    (reference: dataloader.py:462 get_train_valid_test_data_iterators).
    split selects the train/valid/test partition per data.split."""
    B = global_batch or cfg.train.global_train_batch_size
    if cfg.data.dataset == "megatron" and cfg.data.data_path:
        from .datasets import build_pretraining_dataset
        ds = build_pretraining_dataset(
            cfg.data.data_path, cfg.model.seq_length,
            num_samples=max(B * max(cfg.train.train_iters, 1),
                            cfg.data.synthetic_dataset_size),
            seed=cfg.train.seed)
    else:
        ds = SyntheticCausalLMDataset(
            cfg.model.vocab_size, cfg.model.seq_length,
            size=max(cfg.data.synthetic_dataset_size, B), seed=cfg.train.seed,
            eod_token=cfg.data.eod_token_id,
            mean_doc_length=cfg.data.synthetic_mean_doc_length)
    if cfg.model.model_type == "t5":
        s_enc = cfg.model.encoder_seq_length or cfg.model.seq_length
        if cfg.data.dataset == "megatron" and cfg.data.data_path:
            # span corruption over the token stream (t5 pretraining
            # objective; datasets/t5_dataset.py)
            from .datasets.t5_dataset import T5MaskedDataset
            t5ds = T5MaskedDataset(ds, s_enc, cfg.model.seq_length,
                                   cfg.model.vocab_size, seed=cfg.train.seed)
            idx = 0
            while True:
                items = [t5ds[(idx + i) % len(t5ds)] for i in range(B)]
                idx = (idx + B) % len(t5ds)
                enc = torch.stack([it["enc_input_ids"] for it in items])
                dec = torch.stack([it["dec_tokens"] for it in items])
                yield build_enc_dec_batch_context(enc, dec, device)
        g = torch.Generator().manual_seed(cfg.train.seed + 77)
        idx = 0
        while True:
            batch = torch.stack([ds[(idx + i) % len(ds)] for i in range(B)])
            idx = (idx + B) % len(ds)
            enc = torch.randint(0, cfg.model.vocab_size, (B, s_enc),
                                generator=g)
            yield build_enc_dec_batch_context(enc, batch, device)
    lo, hi = split_range(len(ds), cfg.data.split, split)
    n = hi - lo
    idx = 0
    while True:
        batch = torch.stack([ds[lo + (idx + i) % n] for i in range(B)])
        idx = (idx + B) % n
        yield build_batch_context(batch, device,
                                  eod_token=cfg.data.eod_token_id,
                                  eod_mask_loss=cfg.data.eod_mask_loss,
                                  reset_attention_mask=cfg.data.reset_attention_mask,
                                  reset_position_ids=cfg.data.reset_position_ids)
