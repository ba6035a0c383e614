"""Continuous-batching serving engine over the KV-cache generator.

Requests join and leave between decode steps (vLLM-style scheduling
semantics, reference has no serving path): each slot owns a contiguous
row of the persistent KV cache with its own length, the per-step linears
(qkv, proj, mlp, head) are batched across every active slot.

Attention has two paths.  The default runs per slot on its cache row
([slot:slot+1] is a contiguous view — no copies): n_active cache writes
and `decode_attention` launches per layer.  `batched_attention=True` does
one indexed cache write and one `decode_attention_batched` call per layer
for all active slots: per-row lengths and cache rows are device tensors
built once per step, and each K/V row is read once per GQA group.  RoPE at
mixed positions is applied with a pure-torch broadcast (per-slot table
rows), not the shared-table kernel.

`kv_cache_dtype="fp8"` (batched attention only) keeps the caches in
float8_e4m3fn with static per-layer, per-head scales: new rows are quantised
and scattered by one `kv_cache_append` per layer, decode attends to the
bytes directly, and prefill attends to its fresh bf16 K/V through flash and
writes the slot's rows through the same op.

`page_size=N` (batched attention only, either cache dtype) replaces the
per-slot rows by one pool of `num_pages` pages of N positions per layer.  A
request reserves ceil((prompt + max_new_tokens) / N) pages at admission and
is refused when the pool cannot cover them; pages are assigned lazily, the
prompt's at prefill and one more whenever a slot's length crosses a page
boundary, and all return to the free list at release.  A persistent device
table [max_slots, max_seq / N] maps (slot, page index) to a pool page; cache
writes go to (page id, offset) and decode passes the table to
`decode_attention_batched`.

`speculative_tokens=k` (batched attention only; every cache dtype, paged or
not, with or without a sliding window) verifies up to k drafted tokens per
slot and step: the pending token and the drafts run as T = 1 + drafts rows
through the batched linears, their K/V go to the cache at their positions and
one `decode_attention_multi` call per layer attends each of them causally.
Greedy acceptance emits the model's own tokens while the drafts agree with
them, so the output is that of plain greedy decoding in fewer steps.  Drafts
come from prompt lookup (`ngram_draft`) or a `draft_fn`.

`prefill_chunk=N` (batched attention only; every cache kind) runs a prompt in
consecutive chunks of at most N tokens.  Each chunk writes its K/V to the
slot's cache first and then attends the cache through one
`decode_attention_multi` call per layer, so prefill reads what decode will
read (the quantised rows of an fp8 cache) and a long prompt's activations are
bounded by the chunk.  `add_request` still returns the first token at once.

`fused_prologue=True` (batched attention only; every cache kind, decode,
speculative steps and chunked prefill) replaces what stands between the qkv
linear and the attention call of a layer (the split, the table gathers, the
rotation of q and k and the cache write) by one `rope_kv_append` call on the
packed qkv output.  Positions, cache rows and page ids come from the device
tensors that attention reads, so the step builds no per-row write indices on
the host.  The tokens are those of the unfused engine.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch

from ..ops import (decode_attention, decode_attention_batched,
                   decode_attention_multi, flash_attention_fwd_only,
                   kv_cache_append, rope_kv_append)
from .inference import GalvatronGenerator, KVCache

__all__ = ["ContinuousBatchingEngine", "ngram_draft"]


def ngram_draft(history: List[int], k: int) -> List[int]:
    """Prompt-lookup drafts: the up to k tokens that followed the latest
    earlier occurrence of the history's last two tokens; [] without one."""
    if k <= 0 or len(history) < 3:
        return []
    a, b = history[-2], history[-1]
    for i in range(len(history) - 3, -1, -1):
        if history[i] == a and history[i + 1] == b:
            return history[i + 2:i + 2 + k]
    return []


def _rope_rows(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
               interleaved: bool = False):
    """x: [1, b, h, d]; cos/sin: [b, d/2] (one table row per slot)."""
    d2 = x.shape[-1] // 2
    c = cos[None, :, None, :].float()
    s = sin[None, :, None, :].float()
    if interleaved:
        x1, x2 = x[..., 0::2].float(), x[..., 1::2].float()
        y = torch.empty_like(x, dtype=torch.float32)
        y[..., 0::2] = x1 * c - x2 * s
        y[..., 1::2] = x2 * c + x1 * s
        return y.to(x.dtype)
    x1, x2 = x[..., :d2].float(), x[..., d2:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)


class ContinuousBatchingEngine:
    """Greedy decode over a slot pool (world=1 topology)."""

    def __init__(self, model, max_slots: int = 8, max_seq: int = 4096,
                 batched_attention: bool = False, kv_cache_dtype: str = None,
                 kv_scales: torch.Tensor = None, page_size: int = None,
                 num_pages: int = None, speculative_tokens: int = 0,
                 draft_fn: Callable[[List[int], int], List[int]] = None,
                 prefill_chunk: int = None, fused_prologue: bool = False):
        """kv_cache_dtype: None (the model's dtype) or "fp8"; kv_scales:
        fp32 [n_layers, 2, hkv] dequantisation scales of the fp8 cache
        (k, v per layer; None: ones).  page_size: None (one contiguous row
        per slot) or the positions per page of a paged cache, a power of two
        >= 32 that divides max_seq; num_pages: pages in the pool (None:
        max_slots * max_seq / page_size, the contiguous cache's memory).
        speculative_tokens: drafts verified per slot and step (0: plain
        decode; `step()` then returns one token per request, otherwise a
        list); draft_fn(history, k) -> up to k proposed tokens replaces the
        prompt-lookup drafter.  Slots that sample take no drafts.
        prefill_chunk: None (the whole prompt through flash on its fresh
        K/V) or the most tokens of a prompt run at once, a power of two
        >= 32 (batched attention only): every chunk attends the cache.
        fused_prologue: RoPE and the cache write of decode steps,
        speculative steps and prefill chunks through one `rope_kv_append`
        call per layer (batched attention only).  A layer with `q_layernorm`
        keeps the unfused composition, because the norm sits between the
        split and the rotation."""
        if fused_prologue and not batched_attention:
            raise ValueError("fused_prologue needs batched_attention=True")
        if prefill_chunk is not None:
            if not batched_attention:
                raise ValueError("prefill_chunk needs batched_attention=True")
            if prefill_chunk < 32 or prefill_chunk & (prefill_chunk - 1):
                raise ValueError(f"prefill_chunk must be a power of two "
                                 f">= 32, got {prefill_chunk}")
        self.prefill_chunk = prefill_chunk
        if speculative_tokens < 0:
            raise ValueError("speculative_tokens must be >= 0")
        if speculative_tokens and not batched_attention:
            raise ValueError("speculative_tokens needs batched_attention=True")
        self.speculative_tokens = speculative_tokens
        self.draft_fn = draft_fn or ngram_draft
        self.history: Dict[int, List[int]] = {}   # slot -> prompt + outputs
        self.drafted: Dict[int, int] = {}         # request id -> drafts run
        self.accepted: Dict[int, int] = {}        # request id -> drafts kept
        if kv_cache_dtype not in (None, "fp8"):
            raise ValueError(f"kv_cache_dtype must be None or 'fp8', got "
                             f"{kv_cache_dtype!r}")
        if kv_cache_dtype == "fp8" and not batched_attention:
            raise ValueError("kv_cache_dtype='fp8' needs "
                             "batched_attention=True")
        if page_size is None and num_pages is not None:
            raise ValueError("num_pages needs page_size")
        if page_size is not None:
            if not batched_attention:
                raise ValueError("page_size needs batched_attention=True")
            if page_size < 32 or page_size & (page_size - 1) \
                    or max_seq % page_size:
                raise ValueError(f"page_size must be a power of two >= 32 "
                                 f"that divides max_seq, got {page_size}")
            if num_pages is None:
                num_pages = max_slots * max_seq // page_size
        self.page_size = page_size
        self.batched_attention = batched_attention
        self.gen = GalvatronGenerator(model, max_batch=max_slots,
                                      max_seq=max_seq)
        m = model.cfg.model
        self.margs = m
        self.max_slots = max_slots
        self.max_seq = max_seq
        # per layer: does the fused prologue run it?
        self._fused = [fused_prologue and getattr(
            layer.attention, "q_layernorm", None) is None
            for layer in self.gen.layers]
        dtype = torch.float8_e4m3fn if kv_cache_dtype == "fp8" \
            else next(self.gen.embedding.parameters()).dtype
        if page_size is None:
            self.cache = KVCache(len(self.gen.layers), max_slots, max_seq,
                                 m.kv_heads, m.head_dim, self.gen._dev,
                                 dtype=dtype)
        else:                                   # pools [num_pages, page, ..]
            self.cache = KVCache(len(self.gen.layers), num_pages, page_size,
                                 m.kv_heads, m.head_dim, self.gen._dev,
                                 dtype=dtype)
            self.free_pages: List[int] = list(range(num_pages))[::-1]
            self.unreserved = num_pages
            self.pages: Dict[int, List[int]] = {}   # slot -> owned pages
            self.reserved: Dict[int, int] = {}      # slot -> pages reserved
            self.page_table = torch.full(
                (max_slots, max_seq // page_size), -1, dtype=torch.int32,
                device=self.gen._dev)
        if kv_scales is not None:
            if not self.cache.fp8 or tuple(kv_scales.shape) != (
                    len(self.gen.layers), 2, m.kv_heads):
                raise ValueError("kv_scales must be [n_layers, 2, hkv] and "
                                 "needs kv_cache_dtype='fp8'")
            sc = kv_scales.to(self.gen._dev, torch.float32)
            self.cache.k_scale = [sc[i, 0].contiguous() for i in range(len(sc))]
            self.cache.v_scale = [sc[i, 1].contiguous() for i in range(len(sc))]
        self.lengths = [0] * max_slots          # attended tokens per slot
        self.budgets: Dict[int, int] = {}       # slot -> tokens remaining
        self.last_tok: Dict[int, int] = {}      # slot -> pending input token
        self.free: List[int] = list(range(max_slots))
        self.slot_of: Dict[int, int] = {}       # request id -> slot
        self.rid_of: Dict[int, int] = {}        # slot -> request id
        self.outputs: Dict[int, List[int]] = {} # request id -> tokens
        self.samplers: Dict[int, tuple] = {}    # slot -> (temp, generator)
        self.eos: Dict[int, int] = {}           # slot -> eos id (or None)
        self._next_rid = 0
        for blk in self.gen.blocks:
            if blk.flat is not None:
                blk.flat.gather_params()
            blk.inner.eval()

    # -- request lifecycle --------------------------------------------------
    def add_request(self, prompt_ids: torch.Tensor, max_new_tokens: int,
                    temperature: float = 0.0, seed: int = 0,
                    eos_id: int = None) -> int:
        """prompt_ids: [s]; prefills a slot, producing the request's
        FIRST generated token immediately.  Returns a request id whose
        tokens accumulate in `self.outputs[rid]` (kept after release).
        temperature > 0 samples with a per-request seeded generator."""
        assert self.free, "no free slots"
        assert prompt_ids.dim() == 1 and max_new_tokens >= 1
        sp = prompt_ids.shape[0]
        assert sp + max_new_tokens <= self.max_seq
        if self.page_size is not None:
            need = -(-(sp + max_new_tokens) // self.page_size)
            if need > self.unreserved:
                raise RuntimeError(
                    f"KV page pool exhausted: the request needs {need} "
                    f"pages, {self.unreserved} are unreserved "
                    f"({need - self.unreserved} short)")
        slot = self.free.pop()
        rid = self._next_rid
        self._next_rid += 1
        if self.page_size is not None:
            self.unreserved -= need
            self.reserved[slot] = need
            self.pages[slot] = []
            self._grow(slot, sp)
            view = _PagedSlotCache(self.cache, self.pages[slot],
                                   self.page_size)
        else:
            # single-slot prefill on the slot's contiguous cache row
            view = _SlotCache(self.cache, slot)
        if self.prefill_chunk is None:
            logits = self._prefill(prompt_ids.unsqueeze(0), view)
        else:
            logits = self._prefill_chunked(prompt_ids.unsqueeze(0), view, slot)
        if temperature > 0:
            g = torch.Generator(device="cpu").manual_seed(seed)
            self.samplers[slot] = (temperature, g)
            first = self._sample(logits[0], slot)
        else:
            self.samplers.pop(slot, None)
            first = int(logits.argmax(-1))
        self.outputs[rid] = [first]
        if self.speculative_tokens:
            self.history[slot] = prompt_ids.tolist() + [first]
            self.drafted[rid] = self.accepted[rid] = 0
        self.slot_of[rid] = slot
        self.rid_of[slot] = rid
        self.lengths[slot] = sp
        self.last_tok[slot] = first
        self.eos[slot] = eos_id
        self.budgets[slot] = max_new_tokens - 1
        if self.budgets[slot] == 0 or (eos_id is not None
                                       and first == eos_id):
            self.release(rid)
        return rid

    def _grow(self, slot: int, length: int) -> None:
        """Give `slot` the pages that `length` positions need (within its
        reservation) and enter them in the device table."""
        own = self.pages[slot]
        first = len(own)
        while len(own) * self.page_size < length:
            own.append(self.free_pages.pop())
        if len(own) > first:
            self.page_table[slot, first:len(own)] = torch.tensor(
                own[first:], dtype=torch.int32, device=self.page_table.device)

    def _prologue(self, li: int, layer, x: torch.Tensor, lengths_t, q_lens_t,
                  slot32, paged) -> torch.Tensor:
        """Layer li's fused prologue on the normed rows x (n*T of them, row
        major in (slot row, token)): qkv linear, then one `rope_kv_append`,
        which leaves K/V in the cache.  -> q [n, T, hq, d]"""
        attn, cache = layer.attention, self.cache
        cos = sin = None
        if layer.rotary is not None:
            cos, sin = layer.rotary.full_tables(self.max_seq, self.gen._dev)
        return rope_kv_append(
            attn.linear_qkv(x), attn.num_groups_local, attn.q_per_group, cos,
            sin, lengths_t, q_lens_t, slot32, cache.k[li], cache.v[li],
            cache.k_scale[li], cache.v_scale[li],
            interleaved=getattr(attn, "rope_interleaved", False), **paged)

    def _prefill(self, ids: torch.Tensor, view: "_SlotCache"):
        gen = self.gen
        h = gen.embedding.word_embeddings(ids)
        for li, layer in enumerate(gen.layers):
            attn = layer.attention
            residual = h
            x = layer.input_norm(h)
            q, k, v = gen._split_qkv(attn, attn.linear_qkv(x))
            if getattr(attn, "q_layernorm", None) is not None:
                q = attn.q_layernorm(q)
                k = attn.k_layernorm(k)
            if layer.rotary is not None:
                cos, sin = layer.rotary.full_tables(q.shape[0], h.device)
                from .transformer.rope import apply_rope_qk
                q, k = apply_rope_qk(q.contiguous(), k.contiguous(),
                                     cos, sin,
                                     interleaved=getattr(
                                         attn, "rope_interleaved", False))
            view.write(li, k.permute(1, 0, 2, 3), v.permute(1, 0, 2, 3), 0)
            qb = q.permute(1, 0, 2, 3).contiguous()
            kb = k.permute(1, 0, 2, 3).contiguous()
            vb = v.permute(1, 0, 2, 3).contiguous()
            ob, _ = flash_attention_fwd_only(
                qb, kb, vb, causal=True, softmax_scale=gen.scale,
                window=getattr(gen, "window", None))
            o = ob.permute(1, 0, 2, 3).reshape(q.shape[0], 1, -1)
            h = residual + attn.linear_proj(o)
            residual = h
            h = residual + layer.mlp(layer.post_attn_norm(h))
        h = gen.final_norm.norm(h[-1:])
        return gen.lm_head.lm_head(h)[0].float()

    @torch.no_grad()
    def _prefill_chunked(self, ids: torch.Tensor, view: "_SlotCache",
                         slot: int):
        """The prompt in consecutive chunks of at most `prefill_chunk`
        tokens.  Per chunk and layer: RoPE at the chunk's positions, K/V into
        the slot's cache rows or pages (quantised for fp8), then one
        `decode_attention_multi` call of the chunk's tokens against the
        cache, the first chunk included: prefill attends what decode will
        attend.  Only the last chunk computes logits."""
        gen, dev, cache = self.gen, self.gen._dev, self.cache
        sp = ids.shape[1]
        i32 = dict(dtype=torch.int32, device=dev)
        slot32 = torch.tensor([slot], **i32)
        paged = {} if self.page_size is None \
            else {"page_table": self.page_table}
        for pos in range(0, sp, self.prefill_chunk):
            c = min(self.prefill_chunk, sp - pos)
            lengths_t = torch.tensor([pos + c], **i32)
            q_lens_t = torch.tensor([c], **i32)
            h = gen.embedding.word_embeddings(ids[:, pos:pos + c])
            for li, layer in enumerate(gen.layers):
                attn = layer.attention
                residual = h
                x = layer.input_norm(h)
                if self._fused[li]:
                    q = self._prologue(li, layer, x, lengths_t, q_lens_t,
                                       slot32, paged)
                else:
                    q, k, v = gen._split_qkv(attn, attn.linear_qkv(x))
                    if getattr(attn, "q_layernorm", None) is not None:
                        q = attn.q_layernorm(q)
                        k = attn.k_layernorm(k)
                    if layer.rotary is not None:
                        cos, sin = layer.rotary.full_tables(self.max_seq, dev)
                        from .transformer.rope import apply_rope_qk
                        q, k = apply_rope_qk(
                            q.contiguous(), k.contiguous(), cos[pos:pos + c],
                            sin[pos:pos + c], interleaved=getattr(
                                attn, "rope_interleaved", False))
                    view.write(li, k.permute(1, 0, 2, 3),
                               v.permute(1, 0, 2, 3), pos)
                    q = q.permute(1, 0, 2, 3).contiguous()
                o = decode_attention_multi(
                    q, cache.k[li], cache.v[li], lengths_t, q_lens_t, slot32,
                    window=getattr(gen, "window", None), max_len=pos + c,
                    softmax_scale=gen.scale, k_scale=cache.k_scale[li],
                    v_scale=cache.v_scale[li], **paged)
                h = residual + attn.linear_proj(o.reshape(c, 1, -1))
                residual = h
                h = residual + layer.mlp(layer.post_attn_norm(h))
        h = gen.final_norm.norm(h[-1:])
        return gen.lm_head.lm_head(h)[0].float()

    @torch.no_grad()
    def step(self) -> Dict[int, int]:
        """One decode step for every active slot.  Returns {rid: token};
        requests whose budget hits zero are released after their token
        (their outputs stay readable in `self.outputs`)."""
        if self.speculative_tokens:
            return self._step_speculative()
        active = sorted(self.budgets)
        if not active:
            return {}
        gen = self.gen
        dev = gen._dev
        ids = torch.tensor([[self.last_tok[s] for s in active]],
                           device=dev)                      # [1, n]
        pos = torch.tensor([self.lengths[s] for s in active], device=dev)
        if self.batched_attention:
            slot_t = torch.tensor(active, device=dev)
            slot32 = slot_t.int()
            # where the new rows go: (cache row, position), or paged
            # (page id, offset in the page)
            if self.page_size is not None:
                for s in active:         # a length that crosses a boundary
                    self._grow(s, self.lengths[s] + 1)
            if not all(self._fused):     # the fused prologue needs none
                wr_t, wr_pos = slot_t, pos
                if self.page_size is not None:
                    wr_t = torch.tensor(
                        [self.pages[s][self.lengths[s] // self.page_size]
                         for s in active], device=dev)
                    wr_pos = pos % self.page_size
                wr32, wr_pos32 = wr_t.int(), wr_pos.int()
            paged = {} if self.page_size is None \
                else {"page_table": self.page_table}
            lengths_t = (pos + 1).int()      # the new token is attended too
            if any(self._fused):
                q_lens_t = torch.ones_like(lengths_t)
            max_len = max(self.lengths[s] for s in active) + 1
        h = gen.embedding.word_embeddings(ids.transpose(0, 1))  # [1, n, hd]
        for li, layer in enumerate(gen.layers):
            attn = layer.attention
            residual = h
            x = layer.input_norm(h)
            if self._fused[li]:          # K/V are in the cache after this
                q = self._prologue(li, layer, x, lengths_t, q_lens_t, slot32,
                                   paged).transpose(0, 1)   # [1, n, hq, d]
            else:
                q, k, v = gen._split_qkv(attn, attn.linear_qkv(x))
                if getattr(attn, "q_layernorm", None) is not None:
                    q = attn.q_layernorm(q)
                    k = attn.k_layernorm(k)
                if layer.rotary is not None:
                    cos_t, sin_t = layer.rotary.full_tables(self.max_seq, dev)
                    il = getattr(attn, "rope_interleaved", False)
                    q = _rope_rows(q, cos_t[pos], sin_t[pos], il)
                    k = _rope_rows(k, cos_t[pos], sin_t[pos], il)
            if self.batched_attention:
                cache = self.cache
                if self._fused[li]:
                    pass
                elif cache.fp8:
                    kv_cache_append(k[0], v[0], cache.k[li], cache.v[li],
                                    wr32, wr_pos32, cache.k_scale[li],
                                    cache.v_scale[li])
                else:
                    cache.k[li][wr_t, wr_pos] = k[0]
                    cache.v[li][wr_t, wr_pos] = v[0]
                outs = [decode_attention_batched(
                    q[0], cache.k[li], cache.v[li], lengths_t,
                    slot32, max_len=max_len, softmax_scale=gen.scale,
                    window=getattr(gen, "window", None),
                    k_scale=cache.k_scale[li], v_scale=cache.v_scale[li],
                    **paged)]
            else:
                outs = self._attend_per_slot(li, active, q, k, v)
            o = torch.cat(outs, 0).unsqueeze(0).reshape(1, len(active), -1)
            h = residual + attn.linear_proj(o)
            residual = h
            h = residual + layer.mlp(layer.post_attn_norm(h))
        h = gen.final_norm.norm(h)
        logits = gen.lm_head.lm_head(h)[0].float()          # [n, V]
        greedy = logits.argmax(-1)
        out: Dict[int, int] = {}
        for i, s in enumerate(active):
            t = self._sample(logits[i], s) if s in self.samplers \
                else int(greedy[i])
            rid = self.rid_of[s]
            out[rid] = t
            self.outputs[rid].append(t)
            self.lengths[s] += 1
            self.last_tok[s] = t
            self.budgets[s] -= 1
            if self.budgets[s] == 0 or (self.eos.get(s) is not None
                                        and t == self.eos[s]):
                self.release(rid)
        return out

    def _step_speculative(self) -> Dict[int, List[int]]:
        """One verification step: every active slot runs its pending token
        and its drafts as rows (i, t), t < q_len_i <= T, of one batch."""
        active = sorted(self.budgets)
        if not active:
            return {}
        gen, dev, n = self.gen, self.gen._dev, len(active)
        drafts = []
        for s in active:
            # emitting needs budget: a draft beyond budget - 1 cannot be used,
            # and length + 1 + drafts stays inside the request's reservation
            k = min(self.speculative_tokens, self.budgets[s] - 1)
            d = [] if s in self.samplers or k <= 0 \
                else [int(x) for x in self.draft_fn(self.history[s], k)][:k]
            drafts.append(d)
        T = 1 + max(len(d) for d in drafts)
        q_lens = [1 + len(d) for d in drafts]
        ids = torch.tensor([[self.last_tok[s]] + d + [0] * (T - 1 - len(d))
                            for s, d in zip(active, drafts)], device=dev)
        base = torch.tensor([self.lengths[s] for s in active], device=dev)
        if self.page_size is not None:
            for s, ql in zip(active, q_lens):
                self._grow(s, self.lengths[s] + ql)
        if not all(self._fused):         # the fused prologue needs none
            pos = (base[:, None] + torch.arange(T, device=dev)) \
                .clamp_(max=self.max_seq - 1).reshape(-1)          # [n*T]
            # rows (i, t) that are real, and where their K/V go
            real = [(i, t) for i in range(n) for t in range(q_lens[i])]
            real_t = torch.tensor([i * T + t for i, t in real], device=dev)
            wr_pos = pos[real_t]
            if self.page_size is None:
                wr_t = torch.tensor([active[i] for i, _ in real], device=dev)
            else:
                wr_t = torch.tensor(
                    [self.pages[active[i]][(self.lengths[active[i]] + t)
                                           // self.page_size]
                     for i, t in real], device=dev)
                wr_pos = wr_pos % self.page_size
            wr32, wr_pos32 = wr_t.int(), wr_pos.int()
        paged = {} if self.page_size is None \
            else {"page_table": self.page_table}
        q_lens_t = torch.tensor(q_lens, dtype=torch.int32, device=dev)
        lengths_t = base.int() + q_lens_t      # the new tokens are attended
        slot32 = torch.tensor(active, dtype=torch.int32, device=dev)
        max_len = max(self.lengths[s] + ql for s, ql in zip(active, q_lens))
        h = gen.embedding.word_embeddings(ids.reshape(1, -1).transpose(0, 1))
        cache = self.cache
        for li, layer in enumerate(gen.layers):
            attn = layer.attention
            residual = h
            x = layer.input_norm(h)
            if self._fused[li]:
                q = self._prologue(li, layer, x, lengths_t, q_lens_t, slot32,
                                   paged)
            else:
                q, k, v = gen._split_qkv(attn, attn.linear_qkv(x))
                if getattr(attn, "q_layernorm", None) is not None:
                    q = attn.q_layernorm(q)
                    k = attn.k_layernorm(k)
                if layer.rotary is not None:
                    cos_t, sin_t = layer.rotary.full_tables(self.max_seq, dev)
                    il = getattr(attn, "rope_interleaved", False)
                    q = _rope_rows(q, cos_t[pos], sin_t[pos], il)
                    k = _rope_rows(k, cos_t[pos], sin_t[pos], il)
                if cache.fp8:
                    kv_cache_append(k[0][real_t], v[0][real_t], cache.k[li],
                                    cache.v[li], wr32, wr_pos32,
                                    cache.k_scale[li], cache.v_scale[li])
                else:
                    cache.k[li][wr_t, wr_pos] = k[0][real_t]
                    cache.v[li][wr_t, wr_pos] = v[0][real_t]
                q = q[0].reshape(n, T, *q.shape[2:])
            o = decode_attention_multi(
                q, cache.k[li], cache.v[li], lengths_t, q_lens_t, slot32,
                window=getattr(gen, "window", None), max_len=max_len,
                softmax_scale=gen.scale, k_scale=cache.k_scale[li],
                v_scale=cache.v_scale[li], **paged)
            h = residual + attn.linear_proj(o.reshape(1, n * T, -1))
            residual = h
            h = residual + layer.mlp(layer.post_attn_norm(h))
        h = gen.final_norm.norm(h)
        logits = gen.lm_head.lm_head(h)[0].float()          # [n*T, V]
        greedy = logits.argmax(-1).reshape(n, T).tolist()
        out: Dict[int, List[int]] = {}
        for i, (s, d) in enumerate(zip(active, drafts)):
            rid, eos = self.rid_of[s], self.eos.get(s)
            g = greedy[i]
            if s in self.samplers:
                g = [self._sample(logits[i * T], s)]
            emitted = []
            for j in range(len(d) + 1):      # g[j] follows the accepted j
                emitted.append(g[j])
                if len(emitted) == self.budgets[s] or g[j] == eos \
                        or j == len(d) or d[j] != g[j]:
                    break
            out[rid] = emitted
            self.outputs[rid].extend(emitted)
            self.history[s].extend(emitted)
            self.drafted[rid] += len(d)
            self.accepted[rid] += len(emitted) - 1
            # rejected positions stay above the length and are overwritten
            self.lengths[s] += len(emitted)
            self.last_tok[s] = emitted[-1]
            self.budgets[s] -= len(emitted)
            if self.budgets[s] == 0 or emitted[-1] == eos:
                self.release(rid)
        return out

    def _attend_per_slot(self, li, active, q, k, v):
        outs = []
        for i, s in enumerate(active):
            L = self.lengths[s]
            self.cache.k[li][s, L] = k[0, i]
            self.cache.v[li][s, L] = v[0, i]
            o = decode_attention(q[:, i], self.cache.k[li][s:s + 1],
                                 self.cache.v[li][s:s + 1], L + 1,
                                 softmax_scale=self.gen.scale,
                                 window=getattr(self.gen, "window", None))
            outs.append(o)
        return outs

    def _sample(self, logits_row: torch.Tensor, slot: int) -> int:
        temp, g = self.samplers[slot]
        probs = torch.softmax(logits_row.float().cpu() / temp, dim=-1)
        return int(torch.multinomial(probs, 1, generator=g))

    def release(self, rid: int) -> None:
        slot = self.slot_of.pop(rid, None)
        if slot is None:
            return  # idempotent: already released
        self.samplers.pop(slot, None)
        self.eos.pop(slot, None)
        self.rid_of.pop(slot, None)
        self.budgets.pop(slot, None)
        self.last_tok.pop(slot, None)
        self.history.pop(slot, None)
        self.lengths[slot] = 0
        if self.page_size is not None:
            self.free_pages.extend(self.pages.pop(slot))
            self.unreserved += self.reserved.pop(slot)
            self.page_table[slot].fill_(-1)
        self.free.append(slot)

    def collect(self, rid: int) -> List[int]:
        """Return-and-delete a request's output tokens: the long-running
        server path, so `outputs` does not grow without bound."""
        return self.outputs.pop(rid, [])

    @property
    def n_active(self) -> int:
        return len(self.budgets)


class _SlotCache:
    """KVCache adapter exposing one slot's contiguous row."""

    def __init__(self, cache: KVCache, slot: int):
        self.cache = cache
        self.slot = slot

    def write(self, layer: int, k, v, pos: int) -> None:
        s = k.shape[1]
        c = self.cache
        if c.fp8:
            i32 = dict(dtype=torch.int32, device=k.device)
            kv_cache_append(k[0], v[0], c.k[layer], c.v[layer],
                            torch.full((s,), self.slot, **i32),
                            torch.arange(pos, pos + s, **i32),
                            c.k_scale[layer], c.v_scale[layer])
            return
        c.k[layer][self.slot, pos:pos + s] = k[0]
        c.v[layer][self.slot, pos:pos + s] = v[0]


class _PagedSlotCache:
    """KVCache adapter writing one slot's positions through its pages."""

    def __init__(self, cache: KVCache, pages: List[int], page_size: int):
        self.cache = cache
        self.pages = pages
        self.page_size = page_size

    def write(self, layer: int, k, v, pos: int) -> None:
        c = self.cache
        p = torch.arange(pos, pos + k.shape[1], device=k.device)
        ids = torch.tensor(self.pages, device=k.device)[p // self.page_size]
        off = p % self.page_size
        if c.fp8:
            kv_cache_append(k[0], v[0], c.k[layer], c.v[layer], ids.int(),
                            off.int(), c.k_scale[layer], c.v_scale[layer])
            return
        c.k[layer][ids, off] = k[0]
        c.v[layer][ids, off] = v[0]
