"""ContinuousBatchingEngine(page_size=32) on the CPU (fp32, torch paths):
the greedy tokens of the contiguous batched engine, request by request, from
a pool smaller than max_slots * max_seq; admission by reservation."""
import pytest
import torch

from hetu_galvatron_amd.runtime.serving import ContinuousBatchingEngine

MAX_SLOTS, MAX_SEQ, PAGE, NUM_PAGES = 4, 128, 32, 7      # 16 pages contiguous


def run_schedule(model, vocab, **kw):
    """Requests join and leave between steps: 30 + 6 crosses a page boundary
    while decoding, the 60-token request is refused until 40 + 3 has left and
    then takes over its pages.  -> the tokens of every request, in order."""
    eng = ContinuousBatchingEngine(model, max_slots=MAX_SLOTS,
                                   max_seq=MAX_SEQ, batched_attention=True,
                                   **kw)
    g = torch.Generator().manual_seed(5)
    p30, p40, p5, p60 = (torch.randint(0, vocab, (n,), generator=g)
                         .to(eng.gen._dev) for n in (30, 40, 5, 60))
    rids = [eng.add_request(p30, 6), eng.add_request(p40, 3)]
    eng.step()
    rids.append(eng.add_request(p5, 4))
    if eng.page_size is not None:            # 5 of 7 pages reserved, 3 needed
        with pytest.raises(RuntimeError, match="1 short"):
            eng.add_request(p60, 10)
        assert len(eng.free) == 1
    eng.step()                               # 40 + 3 leaves
    rids.append(eng.add_request(p60, 10))
    while eng.n_active:
        eng.step()
    if eng.page_size is not None:
        assert sorted(eng.free_pages) == list(range(NUM_PAGES))
        assert eng.unreserved == NUM_PAGES and not eng.pages
    return [eng.outputs[r] for r in rids]


def test_paged_engine_generates_the_contiguous_tokens():
    from tests.core.test_serving import make_model
    model = make_model()
    want = run_schedule(model, 512)
    got = run_schedule(model, 512, page_size=PAGE, num_pages=NUM_PAGES)
    assert got == want


def test_page_size_is_checked():
    from tests.core.test_serving import make_model
    model = make_model()
    for kw, msg in (({"batched_attention": False}, "batched_attention"),
                    ({"page_size": 48}, "power of two")):
        with pytest.raises(ValueError, match=msg):
            ContinuousBatchingEngine(model, **{
                "max_slots": 2, "max_seq": 96, "batched_attention": True,
                "page_size": 32, **kw})
