"""`decode_attention_batched` off the native path (fp32 on the CPU): bit for
bit the per-row `decode_attention` calls it stands for."""
import pytest
import torch

from hetu_galvatron_amd.ops import decode_attention, decode_attention_batched


@pytest.mark.parametrize("window", [None, 5])
def test_batched_fallback_equals_per_row(window):
    g = torch.Generator().manual_seed(3)
    S, max_s, hq, hkv, d = 5, 40, 4, 2, 16
    lengths, slots = [1, 40, 17, 0, 50], [3, 0, 4, 1, 2]
    q = torch.randn(len(lengths), hq, d, generator=g)
    kc = torch.randn(S, max_s, hkv, d, generator=g)
    vc = torch.randn(S, max_s, hkv, d, generator=g)
    o = decode_attention_batched(
        q, kc, vc, torch.tensor(lengths, dtype=torch.int32),
        torch.tensor(slots, dtype=torch.int32), max_len=33, window=window)
    for i, (L, s) in enumerate(zip(lengths, slots)):
        L = min(L, 33)                       # a length above max_len: clamped
        want = decode_attention(q[i:i + 1], kc[s:s + 1], vc[s:s + 1], L,
                                window=window) if L else torch.zeros(1, hq, d)
        assert torch.equal(o[i:i + 1], want), i


def test_engine_batched_flag_changes_no_token():
    """fp32 on the CPU: the engine generates the same tokens either way."""
    from hetu_galvatron_amd.runtime.serving import ContinuousBatchingEngine
    from tests.core.test_serving import make_model
    model = make_model()
    torch.manual_seed(5)
    prompts = [torch.randint(0, 512, (n,)) for n in (5, 12, 3)]
    outs = []
    for flag in (False, True):
        eng = ContinuousBatchingEngine(model, max_slots=3, max_seq=32,
                                       batched_attention=flag)
        ps = [p.to(eng.gen._dev) for p in prompts]
        rids = [eng.add_request(ps[0], 5), eng.add_request(ps[1], 3)]
        eng.step()
        rids.append(eng.add_request(ps[2], 4))
        while eng.n_active:
            eng.step()
        outs.append([eng.outputs[r] for r in rids])
    assert outs[0] == outs[1]
