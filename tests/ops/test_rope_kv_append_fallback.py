"""`ops.rope_kv_append`, torch path, against an fp64 rotation of the same
inputs, on the one shape that holds the edges: n = 5 rows of T = 5 tokens,
G = 2, qpg = 3, a capacity of 64 positions.  Row 0 (slot 2, positions 29..33)
crosses a page boundary and its second page is invalid in the paged case, row
1 is one token at position 0, row 2 has no tokens, row 3 (slot 3: outside
S = 3) ends on the last position, row 4 has slot -1."""
import pytest
import torch

from hetu_galvatron_amd.ops import kv_cache_append, rope_kv_append

CAP, PAGE = 64, 32
EDGE = dict(G=2, qpg=3, T=5, q_lens=(5, 1, 0, 3, 2),
            lengths=(34, 1, 7, 64, 40), slots=(2, 0, 1, 3, -1))
FLAGSHIP = dict(G=8, qpg=4, T=1, q_lens=(1, 1, 1), lengths=(1, 33, 64),
                slots=(1, 3, 0))
KINDS = [(fp8, paged) for fp8 in (False, True) for paged in (False, True)]


def make_case(D, fp8, paged, S=4, shape=EDGE, device="cpu"):
    """-> (positional args up to slots with cos/sin, keyword args with the
    sentinel-filled caches, targets): targets[(i, t)] is the (cache row,
    position) that live token (i, t) writes, or None for an invalid page."""
    g = torch.Generator().manual_seed(D + S)
    G, qpg, T = shape["G"], shape["qpg"], shape["T"]
    n = len(shape["slots"])
    qkv = torch.randn(n * T, G * (qpg + 2) * D, generator=g).bfloat16()
    ang = torch.arange(CAP)[:, None] * 10000.0 ** (
        -torch.arange(0, D, 2) / D)[None]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=device)
    dtype = torch.float8_e4m3fn if fp8 else torch.bfloat16
    rows = (2 * S, PAGE) if paged else (S, CAP)
    kw = {"k_cache": torch.full((*rows, G, D), 7.0).to(dtype).to(device),
          "v_cache": torch.full((*rows, G, D), -3.0).to(dtype).to(device)}
    if fp8:
        kw["k_scale"] = torch.linspace(0.75, 1.5, G).to(device)
    table = None
    if paged:                                 # rows in a permuted order
        table = torch.randperm(2 * S, generator=g).reshape(S, 2).tolist()
        table[2][1] = -1
        kw["page_table"] = i32(table)
    targets = {}
    for i, (L, ql, s) in enumerate(zip(shape["lengths"], shape["q_lens"],
                                       shape["slots"])):
        for t in range(ql if 0 <= s < S else 0):
            p = L - ql + t
            tgt = (table[s][p // PAGE], p % PAGE) if paged else (s, p)
            targets[(i, t)] = tgt if tgt[0] >= 0 else None
    args = [qkv.to(device), G, qpg, ang.cos().to(device),
            ang.sin().to(device), i32(shape["lengths"]),
            i32(shape["q_lens"]), i32(shape["slots"])]
    return args, kw, targets


def rot64(x, c, s, il):
    """fp64 rotation of x [..., D] and the bound on an element's error: one
    bf16 rounding with a factor 2 of margin plus the three fp32 roundings."""
    x, c, s = x.double(), c.double(), s.double()
    x1, x2 = (x[..., 0::2], x[..., 1::2]) if il else x.chunk(2, -1)
    y = [x1 * c - x2 * s, x2 * c + x1 * s]
    m = [(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()]
    join = (lambda a: torch.stack(a, -1).flatten(-2)) if il \
        else (lambda a: torch.cat(a, -1))
    y, m = join(y), join(m)
    return y, 2.0 ** -8 * y.abs() + 2.0 ** -22 * m


@pytest.mark.parametrize("S", [4, 3])
@pytest.mark.parametrize("il", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("fp8,paged", KINDS)
@pytest.mark.parametrize("D", [64, 128])
def test_fallback_against_fp64(D, fp8, paged, il, S):
    args, kw, targets = make_case(D, fp8, paged, S)
    qkv, G, qpg, cos, sin, lengths, q_lens, _ = args
    T = EDGE["T"]
    x = qkv.view(-1, T, G, qpg + 2, D)
    q = rope_kv_append(*args, **kw, interleaved=il)
    assert q.shape == (x.shape[0], T, G * qpg, D) and q.dtype == qkv.dtype
    # the rotated k as bf16 rows: the same call on a bf16 cache
    _, kwb, _ = make_case(D, False, paged, S)
    rope_kv_append(*args, **kwb, interleaved=il)
    want = make_case(D, fp8, paged, S)[1]
    want_k, want_v = want["k_cache"], want["v_cache"]
    written = torch.zeros(kwb["k_cache"].shape[:2], dtype=torch.bool)
    assert (None in targets.values()) == paged
    for i in range(x.shape[0]):
        for t in range(T):
            if (i, t) not in targets:
                assert not q[i, t].any()
                continue
            p = int(lengths[i] - q_lens[i]) + t
            y, bound = rot64(x[i, t, :, :qpg + 1], cos[p], sin[p], il)
            got = q[i, t].view(G, qpg, D).double()
            assert ((got - y[:, :qpg]).abs() <= bound[:, :qpg]).all()
            if targets[(i, t)] is None:
                continue
            tgt = targets[(i, t)]
            written[tgt] = True
            kb = kwb["k_cache"][tgt]
            assert ((kb.double() - y[:, qpg]).abs() <= bound[:, qpg]).all()
            assert torch.equal(kwb["v_cache"][tgt], x[i, t, :, qpg + 1])
            one = lambda v: torch.tensor([v], dtype=torch.int32)
            kv_cache_append(kb[None], x[i, t, :, qpg + 1][None], want_k,
                            want_v, one(tgt[0]), one(tgt[1]),
                            kw.get("k_scale"))
    assert written.sum() == sum(v is not None for v in targets.values())
    # nothing but the live tokens' rows has changed, and those hold what
    # `kv_cache_append` stores for the rotated k and for v
    for got, want in ((kw["k_cache"], want_k), (kw["v_cache"], want_v)):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_fallback_without_rotation():
    args, kw, targets = make_case(64, False, False)
    args[3] = args[4] = None
    q = rope_kv_append(*args, **kw)
    x = args[0].view(5, 5, 2, 5, 64)
    for (i, t), tgt in targets.items():
        assert torch.equal(q[i, t].view(2, 3, 64), x[i, t, :, :3])
        assert torch.equal(kw["k_cache"][tgt], x[i, t, :, 3])
