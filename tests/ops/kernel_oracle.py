"""fp64 oracles, comparison rules and shared inputs for the kernel edge tests.

A plain helper module (not a conftest): `test_kernel_oracle.py` checks on the
CPU that the rules below accept the fp32 `reference_ops` and reject planted
mutants; `test_gpu_kernel_edges.py` applies the same rules, on the same
inputs, to the HIP kernels.

Oracles
-------
Every oracle is written from the operation's definition and evaluates it in
fp64 on the kernel's actual inputs (the bf16 / fp32 values cast up).  Where a
backward consumes a statistic that the forward saved (invrms, mean, invstd,
gmax, sumexp) the oracle takes the value it is given, so a test can hand it
the kernel's own statistic and isolate the pass under test.

Comparison rules
----------------
1. Bitwise row independence (`assert_rows_bitwise`).  For kernels whose rows
   do not interact, rows of a large call must `torch.equal` the same rows
   run alone in a small call.  No tolerance.

2. fp32 accumulations (`assert_accum`; dw, db, sumexp, dprobs, scatter-adds,
   grouped dW, the fp32 optimizer state).  With E_ref = max|ref32 - oracle|,
   the error of the fp32 `reference_ops` result on the same inputs,

       max|got - oracle|  <=  ACCUM_MULT * max(E_ref, 2^-24 * max|oracle|)

   ACCUM_MULT = 32.  The second term is half an fp32 ulp of the largest
   result, the rounding of the stored value itself; it only matters where
   the reference happens to be exact (short sums, empty experts).

3. Element outputs (`assert_elem`; bf16 or fp32).  The oracle is rounded to
   the output dtype and every element must satisfy

       |got - round_out(oracle)|  <=  ulp_out(|oracle|) + 2^-20 * scale

   ulp_out(a) is one unit in the last place of the output dtype at
   magnitude a (2^(floor(log2 a) - 7) for bf16, - 23 for fp32, 0 at a = 0).
   `scale` is the magnitude of the largest term the fp32 evaluation goes
   through, so that 2^-20 * scale covers the few fp32 roundings of a
   cancelling expression; it defaults to |oracle| and is given per op:

     norm y          |oracle|                    (rmsnorm)
                     (|x|+|mean|)*invstd*|w|+|b| (layernorm: x - mean cancels)
     norm dx         invrms * max_i|dy_i w_i| * (1 + |xhat|)  (+ |dsum|)
     ln dx           invstd * max_i|dy_i w_i| * (2 + |xhat|)
     mean            max_i|x_i|
     swiglu y        |oracle| * (1 + |gate|)     (__expf: the argument's
                                                  rounding scales with it)
     swiglu dx       [|dy u| sig, |dy g| sig] * (1 + |gate|)
                     (dgate's factor 1 + g(1 - sig) cancels near g = -1.28)
     rope            |x1| + |x2|
     ce dlogits      |gout| * (p * (1 + |logit - max|) + onehot)
     unpermute, grouped GEMM fwd / dA
                     the same product with every operand's absolute value

   adamw `out` is not under this rule: it is the cast of the kernel's own
   new master and must `torch.equal` that master cast to the out dtype.

Poisoned outputs
----------------
`poison` allocates NaN-filled blocks of the outputs' sizes and frees them just
before a kernel call, so the caching allocator hands them to `at::empty`; the
GPU tests then assert `isfinite` over every output, which turns a row or tail
that the kernel never wrote into NaN instead of plausible stale data.
`poison` checks itself on the GPU: a repeated allocation of the same sizes
must read all-NaN, or it raises.
"""
from __future__ import annotations

import math

import torch

ACCUM_MULT = 32.0
ELEM_ABS = 2.0 ** -20
_MANT = {torch.bfloat16: 7, torch.float32: 23}


def f64(t):
    return t.detach().to("cpu", torch.float64)


# ---------------------------------------------------------------------------
# fp64 oracles
# ---------------------------------------------------------------------------
def rmsnorm_fwd(x, w, eps, res=None):
    """-> y, invrms (and the sum when res is given)."""
    x, w = f64(x), f64(w)
    if res is not None:
        # the kernel rounds the sum to the input dtype only for sum_out;
        # it normalizes the unrounded fp32 sum
        x = x + f64(res)
    invrms = 1.0 / torch.sqrt((x * x).mean(-1) + eps)
    y = x * invrms.unsqueeze(-1) * w
    return (y, invrms) if res is None else (y, invrms, x)


def rmsnorm_bwd(dy, x, w, invrms, dsum=None):
    dy, x, w, r = f64(dy), f64(x), f64(w), f64(invrms).unsqueeze(-1)
    H = x.shape[-1]
    xhat = x * r
    dxhat = dy * w
    dx = r * (dxhat - xhat * (dxhat * xhat).sum(-1, keepdim=True) / H)
    if dsum is not None:
        dx = dx + f64(dsum)
    dw = (dy * xhat).reshape(-1, H).sum(0)
    return dx, dw


def rmsnorm_dx_scale(dy, x, w, invrms, dsum=None):
    dy, x, w, r = f64(dy), f64(x), f64(w), f64(invrms).unsqueeze(-1)
    big = (dy * w).abs().amax(-1, keepdim=True)
    s = r * big * (1 + (x * r).abs())
    return s if dsum is None else s + f64(dsum).abs()


def layernorm_fwd(x, w, b, eps):
    x, w, b = f64(x), f64(w), f64(b)
    mean = x.mean(-1)
    var = ((x - mean.unsqueeze(-1)) ** 2).mean(-1)
    invstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean.unsqueeze(-1)) * invstd.unsqueeze(-1) * w + b
    return y, mean, invstd


def layernorm_y_scale(x, w, b, eps):
    _, mean, invstd = layernorm_fwd(x, w, b, eps)
    x, w, b = f64(x), f64(w), f64(b)
    return ((x.abs() + mean.abs().unsqueeze(-1)) * invstd.unsqueeze(-1)
            * w.abs() + b.abs())


def layernorm_bwd(dy, x, w, mean, invstd):
    dy, x, w = f64(dy), f64(x), f64(w)
    m, r = f64(mean).unsqueeze(-1), f64(invstd).unsqueeze(-1)
    H = x.shape[-1]
    xhat = (x - m) * r
    dxhat = dy * w
    dx = r * (dxhat - dxhat.sum(-1, keepdim=True) / H
              - xhat * (dxhat * xhat).sum(-1, keepdim=True) / H)
    dw = (dy * xhat).reshape(-1, H).sum(0)
    db = dy.reshape(-1, H).sum(0)
    return dx, dw, db


def layernorm_dx_scale(dy, x, w, mean, invstd):
    dy, x, w = f64(dy), f64(x), f64(w)
    m, r = f64(mean).unsqueeze(-1), f64(invstd).unsqueeze(-1)
    big = (dy * w).abs().amax(-1, keepdim=True)
    return r * big * (2 + ((x - m) * r).abs())


def swiglu_fwd(x):
    g, u = f64(x).chunk(2, dim=-1)
    return g / (1 + torch.exp(-g)) * u


def swiglu_bwd(dy, x):
    g, u = f64(x).chunk(2, dim=-1)
    dy = f64(dy)
    sig = 1 / (1 + torch.exp(-g))
    return torch.cat([dy * u * sig * (1 + g * (1 - sig)), dy * g * sig], -1)


def swiglu_scale(x, dy=None):
    """Scale of y (dy None) or of dx = [dgate, dup].  dgate's factor
    1 + g*(1 - sig) cancels near g = -1.28, so its scale is taken before
    that factor."""
    g, u = f64(x).chunk(2, dim=-1)
    sig = 1 / (1 + torch.exp(-g))
    if dy is None:
        return (g * sig * u).abs() * (1 + g.abs())
    dy = f64(dy).abs()
    amp = sig * (1 + g.abs())
    return torch.cat([dy * u.abs() * amp, dy * g.abs() * amp], -1)


def rope(x, cos, sin, conj=False):
    """NEOX half rotation.  x [s, b, h, d]; cos/sin [s, d/2] or, with
    per-row tables, [s, b, d/2]."""
    x, c, s = f64(x), f64(cos), f64(sin)
    d2 = x.shape[-1] // 2
    x1, x2 = x[..., :d2], x[..., d2:]
    if c.dim() == 2:
        c, s = c[:, None, None, :], s[:, None, None, :]
    else:
        c, s = c[:, :, None, :], s[:, :, None, :]
    if conj:
        s = -s
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def rope_scale(x):
    x = f64(x)
    d2 = x.shape[-1] // 2
    a = x[..., :d2].abs() + x[..., d2:].abs()
    return torch.cat([a, a], -1)


def ce_max(logits):
    return f64(logits).max(-1).values


def ce_sum_target(logits, target, gmax, vocab_start):
    """-> sumexp, tlogit (0 for a target outside [vocab_start, +V))."""
    lf = f64(logits)
    V = lf.shape[-1]
    sumexp = torch.exp(lf - f64(gmax).unsqueeze(-1)).sum(-1)
    t = target.detach().cpu() - vocab_start
    on = (t >= 0) & (t < V)
    tl = lf.gather(-1, t.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    return sumexp, torch.where(on, tl, torch.zeros_like(tl))


def ce_bwd(logits, target, gmax, sumexp, gout, vocab_start, with_scale=False):
    lf = f64(logits)
    V = lf.shape[-1]
    z = lf - f64(gmax).unsqueeze(-1)
    p = torch.exp(z) / f64(sumexp).unsqueeze(-1)
    t = target.detach().cpu() - vocab_start
    on = (t >= 0) & (t < V)
    onehot = torch.zeros_like(p)
    onehot.scatter_(-1, t.clamp(0, V - 1).unsqueeze(-1),
                    on.to(torch.float64).unsqueeze(-1))
    g = f64(gout).unsqueeze(-1)
    out = (p - onehot) * g
    if with_scale:
        return out, g.abs() * (p * (1 + z.abs()) + onehot)
    return out


def adamw_step(master, g, m, v, step, lr, beta1, beta2, eps, wd, gscale=1.0):
    """One decoupled-weight-decay Adam step -> new (master, m, v)."""
    master, g, m, v = f64(master), f64(g) * gscale, f64(m), f64(v)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    mhat = m / (1 - beta1 ** step)
    vhat = v / (1 - beta2 ** step)
    master = master - lr * (mhat / (torch.sqrt(vhat) + eps) + wd * master)
    return master, m, v


def grad_accum(flat, g, offset):
    out = f64(flat).clone()
    out[offset:offset + g.numel()] += f64(g).reshape(-1)
    return out


def moe_permute(x, rows):
    return f64(x)[rows.cpu()]


def moe_permute_bwd(dy, rows, n):
    dy = f64(dy)
    out = torch.zeros(n, dy.shape[-1], dtype=torch.float64)
    out.index_add_(0, rows.cpu(), dy)
    return out


def moe_unpermute(back, probs, order, n, k):
    """out[t] = sum_j probs[i] * back[i] over the k sorted slots i with
    order[i] // k == t."""
    back, probs, order = f64(back), f64(probs), order.cpu()
    out = torch.zeros(n, back.shape[-1], dtype=torch.float64)
    if back.shape[0]:
        out.index_add_(0, order // k, back * probs.unsqueeze(-1))
    return out


def moe_unpermute_bwd(dout, back, probs, order, k):
    """-> dback, dprobs."""
    dout, back, probs = f64(dout), f64(back), f64(probs)
    g = dout[order.cpu() // k] if back.shape[0] else back
    return g * probs.unsqueeze(-1), (g * back).sum(-1)


def grouped_gemm(a, w, counts):
    a, w = f64(a), f64(w)
    outs, s = [], 0
    for e, m in enumerate(counts):
        outs.append(a[s:s + m] @ w[e])
        s += m
    return torch.cat(outs) if outs else a.new_zeros(0, w.shape[2])


def grouped_gemm_bwd(dc, a, w, counts):
    """-> dA, dW."""
    dc, a, w = f64(dc), f64(a), f64(w)
    da = torch.zeros_like(a)
    dw = torch.zeros_like(w)
    s = 0
    for e, m in enumerate(counts):
        da[s:s + m] = dc[s:s + m] @ w[e].T
        dw[e] = a[s:s + m].T @ dc[s:s + m]
        s += m
    return da, dw


# ---------------------------------------------------------------------------
# comparison rules
# ---------------------------------------------------------------------------
class RuleFailure(AssertionError):
    pass


def ulp_at(mag64, dtype):
    """One unit in the last place of `dtype` at magnitude mag64 (0 at 0)."""
    _, e = torch.frexp(mag64)           # mag = m * 2^e, m in [0.5, 1)
    u = torch.ldexp(torch.ones_like(mag64), e - 1 - _MANT[dtype])
    return torch.where(mag64 > 0, u, torch.zeros_like(u))


def elem_excess(got, oracle, scale=None):
    """max over elements of |got - round(oracle)| / bound (<= 1 passes)."""
    dtype = got.dtype
    assert dtype in _MANT, dtype
    assert got.shape == oracle.shape, (got.shape, oracle.shape)
    if got.numel() == 0:
        return 0.0
    o = oracle.to(torch.float64)
    scale = o.abs() if scale is None else scale.to(torch.float64)
    bound = ulp_at(o.abs(), dtype) + ELEM_ABS * scale
    err = (f64(got) - o.to(dtype).to(torch.float64)).abs()
    # 0/0 (both exact) passes; anything non-finite fails
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    return float(ratio.max())


def assert_elem(got, oracle, scale=None, what=""):
    r = elem_excess(got, oracle, scale)
    print(f"[elem] {what}: max err/bound = {r:.3g}")
    if not r <= 1.0:
        raise RuleFailure(f"{what}: element rule missed, err/bound = {r:.4g}")
    return r


def accum_bound(ref32, oracle, mult=ACCUM_MULT):
    o = oracle.to(torch.float64)
    if o.numel() == 0:
        return 0.0
    e_ref = float((f64(ref32) - o).abs().max())
    floor = 2.0 ** -24 * float(o.abs().max())
    return mult * max(e_ref, floor)


def accum_excess(got, ref32, oracle, mult=ACCUM_MULT):
    """max|got - oracle| / bound (<= 1 passes)."""
    assert got.shape == oracle.shape, (got.shape, oracle.shape)
    if got.numel() == 0:
        return 0.0
    err = float(torch.nan_to_num((f64(got) - oracle.to(torch.float64)).abs(),
                                 nan=math.inf).max())
    bound = accum_bound(ref32, oracle, mult)
    if err == 0:
        return 0.0
    return err / bound if bound > 0 else math.inf


def assert_accum(got, ref32, oracle, what="", mult=ACCUM_MULT):
    r = accum_excess(got, ref32, oracle, mult)
    print(f"[accum] {what}: max err / ({mult:g} x reference error) = {r:.3g}"
          f"  (kernel/reference error ratio {r * mult:.3g})")
    if not r <= 1.0:
        raise RuleFailure(f"{what}: accumulation rule missed, "
                          f"err/bound = {r:.4g} at {mult:g}x")
    return r


def assert_rows_bitwise(big, small, rows, what=""):
    """rows of the large call == the same rows run alone."""
    sel = big[torch.as_tensor(rows, device=big.device)]
    if not torch.equal(sel, small):
        bad = (sel != small).reshape(len(rows), -1).any(-1).nonzero().flatten()
        raise RuleFailure(f"{what}: rows {[rows[i] for i in bad.tolist()]} "
                          "differ between the large call and the same rows "
                          "run alone")


POISON_CHECKED = [0]       # blocks whose re-allocation was seen to read NaN


def poison(device, *specs):
    """specs: (shape, dtype).  NaN-fill blocks of those sizes and free them,
    so the next at::empty of the same size gets NaN, not stale data.

    On the GPU the guard checks itself: the same sizes are allocated again
    with torch.empty and must read all-NaN.  Where the allocator hands out
    another block (an equal-sized free one with stale data), that block is
    filled and freed too, until a repeated allocation reads NaN; if that
    never happens the isfinite checks would be vacuous, and this raises."""
    shapes = [((s,) if isinstance(s, int) else tuple(s), dt)
              for s, dt in specs]
    blocks = [torch.full(s, float("nan"), dtype=dt, device=device)
              for s, dt in shapes]
    del blocks
    if torch.device(device).type != "cuda" or not shapes:
        return
    for _ in range(4):
        again = [torch.empty(s, dtype=dt, device=device) for s, dt in shapes]
        clean = all(bool(torch.isnan(t).all()) for t in again)
        if not clean:
            for t in again:
                t.fill_(float("nan"))
        del again
        if clean:
            POISON_CHECKED[0] += len(shapes)
            return
    raise RuleFailure("poison: a freed NaN block is not what the allocator "
                      f"hands out next for {shapes}")


def assert_finite(*tensors, what=""):
    for i, t in enumerate(tensors):
        if not bool(torch.isfinite(t).all()):
            bad = (~torch.isfinite(t)).nonzero()[0].tolist()
            raise RuleFailure(f"{what}: output {i} holds a non-finite value "
                              f"at {bad} (an element the kernel never wrote?)")


# ---------------------------------------------------------------------------
# shared inputs (built on the CPU from fixed seeds; the GPU tests move them)
# ---------------------------------------------------------------------------
NORM_WIDTHS = [8, 1600, 2056, 5120, 12288, 16384]      # at n = 3
NORM_ROWS = [(2048, 264), (2049, 264), (4099, 264),
             (2048, 1032), (2049, 1032), (4099, 1032)]
NORM_EPS = 1e-5
CE_WIDTHS = [7, 8, 2055, 50257]                         # at n = 64
CE_GRID = (2051, 2055)
ADAMW_SIZES = [1, 7, 8, 9, 2048 * 256 * 8 + 8 * 256 + 5]
ADAMW_TENSORS = list(zip(ADAMW_SIZES, [0, 3, 1, 0, 3]))  # (n, view offset)
GRAD_ACCUM_CASES = [(5, 0), (7, 123), (4097, 123), (2048 * 256 * 8 + 13, 1)]
MOE_CASES = [(64, 8, 1), (64, 8, 2), (64, 128, 1), (64, 128, 2),
             (4100, 1032, 1)]                           # (n, h, k)
GG_CASES = [([1], 128, 128), ([129, 0, 127], 128, 128),
            ([0, 0, 5, 0], 128, 128), ([0, 0, 0], 128, 128),
            ([100], 128, 128), ([129, 0, 127], 128, 256),
            ([40, 3], 160, 128)]                        # (counts, K, N)
GRID_ROWS = 2048                                        # row-kernel grid cap


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def norm_inputs(n, H, dtype, seed=0):
    """x, w, b, dy: asymmetric (a column ramp on x, w and b not centred)."""
    g = _gen(1000 + seed)
    ramp = torch.linspace(-0.5, 1.0, H)
    x = (torch.randn(n, H, generator=g) * 1.5 + ramp).to(dtype)
    w = (torch.randn(H, generator=g) * 0.1 + 1.0).to(dtype)
    b = (torch.randn(H, generator=g) * 0.1 + 0.05).to(dtype)
    dy = (torch.randn(n, H, generator=g) * (1.0 + ramp.abs())).to(dtype)
    return x, w, b, dy


def norm_special_rows(H, dtype, seed=0):
    """Row 0 all zero, row 1 constant, rows 2.. offset rows: mean 64 with
    std 0.05 in fp32, mean 64 on the bf16 grid (spacing 0.5) in bf16."""
    g = _gen(2000 + seed)
    x, w, b, dy = norm_inputs(6, H, dtype, seed)
    x = x.float()
    x[0] = 0.0
    x[1] = 3.0
    if dtype == torch.float32:
        x[2:] = 64.0 + 0.05 * torch.randn(4, H, generator=g)
    else:
        x[2:] = 64.0 + 0.5 * torch.randint(-2, 3, (4, H), generator=g).float()
    return x.to(dtype), w, b, dy


def add_rmsnorm_inputs(n, H, special=False):
    """x, res, w, dy, dsum in bf16 for the fused residual-add rmsnorm (bf16
    only).  special: six rows whose sum x + res is exactly zero (row 0),
    constant 5 (row 1) and has mean 64 (rows 2..)."""
    bf = torch.bfloat16
    x, w, _, dy = norm_special_rows(H, bf) if special \
        else norm_inputs(n, H, bf)
    res, _, _, dsum = norm_inputs(x.shape[0], H, bf, seed=1)
    if special:
        x[0] = -res[0]
        res[1] = 2.0
        res[2:] = (res[2:].float() * 0.125).to(bf)
    return x, res, w, dy, dsum


def onepass_variance_fp32(x):
    """The defect: var = E[x^2] - mean^2 evaluated in fp32."""
    xf = x.float()
    mean = xf.mean(-1)
    return (xf * xf).mean(-1) - mean * mean


def ce_inputs(n, V, dtype, seed=0):
    """logits, target, vocab_start, gout.  Row maxima are planted (row % 4:
    0 a tail column, 1 the last vector packet, 2 column 0, 3 plain random)
    and the targets cycle through the first column, the last vector column,
    a tail column, one off the shard on each side, far off, and random."""
    g = _gen(3000 + seed)
    V8 = V & ~7
    vocab_start = 3 * V + 1
    logits = torch.randn(n, V, generator=g) * 4
    r = torch.arange(n)
    # the last column: in the scalar tail when V % 8 != 0; for V = 8 there
    # is no tail and it is simply column 7 of the only packet
    pack_col = max(V8 - 3, 0)
    logits[r[r % 4 == 0], V - 1] = 30.0
    logits[r[r % 4 == 1], pack_col] = 29.0
    logits[r[r % 4 == 2], 0] = 31.0
    logits = logits.to(dtype)
    choices = [0, max(V8 - 1, 0), V - 1, -1, V, 10 * V + 3]
    t_local = torch.randint(0, V, (n,), generator=g)
    for i, c in enumerate(choices):
        t_local[r % 7 == i] = c
    gout = torch.randn(n, generator=g)
    gout[r % 5 == 4] = 0.0
    return logits, t_local + vocab_start, vocab_start, gout


def swiglu_inputs(rows, F, dtype, seed=0):
    g = _gen(4000 + seed)
    x = (torch.randn(rows, 2 * F, generator=g) * 2.0 + 0.25).to(dtype)
    dy = (torch.randn(rows, F, generator=g) + 0.1).to(dtype)
    return x, dy


def rope_inputs(s, b, h, d, dtype, seed=0):
    from hetu_galvatron_amd.ops.reference_ops import rope_freqs
    g = _gen(5000 + seed)
    x = (torch.randn(s, b, h, d, generator=g) + 0.2).to(dtype)
    cos, sin = rope_freqs(s, d)
    return x, cos, sin


def rope_row_tables(s, b, d, seed=0):
    """[s, b, d/2] tables whose positions restart mid-row, at a different
    place in every batch row (packed documents)."""
    from hetu_galvatron_amd.ops.reference_ops import rope_freqs
    cos, sin = rope_freqs(s, d)
    pos = torch.empty(s, b, dtype=torch.long)
    for j in range(b):
        cut = (s // 3) * (j + 1) // b + 1 + j
        p = torch.arange(s)
        pos[:, j] = torch.where(p < cut, p, p - cut)
    return cos[pos], sin[pos], pos


ADAMW_HYPER = [
    # step, lr, beta1, beta2, eps, wd, gscale
    dict(step=1, lr=0.05, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.5,
         gscale=0.37),
    dict(step=100000, lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.0,
         gscale=1.0),
]


def adamw_inputs(n, g_dtype, seed=0, offset=0):
    """Flat buffers master, g, m, v of n + offset elements; the optimizer's
    tensors are the views [offset:] (the runtime passes views into flat
    buffers, so an odd offset leaves every 16-byte packet misaligned).
    Every 5th element has g = 0 and v = 0 (denominator = eps) with a tiny
    m, so that the step stays of ordinary size."""
    gen = _gen(6000 + seed)
    tot = n + offset
    master = torch.randn(tot, generator=gen) + 0.3
    g = (torch.randn(tot, generator=gen) * 2 + 0.1).to(g_dtype)
    m = torch.randn(tot, generator=gen) * 0.1
    v = torch.rand(tot, generator=gen) * 0.01 + 1e-4
    z = torch.arange(tot) % 5 == 3
    g[z] = 0
    v[z] = 0
    m[z] = 1e-9 * (1 + torch.arange(tot)[z] % 3).float()
    return master, g, m, v


def ref_adamw(master, g, m, v, out_dtype, hp):
    """reference_ops.adamw_step on clones (gscale folded into the grads in
    fp32, as the reference path does) -> master, m, v, out."""
    from hetu_galvatron_amd.ops import reference_ops as ref
    master, m, v = master.clone(), m.clone(), v.clone()
    out = torch.zeros(master.shape, dtype=out_dtype)
    ref.adamw_step([out], [g.float() * hp["gscale"]], [m], [v], [master],
                   hp["step"], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"],
                   hp["wd"])
    return master, m, v, out


def moe_inputs(n, h, E, k, dtype, seed=0):
    """x [n, h], probs (sorted) [m], order, rows, dout.  Token 0's k slots
    all go to one expert."""
    g = _gen(7000 + seed)
    x = (torch.randn(n, h, generator=g) + 0.2).to(dtype)
    idx = torch.randint(0, E, (n, k), generator=g)
    if n:
        idx[0] = E - 1
    probs = torch.softmax(torch.randn(n, k, generator=g), -1).reshape(-1)
    order = torch.argsort(idx.reshape(-1), stable=True)
    rows = torch.div(order, k, rounding_mode="floor")
    dout = (torch.randn(n, h, generator=g) - 0.1).to(dtype)
    back = (torch.randn(n * k, h, generator=g) + 0.1).to(dtype)
    return x, probs[order].contiguous(), order, rows, dout, back


def grad_accum_inputs(n, off, g_dtype):
    gen = _gen(n)
    flat = torch.randn(n + off + 9, generator=gen)
    g = (torch.randn(n, generator=gen) + 0.1).to(g_dtype)
    return flat, g


def gg_inputs(counts, K, N, seed=0):
    g = _gen(8000 + seed)
    E, M = len(counts), sum(counts)
    a = (torch.randn(M, K, generator=g) / 8 + 0.02).bfloat16()
    w = (torch.randn(E, K, N, generator=g) / 8 - 0.01).bfloat16()
    dc = (torch.randn(M, N, generator=g) + 0.05).bfloat16()
    return a, w, dc
