"""HIP kernels at the shapes, dtypes and edges where they can go wrong.

Every kernel outside attention (norms, cross entropy, swiglu, rope, adamw,
grad_accum, MoE permute / unpermute, grouped GEMM) is compared with the fp64
oracles of kernel_oracle.py under its three rules: bitwise row independence
between a large call and the same rows run alone (the grid-stride regime),
a multiple of the fp32 reference's own error for fp32 accumulations, and
one output ulp plus a scaled fp32 term for element outputs.  Outputs are
allocated over NaN-poisoned memory and checked with isfinite, so an element
the kernel never wrote shows.  Inputs come from kernel_oracle.py, where
test_kernel_oracle.py checks on the CPU that the reference passes the same
rules on them and that planted mutants do not.
"""
import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref

from . import kernel_oracle as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
BF16 = torch.bfloat16
DTYPES = [BF16, F32]
EPS = ko.NORM_EPS


def _ids(v):
    return str(v).replace("torch.", "").replace(" ", "")


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def dev(*ts):
    out = tuple(t.to(DEV) for t in ts)
    return out if len(out) > 1 else out[0]


def call(fn, *args, outs=(), what=""):
    """fn(*args) with its outputs allocated over NaN-poisoned blocks; every
    returned tensor must be finite."""
    ko.poison(DEV, *outs)
    r = fn(*args)
    ko.assert_finite(*(r if isinstance(r, (tuple, list)) else (r,)),
                     what=what or getattr(fn, "__name__", "kernel"))
    return r


def test_poison_takes():
    """The guard itself: after poison, an at::empty of a poisoned size reads
    NaN, for a small-pool block and a large one (poison raises otherwise)."""
    before = ko.POISON_CHECKED[0]
    specs = [((3, 8), BF16), ((4099, 1032), F32)]
    ko.poison(DEV, *specs)
    assert ko.POISON_CHECKED[0] == before + len(specs)
    for shape, dt in specs:
        assert bool(torch.isnan(torch.empty(shape, dtype=dt,
                                            device=DEV)).all())


def alone(n):
    """Rows to re-run alone: first and last of every grid-stride sweep."""
    G = ko.GRID_ROWS
    rows = {0, 1, n - 1}
    for k in range(1, (n + G - 1) // G):
        rows |= {k * G - 1, k * G, min(k * G + 2, n - 1)}
    return sorted(r for r in rows if 0 <= r < n)


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------
def _check_rmsnorm(x, w, dy, tag, rows=None):
    e = ext()
    n, H = x.shape
    dt = x.dtype
    G = min(n, ko.GRID_ROWS)
    xd, wd, dyd = dev(x, w, dy)
    y, inv = call(e.rmsnorm_fwd, xd, wd, EPS,
                  outs=[((n, H), dt), ((n,), F32)], what=f"rms fwd {tag}")
    y64, inv64 = ko.rmsnorm_fwd(x, w, EPS)
    ko.assert_elem(y.cpu(), y64, what=f"rms y {tag}")
    ko.assert_elem(inv.cpu(), inv64, what=f"rms invrms {tag}")
    dx, dw = call(e.rmsnorm_bwd, dyd, xd, wd, inv,
                  outs=[((n, H), dt), ((G, H), F32)], what=f"rms bwd {tag}")
    invc = inv.cpu()                       # the kernel's own statistic
    dx64, dw64 = ko.rmsnorm_bwd(dy, x, w, invc)
    ko.assert_elem(dx.cpu(), dx64, ko.rmsnorm_dx_scale(dy, x, w, invc),
                   f"rms dx {tag}")
    _, dw32 = ref.rmsnorm_bwd(dy, x, w, invc)
    ko.assert_accum(dw.cpu(), dw32, dw64, f"rms dw {tag}")
    if rows:
        idx = torch.tensor(rows, device=DEV)
        xs, dys = xd[idx].contiguous(), dyd[idx].contiguous()
        ys, invs = e.rmsnorm_fwd(xs, wd, EPS)
        ko.assert_rows_bitwise(y, ys, rows, f"rms y {tag}")
        ko.assert_rows_bitwise(inv, invs, rows, f"rms invrms {tag}")
        dxs, _ = e.rmsnorm_bwd(dys, xs, wd, invs)
        ko.assert_rows_bitwise(dx, dxs, rows, f"rms dx {tag}")


def _check_layernorm(x, w, b, dy, tag, rows=None):
    e = ext()
    n, H = x.shape
    dt = x.dtype
    G = min(n, ko.GRID_ROWS)
    xd, wd, bd, dyd = dev(x, w, b, dy)
    y, mean, invstd = call(e.layernorm_fwd, xd, wd, bd, EPS,
                           outs=[((n, H), dt), ((n,), F32), ((n,), F32)],
                           what=f"ln fwd {tag}")
    y64, mean64, invstd64 = ko.layernorm_fwd(x, w, b, EPS)
    ko.assert_elem(mean.cpu(), mean64, ko.f64(x).abs().amax(-1),
                   f"ln mean {tag}")
    ko.assert_elem(invstd.cpu(), invstd64, what=f"ln invstd {tag}")
    ko.assert_elem(y.cpu(), y64, ko.layernorm_y_scale(x, w, b, EPS),
                   f"ln y {tag}")
    dx, dw, db = call(e.layernorm_bwd, dyd, xd, wd, mean, invstd,
                      outs=[((n, H), dt), ((2, G, H), F32)],
                      what=f"ln bwd {tag}")
    mc, rc = mean.cpu(), invstd.cpu()      # the kernel's own statistics
    dx64, dw64, db64 = ko.layernorm_bwd(dy, x, w, mc, rc)
    ko.assert_elem(dx.cpu(), dx64, ko.layernorm_dx_scale(dy, x, w, mc, rc),
                   f"ln dx {tag}")
    _, dw32, db32 = ref.layernorm_bwd(dy, x, w, mc, rc)
    ko.assert_accum(dw.cpu(), dw32, dw64, f"ln dw {tag}")
    ko.assert_accum(db.cpu(), db32, db64, f"ln db {tag}")
    if rows:
        idx = torch.tensor(rows, device=DEV)
        xs, dys = xd[idx].contiguous(), dyd[idx].contiguous()
        ys, ms, rs = e.layernorm_fwd(xs, wd, bd, EPS)
        ko.assert_rows_bitwise(y, ys, rows, f"ln y {tag}")
        ko.assert_rows_bitwise(mean, ms, rows, f"ln mean {tag}")
        ko.assert_rows_bitwise(invstd, rs, rows, f"ln invstd {tag}")
        dxs, _, _ = e.layernorm_bwd(dys, xs, wd, ms, rs)
        ko.assert_rows_bitwise(dx, dxs, rows, f"ln dx {tag}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("H", ko.NORM_WIDTHS)
def test_norm_widths(H, dtype):
    """Every VPT variant, full and partial combs, at n = 3."""
    x, w, b, dy = ko.norm_inputs(3, H, dtype)
    _check_rmsnorm(x, w, dy, f"n=3 H={H}")
    _check_layernorm(x, w, b, dy, f"n=3 H={H}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,H", ko.NORM_ROWS)
def test_norm_grid_stride(n, H, dtype):
    """At the grid cap (one row per block), one past it (one block does two
    rows) and 4099 (a mix of three and two rows per block)."""
    x, w, b, dy = ko.norm_inputs(n, H, dtype)
    _check_rmsnorm(x, w, dy, f"n={n} H={H}", alone(n))
    _check_layernorm(x, w, b, dy, f"n={n} H={H}", alone(n))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_norm_special_rows(dtype):
    """An all-zero row, a constant row and rows with mean 64: std 0.05 in
    fp32 (where var = E[x^2] - mean^2 in fp32 was 10-26 % off or negative)
    and on the bf16 grid in bf16."""
    x, w, b, dy = ko.norm_special_rows(1600, dtype)
    _check_rmsnorm(x, w, dy, "special rows")
    _check_layernorm(x, w, b, dy, "special rows")


def _check_add_rmsnorm(x, res, w, dy, dsum, tag, rows=None):
    """The residual-add path of the rmsnorm kernels: the res load and
    sum_out store in the forward, the dsum fold in the backward."""
    e = ext()
    n, H = x.shape
    G = min(n, ko.GRID_ROWS)
    xd, wd, dyd, resd, dsumd = dev(x, w, dy, res, dsum)
    y, s, inv = call(e.add_rmsnorm_fwd, xd, resd, wd, EPS,
                     outs=[((n, H), BF16), ((n, H), BF16), ((n,), F32)],
                     what=f"add_rms fwd {tag}")
    y64, inv64, s64 = ko.rmsnorm_fwd(x, w, EPS, res)
    ko.assert_elem(s.cpu(), s64, what=f"add_rms sum {tag}")
    ko.assert_elem(inv.cpu(), inv64, what=f"add_rms invrms {tag}")
    ko.assert_elem(y.cpu(), y64, what=f"add_rms y {tag}")
    dx, dw = call(e.add_rmsnorm_bwd, dyd, dsumd, s, wd, inv,
                  outs=[((n, H), BF16), ((G, H), F32)],
                  what=f"add_rms bwd {tag}")
    sc, invc = s.cpu(), inv.cpu()          # the kernel's own sum and invrms
    dx64, dw64 = ko.rmsnorm_bwd(dy, sc, w, invc, dsum)
    ko.assert_elem(dx.cpu(), dx64, ko.rmsnorm_dx_scale(dy, sc, w, invc, dsum),
                   f"add_rms dx {tag}")
    _, dw32 = ref.rmsnorm_bwd(dy, sc, w, invc)
    ko.assert_accum(dw.cpu(), dw32, dw64, f"add_rms dw {tag}")
    if rows:
        idx = torch.tensor(rows, device=DEV)
        ys, ss, invs = e.add_rmsnorm_fwd(xd[idx].contiguous(),
                                         resd[idx].contiguous(), wd, EPS)
        ko.assert_rows_bitwise(y, ys, rows, f"add_rms y {tag}")
        ko.assert_rows_bitwise(s, ss, rows, f"add_rms sum {tag}")
        ko.assert_rows_bitwise(inv, invs, rows, f"add_rms invrms {tag}")
        dxs, _ = e.add_rmsnorm_bwd(dyd[idx].contiguous(),
                                   dsumd[idx].contiguous(), ss, wd, invs)
        ko.assert_rows_bitwise(dx, dxs, rows, f"add_rms dx {tag}")


@pytest.mark.parametrize("H", ko.NORM_WIDTHS)
def test_add_rmsnorm_widths(H):
    """The residual-add path at every VPT variant and partial comb."""
    _check_add_rmsnorm(*ko.add_rmsnorm_inputs(3, H), f"n=3 H={H}")


@pytest.mark.parametrize("n,H", ko.NORM_ROWS)
def test_add_rmsnorm_grid_stride(n, H):
    _check_add_rmsnorm(*ko.add_rmsnorm_inputs(n, H), f"n={n} H={H}", alone(n))


def test_add_rmsnorm_special_rows():
    """x + res exactly zero, constant, and with mean 64."""
    _check_add_rmsnorm(*ko.add_rmsnorm_inputs(6, 1600, special=True),
                       "special rows")


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------
CE_CASES = [(64, V) for V in ko.CE_WIDTHS] + [ko.CE_GRID]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,V", CE_CASES)
def test_vocab_ce_edges(n, V, dtype):
    """Tail-only, one packet, a full sweep plus a tail, gpt2's odd 50257
    (row bases 2-byte aligned in bf16) and n past the grid cap; planted
    row maxima; targets on the first, last-vector and tail columns, one off
    the shard on either side and far off."""
    e = ext()
    logits, target, vs, gout = ko.ce_inputs(n, V, dtype)
    ld, td, gd = dev(logits, target, gout)
    stat = [((n,), F32)]
    gmax = call(e.ce_max, ld, outs=stat, what="ce_max")
    assert torch.equal(gmax.cpu().double(), ko.ce_max(logits)), "ce max"
    se, tl = call(e.ce_sum_target, ld, td, gmax, vs, outs=stat * 2,
                  what="ce_sum_target")
    gm = gmax.cpu()
    se64, tl64 = ko.ce_sum_target(logits, target, gm, vs)
    se32, _ = ref.vocab_ce_fwd_local(logits, target, gm, vs, vs + V)
    ko.assert_accum(se.cpu(), se32, se64, f"ce sumexp V={V}")
    assert torch.equal(tl.cpu().double(), tl64), "ce target logit"

    inp = ld.clone()
    dl = e.ce_bwd(inp, td, gmax, dev(se32), gd, vs)
    assert dl.data_ptr() == inp.data_ptr() and dl.shape == inp.shape, \
        "ce_bwd must write in place"
    ko.assert_finite(dl, what="ce_bwd")
    dl64, scale = ko.ce_bwd(logits, target, gm, se32, gout, vs, True)
    ko.assert_elem(dl.cpu(), dl64, scale, f"ce dlogits V={V}")
    assert bool((dl[gd == 0] == 0).all()), "rows with gout = 0 must be zero"

    if n > ko.GRID_ROWS:
        rows = alone(n)
        idx = torch.tensor(rows, device=DEV)
        ls, ts = ld[idx].contiguous(), td[idx].contiguous()
        gmax_s = e.ce_max(ls)
        ko.assert_rows_bitwise(gmax, gmax_s, rows, "ce max")
        se_s, tl_s = e.ce_sum_target(ls, ts, gmax_s, vs)
        ko.assert_rows_bitwise(se, se_s, rows, "ce sumexp")
        ko.assert_rows_bitwise(tl, tl_s, rows, "ce target logit")
        dl_s = e.ce_bwd(ls.clone(), ts, gmax_s, dev(se32)[idx].contiguous(),
                        gd[idx].contiguous(), vs)
        ko.assert_rows_bitwise(dl, dl_s, rows, "ce dlogits")


# ---------------------------------------------------------------------------
# swiglu / rope
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("rows,F", [(5, 8), (2052, 2056)])
def test_swiglu_edges(rows, F, dtype):
    """One packet per row, and 2052 x 257 packets: past the grid cap of
    2048 x 256 threads, so the last 12 rows run in a second sweep."""
    e = ext()
    x, dy = ko.swiglu_inputs(rows, F, dtype)
    xd, dyd = dev(x, dy)
    y = call(e.swiglu_fwd, xd, outs=[((rows, F), dtype)], what="swiglu fwd")
    ko.assert_elem(y.cpu(), ko.swiglu_fwd(x), ko.swiglu_scale(x), "swiglu y")
    dx = call(e.swiglu_bwd, dyd, xd, outs=[((rows, 2 * F), dtype)],
              what="swiglu bwd")
    ko.assert_elem(dx.cpu(), ko.swiglu_bwd(dy, x), ko.swiglu_scale(x, dy),
                   "swiglu dx")
    if rows * (F // 8) > ko.GRID_ROWS * 256:
        first2 = ko.GRID_ROWS * 256 // (F // 8)     # first row of sweep 2
        sel = sorted({0, 1, first2 - 1, first2, first2 + 1, rows - 1})
        idx = torch.tensor(sel, device=DEV)
        xs, dys = xd[idx].contiguous(), dyd[idx].contiguous()
        ko.assert_rows_bitwise(y, e.swiglu_fwd(xs), sel, "swiglu y")
        ko.assert_rows_bitwise(dx, e.swiglu_bwd(dys, xs), sel, "swiglu dx")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("d", [16, 64, 128, 256])
def test_rope_head_dims(d, dtype):
    e = ext()
    s, b, h = 5, 2, 3
    x, cos, sin = ko.rope_inputs(s, b, h, d, dtype)
    xd, cd, sd = dev(x, cos, sin)
    for conj in (False, True):
        y = call(e.rope_fwd, xd, cd, sd, conj, outs=[(x.shape, dtype)],
                 what=f"rope d={d}")
        ko.assert_elem(y.cpu(), ko.rope(x, cos, sin, conj), ko.rope_scale(x),
                       f"rope d={d} conj={conj}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_rope_past_grid_cap(dtype):
    """s=2052, b=2, h=32, d=64 is 525312 packets, past the cap of 524288:
    the far end runs in a second sweep and must equal, bit for bit, a call
    on the last two s-rows with their table rows."""
    e = ext()
    s, b, h, d = 2052, 2, 32, 64
    x, cos, sin = ko.rope_inputs(s, b, h, d, dtype)
    xd, cd, sd = dev(x, cos, sin)
    for conj in (False, True):
        y = call(e.rope_fwd, xd, cd, sd, conj, outs=[(x.shape, dtype)],
                 what="rope large")
        ko.assert_elem(y.cpu(), ko.rope(x, cos, sin, conj), ko.rope_scale(x),
                       f"rope large conj={conj}")
        tail = e.rope_fwd(xd[-2:].contiguous(), cd[-2:].contiguous(),
                          sd[-2:].contiguous(), conj)
        assert torch.equal(y[-2:], tail), "rope: far end differs when run alone"
        head = e.rope_fwd(xd[:2].contiguous(), cd[:2].contiguous(),
                          sd[:2].contiguous(), conj)
        assert torch.equal(y[:2], head), "rope: first rows differ when run alone"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_rope_per_row_tables(dtype):
    """apply_rope_qk with [s, b, d/2] tables (packed documents: positions
    restart mid-row, elsewhere in every batch row), forward and backward,
    against an fp64 rope_apply_neox_batched."""
    from hetu_galvatron_amd.runtime.transformer.rope import apply_rope_qk
    s, b, d = 37, 3, 64
    q, _, _ = ko.rope_inputs(s, b, 4, d, dtype)
    k, _, _ = ko.rope_inputs(s, b, 2, d, dtype, seed=1)
    dq, _, _ = ko.rope_inputs(s, b, 4, d, dtype, seed=2)
    cos, sin, _ = ko.rope_row_tables(s, b, d)
    qd = dev(q).requires_grad_(True)
    kd, dqd, cd, sd = dev(k, dq, cos, sin)
    yq, yk = apply_rope_qk(qd, kd, cd, sd)
    assert yq.shape == q.shape and yk.shape == k.shape
    ko.assert_finite(yq, yk, what="rope per-row")
    ko.assert_elem(yq.detach().cpu(), ko.rope(q, cos, sin), ko.rope_scale(q),
                   "rope per-row q")
    ko.assert_elem(yk.cpu(), ko.rope(k, cos, sin), ko.rope_scale(k),
                   "rope per-row k")
    yq.backward(dqd)
    ko.assert_elem(qd.grad.cpu(), ko.rope(dq, cos, sin, True),
                   ko.rope_scale(dq), "rope per-row dq")


# ---------------------------------------------------------------------------
# adamw / grad_accum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hp", ko.ADAMW_HYPER, ids=["step1", "step100000"])
@pytest.mark.parametrize("g_dtype,o_dtype",
                         [(g, o) for g in DTYPES for o in DTYPES], ids=_ids)
def test_fused_adamw_edges(g_dtype, o_dtype, hp):
    """All four (grad, out) dtypes; n = 1, 7, 8, 9 and a second sweep plus a
    tail; views at odd element offsets into their flat buffers, as the
    optimizer passes them; step 1 with wd and gscale, step 100000 with
    wd = 0; every 5th element with g = 0 and v = 0."""
    PAD = 5
    cpu, views, obufs = [], ([], [], [], [], []), []
    for i, (n, off) in enumerate(ko.ADAMW_TENSORS):
        base = ko.adamw_inputs(n, g_dtype, seed=i, offset=off)
        cpu.append(tuple(t[off:] for t in base))
        for lst, t in zip(views, base):
            lst.append(dev(t)[off:])
        obuf = torch.full((off + n + PAD,), 7.0, dtype=o_dtype, device=DEV)
        obufs.append(obuf)
        views[4].append(obuf[off:off + n])
    masters, grads, ms, vs, outs = views
    ext().fused_adamw(masters, grads, ms, vs, outs, hp["step"], hp["lr"],
                      hp["beta1"], hp["beta2"], hp["eps"], hp["wd"],
                      hp["gscale"])
    for i, (n, off) in enumerate(ko.ADAMW_TENSORS):
        master, g, m, v = cpu[i]
        rm, rmm, rv, _ = ko.ref_adamw(master, g, m, v, o_dtype, hp)
        om, omm, ov = ko.adamw_step(master, g, m, v, **hp)
        tag = f"n={n} off={off}"
        ko.assert_finite(masters[i], ms[i], vs[i], outs[i], what=tag)
        ko.assert_accum(masters[i].cpu(), rm, om, f"adamw master {tag}")
        ko.assert_accum(ms[i].cpu(), rmm, omm, f"adamw m {tag}")
        ko.assert_accum(vs[i].cpu(), rv, ov, f"adamw v {tag}")
        # out is the cast of the kernel's own new master: identity in
        # fp32, round to nearest even in bf16, so bit-exact
        assert torch.equal(outs[i], masters[i].to(o_dtype)), \
            f"adamw out is not the cast of the new master, {tag}"
        assert bool((obufs[i][:off] == 7).all()) and \
            bool((obufs[i][off + n:] == 7).all()), f"adamw wrote outside {tag}"


@pytest.mark.parametrize("g_dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,off", ko.GRAD_ACCUM_CASES)
def test_grad_accum_edges(n, off, g_dtype):
    """fp32 and bf16 grads, n < 8, n past the grid cap, odd offsets."""
    flat, g = ko.grad_accum_inputs(n, off, g_dtype)
    fd = dev(flat)
    ext().grad_accum(fd, dev(g), off)
    got = fd.cpu()
    ko.assert_elem(got, ko.grad_accum(flat, g, off), what="grad_accum")
    assert torch.equal(got[:off], flat[:off]) and \
        torch.equal(got[off + n:], flat[off + n:]), "grad_accum wrote outside"


# ---------------------------------------------------------------------------
# MoE permute / unpermute
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,h,k", ko.MOE_CASES)
def test_moe_edges(n, h, k, dtype):
    """Forward, backward and dprobs (the router's only gradient through
    the merge) against fp64 and autograd through the pure-torch merge; a
    token whose k slots share one expert; 4100 x 129 packets pass the grid
    cap.  dprobs and the permute backward use float atomics: accumulation
    rule, never bitwise."""
    from hetu_galvatron_amd.ops.functional import moe_permute, moe_unpermute
    e = ext()
    x, probs, order, rows, dout, back = ko.moe_inputs(n, h, 4, k, dtype)
    m = n * k
    xd = dev(x).requires_grad_(True)
    backd = dev(back).requires_grad_(True)
    pd = dev(probs).requires_grad_(True)
    od, rd, doutd = dev(order, rows, dout)

    ko.poison(DEV, ((m, h), dtype))
    perm = moe_permute(xd, rd)
    assert torch.equal(perm.detach().cpu(), x[rows]), "permute"
    ko.poison(DEV, ((n, h), dtype))
    out = moe_unpermute(backd, pd, od, n, k)
    ko.assert_finite(out, what="unpermute")
    ko.assert_elem(out.detach().cpu(), ko.moe_unpermute(back, probs, order, n, k),
                   ko.moe_unpermute(back.abs(), probs, order, n, k),
                   "unpermute")
    ko.poison(DEV, ((m, h), dtype))
    out.backward(doutd)
    ko.assert_finite(backd.grad, pd.grad, what="unpermute bwd")
    db64, dp64 = ko.moe_unpermute_bwd(dout, back, probs, order, k)
    ko.assert_elem(backd.grad.cpu(), db64, what="unpermute dback")
    # dprobs: autograd through the pure-torch merge in fp32
    b32 = back.float()
    p32 = probs.clone().requires_grad_(True)
    full = b32.new_zeros(m, h)
    full[order] = b32 * p32.unsqueeze(-1)
    full.reshape(n, k, h).sum(1).backward(dout.float())
    assert pd.grad.dtype == F32
    ko.assert_accum(pd.grad.cpu(), p32.grad, dp64, "dprobs")

    # permute backward: the scatter-add of repeated source rows
    perm.backward(backd.detach())
    acc64 = ko.moe_permute_bwd(back, rows, n)
    if dtype == F32:
        acc32 = torch.zeros(n, h).index_add_(0, rows, back.float())
        ko.assert_accum(xd.grad.cpu(), acc32, acc64, "permute bwd")
    else:
        ko.assert_elem(xd.grad.cpu(), acc64,
                       ko.moe_permute_bwd(back.abs(), rows, n), "permute bwd")

    if m * (h // 8) > ko.GRID_ROWS * 256 and k == 1:
        sel = [0, 1, m - 2, m - 1]          # the last rows: second sweep
        idx = torch.tensor(sel, device=DEV)
        ko.assert_rows_bitwise(perm.detach(),
                               e.moe_permute(xd.detach(), rd[idx].contiguous()),
                               sel, "permute")
        # token t alone: its one slot, a problem of len(sel) tokens
        slot = torch.argsort(od)[idx]
        small = e.moe_unpermute(backd.detach()[slot].contiguous(),
                                pd.detach()[slot].contiguous(),
                                torch.arange(len(sel), device=DEV),
                                len(sel), 1)
        ko.assert_rows_bitwise(out.detach(), small, sel, "unpermute")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_moe_empty(dtype):
    """m = 0 and n = 0: no launch, well-shaped empty or zero results."""
    from hetu_galvatron_amd.ops.functional import moe_permute, moe_unpermute
    e = ext()
    h, k = 128, 2
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    x0 = torch.zeros(0, h, dtype=dtype, device=DEV)
    x5 = torch.ones(5, h, dtype=dtype, device=DEV)
    p0 = torch.zeros(0, device=DEV)
    assert moe_permute(x0, none).shape == (0, h)              # n = 0
    assert moe_permute(x5, none).shape == (0, h)              # m = 0
    assert moe_unpermute(x0, p0, none, 0, k).shape == (0, h)
    acc = e.moe_permute_bwd(x0, none, 5)
    assert acc.shape == (5, h) and bool((acc == 0).all())
    assert e.moe_permute_bwd(x0, none, 0).shape == (0, h)
    dback, dprobs = e.moe_unpermute_bwd(x0, x0, p0, none)
    assert dback.shape == (0, h) and dprobs.shape == (0,)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# grouped GEMM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("counts,K,N", ko.GG_CASES, ids=_ids)
def test_grouped_gemm_edges(counts, K, N):
    """One row, tiles of 129 / 0 / 127 rows, leading and trailing empty
    experts, every expert empty, E = 1, a second column tile, and K = 160
    (K % 32 but not % 128) through the raw forward binding."""
    from hetu_galvatron_amd.ops.functional import _gg_tiles, grouped_gemm
    e = ext()
    E, M = len(counts), sum(counts)
    a, w, dc = ko.gg_inputs(counts, K, N)
    ad, wd, dcd = dev(a, w, dc)
    c64 = ko.grouped_gemm(a, w, counts)
    c_scale = ko.grouped_gemm(a.abs(), w.abs(), counts)
    if K % 128:
        tiles, _ = _gg_tiles(counts, DEV)
        c = call(e.grouped_gemm, ad, wd, tiles, N, False,
                 outs=[((M, N), BF16)], what="grouped fwd")
        ko.assert_elem(c.cpu(), c64, c_scale, "grouped fwd (raw)")
        return
    ad.requires_grad_(True)
    wd.requires_grad_(True)
    ko.poison(DEV, ((M, N), BF16))
    c = grouped_gemm(ad, wd, counts)
    assert c.shape == (M, N)
    ko.assert_finite(c, what="grouped fwd")
    ko.assert_elem(c.detach().cpu(), c64, c_scale, "grouped fwd")
    ko.poison(DEV, ((M, K), BF16), ((E, K, N), F32))
    c.backward(dcd)
    ko.assert_finite(ad.grad, wd.grad, what="grouped bwd")
    da64, dw64 = ko.grouped_gemm_bwd(dc, a, w, counts)
    ko.assert_elem(ad.grad.cpu(), da64,
                   ko.grouped_gemm_bwd(dc.abs(), a.abs(), w.abs(), counts)[0],
                   "grouped dA")
    # dW in fp32 from the raw binding, over poisoned memory
    _, row_off = _gg_tiles(counts, DEV)
    dw = call(e.grouped_gemm_dw, ad.detach(), dcd, row_off, E,
              outs=[((E, K, N), F32)], what="grouped dW")
    dw32 = torch.zeros(E, K, N)
    s = 0
    for i, mi in enumerate(counts):
        dw32[i] = a[s:s + mi].float().T @ dc[s:s + mi].float()
        s += mi
    ko.assert_accum(dw.cpu(), dw32, dw64, "grouped dW")
    assert torch.equal(wd.grad, dw.to(BF16)), "autograd dW != raw dW"
    for i, mi in enumerate(counts):
        if mi == 0:
            assert bool((dw[i] == 0).all()), f"dW of empty expert {i}"


# ---------------------------------------------------------------------------
# empty inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_zero_rows(dtype):
    """n = 0 rows: nothing is launched (a grid of zero blocks is an invalid
    launch) and the outputs are well-shaped, dw / db zero."""
    e = ext()
    H = 264

    def z(*shape, dt=dtype):
        return torch.zeros(*shape, dtype=dt, device=DEV)

    x, w = z(0, H), z(H) + 1
    y, inv = e.rmsnorm_fwd(x, w, EPS)
    assert y.shape == (0, H) and inv.shape == (0,)
    dx, dw = e.rmsnorm_bwd(x, x, w, inv)
    assert dx.shape == (0, H) and dw.shape == (H,) and bool((dw == 0).all())
    y, mean, invstd = e.layernorm_fwd(x, w, w, EPS)
    assert y.shape == (0, H) and mean.shape == (0,) and invstd.shape == (0,)
    dx, dw, db = e.layernorm_bwd(x, x, w, mean, invstd)
    assert dx.shape == (0, H) and bool((dw == 0).all() and (db == 0).all())
    if dtype == BF16:
        y, s, inv = e.add_rmsnorm_fwd(x, x, w, EPS)
        assert y.shape == (0, H) and s.shape == (0, H) and inv.shape == (0,)
        dx, dw = e.add_rmsnorm_bwd(x, x, s, w, inv)
        assert dx.shape == (0, H) and bool((dw == 0).all())
    assert e.swiglu_fwd(z(0, 16)).shape == (0, 8)
    assert e.swiglu_bwd(z(0, 8), z(0, 16)).shape == (0, 16)
    assert e.rope_fwd(z(0, 2, 2, 64), z(0, 32, dt=F32), z(0, 32, dt=F32),
                      False).shape == (0, 2, 2, 64)
    logits, t = z(0, 40), z(0, dt=torch.long)
    gmax = e.ce_max(logits)
    se, tl = e.ce_sum_target(logits, t, gmax, 0)
    assert gmax.shape == (0,) and se.shape == (0,) and tl.shape == (0,)
    assert e.ce_bwd(logits, t, gmax, se, z(0, dt=F32), 0).shape == (0, 40)
    torch.cuda.synchronize()
    assert torch.cuda.current_stream().query()


# ---------------------------------------------------------------------------
# binding argument checks
# ---------------------------------------------------------------------------
def test_binding_checks_rope():
    e = ext()
    s, b, h, d = 6, 2, 2, 64
    x, cos, sin = dev(*ko.rope_inputs(s, b, h, d, BF16))
    with pytest.raises(RuntimeError, match="cos_t"):
        e.rope_fwd(x, cos[:s - 1], sin[:s - 1], False)        # short table
    with pytest.raises(RuntimeError, match="cos_t"):
        e.rope_fwd(x, cos[:, :d // 2 - 8], sin[:, :d // 2 - 8], False)
    with pytest.raises(RuntimeError, match="cos_t"):
        e.rope_fwd(x, cos[:, None, :], sin[:, None, :], False)  # 3-D
    with pytest.raises(RuntimeError, match="sin_t"):
        e.rope_fwd(x, cos, sin[:s - 1], False)
    with pytest.raises(RuntimeError, match="cos_t"):
        e.rope_fwd(x, cos.cpu(), sin.cpu(), False)
    with pytest.raises(RuntimeError, match="rope_fwd: x"):
        e.rope_fwd(x.half(), cos, sin, False)
    # a longer table is a prefix read: allowed, and equal to the exact one
    long_c = torch.cat([cos, cos])
    long_s = torch.cat([sin, sin])
    assert torch.equal(e.rope_fwd(x, long_c, long_s, False),
                       e.rope_fwd(x, cos, sin, False))


def test_binding_checks_swiglu():
    e = ext()
    x, dy = dev(*ko.swiglu_inputs(5, 16, BF16))
    with pytest.raises(RuntimeError, match="dy"):
        e.swiglu_bwd(dy[:4].contiguous(), x)
    with pytest.raises(RuntimeError, match="dy"):
        e.swiglu_bwd(x, x)                       # [5, 2F] instead of [5, F]
    with pytest.raises(RuntimeError, match="dy"):
        e.swiglu_bwd(dy.float(), x)
    with pytest.raises(RuntimeError, match="swiglu_fwd: x"):
        e.swiglu_fwd(x.half())
    with pytest.raises(RuntimeError, match="swiglu_fwd: x"):
        e.swiglu_fwd(x.cpu())


def test_binding_checks_norms():
    e = ext()
    x, w, b, dy = dev(*ko.norm_inputs(4, 264, BF16))
    y, inv = e.rmsnorm_fwd(x, w, EPS)
    _, mean, invstd = e.layernorm_fwd(x, w, b, EPS)
    with pytest.raises(RuntimeError, match="w must"):
        e.rmsnorm_fwd(x, w.float(), EPS)         # weight dtype != x dtype
    with pytest.raises(RuntimeError, match="w must"):
        e.rmsnorm_fwd(x.float(), w, EPS)
    with pytest.raises(RuntimeError, match="w must"):
        e.rmsnorm_fwd(x, w[:256].contiguous(), EPS)
    with pytest.raises(RuntimeError, match="w must"):
        e.rmsnorm_fwd(x, w.cpu(), EPS)
    with pytest.raises(RuntimeError, match="rmsnorm_fwd: x"):
        e.rmsnorm_fwd(x.half(), w.half(), EPS)   # fp16: never reinterpreted
    with pytest.raises(RuntimeError, match="dy must"):
        e.rmsnorm_bwd(dy[:3].contiguous(), x, w, inv)
    with pytest.raises(RuntimeError, match="dy must"):
        e.rmsnorm_bwd(dy.float(), x, w, inv)
    with pytest.raises(RuntimeError, match="w must"):
        e.rmsnorm_bwd(dy, x, w.float(), inv)
    with pytest.raises(RuntimeError, match="invrms must"):
        e.rmsnorm_bwd(dy, x, w, inv[:3])
    with pytest.raises(RuntimeError, match="b must"):
        e.layernorm_fwd(x, w, b.float(), EPS)
    with pytest.raises(RuntimeError, match="w must"):
        e.layernorm_fwd(x, w.float(), b, EPS)
    with pytest.raises(RuntimeError, match="layernorm_fwd: x"):
        e.layernorm_fwd(x.half(), w.half(), b.half(), EPS)
    with pytest.raises(RuntimeError, match="dy must"):
        e.layernorm_bwd(dy[:, :256].contiguous(), x, w, mean, invstd)
    with pytest.raises(RuntimeError, match="mean must"):
        e.layernorm_bwd(dy, x, w, mean.double(), invstd)
    with pytest.raises(RuntimeError, match="res must"):
        e.add_rmsnorm_fwd(x, x[:3].contiguous(), w, EPS)
    with pytest.raises(RuntimeError, match="bf16 only"):
        e.add_rmsnorm_fwd(x.float(), x.float(), w.float(), EPS)
    with pytest.raises(RuntimeError, match="dsum must"):
        e.add_rmsnorm_bwd(dy, dy[:3].contiguous(), x, w, inv)


def test_binding_checks_ce():
    e = ext()
    logits, target, vs, gout = ko.ce_inputs(8, 40, F32)
    ld, td, gd = dev(logits, target, gout)
    gmax = e.ce_max(ld)
    se, _ = e.ce_sum_target(ld, td, gmax, vs)
    with pytest.raises(RuntimeError, match="ce_max: logits"):
        e.ce_max(ld.half())                      # fp16: never reinterpreted
    with pytest.raises(RuntimeError, match="target must"):
        e.ce_sum_target(ld, td.int(), gmax, vs)
    with pytest.raises(RuntimeError, match="target must"):
        e.ce_sum_target(ld, td[:7], gmax, vs)
    with pytest.raises(RuntimeError, match="gmax must"):
        e.ce_sum_target(ld, td, gmax[:7], vs)
    with pytest.raises(RuntimeError, match="sumexp must"):
        e.ce_bwd(ld.clone(), td, gmax, se.double(), gd, vs)
    with pytest.raises(RuntimeError, match="grad_out must"):
        e.ce_bwd(ld.clone(), td, gmax, se, gd[:7], vs)
