"""CPU tests that the comparison rules of kernel_oracle.py have teeth.

For every rule and operation the fp32 `reference_ops` result must pass, on
the very inputs `test_gpu_kernel_edges.py` gives the HIP kernels, and every
mutant (the fp64 oracle with one planted defect) must miss the rule by at
least MUTANT_MARGIN times its bound.  No GPU needed.
"""
import math

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref

from . import kernel_oracle as ko

MUTANT_MARGIN = 10.0
DTYPES = [torch.bfloat16, torch.float32]
EPS = ko.NORM_EPS


def _ids(v):
    return str(v).replace("torch.", "")


def elem_ok(got, oracle, scale=None, what=""):
    ko.assert_elem(got, oracle, scale, what)


def elem_mutant(mut64, oracle, dtype, scale=None, what=""):
    r = ko.elem_excess(mut64.to(dtype), oracle, scale)
    assert r >= MUTANT_MARGIN, f"mutant passes the element rule: {what} {r}"


def accum_mutant(mut64, ref32, oracle, what=""):
    r = ko.accum_excess(mut64, ref32, oracle)
    assert r >= MUTANT_MARGIN, f"mutant passes the accum rule: {what} {r}"


# ---------------------------------------------------------------------------
# the rules themselves
# ---------------------------------------------------------------------------
def test_ulp_at():
    m = torch.tensor([0.0, 1.0, 1.5, 2.0, 0.75, 235.0], dtype=torch.float64)
    assert ko.ulp_at(m, torch.bfloat16).tolist() == \
        [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 1.0]
    assert ko.ulp_at(m, torch.float32)[1].item() == 2.0 ** -23
    # the spacing torch itself uses
    for dt in DTYPES:
        one = torch.tensor(1.0, dtype=dt)
        nxt = torch.nextafter(one.float(), torch.tensor(2.0)) \
            if dt == torch.float32 else torch.tensor(1.0 + 2.0 ** -7)
        assert float(nxt) - 1.0 == float(ko.ulp_at(m[1:2], dt))


def test_elem_rule_edges():
    o = torch.tensor([1.0, -3.0, 0.0, 100.0], dtype=torch.float64)
    assert ko.elem_excess(o.float(), o) == 0.0
    nan = o.float().clone()
    nan[2] = float("nan")
    assert ko.elem_excess(nan, o) == math.inf
    off = o.bfloat16().clone()
    off[3] = 101.0                       # 2 bf16 ulps at 100
    assert ko.elem_excess(off, o) > 1.5
    with pytest.raises(ko.RuleFailure):
        ko.assert_elem(off, o)
    # an element that should be exactly zero may not hold anything else
    stale = o.float().clone()
    stale[2] = 1e-30
    assert ko.elem_excess(stale, o) == math.inf


def test_accum_rule_edges():
    o = torch.tensor([10.0, -2.0, 0.0], dtype=torch.float64)
    ref32 = o.float()                    # an exact reference: the floor holds
    assert ko.accum_bound(ref32, o) == 32 * 2.0 ** -24 * 10.0
    assert ko.accum_excess(ref32, ref32, o) == 0.0
    bad = ref32.clone()
    bad[2] = float("nan")
    assert ko.accum_excess(bad, ref32, o) == math.inf
    with pytest.raises(ko.RuleFailure):
        ko.assert_accum(bad, ref32, o)


def test_bitwise_rule():
    big = torch.arange(40.0).reshape(10, 4)
    rows = [0, 3, 9]
    ko.assert_rows_bitwise(big, big[rows].clone(), rows)
    small = big[rows].clone()
    small[1, 2] = torch.nextafter(small[1, 2], torch.tensor(1e9))
    with pytest.raises(ko.RuleFailure, match=r"rows \[3\]"):
        ko.assert_rows_bitwise(big, small, rows)
    with pytest.raises(ko.RuleFailure):
        ko.assert_finite(torch.tensor([1.0, float("nan")]))


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------
def _norm_reference_passes(x, w, b, dy, dtype, tag):
    # rmsnorm
    y, inv = ref.rmsnorm_fwd(x, w, EPS)
    y64, inv64 = ko.rmsnorm_fwd(x, w, EPS)
    elem_ok(y, y64, what=f"rms y {tag}")
    elem_ok(inv, inv64, what=f"rms invrms {tag}")
    dx, dw = ref.rmsnorm_bwd(dy, x, w, inv)
    dx64, dw64 = ko.rmsnorm_bwd(dy, x, w, inv)
    elem_ok(dx, dx64, ko.rmsnorm_dx_scale(dy, x, w, inv), f"rms dx {tag}")
    ko.assert_accum(dw, dw, dw64, f"rms dw {tag}")
    # layernorm
    y, mean, invstd = ref.layernorm_fwd(x, w, b, EPS)
    y64, mean64, invstd64 = ko.layernorm_fwd(x, w, b, EPS)
    elem_ok(y, y64, ko.layernorm_y_scale(x, w, b, EPS), f"ln y {tag}")
    elem_ok(mean, mean64, ko.f64(x).abs().amax(-1), f"ln mean {tag}")
    elem_ok(invstd, invstd64, what=f"ln invstd {tag}")
    dx, dw, db = ref.layernorm_bwd(dy, x, w, mean, invstd)
    dx64, dw64, db64 = ko.layernorm_bwd(dy, x, w, mean, invstd)
    elem_ok(dx, dx64, ko.layernorm_dx_scale(dy, x, w, mean, invstd),
            f"ln dx {tag}")
    ko.assert_accum(dw, dw, dw64, f"ln dw {tag}")
    ko.assert_accum(db, db, db64, f"ln db {tag}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("H", ko.NORM_WIDTHS)
def test_norm_reference_passes_widths(H, dtype):
    x, w, b, dy = ko.norm_inputs(3, H, dtype)
    _norm_reference_passes(x, w, b, dy, dtype, f"n=3 H={H}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,H", ko.NORM_ROWS)
def test_norm_reference_passes_rows(n, H, dtype):
    x, w, b, dy = ko.norm_inputs(n, H, dtype)
    _norm_reference_passes(x, w, b, dy, dtype, f"n={n} H={H}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_norm_reference_passes_special_rows(dtype):
    x, w, b, dy = ko.norm_special_rows(1600, dtype)
    _norm_reference_passes(x, w, b, dy, dtype, "special rows")


def _add_rmsnorm_reference_passes(x, res, w, dy, dsum, tag):
    y64, inv64, s64 = ko.rmsnorm_fwd(x, w, EPS, res)
    s = (x.float() + res.float())
    y, inv = ref.rmsnorm_fwd(s, w.float(), EPS)
    elem_ok(y.bfloat16(), y64, what=f"add_rms y {tag}")
    elem_ok(s.bfloat16(), s64, what=f"add_rms sum {tag}")
    elem_ok(inv, inv64, what=f"add_rms invrms {tag}")
    sb = s.bfloat16()
    # the kernel adds dsum in fp32 and rounds once
    dx, dw = ref.rmsnorm_bwd(dy.float(), sb.float(), w.float(), inv)
    dx = (dx + dsum.float()).bfloat16()
    dx64, dw64 = ko.rmsnorm_bwd(dy, sb, w, inv, dsum)
    elem_ok(dx, dx64, ko.rmsnorm_dx_scale(dy, sb, w, inv, dsum),
            f"add_rms dx {tag}")
    ko.assert_accum(dw, dw, dw64, f"add_rms dw {tag}")
    # the residual stream's gradient left out of dx
    dx_mut, _ = ko.rmsnorm_bwd(dy, sb, w, inv)
    elem_mutant(dx_mut, dx64, torch.bfloat16,
                ko.rmsnorm_dx_scale(dy, sb, w, inv, dsum),
                "add_rms dx without dsum")
    return sb, inv, dw, dw64


@pytest.mark.parametrize("H", ko.NORM_WIDTHS)
def test_add_rmsnorm_reference_passes_widths(H):
    _add_rmsnorm_reference_passes(*ko.add_rmsnorm_inputs(3, H), f"H={H}")


@pytest.mark.parametrize("n,H", ko.NORM_ROWS)
def test_add_rmsnorm_reference_passes_rows(n, H):
    x, res, w, dy, dsum = ko.add_rmsnorm_inputs(n, H)
    sb, inv, dw32, dw64 = _add_rmsnorm_reference_passes(
        x, res, w, dy, dsum, f"n={n} H={H}")
    if n > ko.GRID_ROWS:
        row = ko.f64(dy) * ko.f64(sb) * ko.f64(inv).unsqueeze(-1)
        accum_mutant(row[:ko.GRID_ROWS].sum(0), dw32, dw64,
                     "add_rms dw: every block's second row lost")


def test_add_rmsnorm_reference_passes_special_rows():
    x, res, w, dy, dsum = ko.add_rmsnorm_inputs(6, 1600, special=True)
    s = x.float() + res.float()
    assert bool((s[0] == 0).all()) and bool((s[1] == 5).all())
    assert bool(((s[2:].mean(-1) - 64).abs() < 0.5).all())
    _add_rmsnorm_reference_passes(x, res, w, dy, dsum, "special rows")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,H", [(4099, 1032), (2049, 264)])
def test_norm_dw_mutants(n, H, dtype):
    """A lost, a doubled and a block's second row must all show in dw/db."""
    x, w, b, dy = ko.norm_inputs(n, H, dtype)
    _, inv = ref.rmsnorm_fwd(x, w, EPS)
    _, dw32 = ref.rmsnorm_bwd(dy, x, w, inv)
    _, dw64 = ko.rmsnorm_bwd(dy, x, w, inv)
    row = ko.f64(dy) * ko.f64(x) * ko.f64(inv).unsqueeze(-1)   # dy * xhat
    accum_mutant(dw64 - row[17], dw32, dw64, "rms dw: row 17 dropped")
    accum_mutant(dw64 + row[n - 1], dw32, dw64, "rms dw: last row twice")
    accum_mutant(row[:ko.GRID_ROWS].sum(0), dw32, dw64,
                 "rms dw: every block's second row lost")

    _, mean, invstd = ref.layernorm_fwd(x, w, b, EPS)
    _, lw32, lb32 = ref.layernorm_bwd(dy, x, w, mean, invstd)
    _, lw64, lb64 = ko.layernorm_bwd(dy, x, w, mean, invstd)
    xhat = (ko.f64(x) - ko.f64(mean).unsqueeze(-1)) \
        * ko.f64(invstd).unsqueeze(-1)
    lrow = ko.f64(dy) * xhat
    accum_mutant(lw64 - lrow[17], lw32, lw64, "ln dw: row dropped")
    accum_mutant(lw64 + lrow[n - 1], lw32, lw64, "ln dw: row twice")
    accum_mutant(lrow[:ko.GRID_ROWS].sum(0), lw32, lw64, "ln dw: 2nd rows")
    accum_mutant(lb64 - ko.f64(dy)[17], lb32, lb64, "ln db: row dropped")
    accum_mutant(lb64 + ko.f64(dy)[n - 1], lb32, lb64, "ln db: row twice")
    accum_mutant(ko.f64(dy)[:ko.GRID_ROWS].sum(0), lb32, lb64,
                 "ln db: 2nd rows")


def test_old_dw_tolerance_is_blind():
    """The rule this replaces: 3e-2*sqrt(rows) + 2e-2*max|ref| lets a
    dropped row through on the same data; the accumulation rule does not."""
    n, H = 4099, 1032
    x, w, _, dy = ko.norm_inputs(n, H, torch.bfloat16)
    _, inv = ref.rmsnorm_fwd(x, w, EPS)
    _, dw32 = ref.rmsnorm_bwd(dy, x, w, inv)
    _, dw64 = ko.rmsnorm_bwd(dy, x, w, inv)
    row = (ko.f64(dy) * ko.f64(x) * ko.f64(inv).unsqueeze(-1))[17]
    old = 3e-2 * math.sqrt(n) + 2e-2 * float(dw32.abs().max())
    assert float(row.abs().max()) < old
    assert ko.accum_excess(dw64 - row, dw32, dw64) > 100


def test_layernorm_onepass_variance_mutant():
    """var = E[x^2] - mean^2 in fp32 on rows with mean 64, std 0.05: the
    statistics and y miss the element rule; the centred reference passes."""
    H = 1600
    x, w, b, _ = ko.norm_special_rows(H, torch.float32)
    y64, mean64, invstd64 = ko.layernorm_fwd(x, w, b, EPS)
    var64 = 1.0 / invstd64 ** 2 - EPS
    var1 = ko.onepass_variance_fp32(x).double()
    rel = ((var1 - var64) / var64).abs()[2:]
    print("one-pass variance relative error on the offset rows:",
          rel.tolist())
    assert float(rel.max()) > 0.05
    invstd_mut = 1.0 / torch.sqrt(var1 + EPS)          # NaN where var1 < -eps
    y_mut = (ko.f64(x) - mean64.unsqueeze(-1)) * invstd_mut.unsqueeze(-1) \
        * ko.f64(w) + ko.f64(b)
    off = slice(2, None)
    elem_mutant(invstd_mut[off], invstd64[off], torch.float32,
                what="ln invstd, one-pass variance")
    elem_mutant(y_mut[off], y64[off], torch.float32,
                ko.layernorm_y_scale(x, w, b, EPS)[off],
                "ln y, one-pass variance")


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------
CE_CASES = [(64, V) for V in ko.CE_WIDTHS] + [ko.CE_GRID]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,V", CE_CASES)
def test_ce_reference_passes(n, V, dtype):
    logits, target, vs, gout = ko.ce_inputs(n, V, dtype)
    gmax64 = ko.ce_max(logits)
    gmax = logits.float().max(-1).values
    assert torch.equal(gmax.double(), gmax64)            # max is exact
    se, tl = ref.vocab_ce_fwd_local(logits, target, gmax, vs, vs + V)
    se64, tl64 = ko.ce_sum_target(logits, target, gmax, vs)
    ko.assert_accum(se, se, se64, f"ce sumexp V={V}")
    assert torch.equal(tl.double(), tl64)                # a pick is exact
    dl = ref.vocab_ce_bwd_local(logits, target, gmax, se, gout, vs, vs + V)
    dl64, scale = ko.ce_bwd(logits, target, gmax, se, gout, vs, True)
    elem_ok(dl, dl64, scale, f"ce dlogits V={V}")
    assert bool((dl[gout == 0] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("V", [7, 2055, 50257])
def test_ce_tail_mutants(V, dtype):
    n = 64
    logits, target, vs, gout = ko.ce_inputs(n, V, dtype)
    V8 = V & ~7
    lf = ko.f64(logits)
    gmax64 = ko.ce_max(logits)
    gmax = gmax64.float()
    se32, _ = ref.vocab_ce_fwd_local(logits, target, gmax, vs, vs + V)
    se64, tl64 = ko.ce_sum_target(logits, target, gmax, vs)
    dl64, scale = ko.ce_bwd(logits, target, gmax, se32, gout, vs, True)

    # tail columns V8..V-1 left out of max / sumexp / dlogits
    head_max = lf[:, :V8].max(-1).values if V8 else \
        torch.full((n,), -3.4e38, dtype=torch.float64)
    planted = torch.arange(n) % 4 == 0                   # max in the tail
    assert bool((head_max[planted] < gmax64[planted]).all())
    se_mut = torch.exp(lf[:, :V8] - gmax64.unsqueeze(-1)).sum(-1)
    accum_mutant(se_mut, se32, se64, "ce sumexp without the tail")
    dl_mut = dl64.clone()
    dl_mut[:, V8:] = lf[:, V8:]                          # never rewritten
    elem_mutant(dl_mut, dl64, dtype, scale, "ce dlogits without the tail")

    # a target in the tail is not found
    t_local = target - vs
    in_tail = (t_local >= V8) & (t_local < V)
    assert bool(in_tail.any())
    tl_mut = torch.where(in_tail, torch.zeros_like(tl64), tl64)
    assert not torch.equal(tl_mut, tl64)
    dl_mut = dl64.clone()
    g = ko.f64(gout)
    rows = in_tail.nonzero().flatten()
    dl_mut[rows, t_local[rows]] += g[rows]               # the -1 is missing
    elem_mutant(dl_mut, dl64, dtype, scale, "ce dlogits, tail target lost")


# ---------------------------------------------------------------------------
# swiglu / rope
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("rows,F", [(5, 8), (2052, 2056)])
def test_swiglu_reference_passes(rows, F, dtype):
    x, dy = ko.swiglu_inputs(rows, F, dtype)
    y64 = ko.swiglu_fwd(x)
    elem_ok(ref.swiglu_fwd(x), y64, ko.swiglu_scale(x), "swiglu y")
    dx64 = ko.swiglu_bwd(dy, x)
    elem_ok(ref.swiglu_bwd(dy, x), dx64, ko.swiglu_scale(x, dy), "swiglu dx")
    # gate and up swapped
    xs = torch.cat(list(x.chunk(2, -1))[::-1], -1)
    elem_mutant(ko.swiglu_fwd(xs), y64, dtype, ko.swiglu_scale(x),
                "swiglu with gate and up swapped")


ROPE_CASES = [(5, 2, 3, 16), (5, 2, 3, 64), (5, 2, 3, 128), (5, 2, 3, 256),
              (2052, 2, 32, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("s,b,h,d", ROPE_CASES)
def test_rope_reference_passes_and_mutants(s, b, h, d, dtype):
    x, cos, sin = ko.rope_inputs(s, b, h, d, dtype)
    sc = ko.rope_scale(x)
    for conj in (False, True):
        y64 = ko.rope(x, cos, sin, conj)
        elem_ok(ref.rope_apply(x, cos, sin, conj), y64, sc,
                f"rope d={d} conj={conj}")
        # the table row of the neighbouring position
        for sh in (1, -1):
            elem_mutant(ko.rope(x, cos.roll(sh, 0), sin.roll(sh, 0), conj),
                        y64, dtype, sc, f"rope cos[s{sh:+d}]")
        # second half with the wrong sign of sin
        d2 = d // 2
        mut = y64.clone()
        xf = ko.f64(x)
        sv = ko.f64(sin)[:, None, None, :] * (-1 if conj else 1)
        mut[..., d2:] = xf[..., d2:] * ko.f64(cos)[:, None, None, :] \
            - xf[..., :d2] * sv
        elem_mutant(mut, y64, dtype, sc, "rope second half, sign of sin")
    # conj is the inverse rotation (up to cos^2 + sin^2 of the fp32 tables)
    back = ko.rope(ko.rope(x, cos, sin), cos, sin, True)
    assert float((back - ko.f64(x)).abs().max()) < 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_rope_row_tables_reference_passes(dtype):
    s, b, h, d = 37, 3, 4, 64
    x, _, _ = ko.rope_inputs(s, b, h, d, dtype)
    cos, sin, pos = ko.rope_row_tables(s, b, d)
    # positions restart mid-row, at another place in every batch row
    restarts = [(pos[1:, j] < pos[:-1, j]).nonzero().flatten().tolist()
                for j in range(b)]
    assert all(len(r) == 1 and 0 < r[0] < s - 1 for r in restarts)
    assert len({r[0] for r in restarts}) == b
    y64 = ko.rope(x, cos, sin)
    elem_ok(ref.rope_apply_neox_batched(x, cos, sin), y64, ko.rope_scale(x),
            "rope per-row tables")
    # the GPU test's other inputs: k (h = 2) forward, dq through the
    # inverse rotation (the backward)
    k, _, _ = ko.rope_inputs(s, b, 2, d, dtype, seed=1)
    elem_ok(ref.rope_apply_neox_batched(k, cos, sin), ko.rope(k, cos, sin),
            ko.rope_scale(k), "rope per-row tables, k")
    dq, _, _ = ko.rope_inputs(s, b, h, d, dtype, seed=2)
    elem_ok(ref.rope_apply_neox_batched(dq, cos, -sin),
            ko.rope(dq, cos, sin, True), ko.rope_scale(dq),
            "rope per-row tables, dq")
    # every batch row reading batch row 0's table
    elem_mutant(ko.rope(x, cos[:, :1].expand(-1, b, -1),
                        sin[:, :1].expand(-1, b, -1)), y64, dtype,
                ko.rope_scale(x), "rope per-row tables ignored")


# ---------------------------------------------------------------------------
# adamw / grad_accum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hp", ko.ADAMW_HYPER, ids=["step1", "step100000"])
@pytest.mark.parametrize("g_dtype,o_dtype",
                         [(g, o) for g in DTYPES for o in DTYPES],
                         ids=lambda v: _ids(v))
@pytest.mark.parametrize("i", range(len(ko.ADAMW_TENSORS)))
def test_adamw_reference_passes(i, g_dtype, o_dtype, hp):
    n, off = ko.ADAMW_TENSORS[i]
    master, g, m, v = (t[off:] for t in
                       ko.adamw_inputs(n, g_dtype, seed=i, offset=off))
    rm, rmm, rv, rout = ko.ref_adamw(master, g, m, v, o_dtype, hp)
    om, omm, ov = ko.adamw_step(master, g, m, v, **hp)
    ko.assert_accum(rm, rm, om, "adamw master")
    ko.assert_accum(rmm, rmm, omm, "adamw m")
    ko.assert_accum(rv, rv, ov, "adamw v")
    # out is the cast of the new master: compared with that master itself
    elem_ok(rout, rm.double(), what="adamw out")
    assert torch.equal(rout, rm.to(o_dtype))


@pytest.mark.parametrize("g_dtype", DTYPES, ids=_ids)
def test_adamw_mutants(g_dtype):
    n = ko.ADAMW_SIZES[-1]
    hp = ko.ADAMW_HYPER[0]                 # step 1, wd 0.5, gscale 0.37
    master, g, m, v = (t[3:] for t in ko.adamw_inputs(n, g_dtype, offset=3))
    rm, rmm, rv, _ = ko.ref_adamw(master, g, m, v, torch.float32, hp)
    om, omm, ov = ko.adamw_step(master, g, m, v, **hp)
    ko.assert_accum(rm, rm, om, "adamw master (large)")
    b1, b2, lr, eps, wd, gs = (hp[k] for k in
                               ("beta1", "beta2", "lr", "eps", "wd", "gscale"))
    bc1, bc2 = 1 - b1 ** hp["step"], 1 - b2 ** hp["step"]
    M, G = ko.f64(master), ko.f64(g) * gs

    # no bias correction
    mut = M - lr * (omm / (torch.sqrt(ov) + eps) + wd * M)
    accum_mutant(mut, rm, om, "adamw without bias correction")
    # weight decay on the updated master instead of the old one
    p1 = M - lr * (omm / bc1) / (torch.sqrt(ov / bc2) + eps)
    accum_mutant(p1 - lr * wd * p1, rm, om, "adamw wd on the new master")
    # gscale applied after the square: v gets gscale * g^2
    g_raw = ko.f64(g)
    v_mut = b2 * ko.f64(v) + (1 - b2) * gs * g_raw * g_raw
    accum_mutant(v_mut, rv, ov, "adamw v, gscale after the square")
    mut = M - lr * ((omm / bc1) / (torch.sqrt(v_mut / bc2) + eps) + wd * M)
    accum_mutant(mut, rm, om, "adamw master, gscale after the square")
    # the denominator is eps where g = 0 and v = 0
    z = (G == 0) & (ko.f64(v) == 0)
    assert int(z.sum()) > n // 6
    mut = om.clone()
    mut[z] = (M - lr * wd * M)[z]           # as if eps were huge
    accum_mutant(mut, rm, om, "adamw: eps ignored")


@pytest.mark.parametrize("g_dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,off", ko.GRAD_ACCUM_CASES)
def test_grad_accum_reference_passes(n, off, g_dtype):
    flat, g = ko.grad_accum_inputs(n, off, g_dtype)
    want = ko.grad_accum(flat, g, off)
    got = flat.clone()
    got[off:off + n] += g.float()
    elem_ok(got, want, what="grad_accum")
    # shifted by one element
    mut = ko.grad_accum(flat, g, off + 1)
    elem_mutant(mut, want, torch.float32, what="grad_accum off by one")


# ---------------------------------------------------------------------------
# MoE / grouped GEMM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("n,h,k", ko.MOE_CASES + [(0, 128, 2)])
def test_moe_reference_passes_and_dprobs_mutant(n, h, k, dtype):
    E = 4
    x, probs, order, rows, dout, back = ko.moe_inputs(n, h, E, k, dtype)
    assert torch.equal(ko.moe_permute(x, rows), ko.f64(x[rows]))
    # the pure-torch merge, in fp32, differentiated by autograd
    b32 = back.float().requires_grad_(True)
    p32 = probs.clone().requires_grad_(True)
    full = b32.new_zeros(n * k, h)
    full[order] = b32 * p32.unsqueeze(-1)
    out = full.reshape(n, k, h).sum(1)
    out.backward(dout.float())
    out64 = ko.moe_unpermute(back, probs, order, n, k)
    elem_ok(out.detach().to(dtype), out64,
            ko.moe_unpermute(back.abs(), probs, order, n, k), "unpermute")
    db64, dp64 = ko.moe_unpermute_bwd(dout, back, probs, order, k)
    elem_ok(b32.grad.to(dtype), db64, what="unpermute dback")
    ko.assert_accum(p32.grad, p32.grad, dp64, "dprobs")
    acc64 = ko.moe_permute_bwd(back, rows, n)
    acc32 = torch.zeros(n, h).index_add_(0, rows, back.float())
    ko.assert_accum(acc32, acc32, acc64, "permute bwd scatter")
    if n == 0:
        return
    # dprobs missing one 8-wide packet of one row's dot product
    i, c = 5, (8 if h > 8 else 0)
    g = ko.f64(dout)[order // k]
    mut = dp64.clone()
    mut[i] -= (g[i, c:c + 8] * ko.f64(back)[i, c:c + 8]).sum()
    accum_mutant(mut, p32.grad, dp64, "dprobs without one packet")
    # token 0's k slots all go to one expert
    assert len({int(e) for e in (order // k == 0).nonzero().flatten()}) == k
    # one source row of the scatter lost
    mut = acc64.clone()
    mut[rows[3]] -= ko.f64(back)[3]
    accum_mutant(mut, acc32, acc64, "permute bwd: one row lost")


@pytest.mark.parametrize("counts,K,N", ko.GG_CASES,
                         ids=lambda v: _ids(v).replace(" ", ""))
def test_grouped_gemm_reference_passes(counts, K, N):
    a, w, dc = ko.gg_inputs(counts, K, N)
    c64 = ko.grouped_gemm(a, w, counts)
    da64, dw64 = ko.grouped_gemm_bwd(dc, a, w, counts)
    outs, s = [], 0
    dw32 = torch.zeros(w.shape)
    da32 = torch.zeros(a.shape)
    for e, m in enumerate(counts):
        outs.append(a[s:s + m].float() @ w[e].float())
        da32[s:s + m] = dc[s:s + m].float() @ w[e].float().T
        dw32[e] = a[s:s + m].float().T @ dc[s:s + m].float()
        s += m
    c32 = torch.cat(outs)
    elem_ok(c32.bfloat16(), c64, ko.grouped_gemm(a.abs(), w.abs(), counts),
            "grouped fwd")
    elem_ok(da32.bfloat16(), da64,
            ko.grouped_gemm_bwd(dc.abs(), a.abs(), w.abs(), counts)[0],
            "grouped dA")
    ko.assert_accum(dw32, dw32, dw64, "grouped dW")
    for e, m in enumerate(counts):
        if m == 0:
            assert bool((dw64[e] == 0).all())
    if sum(counts) > 1:
        # the last row of the last non-empty expert left out of dW
        e = max(i for i, m in enumerate(counts) if m)
        last = sum(counts[:e + 1]) - 1
        mut = dw64.clone()
        mut[e] -= torch.outer(ko.f64(a)[last], ko.f64(dc)[last])
        accum_mutant(mut, dw32, dw64, "grouped dW: one row lost")
