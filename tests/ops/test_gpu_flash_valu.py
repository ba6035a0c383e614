"""Flash attention: the softmax and mask paths of the block bodies.

ops/csrc/flash_attn_body.h spares VALU work per tile: the forward uses the
bare exp2 instruction, one select for rows that have seen no key, one packed
bf16 conversion per word, skips the O rescale while no running max of the
wave moves, and combines the two half-waves without LDS; dq branches once
per tile between an element loop with the mask and one without; dkv packs
its words the same way and still masks every 32-row half.  Every one of
these is meant to leave every output bit alone.  The
cases of tools/flash_valu_cases.py steer each path, through the dense (bshd
and sbhd), varlen, packed and packed-varlen entry points where the entry
point admits the case (bias, window and sq != skv are dense only):

1. dead rows: causal with sq > skv, also windowed; o == 0 and lse == -inf
   exactly on the rows that see no key;
2. underflow: keys that dominate by more than 300 (and by 126..149) in log2
   units, the running max jumping by that much between two tiles.  THE ONE
   GROUP THAT MAY DIFFER FROM THE PARENT'S BITS (a P or alpha below 2^-126 is
   a denormal from exp2f() and 0 from the bare instruction): its digests are
   not compared; outputs and gradients must be finite and within the
   reference tolerance;
3. rescale skip over four forward tiles: every row's max rises in every
   tile / is fixed by the first tile / exactly one row's rises later;
4. the mask paths of dq and dkv: sq = skv in {32, 33, 63, 64, 65, 257} causal and not,
   (65, 129) and (129, 65) with off != 0, non-causal tails, one windowed and
   one biased dense case.  None of these is left out as already held by
   tools/flash_golden.py: that list runs 4 x 4 and 4 x 1 heads, this one
   4 x 2, and it holds no varlen or packed run at all.

All groups are checked against the fp32 reference with the tolerances of
test_gpu_flash_tr.test_tails_vs_reference; groups 1, 3 and 4 are compared
bit for bit with the record the parent build wrote
(flash_golden_valu_parent.json, two identical runs of
tools/flash_valu_cases.py).
"""
import importlib.util
import json
import math
import os

import pytest
import torch

from hetu_galvatron_amd.ops import reference_ops as ref

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))


def _load_cases():
    spec = importlib.util.spec_from_file_location(
        "flash_valu_cases", os.path.join(_ROOT, "tools",
                                         "flash_valu_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = _load_cases()
RUNS = cases.runs()
RUN_IDS = [cases.run_key(n, e) for n, e in RUNS]
RECORDED = [(n, e) for n, e in RUNS if cases.recorded(n)]

with open(os.path.join(_HERE, "flash_golden_valu_parent.json")) as f:
    GOLDEN = json.load(f)


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def dev():
    return torch.device("cuda:0")


_RUNS = {}
_REFS = {}


def run(name, entry):
    """Native forward + backward of a run, once."""
    if (name, entry) not in _RUNS:
        _RUNS[name, entry] = cases.run(ext(), name, entry, dev())
    return _RUNS[name, entry]


def reference(name, inp):
    """fp32 reference of a case, once: every entry point has its inputs."""
    if name not in _REFS:
        c = cases.CASE_BY_NAME[name]
        q, k, v, dout = (inp[n].float() for n in ("q", "k", "v", "dout"))
        bias = inp["bias"].float() if inp["bias"] is not None else None
        scale = 1.0 / math.sqrt(c["d"])
        window = c.get("window")
        o, lse = ref.attention_fwd(q, k, v, c["causal"], scale, bias, window)
        grads = ref.attention_bwd(dout, q, k, v, o, lse, c["causal"], scale,
                                  bias, window)
        _REFS[name] = (o, lse) + tuple(grads)
    return _REFS[name]


def assert_close(a, b, atol, rtol=2e-2, what=""):
    """As in test_gpu_flash_tr: whole tensors, the infinities of lse must
    coincide, the bound is taken over the finite rest."""
    a = a.float().cpu()
    b = b.float().cpu()
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    inf = torch.isinf(b)
    assert torch.equal(inf, torch.isinf(a)) and \
        torch.equal(a[inf], b[inf]), f"{what}: infinities differ"
    a, b = a[~inf], b[~inf]
    if a.numel() == 0:
        return
    err = (a - b).abs().max().item()
    denom = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * denom, \
        f"{what}: max|err|={err:.4e} vs atol={atol} rtol*max={rtol * denom:.4e}"


@pytest.mark.parametrize("name,entry", RUNS, ids=RUN_IDS)
def test_vs_reference(name, entry):
    c = cases.CASE_BY_NAME[name]
    inp, out = run(name, entry)
    o_r, lse_r, *grads = reference(name, inp)
    what = cases.run_key(name, entry)
    for key, val in out.items():
        # lse may hold -inf (dead rows; assert_close matches them up)
        ok = ~torch.isnan(val) if key == "lse" else torch.isfinite(val)
        assert ok.all(), f"{what} {key}: not finite"
    assert_close(out["o"], o_r, 3e-2, what=f"{what} o")
    assert_close(out["lse"], lse_r, 2e-2, what=f"{what} lse")
    packed = entry.startswith("packed")
    for key, r in zip(("dq", "dk", "dv"), grads):
        got = out[key]
        if packed and key != "dq":
            got = cases.sum_group(got)
        assert_close(got, r, 6e-2, rtol=3e-2, what=f"{what} {key}")
    if c.get("bias"):
        assert_close(out["dbias"], grads[3], 6e-2, rtol=3e-2,
                     what=f"{what} dbias")
    if c["group"] == "dead":
        n_dead = c["sq"] - c["skv"]     # rows whose diagonal lies before key 0
        assert n_dead > 0
        assert (out["o"][:, :n_dead] == 0).all(), f"{what}: o of dead rows"
        assert (out["lse"][:, :, :n_dead] == -math.inf).all(), \
            f"{what}: lse of dead rows"
        assert torch.isfinite(out["lse"][:, :, n_dead:]).all(), \
            f"{what}: lse of live rows"


def test_parent_record_covers_every_recorded_run():
    assert sorted(GOLDEN) == sorted(cases.run_key(n, e) for n, e in RECORDED)
    left_out = {cases.CASE_BY_NAME[n]["group"] for n, e in RUNS
                if not cases.recorded(n)}
    assert left_out == {"underflow"}
    for rec in GOLDEN.values():
        assert sorted(rec) == ["dk", "dq", "dv", "lse", "o"]


@pytest.mark.parametrize("name,entry", RECORDED,
                         ids=[cases.run_key(n, e) for n, e in RECORDED])
def test_outputs_match_parent_digests(name, entry):
    _, out = run(name, entry)
    want = GOLDEN[cases.run_key(name, entry)]
    got = cases.digests(out)
    diff = [key for key in got if got[key] != want[key]]
    assert not diff and sorted(got) == sorted(want), \
        f"{name} {entry}: {diff} differ from the parent build bit for bit"
