"""The batched decode kernels against the bits of the build that still had two
chunk bodies and three merge kernels.

tools/decode_golden.py builds every case on the CPU from fixed seeds and runs
the four decode bindings and kv_append_fp8; tests/ops/decode_golden_parent.json
holds the SHA-256 digests of the raw output bytes as that build (named in the
file) wrote them.  The oracle tests beside this file allow a tolerance and
would not notice a reordered sum; these do.  A mismatch is a change of the
kernels' arithmetic, never a reason to record again.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))


def _load_golden_tool():
    spec = importlib.util.spec_from_file_location(
        "decode_golden", os.path.join(_ROOT, "tools", "decode_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


golden = _load_golden_tool()
with open(os.path.join(_HERE, "decode_golden_parent.json")) as f:
    RECORD = json.load(f)
ATTN = dict(golden.ATTN_CASES)
APPEND = dict(golden.APPEND_CASES)


def ext():
    from hetu_galvatron_amd.ops._ext import get_ext
    return get_ext(False)


def test_record_covers_every_case():
    assert len(RECORD["parent"]) == 40
    assert sorted(RECORD["digests"]) == sorted(list(ATTN) + list(APPEND))


@pytest.mark.parametrize("name", list(ATTN))
def test_attention_matches_parent_digest(name):
    o = golden.run_attn(ext(), ATTN[name], torch.device("cuda:0"))
    assert golden.digest(o) == RECORD["digests"][name], \
        f"{name}: o differs from the recorded build bit for bit"


@pytest.mark.parametrize("name", list(APPEND))
def test_append_matches_parent_digest(name):
    caches = golden.run_append(ext(), APPEND[name], torch.device("cuda:0"))
    assert golden.digest(caches) == RECORD["digests"][name], \
        f"{name}: the caches differ from the recorded build bit for bit"
