"""The 1x1-convolution GEMMs (conv1x1.hip, conv1x1_wide.hip, conv1x1_kstream.hip, conv1x1_wgrad.hip, conv1x1_f32.hip) share
their launch code, the selection of the kernel form, the row padding of the planners and the argument check of their entry
points (mrla_amd/csrc/conv1x1_lds.h, conv1x1_args of capi.hip).  tests/golden/conv1x1_plans.json holds what every plan,
row-count and *_supported query answered before they shared it -- each integer of a plan, the code of every refused shape,
dtype and bad argument -- over the grid of scripts/make_conv1x1_plans_golden.py; the built library must answer the same.
Needs the library, no GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_conv1x1_plans_golden as golden  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(golden.OUT) as f:
        return json.load(f)["queries"]


def test_the_file_covers_every_query(recorded):
    assert sorted(recorded) == sorted(golden.QUERIES)
    assert os.path.getsize(golden.OUT) < 1 << 20


@pytest.mark.parametrize("query", sorted(golden.QUERIES))
def test_the_query_answers_what_it_answered_before_the_code_was_shared(recorded, query):
    from mrla_amd import _lib as L
    lib = L.load()
    cases, want = golden.cases(query), recorded[query]
    assert len(cases) == len(want)                 # the file covers the grid it documents
    # accepted shapes, unsupported ones and bad arguments are all in the grid (the fp32 entries take no dtype: their
    # MRLA_EUNSUPPORTED answers are shapes, their MRLA_EINVAL answers extents)
    assert min(golden.kinds(want)) >= golden.FLOOR == 50, golden.kinds(want)
    for args, answer in zip(cases, want):
        assert golden.call(lib, query, args) == answer, (query, args)
