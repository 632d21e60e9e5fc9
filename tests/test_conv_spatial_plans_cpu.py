"""The planners of the three spatial-convolution kernels (conv3x3_wgrad.hip, conv3x3_fwd.hip, stem_wgrad.hip) share their
raster geometry and row split (mrla_amd/csrc/conv_spatial.h).  tests/golden/conv_spatial_plans.json holds what the three
planners answered before they shared it -- every integer of a plan, the *_rows value, the code of every refused shape -- over
the grid of scripts/make_conv_spatial_plans_golden.py; the built library must answer the same.  Needs the library, no GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_conv_spatial_plans_golden as golden  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(golden.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize("entry", sorted(golden.ENTRIES))
def test_the_planner_answers_what_it_answered_before_the_code_was_shared(recorded, entry):
    from mrla_amd import _lib as L
    lib = L.load()
    shapes, want = golden.shapes(entry), recorded["entries"][entry]
    assert len(shapes) == len(want) > 700          # the file covers the grid it documents
    refused = 0
    for shape, answer in zip(shapes, want):
        assert golden.answer(lib, entry, shape, recorded["dtype"]) == answer, (entry, shape)      # (rows and plan agree: answer())
        refused += not isinstance(answer, list)
        assert isinstance(answer, list) or answer in (L.EINVAL, L.EUNSUPPORTED)
    assert 0 < refused < len(want) // 4            # refused shapes are in the grid, and are the exception
    assert os.path.getsize(golden.OUT) < 1 << 20
