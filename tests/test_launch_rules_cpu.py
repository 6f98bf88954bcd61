"""CPU: what the host-side launch rules (csrc/mgp_launch.h: the LDS of a CU, the largest k that fits, the capacity of
the slab kernels) decide without a launch -- the neighbour-count limits and the recommended workspace sizes -- against
tests/golden/launch_limits.json, read from the build BEFORE the rules moved into that header.  No HIP call is made."""

import json
import os

import pytest

from muygpys_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_limits.json")
ES = (4, 8)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _key(*v):
    return ",".join(str(x) for x in v)


@pytest.mark.parametrize("es", ES)
@pytest.mark.parametrize("R", [1, 2, 4, 16])
def test_max_nn_count(golden, es, R):
    assert _lib.load().mgp_max_nn_count(es, R) == golden["max_nn_count"][_key(es, R)]


@pytest.mark.parametrize("es", ES)
def test_max_nn_count_backward(golden, es):
    assert _lib.load().mgp_max_nn_count_backward(es) == golden["max_nn_count_backward"][_key(es)]


@pytest.mark.parametrize("es", ES)
@pytest.mark.parametrize("in_count", [2, 3])
def test_shear_max_nn_count(golden, es, in_count):
    assert _lib.load().mgp_shear_max_nn_count(es, in_count) == golden["shear_max_nn_count"][_key(es, in_count)]


@pytest.mark.parametrize("es", ES)
@pytest.mark.parametrize("k,R,b", [(200, 1, 1), (200, 1, 10**6), (1022, 1, 300)])
def test_large_workspace_bytes(golden, es, k, R, b):
    assert _lib.load().mgp_large_workspace_bytes(es, k, R, b) == golden["large_workspace_bytes"][_key(es, k, R, b)]


@pytest.mark.parametrize("es", ES)
@pytest.mark.parametrize("k", [200, 1022])
@pytest.mark.parametrize("b", [1, 300])
def test_backward_large_workspace_bytes(golden, es, k, b):
    assert _lib.load().mgp_backward_large_workspace_bytes(es, k, b) == golden["backward_large_workspace_bytes"][_key(es, k, b)]
