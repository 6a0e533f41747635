"""The convolution dispatch of the built library decides what tests/golden/conv_dispatch_signatures.json records: the variant of
every convolution descriptor of the pinned plans and edge cases, the argument records of their grouped launches, the groups a
batch-90 Trainer forms and the groups the library must reject (tests/conv_dispatch_signature.py names them and records the
file).  Host code only: the library must be built, no device is needed."""
import json
import os

import pytest

from facenet_amd import _lib
from tests import conv_dispatch_signature as cds

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libfacenet_hip.so is not built")

with open(os.path.join(os.path.dirname(__file__), "golden", "conv_dispatch_signatures.json")) as fh:
    GOLDEN = json.load(fh)


def test_argument_record_sizes(lib):
    assert lib.fn_conv2d_arg_bytes() == 432
    assert lib.fn_conv2d_wgrad_arg_bytes() == 208
    assert GOLDEN["arg_bytes"] == {"conv": 432, "wgrad": 208}


def test_golden_covers_every_case():
    assert sorted(GOLDEN["plans"]) == sorted(cds.PLANS)
    assert sorted(GOLDEN["edges"]) == sorted(cds.edge_descriptors())


@pytest.mark.parametrize("key", sorted(cds.PLANS))
def test_plan_dispatch_unchanged(lib, key):
    plan = cds.lowered(key)
    got = cds.plan_signature(lib, plan)
    print(key, got)
    assert got == GOLDEN["plans"][key]
    if key == "v1_train_90":
        groups, rejected = cds.plan_groups(lib, plan), cds.rejected_groups(lib, plan)
        assert sorted(groups) == sorted(GOLDEN["groups"])
        for name, sig in groups.items():
            assert sig == GOLDEN["groups"][name], name
        assert rejected == GOLDEN["rejected_groups"]


@pytest.mark.parametrize("name", sorted(cds.edge_descriptors()))
def test_edge_descriptor_dispatch_unchanged(lib, name):
    got = cds.descriptor_signature(lib, cds.edge_descriptors()[name])
    print(name, got)
    assert got == GOLDEN["edges"][name]
