"""Every lowering the engine and the Trainer can produce on the host issues the launches, arguments and read / write regions
recorded in tests/golden/plan_signatures.json (op count + SHA-256 per case; tests/plan_signature.py names the cases and
records the file).  Grouping needs the compiled library, so grouped step lists are compared on the GPU instead."""
import json
import os

import pytest

from tests.plan_signature import CASES, digest

with open(os.path.join(os.path.dirname(__file__), "golden", "plan_signatures.json")) as fh:
    GOLDEN = json.load(fh)


def test_golden_covers_every_case():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("key", sorted(CASES))
def test_launch_list_unchanged(key):
    got = digest(key)
    print(key, got)
    assert got == GOLDEN[key]
