"""Every lowering the engine and the Trainer can produce on the host issues the launches, arguments and read / write regions
recorded in tests/golden/plan_signatures.json (op count + SHA-256 per case; tests/plan_signature.py names the cases and
records the file).  Grouping needs the compiled library, so grouped step lists are compared on the GPU instead."""
import functools
import json
import os

import pytest

from tests.plan_signature import CASES, digest, lowered

with open(os.path.join(os.path.dirname(__file__), "golden", "plan_signatures.json")) as fh:
    GOLDEN = json.load(fh)


def test_golden_covers_every_case():
    assert sorted(GOLDEN) == sorted(CASES)


_lowered = functools.lru_cache(maxsize=None)(lowered)      # each case is lowered once for both tests


@pytest.mark.parametrize("key", sorted(CASES))
def test_launch_list_unchanged(key):
    got = digest(key, _lowered(key))
    print(key, got)
    assert got == GOLDEN[key]


def _has_unknown_role(node):
    """Does a launch hold a pointer argument ("ptr", "?"), or a read / write region whose base is "?"?"""
    if not isinstance(node, (list, tuple)):
        return False
    if tuple(node[:2]) == ("ptr", "?") or (len(node) == 4 and node[0] == "?"):
        return True
    return any(_has_unknown_role(v) for v in node)


def test_every_pointer_has_a_role():
    """A pointer or region that lies in no tensor the signature knows is pinned as "somewhere": a change to the launch that
    uses it would go unseen.  Every tensor a launch points at has a name (the trainer's own: ``Trainer.tensors``)."""
    unknown = {}
    for key in sorted(CASES):
        sig = _lowered(key)
        bad = [row[0] for row in (sig["launches"] if isinstance(sig, dict) else sig) if _has_unknown_role(row)]
        if bad:
            unknown[key] = bad
    print(unknown)
    assert not unknown
