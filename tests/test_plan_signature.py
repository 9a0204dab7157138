"""The engines' launch plans and resident memory against tests/golden/plan_signatures.json (scripts/plan_signature.py): op order, every
argument and descriptor field, buffer sharing.  Plans are built on CPU tensors under the emulator; nothing is launched.  A change that
alters a plan on purpose regenerates the fixture with ``python scripts/plan_signature.py --write``."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(ROOT, "scripts", "plan_signature.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)


@pytest.fixture(scope="module")
def recorded():
    with open(P.FIXTURE) as f:
        return json.load(f)


def test_every_configuration_is_recorded(recorded):
    assert {k.split("/")[0] for k in recorded["engines"]} == set(P.CONFIGS)
    shas = {s for e in recorded["engines"].values() for s in e["plans"].values()}
    assert shas == set(recorded["ops"])


@pytest.mark.parametrize("name", list(P.CONFIGS))
def test_plans_and_resident_bytes_are_the_recorded_ones(recorded, name):
    msgs = P.compare(P.all_signatures([name]), recorded)
    assert not msgs, "\n".join(msgs)
