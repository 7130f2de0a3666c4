"""The launch sequence of a forward call, pinned: which launches it makes, in issue order, with the
algorithmic flops and bytes the per-launch profiler records for each (spe_model_profile_*).  The tolerance
tests pass in most modes with a lost activation-scale slot, a swapped branch or a fused path that fell back
to its separate launches; this one does not.  Flops and bytes are products of integers held in doubles, so
the comparison with tests/golden/launch_tables.json (scripts/gen_golden_launch_tables.py) is exact."""
import json
import os

import pytest

from conftest import GOLDEN
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_tables():
    with open(os.path.join(GOLDEN, "launch_tables.json")) as f:
        return json.load(f)


def test_fixture_holds_every_case(golden_tables):
    assert sorted(golden_tables) == sorted(helpers.launch_table_cases())


@pytest.mark.parametrize("name", helpers.launch_table_cases())
def test_launch_table_matches_golden(gpu_device, golden_tables, name):
    got = helpers.run_launch_table_case(name, gpu_device)
    assert len(got) > 0
    assert got == golden_tables[name]
    if name.endswith("-split"):
        # encode then decode as two calls make the launches of the single call
        assert got == golden_tables[name[:-len("-split")]]
    if name.endswith("-aux"):
        # a decoder_norm + heads pair per decoder layer but the last (the golden's name ends in _l<layers>)
        layers = int(name.split("-")[0].rsplit("_l", 1)[1])
        assert len(got) == len(golden_tables[name[:-len("-aux")]]) + 2 * (layers - 1)
