"""Every size query of include/hificar.h answers what it answered before the planners moved onto csrc/hificar_host_util.h's Carver:
tests/golden/workspace_sizes.json, recorded by tools/record_workspace_sizes.py from the library of the commit the file names (never from
the code under test), over batch sizes, frame counts, low-rate factors, precisions and handle kinds chosen to straddle the rounding edges.
The "host" section holds the queries that answer without a device; the "device" section those that answer 0 before finalize, need the
training state, or belong to a handle whose create call sets device state up."""

import json
import os

import pytest

from articulatory_amd import _native
from tools.record_workspace_sizes import cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")


def _compare(section, device):
    with open(GOLDEN) as f:
        want = json.load(f)[section]
    got = dict(cases(_native.load_library(), device))
    assert sorted(got) == sorted(want), "the shape table of tools/record_workspace_sizes.py and the recorded file differ: record it again from the parent"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} size queries changed, e.g. {sorted(wrong.items())[:5]} (got, recorded)"
    return want


def test_host_size_queries_answer_as_recorded():
    want = _compare("host", False)
    assert len(want) >= 1000 and sum(1 for v in want.values() if v) > len(want) // 2  # (a table of refused shapes would pin nothing)


@pytest.mark.gpu
def test_device_size_queries_answer_as_recorded():
    want = _compare("device", True)
    assert len(want) >= 500 and sum(1 for v in want.values() if v) > len(want) // 2
