"""The call order of the engine as a whole (tests/call_matrix.py): return code and full error text of every probe at every state,
against the recording taken from the library before the call state became one state machine (tools/record_call_matrix.py)."""
import json
import os

import pytest

from call_matrix import check_covers, run_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_call_matrix.json")


@pytest.mark.gpu
def test_every_probe_at_every_state_answers_as_recorded(lib, tiny_dir):
    want = json.load(open(GOLDEN))
    check_covers(want)
    got = run_matrix(tiny_dir)
    key = lambda r: (r["engine"], r["state"], r["probe"])
    assert [key(r) for r in got] == [key(r) for r in want]  # every row, none skipped, none added
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, "\n".join(f"{key(g)}: got rc {g['rc']} {g['error']!r}, recorded rc {w['rc']} {w['error']!r}" for g, w in diff)
