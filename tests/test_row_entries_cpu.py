"""The return codes of the four entries that share their checks of rows and views -- njf_field_visible, njf_field_frame,
njf_field_tsdf, njf_field_tsdf_sample -- for every single fault their own CPU tests use and every pair of
two: the code of each case is the one that the commit before the shared checks returned, recorded by
tests/golden/make_row_entries_codes.py into tests/golden/row_entries_codes.json.  These entries judge in classes (every
NJF_E_NULL, then every NJF_E_VALUE, then every NJF_E_SHAPE), and a pair of faults of two classes shows the order.  No GPU: every
call carries a fault and returns before a launch."""
import json
import os

import pytest

import row_entries_cases as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_entries_codes.json")
LETTERS = {-1: "N", -2: "S", -8: "V"}   # NJF_E_NULL, NJF_E_SHAPE, NJF_E_VALUE


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    return hip.load_library()


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("entry", sorted(R.ENTRIES))
def test_every_single_fault_and_every_pair_returns_the_recorded_code(lib, table, entry):
    faults, recorded = R.ENTRIES[entry]["faults"], table[entry]
    todo = list(R.cases(entry))
    # the table was recorded for these faults, in this order: no case left out, none without an answer
    assert [R.label(f) for f in faults] == recorded["faults"] and len(set(recorded["faults"])) == len(faults)
    assert len(todo) == len(recorded["codes"]) > len(faults) and [key for key, _ in todo[:len(faults)]] == recorded["faults"]
    assert set(recorded["codes"]) == set(LETTERS.values())              # every class occurs, and nothing but a refusal
    wrong = {}
    for (key, over), letter in zip(todo, recorded["codes"]):
        code = R.call(lib, entry, over)
        if LETTERS.get(code) != letter:
            wrong[key] = (code, letter)
    assert not wrong, (len(wrong), list(wrong.items())[:10])
