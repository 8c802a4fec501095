#!/usr/bin/env python3
"""Records the return codes of njf_field_visible, njf_field_frame, njf_field_tsdf and njf_field_tsdf_sample for every case of
tests/row_entries_cases.py into tests/golden/row_entries_codes.json, from the library that NJF_HIP_LIB names:

    git archive <parent> | tar -x -C build/parent && python build/parent/__graft_entry__.py
    NJF_HIP_LIB=build/parent/neural-jacobian-field_amd/libnjf_hip.so python tests/golden/make_row_entries_codes.py

Per entry the table holds the faults by name and one letter per case -- N, S, V for NJF_E_NULL, NJF_E_SHAPE, NJF_E_VALUE --, in
the order of ``row_entries_cases.cases``: the singles in the order of the faults, then the pairs.  It is the answer of the commit
BEFORE a change of these entries' checks; tests/test_row_entries_cpu.py holds the working tree to it.  No GPU is needed: a case
that did not fail its checks is an error here, and nothing is written."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import row_entries_cases as R  # noqa: E402
from neural_jacobian_field_amd import hip  # noqa: E402

LETTERS = {-1: "N", -2: "S", -8: "V"}   # NJF_E_NULL, NJF_E_SHAPE, NJF_E_VALUE


def main():
    if "NJF_HIP_LIB" not in os.environ:
        sys.exit("name the library to record in NJF_HIP_LIB")
    lib = hip.load_library()
    table = {}
    for entry in R.ENTRIES:
        codes = {key: R.call(lib, entry, over) for key, over in R.cases(entry)}
        passed = [key for key, code in codes.items() if code not in LETTERS]
        if passed:
            sys.exit(f"{entry}: not refused: {passed[:5]}")
        table[entry] = dict(faults=[R.label(f) for f in R.ENTRIES[entry]["faults"]], codes="".join(LETTERS[c] for c in codes.values()))
        print(entry, len(table[entry]["faults"]), "faults,", len(codes), "cases", file=sys.stderr)
    with open(os.path.join(HERE, "row_entries_codes.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
