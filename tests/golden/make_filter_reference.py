"""Writes tests/golden/filter_reference.json: what tests/clustering_reference.py (project maths back end) leaves of the filter stage
on the cases of tests/filter_cases.py -- candidates with their score bits and counts, the dropped columns with the filter that
dropped them, the picks in pick order, the picked columns, their variant types and the feature bits (or their SHA-256 where the
matrix is large), each case keyed by the SHA-256 of its input.  tests/test_gpu_filter.py reads it;
tests/test_filter_reference.py recomputes every case live and compares.

    python tests/golden/make_filter_reference.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

if __name__ == "__main__":
    import test_filter_reference as T
    out = {name: T.fixture_of(name) for name in T.F.CASES}
    with open(T.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", T.GOLDEN)
