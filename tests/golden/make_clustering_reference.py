"""Writes tests/golden/clustering_reference.json: the outputs of tests/clustering_reference.py (project maths back end) on the
problems of tests/clustering_cases.py, floats as bit patterns.  tests/test_gpu_clustering_reference.py reads it (the Python chain
costs minutes and the GPU suite runs in one process); tests/test_clustering_reference.py recomputes every case live and compares.

    python tests/golden/make_clustering_reference.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

if __name__ == "__main__":
    import test_clustering_reference as T
    refs = T.references()
    out = dict(cases={name: T.as_fixture(refs[(name, "project")]) for name in T.NAMES},
               large_cases={name: T.as_fixture(refs[(name, "project")]) for name in T.LARGE_NAMES},
               pileups={config: T.as_pileup_fixture(T.pileup_reference(config)) for config in T.PILEUPS})
    with open(T.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", T.GOLDEN)
