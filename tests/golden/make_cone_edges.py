"""Writes tests/golden/cone_edges.npz: the extended-precision references of tests/cone_cases.py (needs mpmath) and the Exp allowances measured from the
oracle's restatement.  The inputs are not stored: cone_cases.py regenerates them from their seeds.

    python tests/golden/make_cone_edges.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "oracle")]

import cone_cases  # noqa: E402
import fos_oracle  # noqa: E402

if __name__ == "__main__":
    data = cone_cases.compute_fixture(fos_oracle)
    np.savez_compressed(cone_cases.FIXTURE, **data)
    print("%s: %d bytes; Exp allowance (benign class) %.3e" % (cone_cases.FIXTURE.name, cone_cases.FIXTURE.stat().st_size, data["exp_allowance_benign"]))
