#!/usr/bin/env python3
"""Records the reference's LineIterator (through oracle/_ref/libsfw_ref.so, built by oracle/Makefile where the reference
tree is present) on the segments tests/test_oracle_kat.py checks, as line_iterator.npz: pure data, so that the oracle's
Bresenham restatement is pinned against the real reference code wherever the tests run.

Per segment: `ends` (x0, y0, x1, y1), `lengths` (cells visited), `first` (first cell); `steps` holds every later cell as
the step from the previous one, coded 3 * (dx + 1) + (dy + 1).

Run from the repo root after build():  python tests/golden/reference/make_line_iterator.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import sfw_oracle  # noqa: E402
from test_oracle_kat import line_iterator_cases  # noqa: E402

if __name__ == "__main__":
    if sfw_oracle.ref_lib() is None:
        raise SystemExit("oracle/_ref/libsfw_ref.so is missing: build() it where the reference tree is present")
    cases = line_iterator_cases()
    cells = [sfw_oracle.line_cells(*e, use_ref=True) for e in cases]
    steps = np.concatenate([np.diff(c, axis=0) for c in cells])
    assert np.abs(steps).max() <= 1
    np.savez_compressed(os.path.join(HERE, "line_iterator.npz"), ends=np.array(cases, dtype=np.int32),
                        lengths=np.array([len(c) for c in cells], dtype=np.int32),
                        first=np.array([c[0] for c in cells], dtype=np.int32),
                        steps=(3 * (steps[:, 0] + 1) + steps[:, 1] + 1).astype(np.int8))
