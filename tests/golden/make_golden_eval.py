#!/usr/bin/env python3
"""Record tests/golden/topk_metrics.npz from the READ-ONLY reference's evaluate/metrics.py TopKAccumulator.

Test infrastructure only; run where the reference tree exists:

    python tests/golden/make_golden_eval.py [/root/reference]

The reference class is imported as-is from its own tree (it needs torch and einops only); nothing is copied.
The inputs are built here (planted_inputs, shared with tests/test_eval_metrics.py through the fixture) and stored
with the reference's results: the metric dict after the first accumulate call and after both.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import gen_inputs as gi  # noqa: E402


def planted_inputs(seed=77):
    """Two batches (actual (B, D), top_k (B, k, D)), D = 4. Targets draw from [0, 50) and filler beams from
    [100, 256), so the only matches are the planted ones:
      batch 1 (B = 6, k = 32): full tuples at ranks 0, 4, 5, 9, 10 (rows 0-4), row 5 unmatched except column 2
        alone at rank 7; row 3's first two columns already match at rank 2 (a prefix earlier than the full tuple);
        row 4's tuple appears again at rank 20 (the first must count);
      batch 2 (B = 4, k = 3 < max(ks)): full tuples at ranks 2 and 0, row 2's first column at rank 1, row 3 none."""
    g = gi.rng(seed)
    a1 = g.integers(0, 50, size=(6, 4)).astype(np.int64)
    t1 = g.integers(100, 256, size=(6, 32, 4)).astype(np.int64)
    for row, r in enumerate((0, 4, 5, 9, 10)):
        t1[row, r] = a1[row]
    t1[3, 2, :2] = a1[3, :2]
    t1[4, 20] = a1[4]
    t1[5, 7, 2] = a1[5, 2]
    a2 = g.integers(0, 50, size=(4, 4)).astype(np.int64)
    t2 = g.integers(100, 256, size=(4, 3, 4)).astype(np.int64)
    t2[0, 2] = a2[0]
    t2[1, 0] = a2[1]
    t2[2, 1, 0] = a2[2, 0]
    return a1, t1, a2, t2


def main():
    ref = next((a for a in sys.argv[1:] if os.path.isdir(a)), "/root/reference")
    sys.path.insert(0, ref)
    import torch
    from evaluate.metrics import TopKAccumulator
    ks = [1, 5, 10]
    a1, t1, a2, t2 = planted_inputs()
    acc = TopKAccumulator(ks=ks)
    acc.accumulate(actual=torch.from_numpy(a1), top_k=torch.from_numpy(t1))
    first = acc.reduce()
    acc.accumulate(actual=torch.from_numpy(a2), top_k=torch.from_numpy(t2))
    both = acc.reduce()
    assert list(first) == list(both)
    np.savez(os.path.join(HERE, "topk_metrics.npz"), ks=np.asarray(ks, np.int64), actual1=a1, topk1=t1, actual2=a2,
             topk2=t2, keys=np.asarray(list(both)), values_first=np.asarray(list(first.values()), np.float64),
             values_both=np.asarray(list(both.values()), np.float64))
    print({k: round(v, 4) for k, v in both.items()})


if __name__ == "__main__":
    main()
