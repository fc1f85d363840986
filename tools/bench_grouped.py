#!/usr/bin/env python3
"""bench.py with the MLP chains' weight gradients grouped where the time model says so (ops.group_wgrads()): the
opt-in A/B leg of profiles/r07/group_wgrad. Arguments are bench.py's:
   python3 tools/bench_grouped.py [--dump-outputs DIR] ..."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rq-vae-recommender_amd"))
import torch  # noqa: E402,F401  (load order: torch's HIP runtime first)
from rqvae_hip import ops  # noqa: E402

sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
with ops.group_wgrads():
    runpy.run_path(sys.argv[0], run_name="__main__")
