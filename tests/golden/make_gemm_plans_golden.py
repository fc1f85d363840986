#!/usr/bin/env python3
"""Records what rq_gemm_bf16x3_plan / _pair_plan / _group_plan / _workspace return over the grid of
tests/gemm_plan_support.py as tests/golden/gemm_plans.json. Host-only (no GPU: the planner then assumes 256 CUs, an
MI355X). Generated ONCE from the library of the commit before csrc/gemm_plan.h existed
(RQVAE_HIP_LIB=<that build> python tests/golden/make_gemm_plans_golden.py), so the file pins the plans the header has to
reproduce; regenerate it only when a change means to alter a plan. Layout: gemm_plan_support.record."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gemm_plan_support as G  # noqa: E402


def main():
    default = os.path.join(HERE, "..", "..", "rq-vae-recommender_amd", "rqvae_hip", "librqvae_hip.so")
    out = G.record(ctypes.CDLL(os.environ.get("RQVAE_HIP_LIB", default)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gemm_plans.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(out['shapes'])} shapes, {len(out['tables'])} tables, {len(out['rows'])} rows, "
          f"{len(out['pair_rows'])} pair rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
