#!/usr/bin/env python3
"""Records varlen_attn_{fwd,bwd}_ws_elems over the dispatch grid of tests/test_attn_plan_host.py as
tests/golden/attn_ws_elems.json. Host-only (no GPU). Generated ONCE from the library of the commit before the
dispatch plan existed (RQVAE_HIP_LIB=<that build> python tests/golden/make_attn_ws_golden.py), so the file pins
the sizes the plan has to reproduce; regenerate it only when a change means to alter a workspace size.

Layout (deduplicated): for every (hd, causal, B, H, flags) one table of len(lens) row ids, by max_q; a row holds,
for every max_k in lens, the triple (fwd, bwd with Tk = -1, bwd with Tk = B * max_k), flattened. Tq = B * max_q."""
import ctypes
import json
import os
import sys

LENS = [1, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 256, 257, 801]
HDS = [16, 32, 64, 128]
BH = [[1, 2], [3, 2], [8, 6], [64, 6], [4097, 1]]
# 0, NO_DMA, TWO_PASS, NO_DMA|TWO_PASS, NO_SPLIT, SPLIT_BF16, FEWQ_WG, LPT_SHORT, LPT_SHORT|ORDER_GIVEN, QSPLIT(1), QSPLIT(4)
FLAGS = [0, 1, 2, 3, 4, 8, 16, 32, 32 | 64, 1 << 8, 4 << 8]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    default = os.path.join(here, "..", "..", "rq-vae-recommender_amd", "rqvae_hip", "librqvae_hip.so")
    lib = ctypes.CDLL(os.environ.get("RQVAE_HIP_LIB", default))
    i64, n = ctypes.c_int64, ctypes.c_int64()
    fwd, bwd = lib.varlen_attn_fwd_ws_elems, lib.varlen_attn_bwd_ws_elems
    fwd.argtypes = [i64] * 6 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    bwd.argtypes = [i64] * 7 + [ctypes.c_int, ctypes.c_void_p]

    def size(fn, *args):
        assert fn(*args, ctypes.byref(n)) == 0, args
        return n.value

    rows, row_id, tables = [], {}, {}
    for hd in HDS:
        for causal in (0, 1):
            for B, H in BH:
                for fl in FLAGS:
                    table = []
                    for mq in LENS:
                        row = []
                        for mk in LENS:
                            row += [size(fwd, B, H, hd, mq, mk, B * mq, causal, fl),
                                    size(bwd, B, H, hd, mq, mk, B * mq, -1, fl),
                                    size(bwd, B, H, hd, mq, mk, B * mq, B * mk, fl)]
                        key = tuple(row)
                        if key not in row_id:
                            row_id[key] = len(rows)
                            rows.append(row)
                        table.append(row_id[key])
                    tables[f"{hd},{causal},{B},{H},{fl}"] = table
    out = {"lens": LENS, "hds": HDS, "bh": BH, "flags": FLAGS, "rows": rows, "tables": tables}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "attn_ws_elems.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(tables)} tables, {len(rows)} unique rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
