#!/usr/bin/env python3
"""Timing behind DESIGN §5 'Beam-searched residual quantization' (needs the GPU).

For the shapes (B, D, K, L) = (65536, 64, 256, 3) — the bench's quantize shape — and (12101, 32, 256, 3) — the
Amazon corpus at the Amazon embed dim — and the widths W in {1, 4, 8, 16, 32}: the HIP op
(rqvae_hip.ops.rq_quantize_beam), the greedy kernel (ops.rq_quantize in eval mode, W-independent, timed beside every
width) and the torch composite (modules.beam_quantize.beam_quantize_torch on the device), all three in one process,
interleaved round by round, device events around each call after a warm-up, medians reported. One JSON line per
(shape, W) on stdout; `gate` says whether the HIP op is at least as fast as the composite at W = 8 (exit status 1 if
not).

    python3 tools/beam_quantize_time.py [reps] [warmup]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rq-vae-recommender_amd"))

SHAPES = ((65536, 64, 256, 3), (12101, 32, 256, 3))
WIDTHS = (1, 4, 8, 16, 32)
GATE_W = 8


def main(reps=9, warmup=3):
    import torch
    from modules.beam_quantize import beam_quantize_torch
    from rqvae_hip import ops
    if not torch.cuda.is_available():
        raise SystemExit("beam_quantize_time: no GPU (a timing needs the device)")
    dev = torch.device("cuda", 0)
    ok = True
    for B, D, K, L in SHAPES:
        g = torch.Generator().manual_seed(B + D)
        x = (torch.randn(B, D, generator=g) / D ** 0.5).to(dev)
        cbs = torch.randn(L, K, D, generator=g) / D ** 0.5
        cbs = (cbs * (0.6 ** torch.arange(L, dtype=torch.float32))[:, None, None]).to(dev)
        for W in WIDTHS:
            calls = (("hip", lambda: ops.rq_quantize_beam(x, cbs, W, with_residuals=True)),
                     ("greedy", lambda: ops.rq_quantize(x, cbs, ops.MODE_EVAL)),
                     ("torch", lambda: beam_quantize_torch(x, cbs, W)))
            for _ in range(warmup):
                for _, fn in calls:
                    fn()
            torch.cuda.synchronize()
            ev = {name: [] for name, _ in calls}
            for _ in range(reps):
                for name, fn in calls:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    ev[name].append((a, b))
                torch.cuda.synchronize()   # bounds the composite's live memory to one call
            ms = {name: [a.elapsed_time(b) for a, b in pairs] for name, pairs in ev.items()}
            hp, _ = ops.rq_quantize_beam(x, cbs, W)
            tp, _, _ = beam_quantize_torch(x, cbs, W)
            line = {"B": B, "D": D, "K": K, "L": L, "W": W, "reps": reps, "warmup": warmup,
                    "paths_equal_share": round(float((hp == tp).all(-1).all(-1).float().mean()), 4)}
            for name in ev:
                line[name + "_ms"] = round(statistics.median(ms[name]), 4)
                line[name + "_min_ms"], line[name + "_max_ms"] = round(min(ms[name]), 4), round(max(ms[name]), 4)
            if W == GATE_W:
                line["gate"] = line["hip_ms"] <= line["torch_ms"]
                ok = ok and line["gate"]
            print(json.dumps(line), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(*[int(a) for a in sys.argv[1:3]]))
