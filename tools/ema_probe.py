#!/usr/bin/env python3
"""Measurements behind DESIGN §5 'EMA-maintained codebooks' (needs the GPU).

  overhead [rounds] [iters]        the graphed RQ-VAE trainer at the bench shape (ML-32M dims, 65,536 items a step)
                                   with CODEBOOK_EMA_DECAY 0 / 0.99, alternating in one process; LAST_RUN's
                                   steady-state ms per iteration of every run. On = the two statistics launches captured
                                   with the step plus the eager update after the optimiser step.
  kernels [iters]                  the same trainer with EMA on, for `rocprofv3 --kernel-trace --stats -- python
                                   tools/ema_probe.py kernels`: the device time of the ema_* kernels and of the
                                   codebook-gradient launches (rq_cb_chunk_kernel, rq_cb_chunk_reduce_kernel at this
                                   shape) that EMA makes redundant but the backward still runs.
  evidence [iters] [every] [min]   the rows of DESIGN §5's collapse table (Amazon dims 768 -> [512, 256, 128] -> 32,
                                   K 256, L 3, synthetic corpus, batch 1,024, seed 3; k-means init on / off) with
                                   CODEBOOK_EMA_DECAY = 0.99, without revival and with REVIVE_EVERY = `every` and
                                   REVIVE_EMA_MIN_COUNT = `min` / 100 (default 50: N < 0.5); the trainer's own checkpoint
                                   log and its revive lines.
One JSON line per run on stdout.
"""
import contextlib
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on sys.path)


def _train(decay, revive_every=0, ema_min_count=None, **kw):
    import numpy as np
    import train_rqvae
    np.random.seed(0)
    buf = io.StringIO()
    prev = (train_rqvae.CODEBOOK_EMA_DECAY, train_rqvae.REVIVE_EVERY, train_rqvae.REVIVE_EMA_MIN_COUNT)
    train_rqvae.CODEBOOK_EMA_DECAY, train_rqvae.REVIVE_EVERY, train_rqvae.REVIVE_EMA_MIN_COUNT = \
        decay, revive_every, ema_min_count
    try:
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(buf):
            train_rqvae.train(save_dir_root=tmp + "/", **kw)
    finally:
        train_rqvae.CODEBOOK_EMA_DECAY, train_rqvae.REVIVE_EVERY, train_rqvae.REVIVE_EMA_MIN_COUNT = prev
    lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
    return dict(train_rqvae.LAST_RUN), lines


def _bench_shape(iters):
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    C = bench.CFG
    return dict(iterations=iters, batch_size=65536, learning_rate=C["lr"], weight_decay=C["wd"], dataset=RecDataset.ML_32M,
                do_eval=False, log_every=10 ** 9, save_model_every=10 ** 9,
                vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK, commitment_weight=C["beta"],
                vae_input_dim=C["input_dim"], vae_embed_dim=C["D"], vae_hidden_dims=C["hidden"],
                vae_codebook_size=C["K"], vae_n_cat_feats=0, vae_n_layers=C["L"])


def overhead(rounds=3, iters=400):
    kw = _bench_shape(iters)
    _train(0, **{**kw, "iterations": 20})   # warm the process: code objects, GEMM tuning table
    _train(0.99, **{**kw, "iterations": 20})
    for r in range(rounds):
        for name, decay in (("off", 0), ("on", 0.99)):
            run, _ = _train(decay, **kw)
            print(json.dumps({"round": r, "ema": name, "iter_ms": round(run["iter_ms"], 4),
                              "timed_iters": run["timed_iters"], "step_mode": run["step_mode"], "graphs": run["graphs"]}),
                  flush=True)


def kernels(iters=60):
    run, _ = _train(0.99, **_bench_shape(iters))
    print(json.dumps({"ema": "on", "iters": iters, "iter_ms_under_profiler": round(run["iter_ms"], 4),
                      "graphs": run["graphs"]}), flush=True)


def evidence(iters=3000, every=100, min_count_pct=50):
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    kw = dict(iterations=iters, batch_size=1024, learning_rate=0.0005, weight_decay=0.01, dataset=RecDataset.AMAZON,
              vae_input_dim=768, vae_n_cat_feats=0, vae_hidden_dims=[512, 256, 128], vae_embed_dim=32,
              vae_codebook_size=256, vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK, vae_n_layers=3, do_eval=False,
              save_model_every=iters, log_every=iters, seed=3)
    for kmeans, name, ev in ((k, n, e) for k in (True, False) for n, e in (("off", 0), ("on", every))):
        _, lines = _train(0.99, ev, min_count_pct / 100.0 if ev else None, use_kmeans_init=kmeans, **kw)
        ckpt = [l for l in lines if "max_id_duplicates" in l]
        revs = [l for l in lines if "revived" in l]
        loss = [l for l in lines if "loss" in l]
        print(json.dumps({"kmeans_init": kmeans, "ema_decay": 0.99, "revival": name, "every": ev,
                          "ema_min_count": min_count_pct / 100.0 if ev else None, "iterations": iters,
                          "checkpoint_log": ckpt[-1] if ckpt else None, "last_loss_line": loss[-1] if loss else None,
                          "revive_lines": [{"iter": l["iter"], "revived": l["revived"]} for l in revs[:4] + revs[-4:]]}),
              flush=True)


if __name__ == "__main__":
    from rqvae_hip import gemm_tuning
    gemm_tuning.enable()
    cmd, rest = (sys.argv[1] if len(sys.argv) > 1 else "overhead"), [int(a) for a in sys.argv[2:]]
    {"overhead": overhead, "kernels": kernels, "evidence": evidence}[cmd](*rest)
