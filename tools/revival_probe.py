#!/usr/bin/env python3
"""Measurements behind DESIGN §5 'Codebook usage tracking and dead-code revival' (needs the GPU).

  overhead [rounds] [iters]   the graphed RQ-VAE trainer at the bench shape (ML-32M dims, 65,536 items a step) with
                              usage tracking off / on, alternating in one process; LAST_RUN's steady-state ms per
                              iteration of every run. Tracking on = REVIVE_EVERY beyond the run's length: the counter
                              launch is captured with the step and no revival ever runs.
  evidence [iters] [every]    the trainer at the Amazon dims (768 -> [512, 256, 128] -> 32, K 256, L 3, synthetic
                              corpus), with the k-means init (the trainer's default) and without it (uniform
                              codebooks: a collapse from the first step), each once with revival off and once every
                              `every` iterations, same seed and iterations; the trainer's own checkpoint log
                              (codebook_usage_{l}, max_id_duplicates, rqvae_entropy) and its revive lines.
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


def _train(revive_every, **kw):
    import numpy as np
    import train_rqvae
    np.random.seed(0)
    buf = io.StringIO()
    prev = train_rqvae.REVIVE_EVERY
    train_rqvae.REVIVE_EVERY = revive_every
    try:
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(buf):
            train_rqvae.train(save_dir_root=tmp + "/", **kw)
    finally:
        train_rqvae.REVIVE_EVERY = prev
    lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
    return dict(train_rqvae.LAST_RUN), lines


def overhead(rounds=3, iters=400):
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    C = bench.CFG
    kw = dict(iterations=iters, batch_size=65536, learning_rate=C["lr"], weight_decay=C["wd"], dataset=RecDataset.ML_32M,
              do_eval=False, log_every=10 ** 9, save_model_every=10 ** 9, vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK,
              commitment_weight=C["beta"], vae_input_dim=C["input_dim"], vae_embed_dim=C["D"], vae_hidden_dims=C["hidden"],
              vae_codebook_size=C["K"], vae_n_cat_feats=0, vae_n_layers=C["L"])
    _train(0, **{**kw, "iterations": 20})   # warm the process: code objects, GEMM tuning table
    for r in range(rounds):
        for name, every in (("off", 0), ("on", 10 ** 9)):
            run, _ = _train(every, **kw)
            print(json.dumps({"round": r, "tracking": name, "iter_ms": round(run["iter_ms"], 4),
                              "timed_iters": run["timed_iters"], "step_mode": run["step_mode"], "graphs": run["graphs"]}),
                  flush=True)


def evidence(iters=600, every=50):
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    kw = dict(iterations=iters, batch_size=1024, learning_rate=0.0005, weight_decay=0.01, dataset=RecDataset.AMAZON,
              vae_input_dim=768, vae_n_cat_feats=0, vae_hidden_dims=[512, 256, 128], vae_embed_dim=32,
              vae_codebook_size=256, vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK, vae_n_layers=3, do_eval=False,
              save_model_every=iters, log_every=iters, seed=3)
    for kmeans, name, ev in ((k, n, e) for k in (True, False) for n, e in (("off", 0), ("on", every))):
        _, lines = _train(ev, use_kmeans_init=kmeans, **kw)
        ckpt = [l for l in lines if "max_id_duplicates" in l]
        revs = [l for l in lines if "revived" in l]
        loss = [l for l in lines if "loss" in l]
        print(json.dumps({"kmeans_init": kmeans, "revival": name, "every": ev, "iterations": iters, "checkpoint_log": ckpt[-1] if ckpt else None,
                          "last_loss_line": loss[-1] if loss else None,
                          "revive_lines": [{"iter": l["iter"], "revived": l["revived"]} for l in revs[:4] + revs[-4:]]}), flush=True)


if __name__ == "__main__":
    from rqvae_hip import gemm_tuning
    gemm_tuning.enable()
    cmd, rest = (sys.argv[1] if len(sys.argv) > 1 else "overhead"), [int(a) for a in sys.argv[2:]]
    {"overhead": overhead, "evidence": evidence}[cmd](*rest)
