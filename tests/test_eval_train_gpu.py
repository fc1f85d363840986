"""train_decoder.train with its two evaluation passes (partial: eval loss; full: beam generation into the Hit@k
accumulator) on the synthetic Amazon set cut down to a few eval batches: the results land in LAST_RUN["eval"], and
an evaluation leaves the training run exactly as it found it."""
import glob
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_train_decoder_eval(tmp_path, device, capsys, monkeypatch):
    import numpy as np
    import data.processed as processed
    import train_decoder
    import train_rqvae
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    monkeypatch.setitem(processed.SYNTHETIC_N_USERS, RecDataset.AMAZON, 80)   # 3 eval batches of 32 (the last short)
    vae = dict(vae_input_dim=768, vae_embed_dim=32, vae_hidden_dims=[512, 256, 128], vae_codebook_size=256,
               vae_n_cat_feats=0, vae_n_layers=3)
    np.random.seed(1)
    train_rqvae.train(iterations=10, batch_size=256, dataset=RecDataset.AMAZON, do_eval=False, save_model_every=10,
                      vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK, save_dir_root=str(tmp_path / "vae") + "/",
                      **vae)
    ckpt = sorted(glob.glob(str(tmp_path / "vae" / "checkpoint_*.pt")))[-1]
    kw = dict(iterations=4, batch_size=32, learning_rate=0.0003, dataset=RecDataset.AMAZON, pretrained_rqvae_path=ckpt,
              decoder_embed_dim=64, dropout_p=0.3, attn_heads=4, attn_embed_dim=128, attn_layers=4,
              save_dir_root=str(tmp_path) + "/", save_model_every=10 ** 9, log_every=2, seed=0, **vae)

    def fresh_dropout_keys():
        """Both runs start from the same dropout keys: the host key counter (it only restarts when the torch seed
        changes) and the device-side epoch (advanced by every replayed step) outlive a train() call."""
        from rqvae_hip import ops
        ops._SEED.update(base=None, n=0)
        ops.seed_epoch_set(0)
    capsys.readouterr()
    fresh_dropout_keys()
    m = train_decoder.train(partial_eval_every=2, full_eval_every=4, **kw)
    printed = capsys.readouterr().out
    run = dict(train_decoder.LAST_RUN)
    ev = run["eval"]
    assert m.training and not m.enable_generation and m.transformer.cached_enc_output is None
    assert "tokenizer" not in "".join(n for n, _ in m.named_parameters()) and m.inference_prefix_index is not None
    assert math.isfinite(ev["eval_loss"]) and ev["eval_loss"] > 0 and ev["eval_iter"] == 3 and ev["full_eval_iter"] == 3
    keys = [f"h@{k}_{name}" for i in range(4) for name in (f"slice_:{i + 1}", f"pos_{i}") for k in (1, 5, 10)]
    assert len(keys) == 24 and all(k in ev for k in keys)
    assert all(0.0 <= ev[k] <= 1.0 for k in keys)
    for i in range(4):
        for name in (f"slice_:{i + 1}", f"pos_{i}"):
            assert ev[f"h@1_{name}"] <= ev[f"h@5_{name}"] <= ev[f"h@10_{name}"]
    assert "'h@10_slice_:4'" in printed and printed.count('"eval_loss"') == 2
    with_eval = {n: p.detach().clone() for n, p in m.named_parameters()}
    fresh_dropout_keys()
    m2 = train_decoder.train(partial_eval_every=10 ** 9, full_eval_every=10 ** 9, **kw)
    assert "eval" not in train_decoder.LAST_RUN
    assert set(run) - {"eval"} == set(train_decoder.LAST_RUN)
    for n, p in m2.named_parameters():
        assert torch.equal(p.detach(), with_eval[n]), f"{n}: an evaluation perturbed training"
