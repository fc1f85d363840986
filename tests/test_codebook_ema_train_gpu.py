"""train_rqvae.train with EMA-maintained codebooks (CODEBOOK_EMA_DECAY monkeypatched; off by default): the graphed and
the eager trainer finish with one captured graph, leave the codebooks to the EMA rule, write the "codebook_ema"
checkpoint key beside unchanged model keys, resume from it, and revive by the decayed usage."""
import glob
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

L, K = 3, 256


def _kw(tmp_path, **over):
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    kw = dict(iterations=12, batch_size=512, learning_rate=0.0005, dataset=RecDataset.AMAZON, vae_input_dim=768,
              vae_n_cat_feats=0, vae_hidden_dims=[512, 256, 128], vae_embed_dim=32, vae_codebook_size=K,
              vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK, vae_n_layers=L, do_eval=False,
              save_dir_root=str(tmp_path) + "/", save_model_every=12, log_every=4, seed=3)
    kw.update(over)
    return kw


@pytest.mark.parametrize("graphs", [True, False])
def test_train_rqvae_with_ema_codebooks(graphs, tmp_path, device, capsys, monkeypatch):
    import numpy as np
    import train_rqvae
    monkeypatch.setattr(train_rqvae, "CODEBOOK_EMA_DECAY", 0.9)
    monkeypatch.setattr(train_rqvae, "REVIVE_EVERY", 4)
    monkeypatch.setattr(train_rqvae, "REVIVE_EMA_MIN_COUNT", 0.5)
    np.random.seed(0)
    capsys.readouterr()
    model = train_rqvae.train(cuda_graphs=graphs, **_kw(tmp_path))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{"iter"') and '"revived"' in l]
    assert [l["iter"] for l in lines] == [3, 7, 11]
    assert all(len(l["revived"]) == L and all(0 <= n <= K for n in l["revived"]) for l in lines)
    run = dict(train_rqvae.LAST_RUN)
    assert run["step_mode"] == ("hipgraph" if graphs else "eager")
    if graphs:
        assert run["graphs"] == 1 and run["eager_steps"] == 1, run   # the statistics did not break capture
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert model.code_usage is None   # the decayed usage N stands in for the window counters
    assert not any(l.embedding.weight.requires_grad or l.embedding.weight.grad is not None for l in model.layers)
    e = model.ema
    assert e["decay"] == 0.9 and not e["n"].any() and not e["s"].any()   # every step ended with its update
    assert torch.isfinite(e["N"]).all() and bool((e["N"] >= 0).all()) and torch.isfinite(e["S"]).all()
    # 12 updates of N' = 0.9 N + 0.1 n from N = 1 (re-seated codes restart at 1): a level's N sums to about its rows
    assert bool((e["N"].sum(1) > 0.5 * 512 * (1 - 0.9 ** 12)).all())
    ckpt = sorted(glob.glob(str(tmp_path / "checkpoint_*.pt")))[-1]
    state = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert sorted(state) == ["codebook_ema", "iter", "model", "model_config", "optimizer"]
    assert sorted(state["model"]) == sorted(model.state_dict())
    assert not any("ema" in k or "code_usage" in k for k in state["model"])
    assert sorted(state["codebook_ema"]) == ["N", "S", "decay", "eps"]
    # written after iteration 11; the loop runs iterations + 1 times, so the live state is one update further
    cN, cS = state["codebook_ema"]["N"], state["codebook_ema"]["S"]
    assert cN.shape == (L, K) and cS.shape == (L, K, 32) and cN.dtype == cS.dtype == torch.float32
    assert torch.isfinite(cN).all() and torch.isfinite(cS).all() and not bool((cN == 1).all())
    assert state["codebook_ema"]["decay"] == 0.9 and state["codebook_ema"]["eps"] == 1e-5
    if graphs:   # resume: the EMA state comes back with the weights
        monkeypatch.setattr(train_rqvae, "REVIVE_EVERY", 0)
        m2 = train_rqvae.train(cuda_graphs=False, **_kw(tmp_path, iterations=0, pretrained_rqvae_path=ckpt,
                                                        save_model_every=10 ** 9))
        assert m2.ema is not None and m2.ema["decay"] == 0.9
        assert torch.isfinite(m2.ema["N"]).all() and not torch.equal(m2.ema["N"].cpu(), cN)   # one step moved it
        # that step started from the checkpoint's state: N' = 0.9 N + 0.1 n with 512 rows per level
        assert torch.allclose(m2.ema["N"].sum(1).cpu(), 0.9 * cN.sum(1) + 0.1 * 512, rtol=1e-4)


def test_default_run_has_no_ema_state(tmp_path, device, capsys):
    import numpy as np
    import train_rqvae
    assert train_rqvae.CODEBOOK_EMA_DECAY == 0
    np.random.seed(0)
    model = train_rqvae.train(cuda_graphs=True, **_kw(tmp_path, iterations=4, save_model_every=4))
    capsys.readouterr()
    assert model.ema is None and all(l.embedding.weight.requires_grad for l in model.layers)
    state = torch.load(sorted(glob.glob(str(tmp_path / "checkpoint_*.pt")))[-1], map_location="cpu", weights_only=True)
    assert sorted(state) == ["iter", "model", "model_config", "optimizer"]
    assert len(state["optimizer"]["state"]) == len(list(model.parameters()))   # AdamW still trains the codebooks
