"""train_rqvae.train with dead-code revival on (REVIVE_EVERY monkeypatched; off by default): the graphed and the
eager trainer both finish, print one revive line per revival, keep finite parameters and the checkpoint keys, and
the usage counter does not break the step's capture."""
import glob
import json

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graphs", [True, False])
def test_train_rqvae_with_revival(graphs, tmp_path, device, capsys, monkeypatch):
    import numpy as np
    import train_rqvae
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    monkeypatch.setattr(train_rqvae, "REVIVE_EVERY", 4)
    L, K = 3, 256
    kw = dict(iterations=12, batch_size=64, learning_rate=0.0005, dataset=RecDataset.AMAZON, vae_input_dim=768,
              vae_n_cat_feats=0, vae_hidden_dims=[512, 256, 128], vae_embed_dim=32, vae_codebook_size=K,
              vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK, vae_n_layers=L, do_eval=False,
              save_dir_root=str(tmp_path) + "/", save_model_every=12, log_every=4, seed=3)
    np.random.seed(0)
    capsys.readouterr()
    model = train_rqvae.train(cuda_graphs=graphs, **kw)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{"iter"') and '"revived"' in l]
    assert [l["iter"] for l in lines] == [3, 7, 11]
    for l in lines:
        assert len(l["revived"]) == L and all(isinstance(n, int) and 0 <= n <= K for n in l["revived"])
        assert len(l["codebook_used"]) == L and all(0.0 <= u <= 1.0 for u in l["codebook_used"])
        assert len(l["codebook_perplexity"]) == L and all(0.0 <= p <= K + 1e-6 for p in l["codebook_perplexity"])
    run = dict(train_rqvae.LAST_RUN)
    assert run["step_mode"] == ("hipgraph" if graphs else "eager")
    if graphs:
        assert run["graphs"] == 1 and run["eager_steps"] == 1, run   # the counter did not break capture
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert model.code_usage is not None and model.code_usage.shape == (L, K)
    ckpt = sorted(glob.glob(str(tmp_path / "checkpoint_*.pt")))[-1]
    state = torch.load(ckpt, map_location="cpu", weights_only=True)
    expect = [f"encoder.mlp.{j}.weight" for j in (0, 2, 4, 6)] + [f"decoder.mlp.{j}.weight" for j in (0, 2, 4, 6)] + \
             [f"layers.{l}.embedding.weight" for l in range(L)]
    assert sorted(state["model"]) == sorted(expect)
    assert sorted(state["model"]) == sorted(model.state_dict())
