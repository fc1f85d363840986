"""Stochastic beam search, host side (CPU-only): sample_items' argument contract, the op's refusal of CPU tensors, and
the fp64 reference step itself as a sampler — its first row and its ordered (first, second) pairs against the
renormalised trie distribution, by chi-square."""
import pytest
import torch

import beam_sampled_support as ss
import beam_support as bs


def test_sample_items_argument_errors():
    from modules.model import EncoderDecoderRetrievalModel
    from rqvae_hip import ops
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=4, sem_id_dim=2, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    with pytest.raises(ValueError, match="inference_prefix_index"):
        model.sample_items(None)
    model.inference_prefix_index = bs.ids_tokenizer(bs.FIVE)
    with pytest.raises(ValueError, match="depth 4"):
        model.sample_items(None)       # items are the leaves: the model must generate the whole path
    model.inference_prefix_index = bs.ids_tokenizer(ss.ROWS)
    with pytest.raises(ValueError, match=r"1 <= k and k \* num_embeddings <= 8192"):
        model.sample_items(None, k=0)
    assert ops.BEAM_MAX_N == 8192
    with pytest.raises(ValueError, match=r"k \* num_embeddings <= 8192.*k <= 2048.*k = 2049"):
        model.sample_items(None, k=2049)
    assert model.training and model.transformer.cached_enc_output is None


def test_beam_expand_sampled_refuses_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    trie = bs.ids_tokenizer(bs.FIVE).prefix_trie()
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand_sampled(torch.zeros(2, 12), 3, batch=2, child_off=trie.child_off[0], tok=trie.tok[1],
                                noise=torch.ones(2, 12))


def test_reference_step_is_a_sampler():
    r = ss.recipe()
    chi_first, chi_pair, smallest = ss.chi_squares(r["picks"], r["p"])
    failing = float((~r["ok"]).double().mean())
    print(f"chi-square first {chi_first:.2f} (< {ss.CHI2_FIRST}), pairs {chi_pair:.2f} (< {ss.CHI2_PAIR}); smallest "
          f"expected cell {smallest:.1f}; users failing the {ss.SEP} rule {100 * failing:.3f} %")
    assert smallest >= 5, "precondition: every cell is large enough for the chi-square approximation"
    assert chi_first < ss.CHI2_FIRST
    assert chi_pair < ss.CHI2_PAIR
    assert failing <= 0.01
    # rows come in perturbed order, the root's perturbed score 0 is handed down to every user's first row
    s1 = r["s1"]
    assert (s1["g"][:, 0] == 0).all() and (s1["g"][:, 1] < 0).all()
    # phi is the log of the item's probability
    item = ss.item_index(r["picks"])
    assert torch.allclose(s1["phi"], torch.log(r["p"])[item], rtol=0, atol=1e-12)
