"""Constrained beam decoding, host side (CPU-only): SemanticIdTokenizer.prefix_trie against a brute-force walk of
the corpus rows, its cache, and the argument contracts of generate_next_sem_id(constrained=True) / beam_expand."""
import pytest
import torch

import beam_support as bs


def _check_trie(ids):
    """Walk the trie from the root; at every node compare with the rows that share its path."""
    trie = bs.ids_tokenizer(ids).prefix_trie()
    rows = [tuple(r) for r in ids.tolist()]
    D = ids.shape[1]
    assert trie.depth == D and trie.base == int(ids.max()) + 1
    assert len(trie.tok) == D + 1 and len(trie.child_off) == D
    for p in range(D):
        assert trie.child_off[p].dtype == torch.int32 and trie.tok[p + 1].dtype == torch.int32
        assert trie.child_off[p].numel() == (1 if p == 0 else trie.tok[p].numel()) + 1
        assert int(trie.child_off[p][0]) == 0 and int(trie.child_off[p][-1]) == trie.tok[p + 1].numel()
    assert trie.leaf_item.dtype == torch.int64 and trie.leaf_item.numel() == trie.tok[D].numel() == len(set(rows))
    seen_leaves = 0
    level = [((), 0)]   # (path, node index) of the current level
    for p in range(D):
        nxt = []
        off, tok = trie.child_off[p].tolist(), trie.tok[p + 1].tolist()
        for path, node in level:
            want = sorted({r[p] for r in rows if r[:p] == path})
            got = tok[off[node]:off[node + 1]]
            assert got == want, (p, path)
            nxt += [(path + (t,), off[node] + j) for j, t in enumerate(got)]
        assert len(nxt) == len(tok), "every node of the level is some node's child"
        level = nxt
    for path, node in level:
        assert int(trie.leaf_item[node]) == rows.index(path), path   # list.index: the lowest corpus index
        seen_leaves += 1
    assert seen_leaves == len(set(rows))


def test_prefix_trie_matches_brute_force_random_corpus():
    _check_trie(bs.random_corpus())


def test_prefix_trie_matches_brute_force_five_rows():
    _check_trie(bs.FIVE)
    trie = bs.ids_tokenizer(bs.FIVE).prefix_trie()
    assert trie.tok[1].tolist() == [0, 3] and trie.child_off[0].tolist() == [0, 2]
    assert trie.tok[4].tolist() == [0, 0, 0, 1] and trie.leaf_item.tolist() == [2, 3, 0, 1]


def test_prefix_trie_cache_and_empty_corpus():
    tok = bs.ids_tokenizer(bs.FIVE)
    first = tok.prefix_trie()
    assert tok.prefix_trie() is first, "cached"
    tok.reset()
    with pytest.raises(Exception, match="empty cache"):
        tok.prefix_trie()
    with pytest.raises(Exception, match="empty cache"):
        tok.prefix_table(1)
    # a new corpus through precompute_corpus_ids (the RQ-VAE pass replaced by fixed ids: CPU-only)
    tok.cached_ids = bs.FIVE
    old = tok.prefix_trie()

    class _Out:
        sem_ids = torch.tensor([[1, 1, 1], [1, 1, 1], [2, 0, 1]])

    class _Items:
        x = torch.zeros(3, 8)

        def __len__(self):
            return 3

        def __getitem__(self, idx):
            return self

    tok.rq_vae.get_semantic_ids = lambda x: _Out
    ids = tok.precompute_corpus_ids(_Items())
    assert ids.tolist() == [[1, 1, 1, 0], [1, 1, 1, 1], [2, 0, 1, 0]]
    new = tok.prefix_trie()
    assert new is not old and new.base == 3 and new.tok[1].tolist() == [1, 2] and new.leaf_item.tolist() == [0, 1, 2]


def test_constrained_generation_argument_errors():
    from modules.model import EncoderDecoderRetrievalModel
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=4, sem_id_dim=2, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    with pytest.raises(ValueError, match="requires fused=True"):
        model.generate_next_sem_id(None, top_k=True, sample=False, constrained=True)
    model.inference_prefix_index = bs.ids_tokenizer(bs.FIVE)
    with pytest.raises(ValueError, match="sample=False"):
        model.generate_next_sem_id(None, top_k=True, fused=True, constrained=True)   # the default is sample=True
    with pytest.raises(ValueError, match="sample=False"):
        model.generate_next_sem_id(None, top_k=True, fused=True, sample=True, constrained=True)
    model.inference_prefix_index = None
    with pytest.raises(ValueError, match="inference_prefix_index"):
        model.generate_next_sem_id(None, top_k=True, fused=True, sample=False, constrained=True)
    with pytest.raises(ValueError, match="inference_prefix_index"):
        model.recommend(None)
    model.inference_prefix_index = bs.ids_tokenizer(bs.FIVE)
    model.inference_prefix_index.cached_ids = bs.FIVE[:, :1]
    with pytest.raises(ValueError, match="depth 1"):
        model.generate_next_sem_id(None, top_k=True, fused=True, sample=False, incremental=True, constrained=True)
    model.inference_prefix_index = bs.ids_tokenizer(bs.FIVE)
    with pytest.raises(ValueError, match="depth 4"):
        model.recommend(None)       # items are the leaves: the model must generate the whole path
    with pytest.raises(ValueError, match="k <= 32"):
        model.recommend(None, k=33)
    assert model.training and model.transformer.cached_enc_output is None


def test_beam_expand_refuses_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    trie = bs.ids_tokenizer(bs.FIVE).prefix_trie()
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand(torch.zeros(2, 12), 3, batch=2, child_off=trie.child_off[0], tok=trie.tok[1])
