"""Catalogue filters on the host: SemanticIdTokenizer.item_filter's CPU tables against a brute-force walk of the corpus
rows, and the argument refusals of the model's item_filter / filter_group keywords (no device)."""
import pytest
import torch

import beam_filter_support as fs
import beam_support as bs


def _tok(name):
    ids = fs.corpus_ids(name)
    return bs.ids_tokenizer(ids.clone(), codebook_size=int(ids.max()) + 1), ids


@pytest.mark.parametrize("name", ["five", "random", "straddle"])
def test_item_filter_tables_match_the_rows(name):
    from modules.tokenizer.semids import ItemFilter
    tok, ids = _tok(name)
    n = ids.shape[0]
    mask = fs.seeded_masks(n, 5, seed=11)
    mask[3] = False    # an all-false group
    mask[4] = True     # an all-true group
    filt = tok.item_filter(mask)
    assert isinstance(filt, ItemFilter)
    tables = fs.assert_tables(filt, ids, mask)
    trie = tok.prefix_trie()
    assert not any(t[3].any() for t in tables) and (filt.leaf_item[3] == -1).all(), "nothing allowed: no node, no item"
    assert all(t[4].all() for t in tables), "everything allowed: every node"
    assert torch.equal(filt.leaf_item[4], trie.leaf_item), "everything allowed: the trie's own leaf items"
    one = tok.item_filter(mask[1])     # (N,) is one group
    assert one.groups == 1 and fs.same_filter(one, tok.item_filter(mask[1:2]))
    assert all(torch.equal(a[0], b[1]) for a, b in zip(one.bits, filt.bits))
    assert tok.item_filter(mask) is not filt and fs.same_filter(tok.item_filter(mask), filt), "rebuilt, not cached"


def test_shared_row_reports_the_lowest_allowed_item():
    """Filtering is by item: FIVE's rows 2 and 4 are one leaf, random_corpus' rows 3, 7 and 250 another."""
    tok, ids = _tok("five")
    leaf = int(tok.trie_index().item_leaf[2])
    assert leaf == int(tok.trie_index().item_leaf[4])
    mask = torch.tensor([[1, 1, 0, 1, 1], [1, 1, 0, 1, 0], [0, 0, 1, 0, 1]], dtype=torch.bool)
    filt = tok.item_filter(mask)
    fs.assert_tables(filt, ids, mask)
    assert filt.leaf_item[:, leaf].tolist() == [4, -1, 2]
    for q in range(4):   # the shared path (0, 2, 2, 0) stays reachable while either item is allowed
        node = int(tok.trie_index().leaf_anc[q][leaf])
        assert fs.unpack(filt.bits[q], tok.trie_index().leaf_count[q].numel())[:, node].tolist() == [True, False, True]
    tok, ids = _tok("random")
    leaf = int(tok.trie_index().item_leaf[3])
    mask = torch.ones(3, 300, dtype=torch.bool)
    mask[0, 3] = False
    mask[1, [3, 7]] = False
    mask[2, [3, 7, 250]] = False
    filt = tok.item_filter(mask)
    fs.assert_tables(filt, ids, mask)
    assert filt.leaf_item[:, leaf].tolist() == [7, 250, -1]


def test_word_boundaries():
    """Levels of exactly 32, 33 and 65 nodes: nodes 31, 32, 63 and 64 each set in one group and clear in the other."""
    tok, ids = _tok("straddle")
    assert [c.numel() for c in tok.trie_index().leaf_count] == [32, 33, 65, 70]
    last = ids[:, 0] == 31
    mask = torch.stack([last, ~last, (ids[:, 0] == 30) | last])
    filt = tok.item_filter(mask)
    assert [b.shape[1] for b in filt.bits] == [1, 2, 3, 3]
    l1, l2, l3, _ = fs.assert_tables(filt, ids, mask)
    assert l1[:, 31].tolist() == [True, False, True] and l1[:, 30].tolist() == [False, True, True]
    assert l2[:, 32].tolist() == [True, False, True] and l2[:, 31].tolist() == [False, True, True]
    assert l3[:, 64].tolist() == [True, False, True] and l3[:, 63].tolist() == [False, True, True]
    assert l3[:, 32].tolist() == [False, True, False] and l3[:, 31].tolist() == [False, True, False]
    assert int(filt.bits[0][0, 0]) == -2 ** 31 and int(filt.bits[0][1, 0]) == 2 ** 31 - 1, "bit 31 is the sign bit"


def test_item_filter_refuses_bad_masks():
    tok, ids = _tok("five")
    for bad in (torch.ones(4, dtype=torch.bool), torch.ones(2, 6, dtype=torch.bool), torch.ones(5, dtype=torch.int64),
                torch.ones(1, 1, 5, dtype=torch.bool), torch.tensor(True)):
        with pytest.raises(ValueError, match="item_filter: mask must be bool"):
            tok.item_filter(bad)
    tok.reset()
    with pytest.raises(Exception, match="empty cache"):
        tok.item_filter(torch.ones(5, dtype=torch.bool))


def test_model_argument_errors():
    from data.schemas import TokenizedSeqBatch
    from modules.model import EncoderDecoderRetrievalModel
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=12, sem_id_dim=4, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    model.inference_prefix_index = tok = bs.ids_tokenizer(bs.FIVE.clone())
    one = torch.ones(5, dtype=torch.bool)
    for kw in (dict(), dict(fused=True), dict(fused=True, sample=False), dict(fused=True, incremental=True)):
        for flt in (dict(item_filter=one), dict(item_filter=tok.item_filter(one)),
                    dict(item_filter=one, filter_group=torch.zeros(3, dtype=torch.int64))):
            with pytest.raises(ValueError, match="item_filter / filter_group require constrained=True"):
                model.generate_next_sem_id(None, top_k=True, **flt, **kw)
    z = torch.zeros(3, 8, dtype=torch.int64)
    batch = TokenizedSeqBatch(user_ids=z[:, :1], sem_ids=z, sem_ids_fut=None, seq_mask=z.bool(), token_type_ids=z,
                              token_type_ids_fut=None)
    constrained = dict(top_k=True, fused=True, sample=False, constrained=True)
    two = torch.ones(2, 5, dtype=torch.bool)
    for flt in (two, tok.item_filter(two)):
        with pytest.raises(ValueError, match="item_filter has 2 groups"):
            model.generate_next_sem_id(batch, item_filter=flt, **constrained)
        with pytest.raises(ValueError, match="item_filter has 2 groups"):
            model.recommend(batch, item_filter=flt)
        with pytest.raises(ValueError, match="item_filter has 2 groups"):
            model.sample_items(batch, item_filter=flt)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3)):
        with pytest.raises(ValueError, match="filter_group must be .B,. integer with B = 3"):
            model.recommend(batch, item_filter=two, filter_group=bad)
        with pytest.raises(ValueError, match="filter_group must be .B,. integer with B = 3"):
            model.sample_items(batch, item_filter=two, filter_group=bad)
    with pytest.raises(ValueError, match="filter_group without item_filter"):
        model.recommend(batch, filter_group=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="item_filter: mask must be bool"):
        model.recommend(batch, item_filter=torch.ones(4, dtype=torch.bool))
    assert model.training and model.transformer.cached_enc_output is None


def test_filter_ops_refuse_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    tok = bs.ids_tokenizer(bs.FIVE.clone())
    idx = tok.trie_index()
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.trie_allowed_nodes(torch.ones(1, 5, dtype=torch.bool), idx.item_leaf, idx.leaf_anc,
                               [c.numel() for c in idx.leaf_count])
