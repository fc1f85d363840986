"""Per-item score bias without a device: SemanticIdTokenizer.item_bias on CPU tensors (the plain-torch tables) against
the brute-force walk of the corpus rows, bit for bit; the argument errors of item_bias and recommend; the three new C
entry points' refusals through the typed library (argument checks run on the host)."""
import ctypes

import pytest
import torch

import beam_support as bs
import bias_support as bi


def _tok(name):
    ids = bi.table_ids(name)
    return bs.ids_tokenizer(ids.clone()), bs.Corpus(ids)


@pytest.mark.parametrize("name", bi.TABLE_CORPORA)
def test_item_bias_tables_match_the_rows(name):
    from modules.tokenizer.semids import ItemBias
    tok, corpus = _tok(name)
    bias = bi.awkward_bias(corpus.ids)
    assert bias[0].isnan().any() and (bias[0] == float("inf")).any() and (bias[0] == bi.NINF).any()
    assert any(x == 0.0 and str(x) == "-0.0" for x in bias[0].tolist()) and (bias[1] == bi.NINF).all()
    got = tok.item_bias(bias)
    assert isinstance(got, ItemBias) and got.groups == 3
    upper, leaf_item = bi.brute_tables(corpus, bias)
    bi.assert_tables(got, upper, leaf_item)
    assert all(torch.isneginf(u[1]).all() for u in got.upper) and (got.leaf_item[1] == -1).all(), "the all -inf row"
    assert not any(u.isnan().any() or (u == float("inf")).any() for u in got.upper), "NaN and +inf are -inf"
    assert not any((bi.bits_of(u) == -2 ** 31).any() for u in got.upper), "-0.0 is +0.0"
    one = tok.item_bias(bias[2])   # (N,): one group
    bi.assert_tables(one, [u[2:3] for u in upper], leaf_item[2:3], "1-D: ")
    # the last level's bound is the chosen item's own (cleaned) bias
    for g in (0, 2):
        live = got.leaf_item[g] >= 0
        want = torch.tensor([bi.clean(x) for x in bias[g][got.leaf_item[g][live]].tolist()])
        assert torch.equal(bi.bits_of(got.upper[-1][g][live]), bi.bits_of(want))


def test_shared_row_reports_the_max_bias_item_then_the_lowest():
    """random_corpus' rows 3, 7 and 250 are one leaf: items 7 and 250 tie at the max, above item 3."""
    tok, corpus = _tok("random")
    bias = bi.awkward_bias(corpus.ids)
    assert float(bias[0, 3]) < float(bias[0, 7]) == float(bias[0, 250])
    leaf = int(tok.trie_index().item_leaf[3])
    assert leaf == int(tok.trie_index().item_leaf[7]) == int(tok.trie_index().item_leaf[250])
    got = tok.item_bias(bias)
    assert int(got.leaf_item[0, leaf]) == 7 and float(got.upper[-1][0, leaf]) == 7.5
    flat = tok.item_bias(torch.zeros(300))
    assert int(flat.leaf_item[0, leaf]) == 3, "equal biases: the lowest index, the trie's own leaf_item"
    assert torch.equal(flat.leaf_item[0], tok.prefix_trie().leaf_item)
    hidden = torch.zeros(300)
    hidden[[3, 7]] = bi.NINF
    assert int(tok.item_bias(hidden).leaf_item[0, leaf]) == 250


def test_item_bias_refuses_bad_tables():
    tok, _ = _tok("c5")
    for bad in (torch.zeros(4), torch.zeros(2, 6), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.bool),
                torch.zeros(1, 1, 5), torch.tensor(0.0)):
        with pytest.raises(ValueError, match="item_bias: bias must be float32"):
            tok.item_bias(bad)
    assert tok.item_bias(torch.zeros(0, 5)).groups == 0


def test_model_argument_errors():
    from data.schemas import TokenizedSeqBatch
    from modules.model import EncoderDecoderRetrievalModel
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=12, sem_id_dim=4, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    model.inference_prefix_index = tok = bs.ids_tokenizer(bs.FIVE.clone())
    z = torch.zeros(3, 8, dtype=torch.int64)
    batch = TokenizedSeqBatch(user_ids=z[:, :1], sem_ids=z, sem_ids_fut=None, seq_mask=z.bool(), token_type_ids=z,
                              token_type_ids_fut=None)
    two = torch.zeros(2, 5)
    for b in (two, tok.item_bias(two)):
        with pytest.raises(ValueError, match="item_bias has 2 groups"):
            model.recommend(batch, item_bias=b)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3)):
        with pytest.raises(ValueError, match="bias_group must be .B,. integer with B = 3"):
            model.recommend(batch, item_bias=two, bias_group=bad)
    with pytest.raises(ValueError, match="bias_group without item_bias"):
        model.recommend(batch, bias_group=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="item_bias: bias must be float32"):
        model.recommend(batch, item_bias=torch.zeros(4))
    with pytest.raises(ValueError, match="item_bias: bias must be float32"):
        model.recommend(batch, item_bias=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="write the filter into the bias as -inf"):
        model.recommend(batch, item_bias=torch.zeros(5), item_filter=torch.ones(5, dtype=torch.bool))
    assert model.training and model.transformer.cached_enc_output is None


def test_bias_ops_refuse_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    tok = bs.ids_tokenizer(bs.FIVE.clone())
    idx, trie = tok.trie_index(), tok.prefix_trie()
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.trie_bias_nodes(torch.zeros(1, 5), idx.item_leaf, idx.leaf_anc, [c.numel() for c in idx.leaf_count])
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand_biased(torch.zeros(2, 12), 3, batch=2, child_off=trie.child_off[0], tok=trie.tok[1],
                               bias=torch.zeros(1, trie.tok[1].numel()), bias_group=torch.zeros(2, dtype=torch.int32))


def test_entry_points_refuse_bad_sizes():
    """-22 from the argument checks, which run on the host: no pointer is dereferenced, no device is touched."""
    import torch  # noqa: F401  (load order: torch's HIP runtime first)
    from rqvae_hip import _lib
    lib = _lib.load()
    assert lib.rq_abi_version() == 4
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused before a launch

    def expand(fn, n_children=5, n_bias=5, G=1, bias=one, kprev=1, k=2, V=8, P=0):
        return fn(one, 1.0, None, one, 1, one, n_children, None, None, 1, kprev, V, P, k, one, one, one, one, one, None,
                  0, bias, n_bias, G, one, None)

    for fn, name in ((lib.rq_beam_expand_biased, b"rq_beam_expand_biased"),
                     (lib.rq_beam_expand_wide_biased, b"rq_beam_expand_wide_biased")):
        assert expand(fn, n_bias=4) == -22 and b"n_bias == n_children" in lib.rq_last_error()
        assert name in lib.rq_last_error()
        assert expand(fn, n_children=5, n_bias=-1) == -22
        assert expand(fn, G=-1) == -22
        assert expand(fn, bias=None) == -22 and b"null bias" in lib.rq_last_error()
        assert expand(fn, k=0) == -22
        assert expand(fn, V=5000) == -22
    # the narrow form keeps three floats per beam in LDS: kprev <= 1024 (V = 1 would otherwise admit 8192 beams)
    assert expand(lib.rq_beam_expand_biased, kprev=2048, V=1) == -22 and b"kprev <= 1024" in lib.rq_last_error()
    assert expand(lib.rq_beam_expand_wide_biased, kprev=2048, V=1) == -22

    P8 = ctypes.c_void_p * 8
    n_nodes = (ctypes.c_int64 * 8)(*([3] * 8))
    tables = P8(*([16] * 8))

    def build(G=1, n_items=5, n_leaves=4, D=4, nn=n_nodes):
        return lib.rq_trie_bias_nodes(one, G, n_items, one, n_leaves, tables, nn, D, tables, one, None)

    assert build(D=9) == -22 and b"rq_trie_bias_nodes" in lib.rq_last_error()
    assert build(D=0) == -22
    assert build(G=-1) == -22
    assert build(n_items=-1) == -22
    assert build(n_items=2 ** 31) == -22
    assert build(n_leaves=-1) == -22
    assert build(nn=(ctypes.c_int64 * 8)(3, -1, 3, 3, 3, 3, 3, 3)) == -22
    assert build(G=0) == 0 and build(n_leaves=0) == 0, "nothing to do: no launch"
