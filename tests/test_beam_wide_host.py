"""Wide constrained beam search without a GPU: the chunk-merge reference the GPU tests trust (test_beam_wide_gpu) against
a brute-force enumeration, the `beams` argument's validation in generate_next_sem_id / recommend / train_decoder, and
beam_expand(wide=...) refusing CPU tensors."""
import pytest
import torch

import beam_support as bs


# ------------------------------------------------------------------------------------------ the helper, on the CPU
def _brute(corpus, V, P):
    """A CPU step function for chunk_merge: beam_support.expand_reference over fp32 log-softmax rows."""
    def expand(logits, node, parents, plp, batch, kprev, k):
        lp = torch.log_softmax(logits, -1)
        live = [[True] * kprev] * batch if P == 0 else (node >= 0).tolist()
        ids, out_lp, parent, out_node, _ = bs.expand_reference(
            corpus, lp, None if P == 0 else parents.tolist(), live, plp, batch, kprev, V, P, k)
        return ids, out_lp, parent, out_node
    return expand


@pytest.mark.parametrize("kprev,P,k,chunk", [(70, 1, 50, 32), (70, 2, 50, 32), (70, 3, 200, 32), (96, 2, 7, 32),
                                             (9, 2, 30, 4), (1, 0, 20, 32)])
def test_chunk_merge_equals_brute_force(kprev, P, k, chunk):
    """Chunked and merged == every beam enumerated at once, on c300 in fp32: ids, scores, parents and nodes, with a
    beam copied into another chunk (equal scores across chunks, child for child: the lower global beam first) and,
    at k = 200, fewer candidates than k (dead rows)."""
    _, corpus = bs.tokenizer("c300", "cpu")
    B, V = 2, 12
    c = bs.wide_inputs(corpus, B, kprev, V, P, seed=70 + kprev + P)
    twins = (3, chunk + 8) if kprev > chunk + 8 else None
    if twins:   # two beams in different chunks on beam 0's (live) node, score for score, ahead of every other beam
        for j in twins:
            c["node"][:, j], c["parents"][:, j], c["parent_lp"][:, j] = c["node"][:, 0], c["parents"][:, 0], 100.0
        x = c["logits"].view(B, kprev, V)
        x[:, twins[1]] = x[:, twins[0]]
    step = _brute(corpus, V, P)
    want = step(c["logits"], c["node"], c["parents"], c["parent_lp"], B, kprev, k)
    got = bs.chunk_merge(step, c, B, kprev, V, P, k, chunk)
    for g, w, what in zip(got, want, ("ids", "lp", "parent", "node")):
        assert g.dtype == w.dtype and torch.equal(g, w), what
    live = want[3] >= 0
    assert live.any() and (k < 200 or (~live).any())
    if twins and P <= 2 and k >= 50:   # every child has a token < V, and 2 x 12 of them fit the k rows
        for b in range(B):
            n = int((want[2][b] == twins[0]).sum())
            assert n > 0 and want[2][b, :2 * n].tolist() == list(twins) * n, "equal scores: the lower beam first"
            assert torch.equal(want[0][b, 0:2 * n:2], want[0][b, 1:2 * n:2]) and torch.equal(want[1][b, 0:2 * n:2],
                                                                                             want[1][b, 1:2 * n:2])


# ------------------------------------------------------------------------------------------ arguments
def _model():
    from modules.model import EncoderDecoderRetrievalModel
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=16, sem_id_dim=4, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    model.inference_prefix_index = bs.tokenizer("c5", "cpu")[0]
    return model


def test_beams_argument_errors():
    model = _model()
    kw = dict(top_k=True, fused=True, sample=False, constrained=True)
    for beams in (0, -1, 1025):
        with pytest.raises(ValueError, match="1 <= beams <= 1024"):
            model.generate_next_sem_id(None, beams=beams, **kw)
        with pytest.raises(ValueError, match="beams <= 1024"):
            model.recommend(None, k=1, beams=beams)
    with pytest.raises(ValueError, match="requires constrained=True"):
        model.generate_next_sem_id(None, top_k=True, fused=True, sample=False, beams=64)
    with pytest.raises(ValueError, match="requires constrained=True"):
        model.generate_next_sem_id(None, beams=16)
    with pytest.raises(ValueError, match="top_k=True"):
        model.generate_next_sem_id(None, beams=64, **{**kw, "top_k": False})
    with pytest.raises(ValueError, match="k <= 64 beams"):
        model.recommend(None, k=65, beams=64)
    with pytest.raises(ValueError, match="k <= 32 beams"):
        model.recommend(None, k=33)
    with pytest.raises(ValueError, match="got k = 0"):
        model.recommend(None, k=0, beams=64)
    assert model.training and model.transformer.cached_enc_output is None


def test_train_decoder_refuses_cutoffs_past_the_beam_width(monkeypatch):
    import train_decoder
    assert train_decoder.EVAL_BEAM_WIDTH == 32 and tuple(train_decoder.EVAL_ITEM_KS) == (1, 5, 10)
    for ks, width in (((1, 5, 50), 32), ((1, 5, 10), 2000), ((0, 5), 32)):
        monkeypatch.setattr(train_decoder, "EVAL_ITEM_KS", ks)
        monkeypatch.setattr(train_decoder, "EVAL_BEAM_WIDTH", width)
        with pytest.raises(ValueError, match="EVAL_ITEM_KS"):
            train_decoder.train(iterations=1)   # raised before anything is read or built


def test_beam_expand_wide_refuses_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    assert ops.BEAM_WIDE_MAX == 1024
    trie = bs.tokenizer("c5", "cpu")[0].prefix_trie()
    for wide in (None, True, False):
        with pytest.raises(RqHipError, match="no CPU fallback"):
            ops.beam_expand(torch.zeros(2, 12), 3, batch=2, child_off=trie.child_off[0], tok=trie.tok[1], wide=wide)
