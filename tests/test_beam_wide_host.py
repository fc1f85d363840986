"""Wide constrained beam search without a GPU: the chunk-merge reference the GPU tests trust (test_beam_wide_gpu) against
a brute-force enumeration, the `beams` argument's validation in generate_next_sem_id / recommend / train_decoder, and
beam_expand(wide=...) refusing CPU tensors."""
import pytest
import torch

import test_beam_expand_gpu as expand_tests   # builders only: nothing here touches a device
import test_beam_gpu as fused_tests

CHUNK = 32   # the beams one narrow-kernel call takes at V = 256 (kprev V <= 8192)


# ------------------------------------------------------------------------------------------ inputs
def cpu_corpus(name):
    """test_beam_expand_gpu._tokenizer's c300 / c5 on the CPU, built apart from its cache (which holds the device's)."""
    tok = fused_tests._hand_tokenizer(torch.device("cpu"), **({} if name == "c300" else {"n": 5}))
    if name == "c300":
        tok.cached_ids[::7, 3] = 13
    else:
        tok.cached_ids = expand_tests._FIVE.clone()
    return tok, expand_tests._Corpus(tok.cached_ids)


def wide_inputs(corpus, B, kprev, V, P, seed):
    """test_beam_expand_gpu._case's beams without its redraw loop (CPU tensors): beams on prefixes of random corpus
    rows, beam 1 of user 0 on beam 0's node, about one in six dead (node -1, parents -1), logits 2 randn."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, corpus.ids.shape[0], (B, kprev), generator=g)
    if kprev > 1:
        rows[0, 1] = rows[0, 0]
    parents = parent_lp = node = None
    if P:
        live = torch.rand(B, kprev, generator=g) > 0.15
        live[:, 0] = True
        live[0, :2] = True   # the two beams on one node are both there
        parents = corpus.ids[rows][:, :, :P].clone()
        node = torch.tensor([[corpus.index[P][tuple(parents[b, j].tolist())] for j in range(kprev)] for b in range(B)],
                            dtype=torch.int32)
        parents[~live] = -1
        node[~live] = -1
        parent_lp = -(5.0 * torch.rand(B, kprev, generator=g)) - 0.1
    return dict(logits=2.0 * torch.randn(B * kprev, V, generator=g), node=node, parents=parents, parent_lp=parent_lp)


# ------------------------------------------------------------------------------------------ chunk-merge
def chunk_merge(expand, c, B, kprev, V, P, k, chunk=CHUNK):
    """The exact k best of kprev beams from a step function that takes at most `chunk` of them: the beams are split
    into chunks (the last padded with dead beams), every chunk runs as its own batch element with the same k, the
    live rows are merged by (score descending, global beam ascending, token ascending) — the top k of a union lies in
    the union of the chunks' top k — and dead rows pad. expand(logits, node, parents, parent_lp, batch, kprev, k) ->
    (ids (batch, k, P + 1), lp (batch, k), parent (batch, k), node (batch, k)), CPU tensors; the merged lp keeps the
    step function's values (and dtype) untouched. P == 0 is one beam per user: nothing to split."""
    logits, node, parents, plp = c["logits"], c["node"], c["parents"], c["parent_lp"]
    if P == 0:
        assert kprev == 1
        n_ch, step = 1, 1
    else:
        step = min(chunk, kprev)
        n_ch = -(-kprev // step)
        pad = n_ch * step - kprev
        if pad:   # dead beams contribute no candidate
            logits = torch.cat([logits.view(B, kprev, V), torch.zeros(B, pad, V)], 1).reshape(-1, V)
            node = torch.cat([node, torch.full((B, pad), -1, dtype=node.dtype)], 1)
            parents = torch.cat([parents, torch.full((B, pad, P), -1, dtype=parents.dtype)], 1)
            plp = torch.cat([plp, torch.zeros(B, pad)], 1)
        node, parents, plp = (node.reshape(B * n_ch, step), parents.reshape(B * n_ch, step, P),
                              plp.reshape(B * n_ch, step))
    ids, lp, parent, out_node = expand(logits.contiguous(), node, parents, plp, B * n_ch, step, k)
    m_ids = torch.full((B, k, P + 1), -1, dtype=torch.int64)
    m_lp = torch.full((B, k), -float("inf"), dtype=lp.dtype)
    m_parent = torch.zeros((B, k), dtype=parent.dtype)
    m_node = torch.full((B, k), -1, dtype=out_node.dtype)
    for b in range(B):
        rows = []
        for ch in range(n_ch):
            e = b * n_ch + ch
            for r in range(k):
                if int(out_node[e, r]) < 0:
                    break   # dead rows come last
                rows.append((-float(lp[e, r]), ch * step + int(parent[e, r]), int(ids[e, r, P]), e, r))
        rows.sort(key=lambda t: t[:3])
        for at, (_, beam, _, e, r) in enumerate(rows[:k]):
            m_ids[b, at], m_lp[b, at], m_parent[b, at], m_node[b, at] = ids[e, r], lp[e, r], beam, out_node[e, r]
    return m_ids, m_lp, m_parent, m_node


# ------------------------------------------------------------------------------------------ the helper, on the CPU
def _brute(corpus, V, P):
    """A CPU step function for chunk_merge: test_beam_expand_gpu._expand_reference over fp32 log-softmax rows."""
    def expand(logits, node, parents, plp, batch, kprev, k):
        lp = torch.log_softmax(logits, -1)
        live = [[True] * kprev] * batch if P == 0 else (node >= 0).tolist()
        ids, out_lp, parent, out_node, _ = expand_tests._expand_reference(
            corpus, lp, None if P == 0 else parents.tolist(), live, plp, batch, kprev, V, P, k)
        return ids, out_lp, parent, out_node
    return expand


@pytest.mark.parametrize("kprev,P,k,chunk", [(70, 1, 50, 32), (70, 2, 50, 32), (70, 3, 200, 32), (96, 2, 7, 32),
                                             (9, 2, 30, 4), (1, 0, 20, 32)])
def test_chunk_merge_equals_brute_force(kprev, P, k, chunk):
    """Chunked and merged == every beam enumerated at once, on c300 in fp32: ids, scores, parents and nodes, with a
    beam copied into another chunk (equal scores across chunks, child for child: the lower global beam first) and,
    at k = 200, fewer candidates than k (dead rows)."""
    _, corpus = cpu_corpus("c300")
    B, V = 2, 12
    c = wide_inputs(corpus, B, kprev, V, P, seed=70 + kprev + P)
    twins = (3, chunk + 8) if kprev > chunk + 8 else None
    if twins:   # two beams in different chunks on beam 0's (live) node, score for score, ahead of every other beam
        for j in twins:
            c["node"][:, j], c["parents"][:, j], c["parent_lp"][:, j] = c["node"][:, 0], c["parents"][:, 0], 100.0
        x = c["logits"].view(B, kprev, V)
        x[:, twins[1]] = x[:, twins[0]]
    step = _brute(corpus, V, P)
    want = step(c["logits"], c["node"], c["parents"], c["parent_lp"], B, kprev, k)
    got = chunk_merge(step, c, B, kprev, V, P, k, chunk)
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
    model.inference_prefix_index = cpu_corpus("c5")[0]
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
    trie = cpu_corpus("c5")[0].prefix_trie()
    for wide in (None, True, False):
        with pytest.raises(RqHipError, match="no CPU fallback"):
            ops.beam_expand(torch.zeros(2, 12), 3, batch=2, child_off=trie.child_off[0], tok=trie.tok[1], wide=wide)
