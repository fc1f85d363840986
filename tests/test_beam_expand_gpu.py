"""Constrained beam decoding on the device: rq_beam_expand (one trie-walking launch per beam step) against an fp64
reference that enumerates the valid continuations from the corpus rows themselves, against the existing
beam_candidates + beam_select kernels, its tie / underflow / bad-table behaviour and argument refusals; then
generate_next_sem_id(constrained=True), recommend() and the Hit@k counters over beams with dead rows."""
import numpy as np
import pytest
import torch

import test_beam_gpu as fused_tests   # the fused-generation fixtures' model / batch / tokenizer builders

pytestmark = pytest.mark.gpu

_FIVE = torch.tensor([[3, 1, 4, 0], [3, 1, 4, 1], [0, 2, 2, 0], [3, 0, 9, 0], [0, 2, 2, 0]])


# ------------------------------------------------------------------------------------------ corpora
class _Corpus:
    """Brute-force view of the corpus rows (CPU): per prefix length P the valid next tokens of every prefix and
    the rank of every prefix among the sorted distinct ones (= its trie node), from the rows, not from the trie."""

    def __init__(self, ids):
        self.ids = ids
        self.rows = [tuple(r) for r in ids.tolist()]
        D = ids.shape[1]
        self.children = [{} for _ in range(D)]
        for r in self.rows:
            for p in range(D):
                self.children[p].setdefault(r[:p], set()).add(r[p])
        self.children = [{pre: sorted(s) for pre, s in lvl.items()} for lvl in self.children]
        self.index = [{pre: i for i, pre in enumerate(sorted({r[:p] for r in self.rows}))} for p in range(D + 1)]
        self.first_row = {}
        for i, r in enumerate(self.rows):
            self.first_row.setdefault(r, i)


_TOKENIZERS = {}


def _tokenizer(name, device, golden=None):
    """(tokenizer on the device, its _Corpus), built once per name.
    c300: 300 x 4 in [0, 12) with some dedup-column tokens set to 13 (>= the V = 12 the kernel tests use);
    c5: five hand-written rows, one duplicated; c3000: 3000 x 4 in [0, 256); golden: the tokenizer fixture's corpus."""
    if name not in _TOKENIZERS:
        if name == "golden":
            tok = fused_tests._corpus_tokenizer(golden("tokenizer"), device)
        elif name == "c300":
            tok = fused_tests._hand_tokenizer(device)
            tok.cached_ids[::7, 3] = 13
        elif name == "c5":
            tok = fused_tests._hand_tokenizer(device, n=5)
            tok.cached_ids = _FIVE.to(device)
        else:
            tok = fused_tests._hand_tokenizer(device, seed=5, n=3000, hi=256)
        _TOKENIZERS[name] = (tok, _Corpus(tok.cached_ids.cpu()))
    return _TOKENIZERS[name]


# ------------------------------------------------------------------------------------------ fp64 reference
def _log_softmax64(logits, T):
    """fp64 log-softmax in the (z - max) - log1p(sum of the other exponentials) form (test_beam_gpu._cand_reference)."""
    z = logits.double() / T
    m, am = z.max(dim=-1, keepdim=True)
    e = torch.exp(z - m).scatter(1, am, 0.0)
    return (z - m) - torch.log1p(e.sum(-1, keepdim=True))


def _expand_reference(corpus, lp, prefixes, live, parent_lp, B, kprev, V, P, k):
    """Per batch element: every (live beam j, valid child token v < V) scored lp[b kprev + j][v] + parent_lp[b][j] in
    fp64, stable descending sort in (beam, token) order, the k best; dead rows (-1, -inf, parent 0, node -1) pad.
    Returns ids (B, k, P + 1), scores (B, k) fp64, parent (B, k), node (B, k), and every user's sorted scores."""
    ids = torch.full((B, k, P + 1), -1, dtype=torch.int64)
    out_lp = torch.full((B, k), -float("inf"), dtype=torch.float64)
    parent = torch.zeros((B, k), dtype=torch.int64)
    node = torch.full((B, k), -1, dtype=torch.int64)
    all_scores = []
    for b in range(B):
        cands = []
        for j in range(kprev):
            if not live[b][j]:
                continue
            pre = tuple(prefixes[b][j]) if P else ()
            for v in corpus.children[P].get(pre, ()):
                if v < V:
                    cands.append((float(lp[b * kprev + j, v]) + (float(parent_lp[b][j]) if P else 0.0), j, v, pre))
        cands.sort(key=lambda c: -c[0])   # stable: equal scores stay in (beam, token) order
        all_scores.append([c[0] for c in cands])
        for r, (s, j, v, pre) in enumerate(cands[:k]):
            ids[b, r] = torch.tensor(pre + (v,))
            out_lp[b, r], parent[b, r], node[b, r] = s, j, corpus.index[P + 1][pre + (v,)]
    return ids, out_lp, parent, node, all_scores


def _separated(scores, k):
    """_separated_case's rule on one user's descending fp64 scores: the top k + 1 pairwise >= 1e-5 relative apart."""
    top = scores[:k + 1]
    return all(a - c >= 1e-5 * abs(a) for a, c in zip(top[:-1], top[1:]))


_CASES = {}


def _case(device, name, B, kprev, V, P, k, T):
    """Seeded inputs of one kernel case and their reference, built once. Beams sit on prefixes of random corpus rows
    (beam 1 of user 0 repeats beam 0's node), about one in six is dead (node -1, parents -1); logits are 2 randn, a
    user whose top k + 1 scores are not separated is redrawn from the same stream."""
    key = (name, B, kprev, V, P, k, T)
    if key in _CASES:
        return _CASES[key]
    tok, corpus = _tokenizer(name, device)
    g = torch.Generator().manual_seed(4000 + 97 * B + 31 * kprev + 7 * V + 3 * P + k + int(10 * T))
    n = corpus.ids.shape[0]
    rows = torch.randint(0, n, (B, kprev), generator=g)
    if kprev > 1:
        rows[0, 1] = rows[0, 0]
    live = torch.ones(B, kprev, dtype=torch.bool)
    parents = parent_lp = node = None
    if P:
        live = torch.rand(B, kprev, generator=g) > 0.15
        live[:, 0] = True
        parents = corpus.ids[rows][:, :, :P].clone()
        node = torch.tensor([[corpus.index[P][tuple(parents[b, j].tolist())] for j in range(kprev)] for b in range(B)],
                            dtype=torch.int32)
        parents[~live] = -1
        node[~live] = -1
        parent_lp = -(5.0 * torch.rand(B, kprev, generator=g)) - 0.1
    logits = 2.0 * torch.randn(B * kprev, V, generator=g)
    pre = parents.tolist() if P else None
    for _ in range(200):
        ref = _expand_reference(corpus, _log_softmax64(logits, T), pre, live.tolist(), parent_lp, B, kprev, V, P, k)
        bad = [b for b in range(B) if not _separated(ref[4][b], k)]
        if not bad:
            break
        for b in bad:
            logits[b * kprev:(b + 1) * kprev] = 2.0 * torch.randn(kprev, V, generator=g)
    assert all(_separated(s, k) for s in ref[4]), "precondition: separated scores"
    _CASES[key] = dict(tok=tok, logits=logits, parents=parents, parent_lp=parent_lp, node=node, ref=ref)
    return _CASES[key]


def _run(device, c, k, P, T, B):
    from rqvae_hip import ops
    trie = c["tok"].prefix_trie()
    d = fused_tests._dev
    return ops.beam_expand(c["logits"].to(device), k, batch=B, child_off=trie.child_off[P], tok=trie.tok[P + 1],
                           node=d(c["node"], device), parents=d(c["parents"], device),
                           parent_lp=d(c["parent_lp"], device), temperature=T)


# corpus, B, kprev, V, P, k
_SHAPES = [("c300", 2, 1, 12, 0, 5), ("c300", 3, 4, 12, 1, 8), ("c300", 3, 4, 12, 3, 8), ("c5", 2, 1, 37, 0, 8),
           ("c5", 2, 3, 37, 2, 8), ("c3000", 2, 32, 256, 1, 32), ("c3000", 2, 32, 256, 2, 32),
           ("c3000", 2, 1, 256, 0, 32),
           ("c300", 2, 6, 12, 1, 8)]   # more than 4 beams: the 16-wave launch with idle waves


def _assert_dead_rows(ids, lp, parent, node):
    dead = node < 0
    assert torch.equal(dead, (ids == -1).all(-1)) and torch.equal(dead, (ids == -1).any(-1))
    assert torch.isneginf(lp[dead]).all() and (parent[dead] == 0).all() and (node[dead] == -1).all()
    assert torch.equal(dead, torch.sort(dead.int(), dim=1, stable=True).values.bool()), "dead rows come last"


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("name,B,kprev,V,P,k", _SHAPES)
def test_beam_expand_vs_fp64(device, name, B, kprev, V, P, k, T):
    c = _case(device, name, B, kprev, V, P, k, T)
    want_ids, want_lp, want_parent, want_node, scores = c["ref"]
    if name == "c300" and P == 3:
        corpus = _tokenizer(name, device)[1]
        assert any(v >= V for kids in corpus.children[3].values() for v in kids), "dedup tokens >= V exist"
        assert any(len(s) < k for s in scores), "dead rows appear"
    ids, lp, parent, node = (t.cpu() for t in _run(device, c, k, P, T, B))
    assert ids.shape == (B, k, P + 1) and ids.dtype == torch.int64 and lp.shape == (B, k) and lp.dtype == torch.float32
    assert parent.shape == node.shape == (B, k) and parent.dtype == node.dtype == torch.int32
    print(f"{name} B={B} kprev={kprev} V={V} P={P} k={k} T={T}: candidates per user {[len(s) for s in scores]}, "
          f"max rel lp err {float(((lp.double() - want_lp).abs() / want_lp.abs())[want_node >= 0].max()):.3e}")
    assert torch.equal(ids, want_ids), "out_ids"
    assert torch.equal(parent.long(), want_parent), "out_parent"
    assert torch.equal(node.long(), want_node), "out_node"
    np.testing.assert_allclose(lp.double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    _assert_dead_rows(ids, lp, parent, node)


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("name,B,kprev,V,P,k", _SHAPES)
def test_beam_expand_vs_candidates_and_select(device, name, B, kprev, V, P, k, T):
    """beam_candidates over every class followed by beam_select's table search keeps the same valid candidates:
    equal ids and parents and bitwise equal log-probabilities on the rows that hold a valid candidate (all k of them
    where at least k exist; select fills the others with rejected candidates, expand with dead rows)."""
    from rqvae_hip import ops
    c = _case(device, name, B, kprev, V, P, k, T)
    n_valid = [min(k, len(s)) for s in c["ref"][4]]
    if (name, P) in (("c300", 0), ("c300", 1), ("c3000", 0), ("c3000", 1)):
        assert all(n == k for n in n_valid), "at least k valid candidates"
    ids, lp, parent, _ = _run(device, c, k, P, T, B)
    keys, base = c["tok"].prefix_table(P + 1)
    cand_ids, cand_lp = ops.beam_candidates(c["logits"].to(device), V, T)
    s_ids, s_lp, s_parent = ops.beam_select(cand_ids, cand_lp, k, batch=B, keys=keys, base=base,
                                            parents=fused_tests._dev(c["parents"], device),
                                            parent_lp=fused_tests._dev(c["parent_lp"], device), return_parent=True)
    for b, n in enumerate(n_valid):
        assert torch.equal(ids[b, :n], s_ids[b, :n]) and torch.equal(parent[b, :n], s_parent[b, :n]), b
        assert torch.equal(lp[b, :n].view(torch.int32), s_lp[b, :n].view(torch.int32)), "out_lp bitwise"


# ------------------------------------------------------------------------------------------ ties, edge values
def test_beam_expand_ties_underflow_and_dead_rows(device):
    from rqvae_hip import ops
    tok, corpus = _tokenizer("c5", device)
    trie = tok.prefix_trie()
    n3 = corpus.index[1][(3,)]
    # two beams on node (3,) with identical logits and equal parent_lp: children 0 and 1 of each, in (beam, token)
    # order; 4 candidates for k = 6
    node = torch.tensor([[n3, n3]], dtype=torch.int32, device=device)
    parents = torch.tensor([[[3], [3]]], device=device)
    plp = torch.full((1, 2), -0.5, device=device)
    ids, lp, parent, out_node = (t.cpu() for t in ops.beam_expand(
        torch.zeros(2, 16, device=device), 6, batch=1, child_off=trie.child_off[1], tok=trie.tok[2], node=node,
        parents=parents, parent_lp=plp))
    assert ids[0].tolist() == [[3, 0], [3, 1], [3, 0], [3, 1], [-1, -1], [-1, -1]]
    assert parent[0].tolist() == [0, 0, 1, 1, 0, 0]
    kids = [corpus.index[2][(3, 0)], corpus.index[2][(3, 1)]]
    assert out_node[0].tolist() == kids + kids + [-1, -1]
    np.testing.assert_allclose(lp[0, :4].numpy(), -0.5 - np.log(16.0), rtol=1e-6, atol=0)
    assert (lp[0, :4] == lp[0, 0]).all() and torch.isneginf(lp[0, 4:]).all()
    # an underflowing child (p == 0 in fp32) is kept with -inf: below every finite candidate, above the dead rows
    x = torch.full((1, 16), -200.0, device=device)
    x[0, 3] = 0.0
    ids, lp, parent, out_node = (t.cpu() for t in ops.beam_expand(x, 4, batch=1, child_off=trie.child_off[0],
                                                                   tok=trie.tok[1]))
    assert ids[0].tolist() == [[3], [0], [-1], [-1]]
    assert out_node[0].tolist() == [corpus.index[1][(3,)], corpus.index[1][(0,)], -1, -1] and parent[0].tolist() == [0] * 4
    assert lp[0, 0] == 0 and torch.isneginf(lp[0, 1:]).all()
    _assert_dead_rows(ids, lp, parent, out_node)


def test_beam_expand_bad_tables_stay_in_bounds(device):
    """Out-of-range node / child_off entries and tokens >= V or < 0 give no candidates (the result for a bad table is
    otherwise unspecified; every index the kernel forms from these values stays inside the buffers)."""
    from rqvae_hip import ops
    V, k = 8, 6
    tok = torch.tensor([0, 5, 40, 2, 7, -3], dtype=torch.int32, device=device)
    child_off = torch.tensor([-4, 3, 99, 4], dtype=torch.int32, device=device)   # node 0: [0, 3), 1: [3, 6), 2: [6, 4)
    node = torch.tensor([[0, 1, 2, 3, -1, 7]], dtype=torch.int32, device=device)
    g = torch.Generator().manual_seed(11)
    logits = 2.0 * torch.randn(6, V, generator=g)
    parents = torch.arange(6).reshape(1, 6, 1)
    plp = -torch.rand(1, 6, generator=g)
    ids, lp, parent, out_node = (t.cpu() for t in ops.beam_expand(
        logits.to(device), k, batch=1, child_off=child_off, tok=tok, node=node, parents=parents.to(device),
        parent_lp=plp.to(device)))
    lp64 = _log_softmax64(logits, 1.0)
    want = sorted([(float(lp64[j, v]) + float(plp[0, j]), j, v, c) for j, v, c in ((0, 0, 0), (0, 5, 1), (1, 2, 3), (1, 7, 4))],
                  key=lambda c: -c[0])
    assert ids[0, :4].tolist() == [[j, v] for _, j, v, _ in want]
    assert parent[0, :4].tolist() == [j for _, j, _, _ in want] and out_node[0, :4].tolist() == [c for *_, c in want]
    np.testing.assert_allclose(lp[0, :4].double().numpy(), [s for s, *_ in want], rtol=1e-5, atol=0)
    assert (ids[0, 4:] == -1).all() and torch.isneginf(lp[0, 4:]).all() and out_node[0, 4:].tolist() == [-1, -1]


def test_beam_expand_refuses_bad_arguments(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = _tokenizer("c5", device)
    trie = tok.prefix_trie()
    x = torch.zeros(4, 16, device=device)
    lvl0 = dict(child_off=trie.child_off[0], tok=trie.tok[1])
    lvl1 = dict(child_off=trie.child_off[1], tok=trie.tok[2])
    beams = dict(node=torch.zeros(2, 2, dtype=torch.int32, device=device),
                 parents=torch.zeros(2, 2, 1, dtype=torch.int64, device=device), parent_lp=torch.zeros(2, 2, device=device))
    assert ops.beam_expand(x, 3, batch=2, **lvl1, **beams)[0].shape == (2, 3, 2)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand(x.cpu(), 3, batch=4, **lvl0)
    with pytest.raises(RqHipError, match="float32"):
        ops.beam_expand(x.double(), 3, batch=4, **lvl0)
    with pytest.raises(RqHipError, match=r"\(B \* kprev, V\)"):
        ops.beam_expand(x, 3, batch=3, **lvl0)
    with pytest.raises(RqHipError, match="go together"):
        ops.beam_expand(x, 3, batch=2, **lvl1, node=beams["node"])
    with pytest.raises(RqHipError, match="node must be a contiguous torch.int32"):
        ops.beam_expand(x, 3, batch=2, **lvl1, **{**beams, "node": beams["node"].long()})
    with pytest.raises(RqHipError, match="parent_lp must have shape"):
        ops.beam_expand(x, 3, batch=2, **lvl1, **{**beams, "parent_lp": torch.zeros(2, 3, device=device)})
    with pytest.raises(RqHipError, match="child_off must be a contiguous torch.int32"):
        ops.beam_expand(x, 3, batch=4, child_off=trie.child_off[0].long(), tok=trie.tok[1])
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand(torch.zeros(1, 5000, device=device), 3, batch=1, **lvl0)        # V > 4096
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand(torch.zeros(40, 256, device=device), 3, batch=1, **lvl0)        # kprev V > 8192
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand(x, 0, batch=4, **lvl0)
    with pytest.raises(RqHipError, match="rc=-22.*temperature"):
        ops.beam_expand(x, 3, batch=4, **lvl0, temperature=0.0)
    # the envelope's corner runs: V = 4096 with kprev = 2, and more beams asked for than candidates exist
    ids = ops.beam_expand(torch.zeros(2, 4096, device=device), 5, batch=1, **lvl1, node=beams["node"][:1],
                          parents=torch.full((1, 2, 1), 3, device=device), parent_lp=beams["parent_lp"][:1])[0]
    assert ids.shape == (1, 5, 2)
    assert ops.beam_expand(x[:0], 3, batch=0, **lvl0)[0].shape == (0, 3, 1)


# ------------------------------------------------------------------------------------------ generation
def _reference_constrained(model, batch, corpus, k, T=1.0):
    """The constrained search with the expansion in fp64 on the CPU: logits from the model's own forwards over batches
    built as _ForwardSteps (modules/model.py) builds them (dead beams' tokens clamped to 0). Asserts the separation
    precondition at every step. Returns ids (B, k, L1), fp64 log-probabilities (B, k) and the leaf nodes (B, k)."""
    from data.schemas import TokenizedSeqBatch
    from ops.jagged import jagged_to_padded_tensor, padded_to_jagged
    B, L1, V = batch.sem_ids.shape[0], model.sem_id_dim, model.num_embeddings
    dev = batch.sem_ids.device
    was_training = model.training
    model.eval()
    model.transformer.cached_enc_output = None
    try:
        with torch.no_grad():
            cur = TokenizedSeqBatch(user_ids=batch.user_ids, sem_ids=batch.sem_ids, sem_ids_fut=None,
                                    seq_mask=batch.seq_mask, token_type_ids=batch.token_type_ids, token_type_ids_fut=None)
            ids = lp = node = None
            for i in range(L1):
                logits = model.forward(cur).logits.cpu()
                kprev = 1 if i == 0 else k
                assert logits.shape == (B * kprev, V)
                live = [[True] * kprev] * B if i == 0 else (node >= 0).tolist()
                ids, lp, _, node, scores = _expand_reference(corpus, _log_softmax64(logits, T),
                                                             None if i == 0 else ids.tolist(), live, lp, B, kprev, V, i, k)
                assert all(_separated(s, k) for s in scores), f"precondition: separated scores at step {i}"
                if i == L1 - 1:
                    break
                nxt = ids.clamp_min(0).to(dev).flatten(end_dim=1)
                if i == 0:
                    enc = model.transformer.cached_enc_output
                    n_ctx = cur.sem_ids.shape[1] + 1
                    padded = jagged_to_padded_tensor(enc, n_ctx).repeat_interleave(k, dim=0)
                    lengths = enc.offsets().diff().repeat_interleave(k)
                    model.transformer.cached_enc_output = padded_to_jagged(padded.contiguous(), lengths, n_ctx)
                    cur = TokenizedSeqBatch(user_ids=cur.user_ids.repeat_interleave(k, dim=0),
                                            sem_ids=cur.sem_ids.repeat_interleave(k, dim=0), sem_ids_fut=nxt,
                                            token_type_ids_fut=torch.zeros_like(nxt),
                                            seq_mask=cur.seq_mask.repeat_interleave(k, dim=0),
                                            token_type_ids=cur.token_type_ids.repeat_interleave(k, dim=0))
                else:
                    cur = TokenizedSeqBatch(user_ids=cur.user_ids, sem_ids=cur.sem_ids, sem_ids_fut=nxt,
                                            token_type_ids_fut=torch.arange(nxt.shape[1], device=dev).repeat(nxt.shape[0], 1),
                                            seq_mask=cur.seq_mask, token_type_ids=cur.token_type_ids)
    finally:
        model.transformer.cached_enc_output = None
        model.train(was_training)
    return ids, lp, node


_GEN = {}


def _generation_case(golden, device, name):
    """(model with the tokenizer as its prefix index, batch, corpus, {k: reference}); the references are computed
    once per corpus and shared by the tests below."""
    if name not in _GEN:
        z = golden("generation")
        tok, corpus = _tokenizer(name, device, golden)
        model = fused_tests._decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]))
        model.enable_generation = True
        model.inference_prefix_index = tok
        batch = fused_tests._tokenized(z, device)
        _GEN[name] = (model, batch, corpus, {k: _reference_constrained(model, batch, corpus, k) for k in (32, 1)})
    return _GEN[name]


@pytest.mark.parametrize("name", ["golden", "c300"])
def test_constrained_generation_vs_fp64_loop(golden, device, name):
    model, batch, corpus, refs = _generation_case(golden, device, name)
    want_ids, want_lp, want_node = refs[32]
    assert (want_node >= 0).any()
    rng = torch.cuda.get_rng_state()
    kw = dict(temperature=1, top_k=True, fused=True, sample=False, constrained=True)
    got = model.generate_next_sem_id(batch, **kw)
    assert model.training, "train mode restored"
    assert model.transformer.cached_enc_output is None, "encoder cache cleared"
    assert torch.equal(torch.cuda.get_rng_state(), rng), "no generator draw"
    assert got.sem_ids.shape == (3, 32, 4) and got.log_probas.shape == (3, 32)
    assert torch.equal(got.sem_ids.cpu(), want_ids), "beams"
    np.testing.assert_allclose(got.log_probas.cpu().double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    again = model.generate_next_sem_id(batch, **kw)
    assert torch.equal(again.sem_ids, got.sem_ids)
    assert torch.equal(again.log_probas.view(torch.int32), got.log_probas.view(torch.int32)), "two calls bitwise equal"
    inc = model.generate_next_sem_id(batch, incremental=True, **kw)
    assert model.training and model.transformer.cached_enc_output is None
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    assert torch.equal(inc.sem_ids.cpu(), want_ids), "incremental beams"
    np.testing.assert_allclose(inc.log_probas.cpu().double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    rows = set(corpus.rows)
    dead = (got.sem_ids.cpu() == -1).all(-1)
    assert torch.equal(dead, want_node < 0) and torch.isneginf(got.log_probas.cpu()[dead]).all()
    assert all(tuple(r) in rows for r in got.sem_ids.cpu()[~dead].tolist()), "every live beam is a corpus row"


@pytest.mark.parametrize("incremental", [False, True])
def test_constrained_generation_greedy(golden, device, incremental):
    model, batch, corpus, refs = _generation_case(golden, device, "golden")
    want_ids, want_lp, _ = refs[1]
    got = model.generate_next_sem_id(batch, temperature=1, top_k=False, fused=True, sample=False, constrained=True,
                                     incremental=incremental)
    assert got.sem_ids.shape == (3, 4) and got.log_probas.shape == (3,)
    assert torch.equal(got.sem_ids.cpu(), want_ids[:, 0]), "the greedy valid path"
    np.testing.assert_allclose(got.log_probas.cpu().double().numpy(), want_lp[:, 0].numpy(), rtol=1e-5, atol=0)
    assert all(tuple(r) in set(corpus.rows) for r in got.sem_ids.cpu().tolist())


@pytest.mark.parametrize("name", ["golden", "c300", "c5"])
def test_recommend(golden, device, name):
    from modules.model import Recommendation
    model, batch, corpus, refs = _generation_case(golden, device, name)
    want_ids, want_lp, want_node = refs[32]
    rec = model.recommend(batch)
    assert isinstance(rec, Recommendation) and model.training and model.transformer.cached_enc_output is None
    assert rec.item_ids.shape == (3, 10) and rec.item_ids.dtype == torch.int64
    assert rec.sem_ids.shape == (3, 10, 4) and rec.log_probas.shape == (3, 10)
    assert torch.equal(rec.sem_ids.cpu(), want_ids[:, :10]), "the first 10 of the 32 beams"
    np.testing.assert_allclose(rec.log_probas.cpu().double().numpy(), want_lp[:, :10].numpy(), rtol=1e-5, atol=0)
    items, live = rec.item_ids.cpu(), want_node[:, :10] >= 0
    if name == "c5":
        assert (~live).any() and live.any(), "the 4 distinct rows leave dead beams"
    assert (items[~live] == -1).all() and (items[live] >= 0).all()
    assert torch.equal(corpus.ids[items[live]], rec.sem_ids.cpu()[live]), "cached_ids[item_ids] == sem_ids"
    assert items[live].tolist() == [corpus.first_row[tuple(r)] for r in rec.sem_ids.cpu()[live].tolist()], "lowest index"
    full = model.recommend(batch, k=32, incremental=False)
    assert torch.equal(full.sem_ids.cpu(), want_ids) and torch.equal(full.item_ids[:, :10], rec.item_ids)


# ------------------------------------------------------------------------------------------ Hit@k with dead rows
def test_topk_accumulator_counts_dead_rows_like_cpu(device):
    """Beams that end in dead rows (four steps of beam_expand over the 5-row corpus, k = 6 > its 4 distinct items):
    the device counters equal the CPU accumulator's, and a -1 row never matches a target."""
    from evaluate.metrics import TopKAccumulator
    from rqvae_hip import ops
    tok, corpus = _tokenizer("c5", device)
    trie = tok.prefix_trie()
    B, k, V = 4, 6, 12
    g = torch.Generator().manual_seed(21)
    ids = lp = node = None
    for i in range(4):
        logits = 2.0 * torch.randn(B * (1 if i == 0 else k), V, generator=g)
        ids, lp, _, node = ops.beam_expand(logits.to(device), k, batch=B, child_off=trie.child_off[i], tok=trie.tok[i + 1],
                                           node=node, parents=ids, parent_lp=lp)
    beams = ids.cpu()
    assert (beams[:, :4] >= 0).all() and (beams[:, 4:] == -1).all(), "4 live beams and 2 dead rows per user"
    actual = torch.stack([beams[0, 0], beams[1, 2], torch.tensor([3, 1, 9, 0]), beams[3, 3]])
    ks = [1, 3, 6]
    cpu, gpu = TopKAccumulator(ks=ks), TopKAccumulator(ks=ks)
    cpu.accumulate(actual=actual, top_k=beams)
    gpu.accumulate(actual=actual.to(device), top_k=ids)
    assert torch.equal(gpu.counts.cpu(), cpu.counts) and gpu.reduce() == cpu.reduce()
    assert gpu.reduce()["h@6_slice_:4"] == 3 / 4 and gpu.reduce()["h@1_slice_:4"] == 1 / 4
