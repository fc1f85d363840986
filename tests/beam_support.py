"""What the beam-decoder tests share (test_beam_*, test_exclude_*, test_score_*): hand-made corpora and tokenizers, the
generation fixture's model and batch, seeded kernel cases, the fp64 references (one trie-free expansion, one walk over
the model's own full forwards, the chunk-merge) and the bitwise comparisons. Nothing here touches a device at import;
the caches below hold one entry per (case, device type), so every reference is computed once per session."""
import socket

import numpy as np
import torch

import gen_inputs as gi

NONE = 2 ** 31 - 1   # the padding of a blocked-node row
FIVE = torch.tensor([[3, 1, 4, 0], [3, 1, 4, 1], [0, 2, 2, 0], [3, 0, 9, 0], [0, 2, 2, 0]])
CHUNK = 32   # the beams one narrow-kernel call takes at V = 256 (kprev V <= 8192)


def dev(t, device):
    return None if t is None else t.to(device)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------------------------------ corpora and tokenizers
class Corpus:
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


def ids_tokenizer(ids, codebook_size=12):
    """A tokenizer whose corpus ids are set by hand (no RQ-VAE pass)."""
    from modules.tokenizer.semids import SemanticIdTokenizer
    tok = SemanticIdTokenizer(input_dim=8, output_dim=4, hidden_dims=[8], codebook_size=codebook_size,
                              n_layers=ids.shape[1] - 1, n_cat_feats=0)
    tok.cached_ids = ids
    return tok


def hand_tokenizer(device, seed=3, n=300, hi=12):
    """ids_tokenizer over n seeded rows of 4 ids in [0, hi), on the device."""
    g = torch.Generator().manual_seed(seed)
    tok = ids_tokenizer(torch.randint(0, hi, (n, 4), generator=g).to(device), codebook_size=hi)
    tok.cached_ids[0, 0] = hi - 1   # base = hi
    return tok


def random_corpus():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 12, (300, 4), generator=g)
    ids[0, 0] = 11          # base = 12
    ids[[7, 250]] = ids[3].clone()  # one row three times: its leaf maps to the lowest index
    return ids


class Items:
    def __init__(self, x):
        self.x = torch.from_numpy(x)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, idx):
        from data.schemas import SeqBatch
        ids = torch.as_tensor(idx).reshape(1, -1)
        neg = -torch.ones_like(ids[0])
        return SeqBatch(neg, ids, neg, self.x[idx], neg, torch.ones_like(ids, dtype=torch.bool))


def corpus_tokenizer(z, device):
    """The tokenizer fixture's RQ-VAE and its corpus ids, recomputed on the device."""
    from modules.tokenizer.semids import SemanticIdTokenizer
    inp, hid, D, K, L, seed = int(z["inp"]), [int(h) for h in z["hidden"]], int(z["D"]), int(z["K"]), int(z["L"]), int(z["seed"])
    tok = SemanticIdTokenizer(input_dim=inp, output_dim=D, hidden_dims=hid, codebook_size=K, n_layers=L, n_cat_feats=0)
    st = {f"encoder.mlp.{2 * j}.weight": w for j, w in enumerate(gi.mlp_weights([inp] + hid + [D], seed))}
    st.update({f"decoder.mlp.{2 * j}.weight": w for j, w in enumerate(gi.mlp_weights([D] + hid[::-1] + [inp], seed + 1))})
    st.update({f"layers.{l}.embedding.weight": z["codebooks"][l] for l in range(L)})
    tok.rq_vae.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    tok = tok.to(device)
    ids = tok.precompute_corpus_ids(Items(gi.items(int(z["n_items"]), inp, seed)))
    assert np.array_equal(ids.cpu().numpy(), z["corpus_ids"])
    return tok


_TOKENIZERS = {}


def tokenizer(name, device, golden=None):
    """(tokenizer on the device, its Corpus), built once per (name, device type).
    c300: 300 x 4 in [0, 12) with some dedup-column tokens set to 13 (>= the V = 12 the kernel tests use);
    c5: five hand-written rows, one duplicated; c3000: 3000 x 4 in [0, 256); golden: the tokenizer fixture's corpus."""
    key = (name, torch.device(device).type)
    if key not in _TOKENIZERS:
        if name == "golden":
            tok = corpus_tokenizer(golden("tokenizer"), device)
        elif name == "c300":
            tok = hand_tokenizer(device)
            tok.cached_ids[::7, 3] = 13
        elif name == "c5":
            tok = ids_tokenizer(FIVE.clone().to(device))
        else:
            tok = hand_tokenizer(device, seed=5, n=3000, hi=256)
        _TOKENIZERS[key] = (tok, Corpus(tok.cached_ids.cpu()))
    return _TOKENIZERS[key]


# ------------------------------------------------------------------------------------------ model fixtures
def decoder_model(z, device, dropout=0.0, scale_out=1.0, verifier=gi.prefix_verifier):
    from modules.model import EncoderDecoderRetrievalModel
    E, A, H, nl, K, L1, n_max, seed = (int(z[k]) for k in ("E", "A", "H", "n_layers", "K", "L1", "n_max", "seed"))
    model = EncoderDecoderRetrievalModel(embedding_dim=E, attn_dim=A, dropout=dropout, num_heads=H, n_layers=nl,
                                         num_embeddings=K, sem_id_dim=L1, inference_verifier_fn=verifier,
                                         max_pos=n_max * L1, jagged_mode=True)
    with torch.no_grad():
        for name, p in model.named_parameters():
            v = gi.named_param(name, p.shape, seed)
            p.copy_(torch.from_numpy(v * scale_out if name == "out_proj.weight" else v))
    return model.to(device)


def tokenized(z, device):
    from data.schemas import TokenizedSeqBatch
    keys = ("user_ids", "sem_ids", "sem_ids_fut", "seq_mask", "token_type_ids", "token_type_ids_fut")
    return TokenizedSeqBatch(**{k: torch.from_numpy(z[k]).to(device) for k in keys})


# ------------------------------------------------------------------------------------------ select-kernel cases
def select_inputs(B, kprev, n_cand, P, seed, hi=256):
    g = torch.Generator().manual_seed(seed)
    cand_ids = torch.randint(0, hi, (B * kprev, n_cand), generator=g)
    # log-probabilities on a 0.25 grid: plenty of exact ties, which must come out in flat-index order
    cand_lp = -(torch.randint(0, 40, (B * kprev, n_cand), generator=g).float() / 4)
    parents = torch.randint(0, hi, (B, kprev, P), generator=g) if P else None
    parent_lp = -(torch.randint(0, 20, (B, kprev), generator=g).float() / 4) - 0.1 if P else None
    return g, cand_ids, cand_lp, parents, parent_lp


def select_reference(cand_ids, cand_lp, valid, parents, parent_lp, B, k):
    """CPU: the reference's score expression in fp32 and a stable descending sort."""
    n_cand = cand_ids.shape[1]
    ids, lp = cand_ids.reshape(B, -1), cand_lp.reshape(B, -1)
    score = torch.where(valid.reshape(B, -1), 0.0, -10000.0).float() + lp
    score = score + (parent_lp.repeat_interleave(n_cand, dim=1) if parent_lp is not None else 0.0)
    top_lp, idx = torch.sort(score, dim=-1, descending=True, stable=True)
    top_lp, idx = top_lp[:, :k], idx[:, :k]
    out = torch.gather(ids, 1, idx).unsqueeze(-1)
    if parents is not None:
        P = parents.shape[2]
        out = torch.cat([torch.gather(parents, 1, (idx // n_cand).unsqueeze(-1).expand(-1, -1, P)), out], dim=-1)
    return out, top_lp


def assert_select(got, want):
    assert torch.equal(got[0].cpu(), want[0]), "out_ids"
    assert torch.equal(got[1].cpu().view(torch.int32), want[1].view(torch.int32)), "out_lp bitwise"


# ------------------------------------------------------------------------------------------ fp64 expansion
def log_softmax64(logits, T):
    """fp64 log-softmax in the (z - max) - log1p(sum of the other exponentials) form: without the cancellation of
    log(1 - tiny) where one class dominates."""
    z = logits.double() / T
    m, am = z.max(dim=-1, keepdim=True)
    e = torch.exp(z - m).scatter(1, am, 0.0)
    return (z - m) - torch.log1p(e.sum(-1, keepdim=True))


def expand_reference(corpus, lp, prefixes, live, parent_lp, B, kprev, V, P, k):
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


def separated(scores, k):
    """One user's descending fp64 scores: the top k + 1 pairwise >= 1e-5 relative apart, so fp32 rounding cannot
    decide an order."""
    top = scores[:k + 1]
    return all(a - c >= 1e-5 * abs(a) for a, c in zip(top[:-1], top[1:]))


def items_under(corpus, path):
    return [i for i, r in enumerate(corpus.rows) if r[:len(path)] == tuple(path)]


def pad(lists, H=None):
    H = max(1, max(len(l) for l in lists)) if H is None else H
    out = torch.full((len(lists), H), -1, dtype=torch.int64)
    for b, l in enumerate(lists):
        out[b, :len(l)] = torch.tensor(l[:H], dtype=torch.int64)
    return out


# ------------------------------------------------------------------------------------------ expand-kernel cases
# corpus, B, kprev, V, P, k
SHAPES = [("c300", 2, 1, 12, 0, 5), ("c300", 3, 4, 12, 1, 8), ("c300", 3, 4, 12, 3, 8), ("c5", 2, 1, 37, 0, 8),
          ("c5", 2, 3, 37, 2, 8), ("c3000", 2, 32, 256, 1, 32), ("c3000", 2, 32, 256, 2, 32),
          ("c3000", 2, 1, 256, 0, 32),
          ("c300", 2, 6, 12, 1, 8)]   # more than 4 beams: the 16-wave launch with idle waves


def draw_beams(corpus, g, B, kprev, V, P, pair_live=False):
    """One step's inputs from generator g (CPU tensors): beams on prefixes of random corpus rows, beam 1 of user 0 on
    beam 0's node, about one in six dead (node -1, parents -1; with pair_live never one of those two), logits 2 randn."""
    rows = torch.randint(0, corpus.ids.shape[0], (B, kprev), generator=g)
    if kprev > 1:
        rows[0, 1] = rows[0, 0]
    parents = parent_lp = node = None
    if P:
        live = torch.rand(B, kprev, generator=g) > 0.15
        live[:, 0] = True
        if pair_live:
            live[0, :2] = True
        parents = corpus.ids[rows][:, :, :P].clone()
        node = torch.tensor([[corpus.index[P][tuple(parents[b, j].tolist())] for j in range(kprev)] for b in range(B)],
                            dtype=torch.int32)
        parents[~live] = -1
        node[~live] = -1
        parent_lp = -(5.0 * torch.rand(B, kprev, generator=g)) - 0.1
    return dict(logits=2.0 * torch.randn(B * kprev, V, generator=g), node=node, parents=parents, parent_lp=parent_lp)


def wide_inputs(corpus, B, kprev, V, P, seed):
    """draw_beams with the two beams on one node both there, and no separation rule."""
    return draw_beams(corpus, torch.Generator().manual_seed(seed), B, kprev, V, P, pair_live=True)


_CASES = {}


def case(device, name, B, kprev, V, P, k, T):
    """Seeded inputs of one kernel case (draw_beams) and their reference, built once; a user whose top k + 1 scores
    are not separated has its logits redrawn from the same stream."""
    key = (torch.device(device).type, name, B, kprev, V, P, k, T)
    if key in _CASES:
        return _CASES[key]
    tok, corpus = tokenizer(name, device)
    g = torch.Generator().manual_seed(4000 + 97 * B + 31 * kprev + 7 * V + 3 * P + k + int(10 * T))
    c = draw_beams(corpus, g, B, kprev, V, P)
    logits = c["logits"]
    pre = c["parents"].tolist() if P else None
    live = (c["node"] >= 0).tolist() if P else [[True] * kprev] * B
    for _ in range(200):
        ref = expand_reference(corpus, log_softmax64(logits, T), pre, live, c["parent_lp"], B, kprev, V, P, k)
        bad = [b for b in range(B) if not separated(ref[4][b], k)]
        if not bad:
            break
        for b in bad:
            logits[b * kprev:(b + 1) * kprev] = 2.0 * torch.randn(kprev, V, generator=g)
    assert all(separated(s, k) for s in ref[4]), "precondition: separated scores"
    _CASES[key] = dict(c, tok=tok, ref=ref)
    return _CASES[key]


def expand(device, tok, c, B, k, P, T=1.0, **kw):
    """ops.beam_expand over tok's trie level P on the CPU tensors of case c."""
    from rqvae_hip import ops
    trie = tok.prefix_trie()
    return ops.beam_expand(c["logits"].to(device), k, batch=B, child_off=trie.child_off[P], tok=trie.tok[P + 1],
                           node=dev(c["node"], device), parents=dev(c["parents"], device),
                           parent_lp=dev(c["parent_lp"], device), temperature=T, **kw)


def assert_same(got, want, what=""):
    """(out_ids, out_lp, out_parent, out_node) bit for bit."""
    for g, w, name in zip(got, want, ("out_ids", "out_lp", "out_parent", "out_node")):
        g, w = g.cpu(), w.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}{name}"
        if name == "out_lp":
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), f"{what}{name}"


def assert_dead_rows(ids, lp, parent, node):
    dead = node < 0
    assert torch.equal(dead, (ids == -1).all(-1)) and torch.equal(dead, (ids == -1).any(-1))
    assert torch.isneginf(lp[dead]).all() and (parent[dead] == 0).all() and (node[dead] == -1).all()
    assert torch.equal(dead, torch.sort(dead.int(), dim=1, stable=True).values.bool()), "dead rows come last"


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
        n_pad = n_ch * step - kprev
        if n_pad:   # dead beams contribute no candidate
            logits = torch.cat([logits.view(B, kprev, V), torch.zeros(B, n_pad, V)], 1).reshape(-1, V)
            node = torch.cat([node, torch.full((B, n_pad), -1, dtype=node.dtype)], 1)
            parents = torch.cat([parents, torch.full((B, n_pad, P), -1, dtype=parents.dtype)], 1)
            plp = torch.cat([plp, torch.zeros(B, n_pad)], 1)
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


# ------------------------------------------------------------------------------------------ the model's own forwards
def beams_batch(model, cur, generated, first, k):
    """The next full forward's batch for the beams `generated` (B, k, i + 1), built as _ForwardSteps (modules/model.py)
    builds it: after the first step the users (and the cached encoder output) are repeated per beam."""
    from data.schemas import TokenizedSeqBatch
    from ops.jagged import jagged_to_padded_tensor, padded_to_jagged
    nxt = generated.flatten(end_dim=1)
    if not first:
        return TokenizedSeqBatch(user_ids=cur.user_ids, sem_ids=cur.sem_ids, sem_ids_fut=nxt,
                                 token_type_ids_fut=torch.arange(nxt.shape[1], device=nxt.device).repeat(nxt.shape[0], 1),
                                 seq_mask=cur.seq_mask, token_type_ids=cur.token_type_ids)
    enc = model.transformer.cached_enc_output
    n_ctx = cur.sem_ids.shape[1] + 1
    padded = jagged_to_padded_tensor(enc, n_ctx).repeat_interleave(k, dim=0)
    lengths = enc.offsets().diff().repeat_interleave(k)
    model.transformer.cached_enc_output = padded_to_jagged(padded.contiguous(), lengths, n_ctx)
    return TokenizedSeqBatch(user_ids=cur.user_ids.repeat_interleave(k, dim=0),
                             sem_ids=cur.sem_ids.repeat_interleave(k, dim=0), sem_ids_fut=nxt,
                             token_type_ids_fut=torch.zeros_like(nxt),
                             seq_mask=cur.seq_mask.repeat_interleave(k, dim=0),
                             token_type_ids=cur.token_type_ids.repeat_interleave(k, dim=0))


def first_batch(batch):
    from data.schemas import TokenizedSeqBatch
    return TokenizedSeqBatch(user_ids=batch.user_ids, sem_ids=batch.sem_ids, sem_ids_fut=None, seq_mask=batch.seq_mask,
                             token_type_ids=batch.token_type_ids, token_type_ids_fut=None)


def walk_forwards(model, batch, width, step_fn, state=None):
    """The model's own full forwards (eval mode) over `width` beams per user, one per token. After every forward
    step_fn(i, logits on the CPU, state) -> (new state, the beams' tokens so far (B, width, i + 1), every token a
    class the model can embed); the tokens make the next forward's batch. Train mode and the encoder cache are put
    back. Returns the last state."""
    B, L1, V = batch.sem_ids.shape[0], model.sem_id_dim, model.num_embeddings
    was_training = model.training
    model.eval()
    model.transformer.cached_enc_output = None
    try:
        with torch.no_grad():
            cur = first_batch(batch)
            for i in range(L1):
                logits = model.forward(cur).logits.cpu()
                assert logits.shape == (B * (1 if i == 0 else width), V)
                state, tokens = step_fn(i, logits, state)
                if i + 1 < L1:
                    cur = beams_batch(model, cur, tokens.to(batch.sem_ids.device), i == 0, width)
    finally:
        model.transformer.cached_enc_output = None
        model.train(was_training)
    return state


def reference_constrained(model, batch, corpus, k, T=1.0):
    """The constrained search with the expansion in fp64 on the CPU (dead beams' tokens clamped to 0 for the next
    forward). Asserts the separation precondition at every step. Returns ids (B, k, L1), fp64 log-probabilities (B, k)
    and the leaf nodes (B, k)."""
    B, V = batch.sem_ids.shape[0], model.num_embeddings

    def step(i, logits, state):
        kprev = 1 if i == 0 else k
        ids, lp, node = state or (None, None, None)
        live = [[True] * kprev] * B if i == 0 else (node >= 0).tolist()
        ids, lp, _, node, scores = expand_reference(corpus, log_softmax64(logits, T), None if i == 0 else ids.tolist(),
                                                    live, lp, B, kprev, V, i, k)
        assert all(separated(s, k) for s in scores), f"precondition: separated scores at step {i}"
        return (ids, lp, node), ids.clamp_min(0)
    return walk_forwards(model, batch, k, step)


_GEN = {}


def generation_case(golden, device, name):
    """(model with the tokenizer as its prefix index, batch, corpus, {k: reference}) of the generation fixture over
    corpus `name`; the references are computed once per corpus and shared by the expand, exclude, score and wide tests."""
    if name not in _GEN:
        z = golden("generation")
        tok, corpus = tokenizer(name, device, golden)
        model = decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]))
        model.enable_generation = True
        model.inference_prefix_index = tok
        batch = tokenized(z, device)
        _GEN[name] = (model, batch, corpus, {k: reference_constrained(model, batch, corpus, k) for k in (32, 1)})
    return _GEN[name]
