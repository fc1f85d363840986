"""Seen-item exclusion on the device: rq_trie_blocked_nodes against the tokenizer's CPU path, rq_beam_expand's blocked rows
against the unfiltered kernel with a host post-filter (bitwise) and against an fp64 reference over each user's
reduced corpus, generate_next_sem_id / recommend(exclude_items=...) against the fp64 loop over the reduced corpora,
rq_rank_hist against the CPU accumulator, and the evaluator's item-level switches."""
import glob

import numpy as np
import pytest
import torch

import beam_support as bs

pytestmark = pytest.mark.gpu


def _cpu_twin(tok):
    """A CPU tokenizer over the same corpus ids: blocked_nodes' plain-torch path (checked against the brute force in
    test_exclude_host)."""
    return bs.ids_tokenizer(tok.cached_ids.cpu())


# ------------------------------------------------------------------------------------------ blocked nodes
def _histories(corpus, B, H, seed):
    """User 0: every item under one level-1 node first (the whole subtree where H allows), then random items; the
    others: random items with duplicates, padding in between and out-of-range ids."""
    g = torch.Generator().manual_seed(seed)
    n = corpus.ids.shape[0]
    items = torch.randint(0, n, (B, H), generator=g)
    items[torch.rand(B, H, generator=g) < 0.2] = -1
    sub = bs.items_under(corpus, corpus.rows[int(torch.randint(0, n, (1,), generator=g))][:1])
    items[0, :min(H, len(sub))] = torch.tensor(sub[:H])
    if H >= 4:
        items[1, 1] = items[1, 0]
        items[1, 2], items[1, 3] = n, -9
    return items, len(sub) <= H, sub


@pytest.mark.parametrize("name,H", [("c3000", 1), ("c3000", 5), ("c3000", 64), ("c3000", 65), ("c3000", 200),
                                    ("c3000", 1024), ("c5", 3), ("c5", 8), ("c300", 40), ("c300", 300)])
def test_trie_blocked_nodes_matches_cpu_path(device, name, H):
    tok, corpus = bs.tokenizer(name, device)
    items, whole, sub = _histories(corpus, 3, H, seed=300 + H)
    if name == "c300" and H == 300:
        items[2] = torch.arange(300)          # everything: every node of every level
    want = _cpu_twin(tok).blocked_nodes(items)
    got = tok.blocked_nodes(items.to(device))
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (4, 3, H)
    assert torch.equal(got.cpu(), want)
    n_blocked = (want != bs.NONE).sum(-1)          # (D, B)
    print(f"{name} H={H}: blocked nodes per level and user {n_blocked.tolist()}")
    assert (n_blocked[3] > 0).any(), "listed items block their leaves"
    if H >= 40 or name == "c5":
        assert whole and corpus.index[1][corpus.rows[sub[0]][:1]] in want[0, 0].tolist(), "the whole-subtree user"
    if name == "c300" and H == 300:
        assert [int(v) for v in n_blocked[:, 2]] == [len(corpus.index[q]) for q in range(1, 5)]


def test_trie_blocked_nodes_refusals(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = bs.tokenizer("c5", device)
    idx = tok.trie_index()
    with pytest.raises(RqHipError, match="rc=-22|envelope"):
        tok.blocked_nodes(torch.zeros((2, 1025), dtype=torch.int64, device=device))
    with pytest.raises(RqHipError, match="items must be a contiguous torch.int64"):
        ops.trie_blocked_nodes(torch.zeros((2, 3), dtype=torch.int32, device=device), idx.item_leaf, idx.leaf_anc,
                               idx.leaf_count)
    with pytest.raises(RqHipError, match="envelope"):
        ops.trie_blocked_nodes(torch.zeros((2, 3), dtype=torch.int64, device=device), idx.item_leaf, idx.leaf_anc * 3,
                               idx.leaf_count * 3)      # D = 12 > RQ_BEAM_MAX_T
    assert tok.blocked_nodes(torch.zeros((2, 0), dtype=torch.int64, device=device)).shape == (4, 2, 0)
    assert tok.blocked_nodes(torch.zeros((0, 3), dtype=torch.int64, device=device)).shape == (4, 0, 3)


# ------------------------------------------------------------------------------------------ filtered expand
_EXCL = {}


def _reduced_reference(corpus, c, items, logits, B, kprev, V, P, k, T):
    """expand_reference per user over the Corpus of the rows that remain; nodes in the full corpus' index."""
    lp64 = bs.log_softmax64(logits, T)
    pre = c["parents"].tolist() if P else None
    live = (c["node"] >= 0).tolist() if P else [[True] * kprev] * B
    out = []
    for b in range(B):
        gone = {corpus.rows[i] for i in items[b].tolist() if i >= 0}
        left = [r for r in corpus.rows if r not in gone]
        ids = torch.full((1, k, P + 1), -1, dtype=torch.int64)
        res = (ids, torch.full((1, k), -float("inf"), dtype=torch.float64), torch.zeros((1, k), dtype=torch.int64),
               torch.full((1, k), -1, dtype=torch.int64), [[]])
        if left:
            res = bs.expand_reference(bs.Corpus(torch.tensor(left)), lp64[b * kprev:(b + 1) * kprev],
                                      None if pre is None else pre[b:b + 1], live[b:b + 1],
                                      None if not P else c["parent_lp"][b:b + 1], 1, kprev, V, P, k)
        node = torch.tensor([[corpus.index[P + 1][tuple(r)] if r[0] >= 0 else -1 for r in res[0][0].tolist()]])
        out.append((res[0], res[1], res[2], node, res[4][0]))
    return out


def _excl_case(device, name, B, kprev, V, P, k, T=1.0):
    """beam_support.case's beams with histories drawn from each user's own best beams: every item under the
    node of its unfiltered rank 0 (and rank 2 where it has six candidates or more) — blocked —, one item of rank 1's
    subtree where that holds several rows — not blocked — and, in the larger corpora, two random items. A user whose
    top k + 1 scores, before or after the exclusion, are not separated is redrawn from the same stream. Built once."""
    key = (name, B, kprev, V, P, k, T)
    if key in _EXCL:
        return _EXCL[key]
    c = bs.case(device, name, B, kprev, V, P, k, T)
    corpus = bs.tokenizer(name, device)[1]
    g = torch.Generator().manual_seed(9000 + 97 * B + 31 * kprev + 7 * V + 3 * P + k)
    logits = c["logits"].clone()
    pre = c["parents"].tolist() if P else None
    live = (c["node"] >= 0).tolist() if P else [[True] * kprev] * B
    n = corpus.ids.shape[0]
    extra = torch.randint(0, n, (B, 2), generator=g).tolist()
    todo = list(range(B))
    for _ in range(200):
        full = bs.expand_reference(corpus, bs.log_softmax64(logits, T), pre, live, c["parent_lp"], B, kprev, V, P, k)
        lists = []
        for b in range(B):
            paths = [tuple(r) for r in full[0][b].tolist() if r[0] >= 0]
            l = [i for r in ((0, 2) if len(full[4][b]) >= 6 else (0,)) for i in bs.items_under(corpus, paths[r])]
            under = bs.items_under(corpus, paths[1]) if len(paths) > 1 else []
            if len({corpus.rows[i] for i in under}) > 1:
                l.append(under[0])
            lists.append(l + (extra[b] if n >= 300 else []))
        items = bs.pad(lists)
        ref = _reduced_reference(corpus, c, items, logits, B, kprev, V, P, k, T)
        todo = [b for b in range(B) if not (bs.separated(full[4][b], k) and bs.separated(ref[b][4], k))]
        if not todo:
            break
        for b in todo:
            logits[b * kprev:(b + 1) * kprev] = 2.0 * torch.randn(kprev, V, generator=g)
    assert not todo, "precondition: separated scores"
    blocked = _cpu_twin(c["tok"]).blocked_nodes(items)[P]
    _EXCL[key] = dict(c, logits=logits, items=items, blocked=blocked, ref=ref)
    return _EXCL[key]


@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_beam_expand_blocked_equals_postfilter(device, name, B, kprev, V, P, k):
    """Every candidate from the unfiltered kernel (k = kprev V), the rows on a blocked node dropped on the host, the
    first k kept: bitwise what the filtered kernel returns."""
    c = _excl_case(device, name, B, kprev, V, P, k)
    every = [t.cpu() for t in bs.expand(device, c["tok"], c, B, kprev * V, P)]
    got = [t.cpu() for t in bs.expand(device, c["tok"], c, B, k, P, blocked=c["blocked"].to(device))]
    removed = []
    for b in range(B):
        gone = set(c["blocked"][b].tolist()) - {bs.NONE}
        keep = torch.tensor([int(v) >= 0 and int(v) not in gone for v in every[3][b]])
        removed.append(int((~keep[:k] & (every[3][b, :k] >= 0)).sum()))
        idx = keep.nonzero().flatten()[:k]
        want_ids = torch.full((k, P + 1), -1, dtype=torch.int64)
        want_lp = torch.full((k,), -float("inf"))
        want_parent, want_node = torch.zeros(k, dtype=torch.int32), torch.full((k,), -1, dtype=torch.int32)
        m = idx.numel()
        want_ids[:m], want_lp[:m], want_parent[:m], want_node[:m] = (every[0][b, idx], every[1][b, idx],
                                                                     every[2][b, idx], every[3][b, idx])
        bs.assert_same([t[b] for t in got], (want_ids, want_lp, want_parent, want_node), f"user {b}: ")
    print(f"{name} B={B} kprev={kprev} V={V} P={P} k={k}: candidates removed from the top k per user {removed}, "
          f"H={c['items'].shape[1]}")
    assert all(r > 0 for r in removed), "the filter removes candidates from every user's top k"
    bs.assert_dead_rows(*got)


@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_beam_expand_blocked_noop(device, name, B, kprev, V, P, k):
    c = bs.case(device, name, B, kprev, V, P, k, 1.0)
    plain = bs.expand(device, c["tok"], c, B, k, P)
    for blocked in (torch.full((B, 8), bs.NONE, dtype=torch.int32, device=device),
                    torch.zeros((B, 0), dtype=torch.int32, device=device)):   # n_blocked = 0: a null pointer
        got = bs.expand(device, c["tok"], c, B, k, P, blocked=blocked)
        bs.assert_same(got, plain)


@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_beam_expand_blocked_vs_fp64(device, name, B, kprev, V, P, k):
    c = _excl_case(device, name, B, kprev, V, P, k)
    assert all(bs.separated(r[4], k) for r in c["ref"]), "precondition: separated scores"
    ids, lp, parent, node = (t.cpu() for t in bs.expand(device, c["tok"], c, B, k, P, blocked=c["blocked"].to(device)))
    want_ids, want_lp, want_parent, want_node = (torch.cat([r[j] for r in c["ref"]]) for j in range(4))
    live = want_node >= 0
    print(f"{name} B={B} kprev={kprev} V={V} P={P} k={k}: remaining candidates per user {[len(r[4]) for r in c['ref']]}, "
          f"max rel lp err {float(((lp.double() - want_lp).abs() / want_lp.abs())[live].max()):.3e}")
    assert torch.equal(ids, want_ids), "out_ids"
    assert torch.equal(parent.long(), want_parent), "out_parent"
    assert torch.equal(node.long(), want_node), "out_node (full corpus index)"
    np.testing.assert_allclose(lp.double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    bs.assert_dead_rows(ids, lp, parent, node)


def test_beam_expand_blocked_refusals(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    x = torch.zeros(2, 16, device=device)
    lvl0 = dict(child_off=trie.child_off[0], tok=trie.tok[1])
    ok = torch.full((2, 4), bs.NONE, dtype=torch.int32, device=device)
    assert ops.beam_expand(x, 3, batch=2, **lvl0, blocked=ok)[0].shape == (2, 3, 1)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand(x, 3, batch=2, **lvl0, blocked=ok.cpu())
    with pytest.raises(RqHipError, match="blocked must be a contiguous torch.int32"):
        ops.beam_expand(x, 3, batch=2, **lvl0, blocked=ok.long())
    with pytest.raises(RqHipError, match=r"blocked must be \(B, n_blocked <= 1024\)"):
        ops.beam_expand(x, 3, batch=2, **lvl0, blocked=ok[:1])
    with pytest.raises(RqHipError, match=r"blocked must be \(B, n_blocked <= 1024\)"):
        ops.beam_expand(x, 3, batch=2, **lvl0, blocked=torch.zeros((2, 1025), dtype=torch.int32, device=device))
    # an unsorted row filters unspecified children but stays inside the row; a whole level blocked leaves dead rows
    rev = torch.tensor([[1, 0], [1, 0]], dtype=torch.int32, device=device)
    assert ops.beam_expand(x, 3, batch=2, **lvl0, blocked=rev)[0].shape == (2, 3, 1)
    every = torch.tensor([[0, 1], [0, bs.NONE]], dtype=torch.int32, device=device)
    ids, lp, parent, node = ops.beam_expand(x, 3, batch=2, **lvl0, blocked=every)
    assert (ids[0] == -1).all() and torch.isneginf(lp[0]).all() and ids[1, :, 0].tolist() == [3, -1, -1]
    bs.assert_dead_rows(ids.cpu(), lp.cpu(), parent.cpu(), node.cpu())


# ------------------------------------------------------------------------------------------ generation
def _reference_excluded(model, batch, corpus, items, k, T=1.0):
    """beam_support.walk_forwards (the model's own forwards, the expansion in fp64 on the CPU) with every user
    expanded over its own reduced corpus. Returns ids (B, k, L1), fp64 log-probabilities (B, k) — dead rows -1 / -inf —
    and whether the separation precondition held for every user at every step."""
    B, V = batch.sem_ids.shape[0], model.num_embeddings
    left = []
    for b in range(B):
        gone = {corpus.rows[i] for i in items[b].tolist() if i >= 0}
        rows = [r for r in corpus.rows if r not in gone]
        left.append(bs.Corpus(torch.tensor(rows)) if rows else None)

    def step(i, logits, state):
        ids, lp, separated = state
        kprev = 1 if i == 0 else k
        lp64 = bs.log_softmax64(logits, T)
        new_ids = torch.full((B, k, i + 1), -1, dtype=torch.int64)
        new_lp = torch.full((B, k), -float("inf"), dtype=torch.float64)
        for b in range(B):
            if left[b] is None:
                continue
            live = [[True]] if i == 0 else [(ids[b, :, 0] >= 0).tolist()]
            r = bs.expand_reference(left[b], lp64[b * kprev:(b + 1) * kprev], None if i == 0 else ids[b:b + 1].tolist(),
                                    live, None if i == 0 else lp[b:b + 1], 1, kprev, V, i, k)
            separated = separated and bs.separated(r[4][0], k)
            new_ids[b], new_lp[b] = r[0][0], r[1][0]
        return (new_ids, new_lp, separated), new_ids.clamp_min(0)
    return bs.walk_forwards(model, batch, k, step, (None, None, True))


_GEN = {}


def _gen_case(golden, device, name):
    """The generation fixture's model / batch over corpus `name`, histories from every user's own unfiltered beams
    (user 0: the items of three of its best beams; user 1: every item; user 2: the whole level-1 subtree of one of its
    best beams), and the fp64 reference over the reduced corpora. The beams the histories start from move down the
    ranking until the reference's top k + 1 scores are separated at every step (the precondition, asserted). Built
    once."""
    if name not in _GEN:
        model, batch, corpus, refs = bs.generation_case(golden, device, name)
        best = refs[32][0]
        n = corpus.ids.shape[0]
        for v in range(8):
            lists = [[i for r in range(v, v + 3) for i in bs.items_under(corpus, best[0, r].tolist()) if best[0, r, 0] >= 0],
                     list(range(n)),
                     bs.items_under(corpus, best[2, v if best[2, v, 0] >= 0 else 0, :1].tolist())]
            items = bs.pad(lists)
            ids, lp, separated = _reference_excluded(model, batch, corpus, items, 32)
            if separated:
                break
        assert separated, "precondition: separated scores at every step"
        print(f"{name}: histories from beam rank {v}, lengths {[len(l) for l in lists]}")
        _GEN[name] = (model, batch, corpus, items, (ids, lp))
    return _GEN[name]


@pytest.mark.parametrize("name", ["c300", "c5"])
def test_generation_excluding_items_vs_fp64_loop(golden, device, name):
    model, batch, corpus, items, (want_ids, want_lp) = _gen_case(golden, device, name)
    plain = bs.generation_case(golden, device, name)[3][32][0]
    assert not torch.equal(want_ids[0], plain[0]) and (want_ids[0] >= 0).all() == (name == "c300")
    assert (want_ids[1] == -1).all(), "a history that covers the corpus leaves nothing"
    rng = torch.cuda.get_rng_state()
    kw = dict(temperature=1, top_k=True, fused=True, sample=False, constrained=True, exclude_items=items.to(device))
    for incremental in (False, True):
        got = model.generate_next_sem_id(batch, incremental=incremental, **kw)
        assert model.training and model.transformer.cached_enc_output is None
        assert torch.equal(torch.cuda.get_rng_state(), rng), "no generator draw"
        assert torch.equal(got.sem_ids.cpu(), want_ids), f"beams (incremental={incremental})"
        np.testing.assert_allclose(got.log_probas.cpu().double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", ["c300", "c5"])
def test_recommend_excluding_items(golden, device, name):
    model, batch, corpus, items, (want_ids, want_lp) = _gen_case(golden, device, name)
    V, k = model.num_embeddings, 10
    rng = torch.cuda.get_rng_state()
    rec = model.recommend(batch, k=k, exclude_items=items.to(device))
    assert torch.equal(torch.cuda.get_rng_state(), rng) and model.training
    assert rec.item_ids.shape == (3, k) and torch.equal(rec.sem_ids.cpu(), want_ids[:, :k])
    np.testing.assert_allclose(rec.log_probas.cpu().double().numpy(), want_lp[:, :k].numpy(), rtol=1e-5, atol=0)
    got_items, sem = rec.item_ids.cpu(), rec.sem_ids.cpu()
    for b in range(3):
        gone = {corpus.rows[i] for i in items[b].tolist() if i >= 0}
        reachable = {r for r in corpus.rows if r not in gone and max(r) < V}
        live = got_items[b] >= 0
        assert int(live.sum()) == min(k, len(reachable)), "exactly the remaining reachable items, up to k"
        assert torch.equal(live, torch.sort(live.int(), descending=True, stable=True).values.bool()), "dead rows last"
        assert (sem[b][~live] == -1).all() and torch.isneginf(rec.log_probas.cpu()[b][~live]).all()
        listed = {i for i in items[b].tolist() if i >= 0}
        for it, row in zip(got_items[b][live].tolist(), sem[b][live].tolist()):
            assert it not in listed and corpus.rows[it] not in gone, "no listed item, no duplicate of a listed row"
            assert corpus.rows[it] == tuple(row) and it == corpus.first_row[tuple(row)], "item_ids consistent with sem_ids"
        assert len(set(got_items[b][live].tolist())) == int(live.sum())
    assert (got_items[1] == -1).all(), "everything seen: all results dead"
    full = model.recommend(batch, k=32, incremental=False, exclude_items=items.to(device))
    assert torch.equal(full.sem_ids.cpu(), want_ids) and torch.equal(full.item_ids[:, :k], rec.item_ids)
    none = model.recommend(batch, k=k, exclude_items=torch.full((3, 4), -1, device=device))
    assert torch.equal(none.item_ids, model.recommend(batch, k=k).item_ids), "an all-padding history excludes nothing"


# ------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("B", [1, 67])
def test_rank_hist_matches_cpu_accumulator(device, B, k, D):
    from evaluate.metrics import RankAccumulator
    g = torch.Generator().manual_seed(100 * B + 10 * k + D)
    cpu, gpu = RankAccumulator(ks=[1, 5, 10]), RankAccumulator(ks=[1, 5, 10])
    for call in range(2):   # two calls back to back: the histogram accumulates, nothing is read in between
        hi = 3 if D == 4 else 40
        actual = torch.randint(0, hi, (B, D), generator=g)
        topk = torch.randint(0, hi, (B, k, D), generator=g)
        topk[torch.rand(B, k, generator=g) < 0.2] = -1            # dead beams
        if B > 1:
            actual[3::9] = -1                                      # rows without a target
            topk[5, k // 2:] = actual[5]                           # repeated matches: the first counts
        a, t = (actual[:, 0], topk[:, :, 0]) if D == 1 and call == 0 else (actual, topk)   # ids and 1-tuples
        cpu.accumulate(a, t)
        gpu.accumulate(a.to(device), t.to(device))
    assert gpu.hists[k].is_cuda and gpu.hists[k].dtype == torch.int64
    assert torch.equal(gpu.hists[k].cpu(), cpu.hists[k])
    assert int(cpu.hists[k].sum()) == 2 * (B - len(range(3, B, 9)) if B > 1 else 1)
    if B > 1 and k > 1:
        assert int(cpu.hists[k][:k].sum()) > 0 and int(cpu.hists[k][k]) > 0, "hits and misses both occur"
    assert gpu.reduce() == cpu.reduce()


def test_rank_hist_refusals(device):
    from rqvae_hip import ops, RqHipError
    a = torch.zeros((2, 4), dtype=torch.int64, device=device)
    t = torch.zeros((2, 3, 4), dtype=torch.int64, device=device)
    with pytest.raises(RqHipError, match="hist must have shape"):
        ops.rank_hist(a, t, torch.zeros(3, dtype=torch.int64, device=device))
    with pytest.raises(RqHipError, match="need actual"):
        ops.rank_hist(a, t[:, :, :3].contiguous(), torch.zeros(4, dtype=torch.int64, device=device))
    with pytest.raises(RqHipError, match="rc=-22"):
        ops.rank_hist(a[:, :1].contiguous(), torch.zeros((2, 1025, 1), dtype=torch.int64, device=device),
                      torch.zeros(1026, dtype=torch.int64, device=device))
    h = ops.rank_hist(a, t, torch.zeros(4, dtype=torch.int64, device=device))
    assert h.tolist() == [2, 0, 0, 0]


# ------------------------------------------------------------------------------------------ evaluator
def test_train_decoder_item_metrics(tmp_path, device, capsys, monkeypatch):
    """The full eval with the constrained / item-metric / exclude-seen switches on adds recall / ndcg / mrr @ 1, 5, 10
    to its output and leaves the trained parameters bitwise what the same run with today's defaults gives; with the
    defaults the output keys are today's (test_eval_train_gpu's pattern)."""
    import data.processed as processed
    import train_decoder
    import train_rqvae
    from data.processed import RecDataset
    from modules.quantize import QuantizeForwardMode
    from rqvae_hip import ops
    monkeypatch.setitem(processed.SYNTHETIC_N_USERS, RecDataset.AMAZON, 80)   # 3 eval batches of 32 (the last short)
    vae = dict(vae_input_dim=768, vae_embed_dim=32, vae_hidden_dims=[512, 256, 128], vae_codebook_size=256,
               vae_n_cat_feats=0, vae_n_layers=3)
    np.random.seed(1)
    train_rqvae.train(iterations=10, batch_size=256, dataset=RecDataset.AMAZON, do_eval=False, save_model_every=10,
                      vae_codebook_mode=QuantizeForwardMode.ROTATION_TRICK, save_dir_root=str(tmp_path / "vae") + "/",
                      **vae)
    ckpt = sorted(glob.glob(str(tmp_path / "vae" / "checkpoint_*.pt")))[-1]
    kw = dict(iterations=2, batch_size=32, learning_rate=0.0003, dataset=RecDataset.AMAZON, pretrained_rqvae_path=ckpt,
              decoder_embed_dim=64, dropout_p=0.3, attn_heads=4, attn_embed_dim=128, attn_layers=4,
              save_dir_root=str(tmp_path) + "/", save_model_every=10 ** 9, log_every=2, seed=0,
              partial_eval_every=10 ** 9, full_eval_every=2, **vae)

    def run(**switches):
        ops._SEED.update(base=None, n=0)
        ops.seed_epoch_set(0)
        with monkeypatch.context() as m:
            for name, value in switches.items():
                m.setattr(train_decoder, name, value)
            model = train_decoder.train(**kw)
        return model, dict(train_decoder.LAST_RUN["eval"])

    assert not (train_decoder.EVAL_ITEM_METRICS or train_decoder.EVAL_EXCLUDE_SEEN), "both default to off"
    capsys.readouterr()
    m_on, ev = run(EVAL_CONSTRAINED_GENERATION=True, EVAL_ITEM_METRICS=True, EVAL_EXCLUDE_SEEN=True)
    printed = capsys.readouterr().out
    new = [f"{name}@{k}" for k in (1, 5, 10) for name in ("recall", "ndcg", "mrr")]
    hit = [f"h@{k}_{name}" for i in range(4) for name in (f"slice_:{i + 1}", f"pos_{i}") for k in (1, 5, 10)]
    assert set(ev) == set(new) | set(hit) | {"full_eval_iter"}
    assert all(0.0 <= ev[key] <= 1.0 for key in new) and "'recall@10'" in printed and "'ndcg@5'" in printed
    for name in ("recall", "ndcg", "mrr"):
        assert ev[f"{name}@1"] <= ev[f"{name}@5"] <= ev[f"{name}@10"]
    for k in (1, 5, 10):
        assert ev[f"mrr@{k}"] <= ev[f"ndcg@{k}"] <= ev[f"recall@{k}"]
    assert ev["recall@1"] == ev["ndcg@1"] == ev["mrr@1"]
    assert m_on.training and not m_on.enable_generation and m_on.transformer.cached_enc_output is None
    m_off, ev_off = run()
    assert set(ev_off) == set(hit) | {"full_eval_iter"}, "with the defaults the output keys are today's"
    on = dict(m_on.named_parameters())
    for n, p in m_off.named_parameters():
        assert torch.equal(p.detach(), on[n].detach()), f"{n}: the item-level evaluation perturbed training"
