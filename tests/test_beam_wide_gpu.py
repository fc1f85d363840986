"""Wide constrained beam search on the device: rq_beam_expand_wide bit for bit against rq_beam_expand (with and without
blocked rows) where both take the shape, against the chunk-merge of narrow-kernel calls beyond that (test_beam_wide_host checks the
merge itself), its ties / underflow / bad-table behaviour and refusals, an fp64 reference at 96 beams; then
generate_next_sem_id / recommend(beams=...) up to an exhaustive search of the corpus, and the evaluator's switches."""
import glob

import numpy as np
import pytest
import torch

import beam_support as bs

pytestmark = pytest.mark.gpu


def _blocked_from(device, tok, corpus, ids, P):
    """A blocked row per user from tok.blocked_nodes: every item below the unfiltered ranks 0 and 2 (both nodes become
    blocked), one item below rank 1 and two fixed items (blocked only where they are the node's last leaves)."""
    lists = []
    for b in range(ids.shape[0]):
        paths = [r for r in ids[b].tolist() if r[0] >= 0]
        l = [i for r in (0, 2) if r < len(paths) for i in bs.items_under(corpus, paths[r])]
        lists.append(l + (bs.items_under(corpus, paths[1])[:1] if len(paths) > 1 else []) + [7 % len(corpus.rows), 1])
    return tok.blocked_nodes(bs.pad(lists).to(device))[P].contiguous()


_INPUTS = {}


def _inputs(device, name, B, kprev, V, P, seed=0):
    key = (name, B, kprev, V, P, seed)
    if key not in _INPUTS:
        tok, corpus = bs.tokenizer(name, device)
        _INPUTS[key] = (tok, corpus, bs.wide_inputs(corpus, B, kprev, V, P, 5000 + 31 * kprev + 3 * P + B + seed))
    return _INPUTS[key]


# ------------------------------------------------------------------------------------------ 1. the same bits
_DENSE = bs.SHAPES + [("c300", 2, 64, 12, P, 64) for P in (1, 2, 3)]   # 768 keys, more than 32 beams


@pytest.mark.parametrize("with_blocked", [False, True], ids=["plain", "blocked"])
@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("name,B,kprev,V,P,k", _DENSE)
def test_wide_equals_narrow_bitwise(device, name, B, kprev, V, P, k, T, with_blocked):
    if kprev == 64:
        tok, corpus, c = _inputs(device, name, B, kprev, V, P)
    else:
        c = bs.case(device, name, B, kprev, V, P, k, T)
        tok, corpus = bs.tokenizer(name, device)
    kw = {}
    plain = bs.expand(device, tok, c, B, k, P, T, wide=False)
    if with_blocked:
        kw["blocked"] = _blocked_from(device, tok, corpus, plain[0].cpu(), P)
        assert (kw["blocked"] != bs.NONE).any(1).all(), "every user has blocked nodes"
    narrow = bs.expand(device, tok, c, B, k, P, T, wide=False, **kw)
    wide = bs.expand(device, tok, c, B, k, P, T, wide=True, **kw)
    bs.assert_same(wide, narrow)
    if with_blocked:
        assert all(not torch.equal(narrow[0][b], plain[0][b]) for b in range(B)), "the filter removes top candidates"
    bs.assert_dead_rows(*(t.cpu() for t in wide))


# ------------------------------------------------------------------------------------------ 2. beyond the old envelope
def _narrow_step(device, tok, P, T=1.0, blocked=None):
    """chunk_merge's step function on the narrow kernel; `blocked` (B, H) is repeated for every chunk of a user."""
    def expand(logits, node, parents, plp, batch, kprev, k):
        blk = None if blocked is None else blocked.repeat_interleave(batch // blocked.shape[0], dim=0).contiguous()
        out = bs.expand(device, tok, dict(logits=logits, node=node, parents=parents, parent_lp=plp), batch, k, P, T,
                        blocked=blk, wide=False)
        return tuple(t.cpu() for t in out)
    return expand


# B, kprev, P, k on c3000 at V = 256
_BEYOND = [(2, 96, 1, 96), (2, 96, 2, 96), (2, 96, 3, 96), (2, 96, 2, 7), (2, 40, 2, 1024), (1, 1024, 2, 1024),
           (1, 1024, 3, 1000), (2, 1, 0, 300),
           (1, 1024, 1, 1024)]   # about eleven children per beam: the cut falls inside some ten thousand candidates


@pytest.mark.parametrize("B,kprev,P,k", _BEYOND)
def test_wide_equals_chunk_merge(device, B, kprev, P, k):
    V = 256
    tok, corpus, c = _inputs(device, "c3000", B, kprev, V, P)
    want = bs.chunk_merge(_narrow_step(device, tok, P), c, B, kprev, V, P, k)
    got = bs.expand(device, tok, c, B, k, P, wide=True)
    n_live = (want[3] >= 0).sum(1).tolist()
    print(f"c3000 B={B} kprev={kprev} P={P} k={k}: live rows per user {n_live}")
    bs.assert_same(got, want)
    if P:
        assert (c["node"] < 0).any() and c["node"][0, 0] == c["node"][0, 1], "dead beams; two beams on one node"
        auto = bs.expand(device, tok, c, B, k, P, wide=None)   # kprev V > 8192: the dispatch picks the wide kernel
        bs.assert_same(auto, want, "wide=None: ")
    if (kprev, k) == (40, 1024) or P == 0:
        assert all(0 < n < k for n in n_live), "k exceeds the candidates: the tail is dead rows"
        assert P or all(n <= V for n in n_live)
    bs.assert_dead_rows(*(t.cpu() for t in got))


def test_wide_blocked_equals_chunk_merge(device):
    B, kprev, V, P, k = 2, 96, 256, 2, 96
    tok, corpus, c = _inputs(device, "c3000", B, kprev, V, P)
    plain = bs.chunk_merge(_narrow_step(device, tok, P), c, B, kprev, V, P, k)
    blocked = _blocked_from(device, tok, corpus, plain[0], P)
    want = bs.chunk_merge(_narrow_step(device, tok, P, blocked=blocked), c, B, kprev, V, P, k)
    assert all(not torch.equal(want[0][b], plain[0][b]) for b in range(B)), "the filter removes top candidates"
    bs.assert_same(bs.expand(device, tok, c, B, k, P, wide=True, blocked=blocked), want)
    rev = blocked.flip(1).contiguous()   # unsorted: the wrong children are filtered, nothing is read outside the row
    assert bs.expand(device, tok, c, B, k, P, wide=True, blocked=rev)[0].shape == (B, k, P + 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 3. ties at the cut
@pytest.mark.parametrize("k", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("flat", [False, True], ids=["random-row", "equal-logits"])
def test_wide_ties_two_beams_on_one_node(device, k, flat):
    """Two beams on node (3,) of the five-row corpus with one logits row and one parent score: children 0 and 1 of
    each, so every score appears twice (random row) or four times (all-equal logits) and the cut falls between equal
    keys: the lower beam's copy, then the lower token, is kept."""
    tok, corpus = bs.tokenizer("c5", device)
    n3 = corpus.index[1][(3,)]
    row = torch.zeros(16) if flat else 2.0 * torch.randn(16, generator=torch.Generator().manual_seed(3))
    c = dict(logits=row.repeat(2, 1), node=torch.tensor([[n3, n3]], dtype=torch.int32),
             parents=torch.tensor([[[3], [3]]]), parent_lp=torch.full((1, 2), -0.5))
    narrow = bs.expand(device, tok, c, 1, k, 1, wide=False)
    wide = bs.expand(device, tok, c, 1, k, 1, wide=True)
    bs.assert_same(wide, narrow)
    ids, lp, parent, node = (t.cpu() for t in wide)
    first = 0 if flat or row[0] >= row[1] else 1
    order = ([(0, 0), (0, 1), (1, 0), (1, 1)] if flat else
             [(0, first), (1, first), (0, 1 - first), (1, 1 - first)])[:k]
    assert parent[0, :4].tolist() == [j for j, _ in order] and ids[0, :4, 1].tolist() == [v for _, v in order]
    assert node[0, :4].tolist() == [corpus.index[2][(3, v)] for _, v in order]
    assert (node[0, 4:] == -1).all() and torch.isneginf(lp[0, 4:]).all()


@pytest.mark.parametrize("k", [50, 51, 96])
def test_wide_ties_across_chunks(device, k):
    """Beams 48..95 repeat beams 0..47 (node, parent score, logits row): every score appears twice, 48 beams — more
    than one narrow-kernel chunk — apart; an odd k cuts between the two copies of a child."""
    B, kprev, V, P = 2, 96, 256, 2
    tok, corpus, c = _inputs(device, "c3000", B, kprev, V, P, seed=1)
    c = {key: t.clone() for key, t in c.items()}
    for key in ("node", "parents", "parent_lp"):
        c[key][:, 48:] = c[key][:, :48]
    x = c["logits"].view(B, kprev, V)
    x[:, 48:] = x[:, :48]
    want = bs.chunk_merge(_narrow_step(device, tok, P), c, B, kprev, V, P, k)
    assert all(want[2][b, 1] == want[2][b, 0] + 48 and want[1][b, 0] == want[1][b, 1] for b in range(B)), "pairs"
    bs.assert_same(bs.expand(device, tok, c, B, k, P, wide=True), want)


def test_wide_underflow_ranks_above_dead_rows(device):
    tok, corpus = bs.tokenizer("c5", device)
    x = torch.full((1, 16), -200.0)
    x[0, 3] = 0.0
    c = dict(logits=x, node=None, parents=None, parent_lp=None)
    wide = bs.expand(device, tok, c, 1, 4, 0, wide=True)
    bs.assert_same(wide, bs.expand(device, tok, c, 1, 4, 0, wide=False))
    ids, lp, parent, node = (t.cpu() for t in wide)
    assert ids[0].tolist() == [[3], [0], [-1], [-1]] and lp[0, 0] == 0 and torch.isneginf(lp[0, 1:]).all()
    assert node[0].tolist() == [corpus.index[1][(3,)], corpus.index[1][(0,)], -1, -1] and parent[0].tolist() == [0] * 4


# ------------------------------------------------------------------------------------------ 4. fp64
@pytest.mark.parametrize("P", [1, 2])
def test_wide_vs_fp64(device, P):
    name, B, kprev, V, k, T = "c3000", 2, 96, 256, 40, 1.0
    c = bs.case(device, name, B, kprev, V, P, k, T)   # its separation rule and redraw loop
    want_ids, want_lp, want_parent, want_node, scores = c["ref"]
    ids, lp, parent, node = (t.cpu() for t in bs.expand(device, c["tok"], c, B, k, P, T, wide=True))
    print(f"{name} B={B} kprev={kprev} V={V} P={P} k={k}: candidates per user {[len(s) for s in scores]}, "
          f"max rel lp err {float(((lp.double() - want_lp).abs() / want_lp.abs())[want_node >= 0].max()):.3e}")
    assert torch.equal(ids, want_ids), "out_ids"
    assert torch.equal(parent.long(), want_parent), "out_parent"
    assert torch.equal(node.long(), want_node), "out_node"
    np.testing.assert_allclose(lp.double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------ 5. bad tables, refusals
def test_wide_bad_tables_stay_in_bounds(device):
    """test_beam_expand_bad_tables_stay_in_bounds' malformed tables through the wide kernel: the same candidates
    survive; then a child range that repeats a token (equal keys: which copy wins is unspecified, every row is a real
    child or dead)."""
    from rqvae_hip import ops
    V, k = 8, 6
    tok = torch.tensor([0, 5, 40, 2, 7, -3], dtype=torch.int32, device=device)
    child_off = torch.tensor([-4, 3, 99, 4], dtype=torch.int32, device=device)   # node 0: [0, 3), 1: [3, 6), 2: [6, 4)
    node = torch.tensor([[0, 1, 2, 3, -1, 7]], dtype=torch.int32, device=device)
    g = torch.Generator().manual_seed(11)
    logits = 2.0 * torch.randn(6, V, generator=g)
    parents = torch.arange(6).reshape(1, 6, 1)
    plp = -torch.rand(1, 6, generator=g)
    args = dict(batch=1, child_off=child_off, tok=tok, node=node, parents=parents.to(device), parent_lp=plp.to(device))
    wide = ops.beam_expand(logits.to(device), k, wide=True, **args)
    torch.cuda.synchronize()
    bs.assert_same(wide, ops.beam_expand(logits.to(device), k, wide=False, **args))
    ids, lp, parent, out_node = (t.cpu() for t in wide)
    assert sorted(zip(parent[0, :4].tolist(), ids[0, :4, 1].tolist(), out_node[0, :4].tolist())) == \
        [(0, 0, 0), (0, 5, 1), (1, 2, 3), (1, 7, 4)]
    assert (ids[0, 4:] == -1).all() and torch.isneginf(lp[0, 4:]).all() and out_node[0, 4:].tolist() == [-1, -1]
    # a range longer than V whose tokens do not ascend, and a repeated token
    tok = torch.tensor([2, 2, 5, 2, 1, 1, 1, 1, 1, 1, 1, 1], dtype=torch.int32, device=device)
    child_off = torch.tensor([0, 12], dtype=torch.int32, device=device)
    for kk in (2, 5, 20):
        ids, lp, parent, out_node = (t.cpu() for t in ops.beam_expand(
            logits[:2].to(device), kk, batch=1, child_off=child_off, tok=tok, node=node[:, :2].clamp_max(0).contiguous(),
            parents=parents[:, :2].to(device), parent_lp=plp[:, :2].to(device), wide=True))
        torch.cuda.synchronize()
        live = out_node[0] >= 0
        assert live[:min(kk, 2)].all() and ((out_node[0] < 12) & (parent[0] >= 0) & (parent[0] < 2)).all()
        assert all(int(tok[n]) == v for n, v in zip(out_node[0][live].tolist(), ids[0, :, 1][live].tolist()))
        assert (ids[0][~live] == -1).all() and torch.isneginf(lp[0][~live]).all()


def test_wide_refuses_bad_arguments(device):
    from rqvae_hip import ops, RqHipError, _lib
    tok, _ = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    lvl0 = dict(child_off=trie.child_off[0], tok=trie.tok[1])
    for wide in (True, None):
        with pytest.raises(RqHipError, match="wide kernel's envelope"):
            ops.beam_expand(torch.zeros(1025, 16, device=device), 3, batch=1, wide=wide, **lvl0)   # kprev = 1025
    with pytest.raises(RqHipError, match="wide kernel's envelope"):
        ops.beam_expand(torch.zeros(4, 16, device=device), 1025, batch=4, wide=True, **lvl0)
    with pytest.raises(RqHipError, match="wide kernel's envelope"):
        ops.beam_expand(torch.zeros(1, 4097, device=device), 3, batch=1, wide=True, **lvl0)
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand(torch.zeros(40, 256, device=device), 3, batch=1, **lvl0)   # the plain call: still kprev V <= 8192
    with pytest.raises(RqHipError, match="rc=-22.*temperature"):
        ops.beam_expand(torch.zeros(4, 16, device=device), 3, batch=4, wide=True, temperature=0.0, **lvl0)
    assert ops.beam_expand(torch.zeros(0, 16, device=device), 3, batch=0, wide=True, **lvl0)[0].shape == (0, 3, 1)
    assert ops.beam_expand(torch.zeros(2, 4096, device=device), 1024, batch=2, wide=True, **lvl0)[0].shape == (2, 1024, 1)
    typed = _lib.load()
    for kprev, V, k in ((1025, 16, 3), (4, 16, 1025), (1, 4097, 3)):
        rc = typed.rq_beam_expand_wide(None, 1.0, None, None, 1, None, 0, None, None, 1, kprev, V, 0, k, None, None, None,
                                       None, None, 0, None, 0, 0, None, None)
        assert rc == -22 and b"rq_beam_expand_wide: need V <= 4096" in typed.rq_last_error()
        # a blocked row announced but NULL: the envelope is checked before the pointers
        rc = typed.rq_beam_expand_wide(None, 1.0, None, None, 1, None, 0, None, None, 1, kprev, V, 0, k, None, None, None,
                                       None, None, 4, None, 0, 0, None, None)
        assert rc == -22 and b"rq_beam_expand_wide: need V <= 4096" in typed.rq_last_error()


# ------------------------------------------------------------------------------------------ 6. the model
def _calls(monkeypatch, fn):
    """The C entry points fn() goes through, in order."""
    from rqvae_hip import ops
    names, real = [], ops.call
    with monkeypatch.context() as m:
        m.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        out = fn()
    return out, names


def test_beams_32_is_todays_call(golden, device, monkeypatch):
    model, batch, corpus, refs = bs.generation_case(golden, device, "c300")
    kw = dict(temperature=1, top_k=True, fused=True, sample=False, constrained=True)
    today = model.generate_next_sem_id(batch, **kw)
    got, names = _calls(monkeypatch, lambda: model.generate_next_sem_id(batch, beams=32, **kw))
    assert torch.equal(got.sem_ids, today.sem_ids)
    assert torch.equal(got.log_probas.view(torch.int32), today.log_probas.view(torch.int32))
    assert names.count("rq_beam_expand") == 4 and not any("wide" in n for n in names)
    rec_today = model.recommend(batch, k=10)
    rec, names = _calls(monkeypatch, lambda: model.recommend(batch, k=10, beams=32))
    assert torch.equal(rec.item_ids, rec_today.item_ids) and torch.equal(rec.sem_ids, rec_today.sem_ids)
    assert torch.equal(rec.log_probas.view(torch.int32), rec_today.log_probas.view(torch.int32))
    assert names.count("rq_beam_expand") == 4 and not any("wide" in n for n in names)
    wider, names = _calls(monkeypatch, lambda: model.generate_next_sem_id(batch, beams=64, **kw))
    assert wider.sem_ids.shape == (3, 64, 4) and wider.log_probas.shape == (3, 64)
    assert names.count("rq_beam_expand") == 1 and names.count("rq_beam_expand_wide") == 3, "V = 256: wide past step 0"


_EXHAUSTIVE = {}


def _exhaustive(golden, device, incremental):
    if incremental not in _EXHAUSTIVE:
        model, batch, corpus, _ = bs.generation_case(golden, device, "c300")
        rng = torch.cuda.get_rng_state()
        rec = model.recommend(batch, k=300, beams=512, incremental=incremental)
        assert model.training, "train mode restored"
        assert model.transformer.cached_enc_output is None, "encoder cache cleared"
        assert torch.equal(torch.cuda.get_rng_state(), rng), "no generator draw"
        _EXHAUSTIVE[incremental] = rec
    return _EXHAUSTIVE[incremental]


@pytest.mark.parametrize("incremental", [True, False])
def test_recommend_exhaustive_width(golden, device, incremental):
    """512 beams over the 300-row corpus (no level has more than 300 nodes): nothing is pruned, so the result is every
    distinct row once — its first corpus index — in the order of score_items' scores."""
    model, batch, corpus, _ = bs.generation_case(golden, device, "c300")
    assert max(len(lvl) for lvl in corpus.index) <= 300 and max(max(r) for r in corpus.rows) < model.num_embeddings
    rec = _exhaustive(golden, device, incremental)
    assert rec.item_ids.shape == (3, 300) and rec.sem_ids.shape == (3, 300, 4) and rec.log_probas.shape == (3, 300)
    items, lp = rec.item_ids.cpu(), rec.log_probas.cpu()
    firsts = sorted(corpus.first_row.values())
    scores = model.score_items(batch, torch.arange(300, device=device).expand(3, 300).contiguous()).log_probas.cpu()
    for b in range(3):
        live = items[b] >= 0
        assert int(live.sum()) == len(firsts) and live[:len(firsts)].all(), "the live rows come first"
        assert sorted(items[b][live].tolist()) == firsts, "every distinct row once, by its first corpus index"
        assert (rec.sem_ids.cpu()[b][~live] == -1).all() and torch.isneginf(lp[b][~live]).all()
        assert torch.equal(corpus.ids[items[b][live]], rec.sem_ids.cpu()[b][live])
        assert (lp[b][live][:-1] >= lp[b][live][1:]).all(), "non-increasing"
        np.testing.assert_allclose(lp[b][live].numpy(), scores[b][items[b][live]].numpy(), rtol=1e-5, atol=0)


def test_recommend_exhaustive_excluding_items(golden, device):
    model, batch, corpus, _ = bs.generation_case(golden, device, "c300")
    full = _exhaustive(golden, device, True)
    got = model.recommend(batch, k=295, beams=512, exclude_items=full.item_ids[:, :5].contiguous())
    assert torch.equal(got.item_ids, full.item_ids[:, 5:]) and torch.equal(got.sem_ids, full.sem_ids[:, 5:])
    live = (got.item_ids >= 0).cpu()
    assert int(live.sum()) == 3 * (len(corpus.first_row) - 5) and torch.isneginf(got.log_probas.cpu()[~live]).all()
    np.testing.assert_allclose(got.log_probas.cpu()[live].numpy(), full.log_probas[:, 5:].cpu()[live].numpy(),
                               rtol=1e-5, atol=0)


def test_recommend_wide_vs_fp64_loop(golden, device):
    """recommend(k=50, beams=W) against beam_support.reference_constrained at width W: 64, or the first of
    48, 40, 96 at which that reference's own separation precondition holds on this fixture."""
    model, batch, corpus, _ = bs.generation_case(golden, device, "c300")
    ref = None
    for width in (64, 48, 40, 96):
        try:
            ref = bs.reference_constrained(model, batch, corpus, width)
            break
        except AssertionError as e:
            assert "precondition" in str(e)
            print(f"width {width}: {e}")
    assert ref is not None, "no width with separated scores"
    print(f"reference width {width}")
    want_ids, want_lp, want_node = ref
    k = min(50, width)
    for incremental in (True, False):
        rec = model.recommend(batch, k=k, beams=width, incremental=incremental)
        assert torch.equal(rec.sem_ids.cpu(), want_ids[:, :k]), f"beams (incremental={incremental})"
        np.testing.assert_allclose(rec.log_probas.cpu().double().numpy(), want_lp[:, :k].numpy(), rtol=1e-5, atol=0)
        live = want_node[:, :k] >= 0
        assert torch.equal(corpus.ids[rec.item_ids.cpu()[live]], want_ids[:, :k][live])


# ------------------------------------------------------------------------------------------ evaluator
def test_train_decoder_wide_item_metrics(tmp_path, device, capsys, monkeypatch):
    """EVAL_ITEM_KS = (1, 5, 10, 50) at EVAL_BEAM_WIDTH = 64 adds recall / ndcg / mrr @ 50 to the item metrics (their
    @ 1, 5, 10 are still there, the Hit@k keys and the trained parameters do not move); with the defaults the item
    metrics' keys are today's (test_score_gpu.test_train_decoder_sampled_negatives' pattern)."""
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
        torch.manual_seed(1234)
        with monkeypatch.context() as m:
            for name, value in switches.items():
                m.setattr(train_decoder, name, value)
            model = train_decoder.train(**kw)
        return model, dict(train_decoder.LAST_RUN["eval"])

    assert train_decoder.EVAL_BEAM_WIDTH == 32 and tuple(train_decoder.EVAL_ITEM_KS) == (1, 5, 10), "the defaults"
    items_on = dict(EVAL_CONSTRAINED_GENERATION=True, EVAL_ITEM_METRICS=True)
    capsys.readouterr()
    m_wide, ev = run(EVAL_ITEM_KS=(1, 5, 10, 50), EVAL_BEAM_WIDTH=64, **items_on)
    printed = capsys.readouterr().out
    hit = [f"h@{k}_{name}" for i in range(4) for name in (f"slice_:{i + 1}", f"pos_{i}") for k in (1, 5, 10)]
    item = lambda ks: [f"{name}@{k}" for k in ks for name in ("recall", "ndcg", "mrr")]   # noqa: E731
    assert set(ev) == set(hit) | set(item((1, 5, 10, 50))) | {"full_eval_iter"} and "'recall@50'" in printed
    assert all(0.0 <= ev[key] <= 1.0 for key in item((1, 5, 10, 50)))
    for name in ("recall", "ndcg", "mrr"):
        assert ev[f"{name}@10"] <= ev[f"{name}@50"]
    m_def, ev_def = run(**items_on)
    assert set(ev_def) == set(hit) | set(item((1, 5, 10))) | {"full_eval_iter"}, "the defaults give today's keys"
    assert all(ev_def[key] == ev[key] for key in hit), "the Hit@k values (32 beams) do not move"
    wide = dict(m_wide.named_parameters())
    for n, p in m_def.named_parameters():
        assert torch.equal(p.detach(), wide[n].detach()), f"{n}: the wider evaluation perturbed training"
