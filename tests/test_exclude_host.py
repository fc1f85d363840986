"""Seen-item exclusion and item-level metrics, host side (CPU-only): SemanticIdTokenizer.blocked_nodes against a
brute force from the corpus rows, evaluate.metrics.RankAccumulator against TopKAccumulator and a plain Python loop,
and the argument contracts of generate_next_sem_id / recommend(exclude_items=...)."""
import math

import pytest
import torch

import beam_support as bs


def _index(ids):
    """Per level q = 0..D the rank of every prefix among the sorted distinct ones (= its trie node), from the rows."""
    rows = [tuple(r) for r in ids.tolist()]
    return [{pre: i for i, pre in enumerate(sorted({r[:q] for r in rows}))} for q in range(ids.shape[1] + 1)]


def _brute_blocked(ids, items):
    """(D, B, H) as blocked_nodes returns it: for every level and every prefix, blocked iff all rows under it are
    excluded rows (rows equal to the row of a listed item)."""
    rows = [tuple(r) for r in ids.tolist()]
    n, D = len(rows), ids.shape[1]
    index = _index(ids)
    B, H = items.shape
    out = torch.full((D, B, H), bs.NONE, dtype=torch.int32)
    for b in range(B):
        excluded = {rows[i] for i in items[b].tolist() if 0 <= i < n}
        for q in range(1, D + 1):
            blocked = sorted(node for pre, node in index[q].items()
                             if all(r in excluded for r in rows if r[:q] == pre))
            assert len(blocked) <= H
            out[q - 1, b, :len(blocked)] = torch.tensor(blocked, dtype=torch.int32)
    return out


def _subtree_items(ids, first_token):
    return [i for i, r in enumerate(ids.tolist()) if r[0] == first_token]


def test_blocked_nodes_five_rows():
    ids = bs.FIVE
    tok = bs.ids_tokenizer(ids)
    index = _index(ids)
    items = torch.tensor([[0, 1, -1], [4, -1, -1], [-1, -1, -1], [1, 1, 0], [7, -5, 3]])
    got = tok.blocked_nodes(items)
    assert got.shape == (4, 5, 3) and got.dtype == torch.int32
    assert torch.equal(got, _brute_blocked(ids, items))
    # history {0, 1}: both leaves under (3, 1, 4), so that node and (3, 1) are blocked; (3,) still has (3, 0, 9, 0)
    assert got[3, 0].tolist() == [index[4][(3, 1, 4, 0)], index[4][(3, 1, 4, 1)], bs.NONE]
    assert got[2, 0].tolist() == [index[3][(3, 1, 4)], bs.NONE, bs.NONE]
    assert got[1, 0].tolist() == [index[2][(3, 1)], bs.NONE, bs.NONE]
    assert got[0, 0].tolist() == [bs.NONE] * 3
    # history {4}: the duplicated row's one leaf is blocked, so item 2 goes with item 4 — and (0,) has no other row
    assert got[3, 1].tolist() == [index[4][(0, 2, 2, 0)], bs.NONE, bs.NONE]
    assert got[0, 1].tolist() == [index[1][(0,)], bs.NONE, bs.NONE]
    assert int(tok.trie_index().item_leaf[2]) == int(tok.trie_index().item_leaf[4])
    assert (got[:, 2] == bs.NONE).all(), "all padding"
    assert torch.equal(got[:, 3], got[:, 0]), "duplicates and order do not matter"
    assert got[3, 4].tolist() == [index[4][(3, 0, 9, 0)], bs.NONE, bs.NONE], "out-of-range ids count as padding"


def test_blocked_nodes_random_corpus():
    ids = bs.random_corpus()
    tok = bs.ids_tokenizer(ids)
    index = _index(ids)
    n = ids.shape[0]
    g = torch.Generator().manual_seed(17)
    H = 40
    sub = _subtree_items(ids, int(ids[5, 0]))          # exactly all rows under one level-1 node
    assert 0 < len(sub) <= H
    items = torch.full((6, H), -1, dtype=torch.int64)
    items[0, :len(sub)] = torch.tensor(sub)[torch.randperm(len(sub), generator=g)]
    items[1] = torch.randint(0, n, (H,), generator=g)
    items[2, ::2] = torch.randint(0, n, (H // 2,), generator=g)      # padding in between
    items[3, :10] = torch.tensor([3, 7, 250, 3, 3, n, n + 5, -7, 10 ** 12, 7])   # the tripled row, out-of-range ids
    items[4, :H // 2] = items[1, :H // 2]                                       # duplicates
    items[4, H // 2:] = items[1, :H // 2]
    got = tok.blocked_nodes(items)
    assert torch.equal(got, _brute_blocked(ids, items))
    node1 = index[1][(int(ids[5, 0]),)]
    assert got[0, 0].tolist() == [node1] + [bs.NONE] * (H - 1), "the whole-subtree user blocks its level-1 node"
    for q in range(1, 5):   # ... and every descendant of it
        want = sorted(v for pre, v in index[q].items() if pre[0] == int(ids[5, 0]))
        assert got[q - 1, 0, :len(want)].tolist() == want
    assert (got[:, 5] == bs.NONE).all(), "an empty history blocks nothing"
    for q in range(4):
        live = got[q][got[q] != bs.NONE]
        assert (got[q, :, 1:] >= got[q, :, :-1]).all() and live.numel() > 0
    # every item: every node of every level is blocked; H = 0 gives an empty fixed-shape result
    everything = tok.blocked_nodes(torch.arange(n).unsqueeze(0))
    for q in range(1, 5):
        n_q = len(index[q])
        assert everything[q - 1, 0, :n_q].tolist() == list(range(n_q)) and (everything[q - 1, 0, n_q:] == bs.NONE).all()
    assert tok.blocked_nodes(torch.zeros((2, 0), dtype=torch.int64)).shape == (4, 2, 0)


def test_trie_index_cache_follows_the_trie():
    tok = bs.ids_tokenizer(bs.FIVE)
    idx = tok.trie_index()
    assert tok.trie_index() is idx, "cached"
    assert idx.item_leaf.dtype == torch.int32 and idx.item_leaf.tolist() == [2, 3, 0, 1, 0]
    assert [c.tolist() for c in idx.leaf_count] == [[1, 3], [1, 1, 2], [1, 1, 2], [1, 1, 1, 1]]
    assert idx.leaf_anc[3].tolist() == [0, 1, 2, 3] and idx.leaf_anc[0].tolist() == [0, 1, 1, 1]
    tok.reset()
    assert tok._trie_index is None
    with pytest.raises(Exception, match="empty cache"):
        tok.trie_index()


# ------------------------------------------------------------------------------------------ RankAccumulator
def _loop_metrics(batches, ks):
    """recall / ndcg / mrr @ k by a plain loop over rows: one relevant target, the first matching beam counts."""
    ranks = []
    for actual, topk in batches:
        for a, beams in zip(actual.tolist(), topk.tolist()):
            if (a[0] if isinstance(a, list) else a) < 0:
                continue
            hits = [r for r, t in enumerate(beams) if t == a]
            ranks.append(hits[0] if hits else None)
    out = {}
    for k in ks:
        top = [r for r in ranks if r is not None and r < k]
        out[f"recall@{k}"] = len(top) / len(ranks)
        out[f"ndcg@{k}"] = math.fsum(1.0 / math.log2(r + 2) for r in top) / len(ranks)
        out[f"mrr@{k}"] = math.fsum(1.0 / (r + 1) for r in top) / len(ranks)
    return out


def _assert_close(got, want):
    assert list(got) == list(want)
    for key in want:
        assert got[key] == pytest.approx(want[key], rel=1e-12, abs=0), key


def test_rank_accumulator_matches_topk_accumulator(golden):
    from evaluate.metrics import RankAccumulator, TopKAccumulator
    z = golden("topk_metrics")
    ks = [int(k) for k in z["ks"]]
    batches = [(torch.from_numpy(z["actual1"]), torch.from_numpy(z["topk1"])),
               (torch.from_numpy(z["actual2"]), torch.from_numpy(z["topk2"]))]
    assert batches[0][1].shape[1] == 32 and batches[1][1].shape[1] == 3, "two beam widths, one below ks[1]"
    hit, rank = TopKAccumulator(ks=ks), RankAccumulator(ks=ks)
    for a, t in batches:
        hit.accumulate(actual=a, top_k=t)
        rank.accumulate(actual=a, top_k=t)
    want, got = hit.reduce(), rank.reduce()
    D = batches[0][0].shape[1]
    assert any(0 < want[f"h@{k}_slice_:{D}"] < 1 for k in ks)
    for k in ks:
        assert got[f"recall@{k}"] == want[f"h@{k}_slice_:{D}"]
    _assert_close(got, _loop_metrics(batches, ks))


def test_rank_accumulator_item_ids_and_edge_rows():
    from evaluate.metrics import RankAccumulator
    actual = torch.tensor([7, 3, -1, 5, 9, 2])
    topk = torch.tensor([[7, 7, 1, 0],      # duplicated beams: the first match counts (rank 0)
                         [1, 3, 3, -1],     # rank 1
                         [-1, -1, -1, -1],  # no target: skipped, although a dead beam "equals" -1
                         [4, -1, -1, -1],   # dead beams never match: a miss
                         [0, 1, 2, 9],      # rank 3
                         [-1, -1, -1, -1]])  # all dead: a miss
    acc = RankAccumulator(ks=[1, 2, 4], width=4)
    acc.accumulate(actual, topk)
    assert acc.hists[4].tolist() == [1, 1, 0, 1, 2]
    got = acc.reduce()
    _assert_close(got, _loop_metrics([(actual, topk)], [1, 2, 4]))
    assert got["recall@4"] == 3 / 5 and got["recall@1"] == 1 / 5
    assert got["mrr@4"] == pytest.approx((1 + 1 / 2 + 1 / 4) / 5, rel=1e-12)
    assert got["ndcg@2"] == pytest.approx((1 + 1 / math.log2(3)) / 5, rel=1e-12)
    # tuples and ids agree where the tuple has one column; a narrower second batch keeps its misses apart
    acc2 = RankAccumulator(ks=[1, 2, 4], width=4)
    acc2.accumulate(actual.unsqueeze(-1), topk.unsqueeze(-1))
    assert acc2.reduce() == got
    acc2.accumulate(torch.tensor([8, 6]), torch.tensor([[1, 8], [6, 0]]))
    _assert_close(acc2.reduce(), _loop_metrics([(actual, topk), (torch.tensor([8, 6]), torch.tensor([[1, 8], [6, 0]]))],
                                               [1, 2, 4]))
    with pytest.raises(ValueError, match="built for 1..4"):
        acc.accumulate(actual, torch.zeros(6, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="need actual"):
        acc.accumulate(actual, torch.zeros(5, 4, dtype=torch.int64))


def test_rank_accumulator_empty():
    from evaluate.metrics import RankAccumulator
    acc = RankAccumulator()
    assert acc.reduce() == {}
    acc.accumulate(torch.tensor([-1, -1]), torch.zeros(2, 10, dtype=torch.int64))   # rows without a target only
    assert acc.reduce() == {}
    acc.accumulate(torch.tensor([4]), torch.tensor([[0, 4, 4]]))
    assert acc.reduce()["recall@5"] == 1.0 and acc.reduce()["recall@1"] == 0.0
    acc.reset()
    assert acc.reduce() == {}


def _dp_worker(rank, world, port, arrays, n_first, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        from evaluate.metrics import RankAccumulator
        from rqvae_hip import dp
        dp.init_from_env(backend="gloo")
        batches = [(torch.from_numpy(a), torch.from_numpy(t)) for a, t in arrays]
        acc = RankAccumulator(ks=[1, 5, 10])
        for a, t in (batches[:n_first] if rank == 0 else batches[n_first:]):
            acc.accumulate(a, t)
        q.put((rank, acc.reduce()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_rank_accumulator_reduce_data_parallel(golden):
    """One all-reduce of the fixed (width + 1) vector: rank 0 holds every batch (two beam widths), rank 1 none."""
    import torch.multiprocessing as mp
    from evaluate.metrics import RankAccumulator
    z = golden("topk_metrics")
    arrays = [(z["actual1"], z["topk1"]), (z["actual2"], z["topk2"]), (z["actual1"][::-1].copy(), z["topk1"][:, :7].copy())]
    single = RankAccumulator(ks=[1, 5, 10])
    for a, t in arrays:
        single.accumulate(torch.from_numpy(a), torch.from_numpy(t))
    want = single.reduce()
    assert want and len(single.hists) == 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = bs.free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, arrays, 3, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0] == want and res[1] == want and list(res[0]) == list(want)


# ------------------------------------------------------------------------------------------ argument refusals
def test_exclude_items_argument_errors():
    from data.schemas import TokenizedSeqBatch
    from modules.model import EncoderDecoderRetrievalModel
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=12, sem_id_dim=4, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    model.inference_prefix_index = bs.ids_tokenizer(bs.FIVE)
    seen = torch.tensor([[0, 1], [4, -1]])
    for kw in (dict(), dict(fused=True), dict(fused=True, sample=False), dict(fused=True, incremental=True)):
        with pytest.raises(ValueError, match="exclude_items requires constrained=True"):
            model.generate_next_sem_id(None, top_k=True, exclude_items=seen, **kw)
    z = torch.zeros(3, 8, dtype=torch.int64)
    batch = TokenizedSeqBatch(user_ids=z[:, :1], sem_ids=z, sem_ids_fut=None, seq_mask=z.bool(), token_type_ids=z,
                              token_type_ids_fut=None)
    for bad in (seen, seen[0], torch.zeros(3, 2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="exclude_items must be .B, H. with B = 3"):
            model.generate_next_sem_id(batch, top_k=True, fused=True, sample=False, constrained=True, exclude_items=bad)
        with pytest.raises(ValueError, match="exclude_items must be .B, H. with B = 3"):
            model.recommend(batch, exclude_items=bad)
    assert model.training and model.transformer.cached_enc_output is None


def test_exclusion_ops_refuse_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    tok = bs.ids_tokenizer(bs.FIVE)
    idx = tok.trie_index()
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.trie_blocked_nodes(torch.zeros(2, 3, dtype=torch.int64), idx.item_leaf, idx.leaf_anc, idx.leaf_count)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.rank_hist(torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, 3, 1, dtype=torch.int64),
                      torch.zeros(4, dtype=torch.int64))
