"""CPU side of candidate scoring: evaluate.metrics.ranked_candidates and its use with RankAccumulator on hand-made
ranks, the target-last tie rule of the sampled-negatives evaluation, and the declared surface (switch, symbol)."""
import pytest
import torch


def test_ranked_candidates_by_hand():
    from evaluate.metrics import ranked_candidates
    items = torch.tensor([[10, 11, 12, 13], [20, 21, -1, 23]])
    rank = torch.tensor([[2, 0, 3, 1], [0, 1, 3, 2]], dtype=torch.int32)
    out = ranked_candidates(items, rank)
    assert out.dtype == items.dtype and out.tolist() == [[11, 13, 10, 12], [20, 21, 23, -1]]
    assert torch.equal(out.gather(1, rank.long()), items)
    assert torch.equal(ranked_candidates(items, rank.long()), out)
    with pytest.raises(ValueError, match="need items"):
        ranked_candidates(items, rank[:, :3])
    with pytest.raises(ValueError, match="need items"):
        ranked_candidates(items[0], rank[0])


def test_ranked_candidates_feed_rank_accumulator():
    """Three users, C = 4, the target in the last column: ranks 0, 2 and a user without a target (skipped)."""
    from evaluate.metrics import RankAccumulator, ranked_candidates
    items = torch.tensor([[5, 6, 7, 9], [1, 2, 3, 4], [8, 8, 8, -1]])
    rank = torch.tensor([[1, 2, 3, 0], [0, 1, 3, 2], [0, 1, 2, 3]], dtype=torch.int32)
    target = items[:, -1]
    acc = RankAccumulator(ks=[1, 2, 3], width=4)
    acc.accumulate(actual=target, top_k=ranked_candidates(items, rank))
    assert acc.hists[4].tolist() == [1, 0, 1, 0, 0]
    out = acc.reduce()
    assert out["recall@1"] == 0.5 and out["recall@2"] == 0.5 and out["recall@3"] == 1.0
    assert out["mrr@3"] == pytest.approx((1.0 + 1.0 / 3.0) / 2) and out["ndcg@3"] == pytest.approx((1.0 + 0.5) / 2)


def _stable_rank(scores):
    """The device kernel's rule on the CPU: score descending, ties to the lower candidate index."""
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    return torch.empty_like(order).scatter_(1, order, torch.arange(scores.shape[1]).expand_as(order)).to(torch.int32)


def test_target_last_loses_ties():
    """A negative that shares the target's sem-ID row has the target's score. With the target in the LAST column the
    tie goes to the negative (the lower index): a tie counts against the model. In the first column it would count for
    it."""
    from evaluate.metrics import RankAccumulator, ranked_candidates
    scores = torch.tensor([[-3.0, -1.5, -2.0, -1.5]])   # candidate 1 ties with the target
    last = torch.tensor([[40, 41, 42, 7]])
    acc = RankAccumulator(ks=[1, 2], width=4)
    acc.accumulate(actual=torch.tensor([7]), top_k=ranked_candidates(last, _stable_rank(scores)))
    assert acc.reduce()["recall@1"] == 0.0 and acc.reduce()["recall@2"] == 1.0
    first = torch.tensor([[7, 41, 42, 40]])
    acc = RankAccumulator(ks=[1, 2], width=4)
    acc.accumulate(actual=torch.tensor([7]), top_k=ranked_candidates(first, _stable_rank(scores[:, [3, 1, 2, 0]])))
    assert acc.reduce()["recall@1"] == 1.0


def test_scoring_surface_is_declared():
    import train_decoder
    from modules.model import EncoderDecoderRetrievalModel, Scores
    from rqvae_hip import _lib, ops
    assert train_decoder.EVAL_SAMPLED_NEGATIVES == 0, "off by default"
    assert Scores._fields == ("log_probas", "rank")
    assert callable(EncoderDecoderRetrievalModel.score_items) and callable(EncoderDecoderRetrievalModel.score_sem_ids)
    assert callable(ops.score_paths) and "rq_score_paths" in _lib._SIGS
