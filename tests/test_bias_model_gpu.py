"""Per-item score bias through the model: recommend(item_bias=...) on the small decoder of the beam tests over the
300-row hand corpus — exhaustive at 1,024 beams against score_items + bias over the whole corpus, the zero bias against
recommend(), a {0, -inf} bias against item_filter, a constructed case that over-fetching misses, incremental on and
off, with exclude_items, and per-user groups."""
import numpy as np
import pytest
import torch

import beam_support as bs
import bias_support as bi

pytestmark = pytest.mark.gpu

_FIX = {}


def _fixture(golden, device):
    """(model with the c300 tokenizer as its prefix index, batch, corpus, every item's raw score for every user from
    score_items, a seeded (2, N) bias)."""
    if not _FIX:
        z = golden("generation")
        tok, corpus = bs.tokenizer("c300", device)
        model = bs.decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]))
        model.enable_generation = True
        model.inference_prefix_index = tok
        batch = bs.tokenized(z, device)
        B, N = batch.sem_ids.shape[0], len(corpus.rows)
        every = torch.arange(N, device=device).expand(B, N).contiguous()
        lp = model.score_items(batch, every).log_probas.cpu()
        g = torch.Generator().manual_seed(23)
        _FIX.update(model=model, batch=batch, tok=tok, corpus=corpus, lp=lp, bias=2.0 * torch.randn(2, N, generator=g))
    return _FIX


def _ranking(f, b, bias_row, gone=()):
    """User b's corpus rows by fp64 score = score_items' log-probability + the bias, descending: (score, log p, item)
    per distinct row, the row's item being its max-bias one, then the lowest index; rows of the items in `gone`, rows
    the model cannot generate and rows hidden by -inf are left out."""
    corpus, lp = f["corpus"], f["lp"]
    gone_rows = {corpus.rows[i] for i in gone}
    best = {}
    for i, r in enumerate(corpus.rows):
        u, l = bi.clean(bias_row[i]), float(lp[b, i])
        if r in gone_rows or u == bi.NINF or l == bi.NINF:
            continue
        if r not in best or u > best[r][2]:
            best[r] = (l + u, l, u, i)
    return sorted(((s, l, i) for s, l, _, i in best.values()), key=lambda t: -t[0])


def _check_exhaustive(f, got, rows_bias, k, gone=None, what=""):
    items, lp, scores = got.item_ids.cpu(), got.log_probas.cpu().double(), got.scores.cpu().double()
    for b in range(items.shape[0]):
        want = _ranking(f, b, rows_bias[b].tolist(), () if gone is None else gone[b])
        assert len(want) > k, "precondition: more than k candidates"
        top = want[:k]
        if bs.separated([t[0] for t in want], k):
            assert items[b].tolist() == [t[2] for t in top], f"{what}user {b}: items in order"
        else:
            cut = want[k - 1][0]
            assert want[k][0] < cut - 1e-5 * abs(cut), "precondition: the k-th score stands clear of the next"
            assert sorted(items[b].tolist()) == sorted(t[2] for t in top), f"{what}user {b}: the item set"
        by_item = {t[2]: t for t in top}
        for r, i in enumerate(items[b].tolist()):
            np.testing.assert_allclose(float(scores[b, r]), by_item[i][0], rtol=1e-5, atol=0)
            np.testing.assert_allclose(float(lp[b, r]), by_item[i][1], rtol=1e-5, atol=0)
        assert (scores[b, :-1] >= scores[b, 1:]).all(), "ordered by scores"


@pytest.mark.parametrize("incremental", [True, False])
def test_exhaustive_search_equals_score_items_plus_bias(golden, device, incremental):
    """1,024 beams hold every node of every level of the 300-row corpus: the biased search is exhaustive and exact."""
    from modules.model import RankedItems
    f = _fixture(golden, device)
    model, batch, bias = f["model"], f["batch"], f["bias"][0]
    k = 10
    got = model.recommend(batch, k=k, beams=1024, incremental=incremental, item_bias=bias.to(device))
    assert isinstance(got, RankedItems) and model.training and model.transformer.cached_enc_output is None
    B = batch.sem_ids.shape[0]
    assert got.item_ids.shape == (B, k) and got.item_ids.dtype == torch.int64 and got.sem_ids.shape == (B, k, 4)
    assert got.log_probas.shape == got.scores.shape == (B, k) and got.scores.dtype == torch.float32
    _check_exhaustive(f, got, [bias] * B, k)
    assert torch.equal(f["corpus"].ids[got.item_ids.cpu()], got.sem_ids.cpu()), "cached_ids[item_ids] == sem_ids"
    # scores is log_probas + the item's own bias, one fp32 add
    own = bias.to(device)[got.item_ids]
    assert torch.equal((got.log_probas + own).view(torch.int32), got.scores.view(torch.int32))
    plain = model.recommend(batch, k=k, beams=1024, incremental=incremental)
    assert not torch.equal(plain.item_ids, got.item_ids), "precondition: the bias changes the list"


def test_zero_bias_is_recommend(golden, device):
    from modules.model import Recommendation
    f = _fixture(golden, device)
    model, batch = f["model"], f["batch"]
    N = len(f["corpus"].rows)
    for beams in (32, 64):
        want = model.recommend(batch, beams=beams)
        assert isinstance(want, Recommendation) and len(want) == 3, "no field is added without a bias"
        got = model.recommend(batch, beams=beams, item_bias=torch.zeros(N, device=device))
        assert torch.equal(got.item_ids, want.item_ids) and torch.equal(got.sem_ids, want.sem_ids)
        assert torch.equal(got.log_probas.view(torch.int32), want.log_probas.view(torch.int32))
        assert torch.equal(got.scores.view(torch.int32), got.log_probas.view(torch.int32))
        built = model.recommend(batch, beams=beams, item_bias=f["tok"].item_bias(torch.zeros(1, N, device=device)))
        assert torch.equal(built.item_ids, got.item_ids), "an ItemBias built once gives the raw tensor's result"


@pytest.mark.parametrize("beams", [32, 64])
def test_zero_or_minus_inf_bias_is_the_item_filter(golden, device, beams):
    f = _fixture(golden, device)
    model, batch = f["model"], f["batch"]
    N = len(f["corpus"].rows)
    mask = torch.rand(N, generator=torch.Generator().manual_seed(5)) < 0.5
    bias = torch.where(mask, 0.0, bi.NINF)
    want = model.recommend(batch, k=5, beams=beams, item_filter=mask.to(device))
    got = model.recommend(batch, k=5, beams=beams, item_bias=bias.to(device))
    assert (want.item_ids >= 0).all(), "precondition: five live rows"
    assert torch.equal(got.item_ids, want.item_ids) and torch.equal(got.sem_ids, want.sem_ids)
    assert torch.equal(got.log_probas.view(torch.int32), want.log_probas.view(torch.int32)), "log_probas bitwise"
    assert mask[got.item_ids.cpu()].all(), "no hidden item"
    assert not torch.equal(model.recommend(batch, k=5, beams=beams).item_ids, want.item_ids), "the mask removes a winner"


def _step0_logits(model, batch):
    was = model.training
    model.eval()
    model.transformer.cached_enc_output = None
    try:
        with torch.no_grad():
            return model.forward(bs.first_batch(batch)).logits.cpu()
    finally:
        model.transformer.cached_enc_output = None
        model.train(was)


def test_boosted_item_behind_an_unlikely_first_token(golden, device):
    """Four beams: an item whose first token the model ranks below fourth place is never generated by recommend(k=4,
    beams=4), whatever is done to its four results afterwards; with a large bias on it the biased search returns it
    first."""
    f = _fixture(golden, device)
    model, batch, corpus = f["model"], f["batch"], f["corpus"]
    V, N = model.num_embeddings, len(corpus.rows)
    logits = _step0_logits(model, batch)
    b = 0
    first = [v for v in corpus.children[0][()] if v < V]
    order = sorted(first, key=lambda v: -float(logits[b, v]))
    assert len(order) > 5
    token = order[-1]   # the valid first token the model likes least
    item = next(i for i, r in enumerate(corpus.rows) if r[0] == token and max(r) < V)
    assert float(f["lp"][b, item]) > bi.NINF, "the model can generate the item"
    plain = model.recommend(batch, k=4, beams=4)
    assert item not in plain.item_ids[b].tolist() and token not in plain.sem_ids[b, :, 0].tolist()
    bias = torch.zeros(N)
    bias[item] = 50.0
    got = model.recommend(batch, k=4, beams=4, item_bias=bias.to(device))
    assert int(got.item_ids[b, 0]) == item and got.sem_ids[b, 0].tolist() == list(corpus.rows[item])
    np.testing.assert_allclose(float(got.log_probas[b, 0]), float(f["lp"][b, item]), rtol=1e-5, atol=0)
    np.testing.assert_allclose(float(got.scores[b, 0]), float(f["lp"][b, item]) + 50.0, rtol=1e-5, atol=0)


@pytest.mark.parametrize("beams", [32, 64])
def test_incremental_on_and_off_agree(golden, device, beams):
    f = _fixture(golden, device)
    model, batch, bias = f["model"], f["batch"], f["bias"][1].to(device)
    inc = model.recommend(batch, beams=beams, incremental=True, item_bias=bias)
    full = model.recommend(batch, beams=beams, incremental=False, item_bias=bias)
    assert torch.equal(inc.item_ids, full.item_ids) and torch.equal(inc.sem_ids, full.sem_ids)
    np.testing.assert_allclose(inc.scores.cpu().numpy(), full.scores.cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(inc.log_probas.cpu().numpy(), full.log_probas.cpu().numpy(), rtol=1e-5, atol=0)


def test_exclude_items_composes(golden, device):
    f = _fixture(golden, device)
    model, batch, bias = f["model"], f["batch"], f["bias"][0]
    B, k = batch.sem_ids.shape[0], 10
    first = model.recommend(batch, k=k, beams=1024, item_bias=bias.to(device))
    gone = [first.item_ids[b, :2].tolist() + [5] for b in range(B)]   # each user's two best and one fixed item
    got = model.recommend(batch, k=k, beams=1024, item_bias=bias.to(device),
                          exclude_items=bs.pad(gone).to(device))
    gone_rows = [{f["corpus"].rows[i] for i in g} for g in gone]
    assert not any(tuple(r) in gone_rows[b] for b in range(B) for r in got.sem_ids[b].cpu().tolist())
    _check_exhaustive(f, got, [bias] * B, k, gone=gone, what="excluded: ")


def test_groups_give_every_user_its_own_row(golden, device):
    f = _fixture(golden, device)
    model, batch, bias = f["model"], f["batch"], f["bias"].to(device)
    built = f["tok"].item_bias(bias)
    assert built.groups == 2
    groups = torch.tensor([0, 1, -1], device=device)
    got = model.recommend(batch, beams=64, item_bias=built, bias_group=groups)
    raw = model.recommend(batch, beams=64, item_bias=bias, bias_group=groups.to(torch.int32))
    assert torch.equal(raw.item_ids, got.item_ids) and torch.equal(raw.scores.view(torch.int32), got.scores.view(torch.int32))
    rows = [model.recommend(batch, beams=64, item_bias=bias[g]) for g in (0, 1)]
    plain = model.recommend(batch, beams=64)
    assert torch.equal(got.item_ids[0], rows[0].item_ids[0]) and torch.equal(got.item_ids[1], rows[1].item_ids[1])
    assert torch.equal(got.item_ids[2], plain.item_ids[2]), "group -1: unbiased"
    assert torch.equal(got.log_probas[2].view(torch.int32), plain.log_probas[2].view(torch.int32))
    assert torch.equal(got.scores[2].view(torch.int32), got.log_probas[2].view(torch.int32))
    swapped = model.recommend(batch, beams=64, item_bias=built, bias_group=torch.tensor([1, 0, -1], device=device))
    assert not torch.equal(swapped.item_ids[0], got.item_ids[0]) and not torch.equal(swapped.item_ids[1], got.item_ids[1]), \
        "two users on different rows get different lists"
    assert torch.equal(swapped.item_ids[0], model.recommend(batch, beams=64, item_bias=bias[1]).item_ids[0])
