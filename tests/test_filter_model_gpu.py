"""Catalogue filters through the model: recommend / sample_items / generate_next_sem_id(constrained=True) with
item_filter= against the same calls on a second tokenizer that holds the allowed rows alone (bitwise: the decoder sees
the same rows at the same row count), no leaked item, score_items' agreement, the sampler's draw contract and the two
forms of the argument. The small decoder of the beam tests over the 300-row hand corpus."""
import numpy as np
import pytest
import torch

import beam_filter_support as fs
import beam_support as bs

pytestmark = pytest.mark.gpu

_FIX = {}


def _fixture(golden, device):
    """(model with the c300 tokenizer as its prefix index, batch, corpus, a shared (N,) mask of about half the items and
    the tokenizer over the rows it keeps, with their corpus indices)."""
    if not _FIX:
        z = golden("generation")
        tok, corpus = bs.tokenizer("c300", device)
        model = bs.decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]))
        model.enable_generation = True
        model.inference_prefix_index = tok
        mask = fs.seeded_masks(len(corpus.rows), 1, seed=5)[0]
        sub_tok, kept, sub = fs.sub_tokenizer(tok, mask, device)
        _FIX.update(model=model, batch=bs.tokenized(z, device), tok=tok, corpus=corpus, mask=mask, sub_tok=sub_tok,
                    kept=kept.to(device), sub=sub)
    return _FIX


def _on_sub_corpus(f, call):
    """call() with the sub-corpus tokenizer as the model's prefix index."""
    f["model"].inference_prefix_index = f["sub_tok"]
    try:
        return call()
    finally:
        f["model"].inference_prefix_index = f["tok"]


def _mapped(f, items):
    """Sub-corpus item ids as corpus indices (-1 stays)."""
    return torch.where(items >= 0, f["kept"][items.clamp_min(0)], -1)


def _same(got, want, f, what):
    assert torch.equal(got.sem_ids, want.sem_ids), f"{what}: sem_ids"
    assert torch.equal(got.item_ids, _mapped(f, want.item_ids)), f"{what}: item ids"
    for name in ("log_probas", "perturbed"):
        if hasattr(got, name):
            assert torch.equal(getattr(got, name).view(torch.int32), getattr(want, name).view(torch.int32)), \
                f"{what}: {name} bitwise"


def _assert_allowed(items, mask_rows, what):
    """Every id >= 0 of items (B, k) is allowed by its user's (N,) mask row (None: unfiltered)."""
    for b, row in enumerate(mask_rows):
        ids = [i for i in items[b].tolist() if i >= 0]
        assert len(set(ids)) == len(ids), f"{what}: distinct items"
        assert row is None or all(bool(row[i]) for i in ids), f"{what}: a disallowed item for user {b}"


@pytest.mark.parametrize("beams", [32, 64])
@pytest.mark.parametrize("incremental", [True, False])
def test_recommend_equals_the_sub_corpus_search(golden, device, incremental, beams):
    f = _fixture(golden, device)
    model, batch, mask = f["model"], f["batch"], f["mask"].to(device)
    kw = dict(k=5, incremental=incremental, beams=beams)
    got = model.recommend(batch, item_filter=mask, **kw)
    want = _on_sub_corpus(f, lambda: model.recommend(batch, **kw))
    assert (got.item_ids >= 0).all(), "precondition: five live rows"
    _same(got, want, f, f"incremental={incremental} beams={beams}")
    _assert_allowed(got.item_ids.cpu(), [f["mask"]] * got.item_ids.shape[0], "recommend")
    plain = model.recommend(batch, **kw)
    assert not torch.equal(plain.item_ids, got.item_ids), "precondition: the mask removes a winner"
    gen = model.generate_next_sem_id(batch, top_k=True, fused=True, sample=False, constrained=True,
                                     incremental=incremental, beams=beams, item_filter=mask)
    assert torch.equal(gen.sem_ids[:, :5], got.sem_ids)
    assert torch.equal(gen.log_probas[:, :5].view(torch.int32), got.log_probas.view(torch.int32))
    assert model.training and model.transformer.cached_enc_output is None


def _exact_exclusion(corpus, mask, item):
    """Excluding `item`'s row composes exactly with the mask: every proper prefix of the row either holds that row alone
    (the node is blocked) or keeps another allowed row, so no node passes both filters that the search over the
    remaining sub-corpus would not have."""
    row = corpus.rows[item]
    left = [r for i, r in enumerate(corpus.rows) if bool(mask[i]) and r != row]
    alone = lambda q: all(r == row for r in corpus.rows if r[:q] == row[:q])
    return all(alone(q) or any(r[:q] == row[:q] for r in left) for q in range(1, len(row)))


def test_recommend_with_exclusion_equals_the_sub_corpus_search(golden, device):
    """item_filter and exclude_items together: the search over the allowed rows minus the listed ones. Each user lists
    the best of its filtered recommendations for which the composition is exact (_exact_exclusion)."""
    f = _fixture(golden, device)
    model, batch, mask = f["model"], f["batch"], f["mask"].to(device)
    first = model.recommend(batch, k=5, item_filter=mask).item_ids.cpu()
    seen = []
    for b in range(first.shape[0]):
        ok = [i for i in first[b].tolist() if i >= 0 and _exact_exclusion(f["corpus"], f["mask"], i)]
        assert ok, "precondition: an item whose exclusion composes exactly"
        seen.append([ok[0]])
    seen = torch.tensor(seen, device=device)
    where = torch.full((len(f["corpus"].rows),), -1, dtype=torch.int64, device=device)
    where[f["kept"]] = torch.arange(f["kept"].numel(), device=device)
    for incremental in (True, False):
        got = model.recommend(batch, k=5, item_filter=mask, exclude_items=seen, incremental=incremental)
        want = _on_sub_corpus(f, lambda: model.recommend(batch, k=5, exclude_items=where[seen], incremental=incremental))
        _same(got, want, f, f"with exclude_items, incremental={incremental}")
        for b in range(seen.shape[0]):
            gone = f["corpus"].rows[int(seen[b, 0])]
            assert gone not in [tuple(r) for r in got.sem_ids[b].tolist()], "the listed row does not return"
        _assert_allowed(got.item_ids.cpu(), [f["mask"]] * seen.shape[0], "recommend + exclude_items")


def test_groups_leak_nothing(golden, device):
    f = _fixture(golden, device)
    model, batch, corpus = f["model"], f["batch"], f["corpus"]
    B = batch.sem_ids.shape[0]
    masks = fs.seeded_masks(len(corpus.rows), 3, seed=9)
    masks[1] = False
    group = torch.tensor([0, 2, -1, 1][:B])
    rows = [None if g < 0 else masks[g] for g in group.tolist()]
    filt = model.inference_prefix_index.item_filter(masks.to(device))
    plain = model.recommend(batch, k=10)
    for fg in (group.to(device), group.to(device).int(), group):   # any integer dtype, any device
        got = model.recommend(batch, k=10, item_filter=filt, filter_group=fg)
        _assert_allowed(got.item_ids.cpu(), rows, "recommend")
        for b, g in enumerate(group.tolist()):
            if g < 0:   # an unfiltered user: the plain search's rows (other users' rows change no bit of them)
                assert torch.equal(got.item_ids[b], plain.item_ids[b])
                assert torch.equal(got.log_probas[b].view(torch.int32), plain.log_probas[b].view(torch.int32))
            if g == 1:
                assert (got.item_ids[b] == -1).all() and torch.isneginf(got.log_probas[b]).all()
        live = got.item_ids >= 0
        assert live[:2].all(), "precondition: ten live rows for the filtered users"
        # shared rows are reported under the lowest allowed index: the row of every id is the returned row
        ids = model.inference_prefix_index.cached_ids[got.item_ids.clamp_min(0)]
        assert torch.equal(ids[live], got.sem_ids[live])
    drawn = model.sample_items(batch, k=6, item_filter=filt, filter_group=group.to(device),
                               generator=torch.Generator(device=device).manual_seed(2))
    _assert_allowed(drawn.item_ids.cpu(), rows, "sample_items")
    assert (drawn.item_ids[:2] >= 0).all()
    with pytest.raises(ValueError, match="item_filter has 3 groups"):
        model.recommend(batch, k=10, item_filter=filt)


def test_score_items_agrees_with_the_filtered_recommendation(golden, device):
    f = _fixture(golden, device)
    model, batch = f["model"], f["batch"]
    rec = model.recommend(batch, k=10, item_filter=f["mask"].to(device))
    got = model.score_items(batch, rec.item_ids)
    live = (rec.item_ids >= 0).cpu()
    lp, want = got.log_probas.cpu().double(), rec.log_probas.cpu().double()
    assert live.any() and torch.isneginf(lp[~live]).all() and torch.isneginf(want[~live]).all()
    np.testing.assert_allclose(lp[live].numpy(), want[live].numpy(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("incremental", [True, False])
def test_sample_items_equals_the_sub_corpus_draw(golden, device, incremental):
    f = _fixture(golden, device)
    model, batch, mask = f["model"], f["batch"], f["mask"].to(device)
    B, k, V, seed = batch.sem_ids.shape[0], 5, model.num_embeddings, 21
    gen = torch.Generator(device=device).manual_seed(seed)
    got = model.sample_items(batch, k=k, incremental=incremental, item_filter=mask, generator=gen)
    want = _on_sub_corpus(f, lambda: model.sample_items(batch, k=k, incremental=incremental,
                                                        generator=torch.Generator(device=device).manual_seed(seed)))
    assert (got.item_ids >= 0).all(), "precondition: five live rows"
    _same(got, want, f, f"sample_items incremental={incremental}")
    _assert_allowed(got.item_ids.cpu(), [f["mask"]] * B, "sample_items")
    assert (got.perturbed[:, 0] == 0).all()
    # the draws: one exponential_ per step on that step's logits, nothing else
    ref = torch.Generator(device=device).manual_seed(seed)
    for i in range(model.sem_id_dim):
        torch.empty(B * (1 if i == 0 else k), V, device=device).exponential_(generator=ref)
    assert torch.equal(gen.get_state(), ref.get_state()), "one exponential_ per step"
    assert model.training and model.transformer.cached_enc_output is None


def test_mask_and_prebuilt_filter_are_one_argument(golden, device):
    f = _fixture(golden, device)
    model, batch, mask = f["model"], f["batch"], f["mask"].to(device)
    filt = model.inference_prefix_index.item_filter(mask)
    zeros = torch.zeros(batch.sem_ids.shape[0], dtype=torch.int64, device=device)
    a = model.recommend(batch, k=5, item_filter=mask)
    for other in (model.recommend(batch, k=5, item_filter=filt),
                  model.recommend(batch, k=5, item_filter=mask.unsqueeze(0), filter_group=zeros),
                  model.recommend(batch, k=5, item_filter=filt, filter_group=zeros)):
        assert torch.equal(a.item_ids, other.item_ids) and torch.equal(a.sem_ids, other.sem_ids)
        assert torch.equal(a.log_probas.view(torch.int32), other.log_probas.view(torch.int32))
    draws = [model.sample_items(batch, k=5, item_filter=flt, generator=torch.Generator(device=device).manual_seed(4))
             for flt in (mask, filt)]
    assert torch.equal(draws[0].item_ids, draws[1].item_ids)
    assert torch.equal(draws[0].perturbed.view(torch.int32), draws[1].perturbed.view(torch.int32))
