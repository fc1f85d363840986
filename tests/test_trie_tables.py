"""A public call's group-table arguments (item_filter / filter_group, item_bias / bias_group), whichever call takes
them. On the host: every argument error of recommend, generate_next_sem_id(constrained=True) and sample_items is raised
before any device work and under the name of the call that was made. On the device: a raw mask or bias tensor gives
recommend's result with the prebuilt ItemFilter / ItemBias bit for bit, and group=None on a one-group table the result
of an explicit all-zero group — filter and bias, with and without exclude_items, on the narrow and the wide kernel.

generate_next_sem_id and sample_items take no item_bias, so the bias errors and the filter-plus-bias refusal are
recommend's alone."""
import pytest
import torch

import beam_support as bs

_CONSTRAINED = dict(top_k=True, fused=True, sample=False, constrained=True)


def _host_model():
    from data.schemas import TokenizedSeqBatch
    from modules.model import EncoderDecoderRetrievalModel
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=12, sem_id_dim=4, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    model.inference_prefix_index = bs.ids_tokenizer(bs.FIVE.clone())
    z = torch.zeros(3, 8, dtype=torch.int64)
    batch = TokenizedSeqBatch(user_ids=z[:, :1], sem_ids=z, sem_ids_fut=None, seq_mask=z.bool(), token_type_ids=z,
                              token_type_ids_fut=None)
    return model, batch


def _calls(model, batch, bias: bool):
    """(name, call) of every public call that takes the table: call(**kw) passes the keywords on."""
    if bias:
        return [("recommend", lambda **kw: model.recommend(batch, **kw))]
    return [("recommend", lambda **kw: model.recommend(batch, **kw)),
            ("generate_next_sem_id", lambda **kw: model.generate_next_sem_id(batch, **_CONSTRAINED, **kw)),
            ("sample_items", lambda **kw: model.sample_items(batch, **kw))]


@pytest.mark.parametrize("arg, group_arg, off, two", [
    ("item_filter", "filter_group", "unfiltered", torch.ones(2, 5, dtype=torch.bool)),
    ("item_bias", "bias_group", "unbiased", torch.zeros(2, 5))])
def test_group_table_errors_carry_the_callers_name(arg, group_arg, off, two):
    """The tiny model is on the CPU: a call that got past its argument checks would fail in the first device op with
    another error, so every ValueError below was raised before any device work."""
    model, batch = _host_model()
    tok = model.inference_prefix_index
    ok_group = torch.zeros(3, dtype=torch.int64)
    for name, call in _calls(model, batch, bias=arg == "item_bias"):
        for table in (two, getattr(tok, arg)(two)):   # raw and prebuilt
            with pytest.raises(ValueError) as e:
                call(**{arg: table})
            assert str(e.value) == (f"{name}: {arg} has 2 groups; {group_arg} (B,) must say which one every user "
                                    f"reads (-1: {off})")
            for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3),
                        torch.zeros(3, dtype=torch.bool)):
                with pytest.raises(ValueError) as e:
                    call(**{arg: table, group_arg: bad})
                assert str(e.value) == (f"{name}: {group_arg} must be (B,) integer with B = 3, got {bad.dtype} "
                                        f"{tuple(bad.shape)}")
        with pytest.raises(ValueError) as e:
            call(**{group_arg: ok_group})
        assert str(e.value) == f"{name}: {group_arg} without {arg}"
        assert model.training and model.transformer.cached_enc_output is None


def test_filter_with_bias_is_refused_under_recommends_name():
    model, batch = _host_model()
    tok = model.inference_prefix_index
    mask, bias = torch.ones(5, dtype=torch.bool), torch.zeros(5)
    for flt in (mask, tok.item_filter(mask)):
        for b in (bias, tok.item_bias(bias)):
            with pytest.raises(ValueError, match="^recommend: item_filter and item_bias cannot be combined; write the "
                                                 "filter into the bias as -inf"):
                model.recommend(batch, item_filter=flt, item_bias=b)
    # the refusal comes first: neither table is looked at
    with pytest.raises(ValueError, match="^recommend: item_filter and item_bias cannot be combined"):
        model.recommend(batch, item_filter=torch.ones(4, dtype=torch.bool), item_bias=torch.zeros(2, 5))


_FIX = {}


def _fixture(golden, device):
    """The bias and filter model tests' set-up: the small decoder over the 300-row hand corpus, B = 3."""
    if not _FIX:
        z = golden("generation")
        tok, corpus = bs.tokenizer("c300", device)
        model = bs.decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]))
        model.enable_generation = True
        model.inference_prefix_index = tok
        batch = bs.tokenized(z, device)
        N = len(corpus.rows)
        g = torch.Generator().manual_seed(31)
        seen = torch.randint(0, N, (batch.sem_ids.shape[0], 6), generator=g)
        seen[1, 4:] = -1
        _FIX.update(model=model, batch=batch, tok=tok, seen=seen.to(device),
                    item_filter=(torch.rand(N, generator=g) < 0.5).to(device),
                    item_bias=(2.0 * torch.randn(N, generator=g)).to(device))
    return _FIX


def _same(got, want, what):
    assert type(got) is type(want)
    for name, a, b in zip(want._fields, got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), f"{what}: {name}"   # dead rows (-1, -inf) included


@pytest.mark.gpu
@pytest.mark.parametrize("excluded", [False, True])
@pytest.mark.parametrize("beams", [32, 64])   # the narrow kernel; the smallest width here that reaches the wide one
@pytest.mark.parametrize("arg, group_arg", [("item_filter", "filter_group"), ("item_bias", "bias_group")])
def test_raw_table_and_default_group_give_the_prebuilt_result(golden, device, arg, group_arg, beams, excluded):
    f = _fixture(golden, device)
    model, batch, raw = f["model"], f["batch"], f[arg]
    B = batch.sem_ids.shape[0]
    kw = dict(k=beams, beams=beams, exclude_items=f["seen"] if excluded else None)
    built = getattr(f["tok"], arg)(raw)
    assert built.groups == 1
    want = model.recommend(batch, **kw, **{arg: built})
    assert (want.item_ids[:, 0] >= 0).all(), "precondition: live rows"
    plain = model.recommend(batch, **kw)
    assert not torch.equal(plain.item_ids, want.item_ids), "precondition: the table changes the list"
    _same(model.recommend(batch, **kw, **{arg: raw}), want, "raw tensor")
    for dtype in (torch.int64, torch.int32):
        zero = torch.zeros(B, dtype=dtype, device=device)
        _same(model.recommend(batch, **kw, **{arg: built, group_arg: zero}), want, f"explicit {dtype} zero group")
        _same(model.recommend(batch, **kw, **{arg: raw, group_arg: zero}), want, f"raw, explicit {dtype} zero group")
