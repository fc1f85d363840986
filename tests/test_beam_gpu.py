"""Decoder evaluation kernels (csrc/beam.hip) and the fused generation path built on them:
rqvae_hip.ops.beam_candidates / beam_select / topk_hits against CPU references written here, and
EncoderDecoderRetrievalModel.generate_next_sem_id(fused=True) against the reference fixture (generation.npz) and
against the unfused path."""
import numpy as np
import pytest
import torch

import beam_support as bs
import gen_inputs as gi

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ beam_candidates
def _cand_reference(logits, noise, T, n_cand):
    """fp64: softmax(logits / T), scores p / noise, stable descending sort -> (sorted scores, ids, log p)."""
    p = torch.softmax(logits.double() / T, dim=-1)
    s = p if noise is None else p / noise.double()
    ss, order = torch.sort(s, dim=-1, descending=True, stable=True)
    ids = order[:, :n_cand]
    # log p without the cancellation of log(1 - tiny) where one class dominates (there fp64's own log(softmax) is
    # off by percents): log p_v = (z_v - max) - log1p(sum of the other classes' exp(z - max))
    z = logits.double() / T
    m, am = z.max(dim=-1, keepdim=True)
    e = torch.exp(z - m).scatter(1, am, 0.0)
    return ss, ids, torch.gather((z - m) - torch.log1p(e.sum(-1, keepdim=True)), 1, ids)


def _draw_rows(g, rows, V, dominant):
    x = 2.0 * torch.randn(rows, V, generator=g)
    if dominant:   # one class takes nearly all the mass; the others are tiny but non-zero in fp32
        x = x - 30.0
        x[:, int(torch.randint(0, V, (1,), generator=g))] = 10.0
    return x


def _separated_case(R, V, n_cand, T, with_noise, seed):
    """Seeded logits (row 0 dominant when R > 1) and noise whose top n_cand + 1 fp64 scores are pairwise separated
    by >= 1e-5 relative in every row (offending rows are redrawn from the same stream), so fp32 rounding of the
    softmax cannot decide an order."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.cat([_draw_rows(g, 1, V, R > 1), _draw_rows(g, R - 1, V, False)]) if R > 1 else _draw_rows(g, 1, V, False)
    noise = torch.empty(R, V).exponential_(generator=g) if with_noise else None
    top = min(n_cand + 1, V)
    for _ in range(200):
        ss = _cand_reference(logits, noise, T, n_cand)[0][:, :top]
        bad = ((ss[:, :-1] - ss[:, 1:]) < 1e-5 * ss[:, :-1]).any(dim=1) if top > 1 else torch.zeros(R, dtype=torch.bool)
        if not bad.any():
            break
        for r in bad.nonzero().flatten().tolist():
            logits[r] = _draw_rows(g, 1, V, R > 1 and r == 0)[0]
            if noise is not None:
                noise[r] = torch.empty(V).exponential_(generator=g)
    ss = _cand_reference(logits, noise, T, n_cand)[0][:, :top]
    assert top == 1 or bool(((ss[:, :-1] - ss[:, 1:]) >= 1e-5 * ss[:, :-1]).all()), "precondition: separated scores"
    return logits, noise


_CAND_SHAPES = [(1, 37, 1), (3, 256, 200), (96, 256, 200), (2, 256, 256), (5, 2000, 200)]


@pytest.mark.parametrize("with_noise", [False, True], ids=["topn", "noise"])
@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("R,V,n_cand", _CAND_SHAPES)
def test_beam_candidates(device, R, V, n_cand, T, with_noise):
    from rqvae_hip import ops
    logits, noise = _separated_case(R, V, n_cand, T, with_noise, seed=1000 + R + V + n_cand + int(10 * T) + with_noise)
    _, ids, lp = _cand_reference(logits, noise, T, n_cand)
    got_ids, got_lp = ops.beam_candidates(logits.to(device), n_cand, T, None if noise is None else noise.to(device))
    assert got_ids.dtype == torch.int64 and got_ids.shape == (R, n_cand) and got_lp.shape == (R, n_cand)
    assert torch.equal(got_ids.cpu(), ids)
    np.testing.assert_allclose(got_lp.cpu().double().numpy(), lp.numpy(), rtol=1e-5, atol=0)


def test_beam_candidates_ties_and_underflow(device):
    from rqvae_hip import ops
    V = 130
    logits = torch.stack([(torch.arange(V) % 5).float(), ((torch.arange(V) * 7) % 3).float(), torch.zeros(V)])
    ids, _ = ops.beam_candidates(logits.to(device), 100, 1.0)
    want = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :100]
    assert torch.equal(ids.cpu(), want), "equal scores: the lower class index first"
    # a probability that underflows to 0 in fp32 has log-probability -inf, as torch.log(softmax) gives
    x = torch.full((1, 70), -200.0)
    x[0, 5] = 0.0
    ids, lp = ops.beam_candidates(x.to(device), 3, 1.0)
    assert ids.cpu().tolist() == [[5, 0, 1]]
    assert lp.cpu()[0, 0] == 0 and torch.isneginf(lp.cpu()[0, 1:]).all()


def test_beam_ops_refuse_bad_arguments(device):
    from rqvae_hip import ops, RqHipError
    x = torch.zeros(2, 16)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_candidates(x, 4)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.topk_hits(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 3, 4, dtype=torch.int64), [1], torch.zeros(8, dtype=torch.int64))
    with pytest.raises(RqHipError, match="rc=-22"):
        ops.beam_candidates(x.to(device), 17)            # n_cand > V
    with pytest.raises(RqHipError, match="rc=-22"):
        ops.beam_candidates(torch.zeros(1, 5000, device=device), 4)   # V > 4096
    with pytest.raises(RqHipError, match="float32"):
        ops.beam_candidates(x.double().to(device), 4)
    ids, lp = ops.beam_candidates(x.to(device), 4)
    with pytest.raises(RqHipError, match="rc=-22"):
        ops.beam_select(ids, lp, 5, batch=2, valid=torch.ones(8, dtype=torch.bool, device=device))   # k > N
    with pytest.raises(RqHipError, match="exactly one"):
        ops.beam_select(ids, lp, 2, batch=2)


# ------------------------------------------------------------------------------------------ beam_select
_SEL_SHAPES = [(3, 1, 200, 0, 32), (3, 32, 200, 1, 32), (1, 32, 200, 3, 32), (2, 1, 1, 0, 1), (2, 1, 1, 2, 1)]


@pytest.mark.parametrize("few_valid", [False, True], ids=["mask", "few-valid"])
@pytest.mark.parametrize("B,kprev,n_cand,P,k", _SEL_SHAPES)
def test_beam_select_mask(device, B, kprev, n_cand, P, k, few_valid):
    from rqvae_hip import ops
    g, cand_ids, cand_lp, parents, parent_lp = bs.select_inputs(B, kprev, n_cand, P, 50 + kprev + n_cand + P)
    N = kprev * n_cand
    if few_valid:   # fewer than k valid candidates and one log-probability: the -10000 ties fill the beams in order
        valid = torch.zeros(B, N, dtype=torch.bool)
        valid[:, torch.randperm(N, generator=g)[:min(5, N - 1)]] = True
        cand_lp = torch.full_like(cand_lp, -1.5)
    else:
        valid = torch.rand(B, N, generator=g) < 0.7
    want = bs.select_reference(cand_ids, cand_lp, valid, parents, parent_lp, B, k)
    got = ops.beam_select(cand_ids.to(device), cand_lp.to(device), k, batch=B, valid=valid.to(device),
                          parents=bs.dev(parents, device), parent_lp=bs.dev(parent_lp, device))
    assert got[0].shape == (B, k, P + 1) and got[1].shape == (B, k)
    bs.assert_select(got, want)


@pytest.mark.parametrize("reference_batching", [True, False])
@pytest.mark.parametrize("B,kprev,n_cand,P,k", _SEL_SHAPES)
def test_beam_select_key_table(device, B, kprev, n_cand, P, k, reference_batching):
    """In-kernel verification against the tokenizer's packed-prefix table == exists_prefix on the materialised
    prefixes: corpus prefixes, absent prefixes, ids >= base (out of range), and the unchecked tail of
    reference_batching (B N = 600 -> the last 8 candidates; B N = 2 -> every candidate)."""
    from rqvae_hip import ops
    tok = bs.hand_tokenizer(device)
    tok.reference_batching = reference_batching
    g, cand_ids, cand_lp, parents, parent_lp = bs.select_inputs(B, kprev, n_cand, P, 90 + kprev + n_cand + P, hi=14)
    N = kprev * n_cand
    corpus = tok.cached_ids.cpu()
    if P:   # most parents are corpus prefixes (so many candidates are valid), some are not, one is out of range
        rows = torch.randint(0, corpus.shape[0], (B, kprev), generator=g)
        keep = torch.rand(B, kprev, generator=g) < 0.8
        parents = torch.where(keep.unsqueeze(-1), corpus[rows][:, :, :P], parents)
        parents[0, 0, 0] = 13
    if N == 1:
        cand_ids[0, 0] = corpus[0, P] if P == 0 else cand_ids[0, 0]
    par = parents.repeat_interleave(n_cand, dim=1).reshape(B * N, P) if P else torch.zeros(B * N, 0, dtype=torch.int64)
    prefixes = torch.cat([par, cand_ids.reshape(B * N, 1)], dim=1)          # (B N, P + 1), flat candidate order
    valid = tok.exists_prefix(prefixes.to(device)).cpu()
    if reference_batching:
        assert not valid[B * N // 16 * 16:].any()
    if N > 1:
        assert valid.any() and not valid.all()
    want = bs.select_reference(cand_ids, cand_lp, valid, parents, parent_lp, B, k)
    keys, base = tok.prefix_table(P + 1)
    assert base == 12 and (N == 1 or (cand_ids >= base).any())
    got = ops.beam_select(cand_ids.to(device), cand_lp.to(device), k, batch=B, keys=keys, base=base,
                          checked=B * N // 16 * 16 if reference_batching else B * N,
                          parents=bs.dev(parents, device), parent_lp=bs.dev(parent_lp, device))
    bs.assert_select(got, want)


# ------------------------------------------------------------------------------------------ fused generation
def test_fused_generation_vs_reference(golden, device):
    """fused=True, sample=False is the reference run with torch.multinomial replaced by the top-n stand-in."""
    z = golden("generation")
    model = bs.decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]))
    model.enable_generation = True
    batch = bs.tokenized(z, device)
    for top_k, tag in ((True, "topk"), (False, "greedy")):
        g = model.generate_next_sem_id(batch, temperature=1, top_k=top_k, fused=True, sample=False)
        assert np.array_equal(g.sem_ids.cpu().numpy(), z[f"{tag}_sem_ids"]), tag
        np.testing.assert_allclose(g.log_probas.cpu().numpy(), z[f"{tag}_log_probas"], rtol=1e-5, atol=0)
    assert model.training and model.transformer.cached_enc_output is None


@pytest.mark.parametrize("reference_batching", [True, False])
def test_fused_generation_prefix_index(golden, device, monkeypatch, reference_batching):
    """The in-kernel table path against the unfused path calling tokenizer.exists_prefix (both with the top-n
    sampler): same beams. The model's ids reach 255, the corpus' base is 759 and its first level has 2 codes, so
    the beams hold verified prefixes, rejected ones and (reference_batching, B = 3) a whole unchecked first step."""
    z = golden("generation")
    tok = bs.corpus_tokenizer(golden("tokenizer"), device)
    tok.reference_batching = reference_batching
    model = bs.decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]), verifier=lambda x: tok.exists_prefix(x))
    model.enable_generation = True
    n_params = len(list(model.parameters()))
    model.inference_prefix_index = tok
    assert len(list(model.parameters())) == n_params and "inference_prefix_index" not in dict(model.named_modules())
    batch = bs.tokenized(z, device)
    with monkeypatch.context() as m:
        m.setattr(torch, "multinomial", gi.topn_multinomial)
        want = model.generate_next_sem_id(batch, temperature=1, top_k=True)
    assert model.training
    got = model.generate_next_sem_id(batch, temperature=1, top_k=True, fused=True, sample=False)
    assert model.training, "train mode restored"
    assert model.transformer.cached_enc_output is None, "encoder cache cleared"
    assert torch.equal(got.sem_ids, want.sem_ids)
    np.testing.assert_allclose(got.log_probas.cpu().numpy(), want.log_probas.cpu().numpy(), rtol=1e-5, atol=0)


def test_fused_generation_sampled_properties(golden, device):
    z = golden("generation")
    tok = bs.corpus_tokenizer(golden("tokenizer"), device)
    tok.reference_batching = False
    model = bs.decoder_model(z, device, scale_out=float(z["out_proj_scale"]))
    model.enable_generation = True
    model.inference_prefix_index = tok
    torch.manual_seed(0)
    out = model.generate_next_sem_id(bs.tokenized(z, device), temperature=1, top_k=True, fused=True, sample=True)
    ids, lp = out.sem_ids.cpu(), out.log_probas.cpu()
    assert ids.shape == (3, 32, 4) and lp.shape == (3, 32)
    assert torch.all(lp[:, :-1] >= lp[:, 1:]), "beams sorted by cumulative log-probability"
    for b in range(3):
        assert len({tuple(r) for r in ids[b].tolist()}) == 32, "a beam's candidates are distinct"
    corpus = set(map(tuple, golden("tokenizer")["corpus_ids"].tolist()))
    ok = lp > -5000
    assert all(tuple(r) in corpus for r in ids[ok].tolist())
    torch.manual_seed(1)
    again = model.generate_next_sem_id(bs.tokenized(z, device), temperature=1, top_k=True, fused=True, sample=True)
    assert not torch.equal(again.sem_ids.cpu(), ids) or not ok.any(), "the draw follows torch's generator"


# ------------------------------------------------------------------------------------------ topk_hits
def test_topk_hits_matches_cpu_accumulator(golden, device):
    from evaluate.metrics import TopKAccumulator
    z = golden("topk_metrics")
    ks = [int(k) for k in z["ks"]]
    batches = [(torch.from_numpy(z["actual1"]), torch.from_numpy(z["topk1"])),
               (torch.from_numpy(z["actual2"]), torch.from_numpy(z["topk2"]))]
    g = torch.Generator().manual_seed(5)   # more rows than one workgroup's waves, more beams than one wave's lanes
    batches.append((torch.randint(0, 3, (37, 4), generator=g), torch.randint(0, 3, (37, 70, 4), generator=g)))
    cpu, gpu = TopKAccumulator(ks=ks), TopKAccumulator(ks=ks)
    for a, t in batches:   # accumulate calls back to back: nothing is read between them
        cpu.accumulate(actual=a, top_k=t)
        gpu.accumulate(actual=a.to(device), top_k=t.to(device))
    assert gpu.counts.is_cuda and gpu.counts.dtype == torch.int64
    assert torch.equal(gpu.counts.cpu(), cpu.counts)
    assert gpu.reduce() == cpu.reduce()
    fix = TopKAccumulator(ks=ks)
    for a, t in batches[:2]:
        fix.accumulate(actual=a.to(device), top_k=t.to(device))
    got = fix.reduce()
    assert list(got) == [str(k) for k in z["keys"]] and list(got.values()) == z["values_both"].tolist()
