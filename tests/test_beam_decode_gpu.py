"""Incremental beam decoding on the device: rq_beam_self_attn against an fp64 softmax, rq_beam_select_parent,
BeamDecodeState's per-step logits against the full forward of the existing generation path, and
generate_next_sem_id(incremental=True) against the golden generation fixture."""
import numpy as np
import pytest
import torch

import beam_support as bs
import gen_inputs as gi

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ rq_beam_self_attn
def _self_attn_case(R, t, H, hd, seed):
    """Step buffers as the decoder leaves them: packed (R_s, 3A) qkv tensors, R_0 = 3 rows when t > 0 (fewer
    than the beams that descend from them), R rows later; the last step's buffer is wider than 3A (a row stride
    the kernel must honour). anc: column 0 repeats the 3 BOS rows, one column is a permutation, the others repeat
    and drop rows at random."""
    g = torch.Generator().manual_seed(seed)
    A = H * hd
    bufs = []
    for s in range(t + 1):
        rows = 3 if (s == 0 and t > 0) else R
        width = 3 * A + (8 if s == t else 0)
        bufs.append(torch.randn(rows, width, generator=g))
    anc = None
    if t > 0:
        cols = [torch.randint(0, 3, (R,), generator=g)]
        for s in range(1, t):
            cols.append(torch.randperm(R, generator=g) if s == 1 else torch.randint(0, R, (R,), generator=g))
        anc = torch.stack(cols, 1).to(torch.int32)
    return bufs, anc


def _self_attn_reference(bufs, anc, R, t, H, hd):
    A = H * hd
    q = bufs[t][:, :A].double().view(R, H, hd)
    ks, vs = [], []
    for s in range(t + 1):
        rows = torch.arange(R) if s == t else anc[:, s].long()
        ks.append(bufs[s][rows, A:2 * A].double().view(R, H, hd))
        vs.append(bufs[s][rows, 2 * A:3 * A].double().view(R, H, hd))
    k, v = torch.stack(ks, 2), torch.stack(vs, 2)                       # (R, H, t + 1, hd)
    p = torch.softmax((q.unsqueeze(2) * k).sum(-1) / hd ** 0.5, dim=-1)
    return (p.unsqueeze(-1) * v).sum(2).reshape(R, A)


@pytest.mark.parametrize("R,t,H,hd", [(1, 0, 1, 16), (70, 1, 4, 16), (70, 3, 2, 64), (33, 7, 1, 128), (5, 2, 3, 32)])
def test_beam_self_attention_vs_fp64(device, R, t, H, hd):
    from rqvae_hip import ops
    A = H * hd
    bufs, anc = _self_attn_case(R, t, H, hd, 1000 + R + 10 * t + hd)
    ref = _self_attn_reference(bufs, anc, R, t, H, hd)
    dev = [b.to(device) for b in bufs]
    assert dev[t].stride(0) > 3 * A
    steps = [(b[:, A:2 * A], b[:, 2 * A:3 * A]) for b in dev]
    out = ops.beam_self_attention(dev[t][:, :A], steps, None if anc is None else anc.to(device), H)
    assert out.shape == (R, A) and out.dtype == torch.float32 and out.is_contiguous()
    got = out.cpu()
    if t == 0:   # one key: weight exp(0) / 1
        assert torch.equal(got.view(torch.int32), bufs[0][:, 2 * A:3 * A].contiguous().view(torch.int32))
    err = (got.double() - ref).abs() - (2e-5 + 2e-4 * ref.abs())
    assert float(err.max()) <= 0, f"max abs err {float((got.double() - ref).abs().max()):.3e}"
    # an explicit scale is honoured (scale 0: uniform weights = the mean of the ancestors' values)
    flat = ops.beam_self_attention(dev[t][:, :A], steps, None if anc is None else anc.to(device), H, scale=0.0).cpu()
    mean = _self_attn_reference([torch.cat([torch.zeros_like(b[:, :2 * A]), b[:, 2 * A:]], 1) for b in bufs], anc,
                                R, t, H, hd)
    assert float(((flat.double() - mean).abs() - (2e-5 + 2e-4 * mean.abs())).max()) <= 0


def test_beam_self_attention_refuses_bad_arguments(device):
    from rqvae_hip import ops, RqHipError
    qkv0, qkv1 = torch.randn(3, 96, device=device), torch.randn(6, 96, device=device)
    s0, s1 = (qkv0[:, 32:64], qkv0[:, 64:]), (qkv1[:, 32:64], qkv1[:, 64:])
    anc = torch.zeros(6, 1, dtype=torch.int32, device=device)
    assert ops.beam_self_attention(qkv1[:, :32], [s0, s1], anc, 2).shape == (6, 32)
    with pytest.raises(RqHipError, match="anc"):
        ops.beam_self_attention(qkv1[:, :32], [s0, s1], None, 2)
    with pytest.raises(RqHipError, match="anc"):
        ops.beam_self_attention(qkv1[:, :32], [s0, s1], anc.long(), 2)
    with pytest.raises(RqHipError, match="one row per beam"):
        ops.beam_self_attention(qkv1[:, :32], [s1, s0], anc, 2)
    with pytest.raises(RqHipError, match="head_dim"):
        ops.beam_self_attention(qkv1[:, :32], [s0, s1], anc, 4)   # hd = 8
    with pytest.raises(RqHipError, match="contiguous last dimension"):
        ops.beam_self_attention(qkv1[:, :64:2], [s0, s1], anc, 2)
    with pytest.raises(RqHipError, match="steps"):
        ops.beam_self_attention(qkv1[:, :32], [s1] * 9, torch.zeros(6, 8, dtype=torch.int32, device=device), 2)
    empty = torch.zeros(0, 96, device=device)
    assert ops.beam_self_attention(empty[:, :32], [(empty[:, 32:64], empty[:, 64:])], None, 2).shape == (0, 32)


# ------------------------------------------------------------------------------------------ return_parent
@pytest.mark.parametrize("B,kprev,n_cand,P,k", [(3, 1, 7, 0, 5), (2, 4, 6, 2, 4)])
def test_beam_select_return_parent(device, B, kprev, n_cand, P, k):
    from rqvae_hip import ops
    g, cand_ids, cand_lp, parents, parent_lp = bs.select_inputs(B, kprev, n_cand, P, 7 + kprev)
    valid = torch.rand(B, kprev * n_cand, generator=g) < 0.7
    score = torch.where(valid, 0.0, -10000.0).float() + cand_lp.reshape(B, -1)
    if parent_lp is not None:
        score = score + parent_lp.repeat_interleave(n_cand, dim=1)
    want_parent = torch.sort(score, dim=-1, descending=True, stable=True).indices[:, :k] // n_cand
    args = (cand_ids.to(device), cand_lp.to(device), k)
    kw = dict(batch=B, valid=valid.to(device), parents=bs.dev(parents, device),
              parent_lp=bs.dev(parent_lp, device))
    plain = ops.beam_select(*args, **kw)
    assert len(plain) == 2
    ids, lp, parent = ops.beam_select(*args, return_parent=True, **kw)
    assert parent.dtype == torch.int32 and parent.shape == (B, k)
    assert torch.equal(parent.cpu().long(), want_parent)
    bs.assert_select((ids, lp), (plain[0].cpu(), plain[1].cpu()))
    bs.assert_select((ids, lp), bs.select_reference(cand_ids, cand_lp, valid, parents, parent_lp, B, k))


# ------------------------------------------------------------------------------------------ teacher-forced steps
def _hd64_case(device):
    """E = 32, A = 128, H = 2 (hd = 64), 2 + 2 layers, K = 32, 4 tokens; B = 4 users with 5, 0, 2 and 3 context
    items (one seq_mask row all False: that user's context is its user token alone)."""
    from data.schemas import TokenizedSeqBatch
    dims = dict(E=32, A=128, H=2, n_layers=4, K=32, L1=4, n_max=5, seed=77)
    model = bs.decoder_model(dims, device)
    g = gi.rng(78)
    B, n_max, L1, K = 4, 5, 4, 32
    mask = np.zeros((B, n_max * L1), bool)
    for b, n in enumerate((5, 0, 2, 3)):
        mask[b, :n * L1] = True
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    batch = TokenizedSeqBatch(user_ids=t(g.integers(0, 10 ** 6, size=(B, 1))),
                              sem_ids=t(np.where(mask, g.integers(0, K, size=mask.shape), -1)), sem_ids_fut=None,
                              seq_mask=t(mask), token_type_ids=t(np.tile(np.arange(L1), (B, n_max))),
                              token_type_ids_fut=None)
    return model, batch


def _golden_case(golden, device):
    z = golden("generation")
    return bs.decoder_model(z, device, scale_out=float(z["out_proj_scale"])), bs.tokenized(z, device)


_PARENTS = {1: [2, 2, 0], 2: [1, 0, 1]}   # per user, rolled by its index: a duplicated parent and a dropped one


def _teacher_forced_logits(model, batch, k):
    """[(incremental logits, full-forward logits)] per step, the beams chosen by hand."""
    from modules.model import BeamDecodeState
    K, L1, B = model.num_embeddings, model.sem_id_dim, batch.sem_ids.shape[0]
    dev = batch.sem_ids.device
    model.eval()
    model.enable_generation = True
    model.transformer.cached_enc_output = None
    pairs = []
    try:
        with torch.no_grad():
            state = BeamDecodeState(model, batch)
            cur = bs.first_batch(batch)
            generated = parent = None
            for i in range(L1):
                got = state.step() if i == 0 else state.step(generated[:, :, -1], parent)
                pairs.append((got, model.forward(cur).logits))
                if i == L1 - 1:
                    break
                b_, j_ = torch.meshgrid(torch.arange(B), torch.arange(k), indexing="ij")
                tokens = ((7 * b_ + 3 * j_ + 11 * i + 5) % K).to(dev)
                if i == 0:
                    parent = torch.zeros(B, k, dtype=torch.int32, device=dev)
                    generated = tokens.unsqueeze(-1)
                else:
                    parent = torch.stack([torch.roll(torch.tensor(_PARENTS[i]), b) for b in range(B)]).to(dev, torch.int32)
                    kept = torch.gather(generated, 1, parent.long().unsqueeze(2).expand(-1, -1, i))
                    generated = torch.cat([kept, tokens.unsqueeze(-1)], dim=-1)
                cur = bs.beams_batch(model, cur, generated, i == 0, k)
    finally:
        model.transformer.cached_enc_output = None
    return pairs


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("case", ["golden-hd16", "hd64"])
def test_decode_state_step_logits(golden, device, case, precision):
    """Every step's logits of BeamDecodeState against model.forward on the whole beams with the repeated encoder
    cache: |err| <= 2e-4 max|logit|, at the exact-fp32 matmul precision and at 'high' (the paired / hoisted /
    residual-epilogue GEMM forms)."""
    model, batch = _golden_case(golden, device) if case == "golden-hd16" else _hd64_case(device)
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(precision)
    try:
        pairs = _teacher_forced_logits(model, batch, 3)
    finally:
        torch.set_float32_matmul_precision(prev)
    B, K = batch.sem_ids.shape[0], model.num_embeddings
    assert len(pairs) == model.sem_id_dim
    for i, (got, want) in enumerate(pairs):
        assert got.shape == want.shape == ((B if i == 0 else 3 * B), K), i
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        print(f"{case} {precision} step {i}: max|err| {err:.3e}, max|logit| {scale:.3e}, ratio {err / scale:.3e}")
        assert err <= 2e-4 * scale, (i, err, scale)


# ------------------------------------------------------------------------------------------ generation
def test_incremental_generation_vs_reference(golden, device):
    z = golden("generation")
    model = bs.decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]))
    model.enable_generation = True
    batch = bs.tokenized(z, device)
    for top_k, tag in ((True, "topk"), (False, "greedy")):
        g = model.generate_next_sem_id(batch, temperature=1, top_k=top_k, fused=True, sample=False, incremental=True)
        assert np.array_equal(g.sem_ids.cpu().numpy(), z[f"{tag}_sem_ids"]), tag
        np.testing.assert_allclose(g.log_probas.cpu().numpy(), z[f"{tag}_log_probas"], rtol=1e-5, atol=0)
    assert model.training and model.transformer.cached_enc_output is None


@pytest.mark.parametrize("reference_batching", [True, False])
def test_incremental_generation_prefix_index(golden, device, reference_batching):
    z = golden("generation")
    tok = bs.corpus_tokenizer(golden("tokenizer"), device)
    tok.reference_batching = reference_batching
    model = bs.decoder_model(z, device, dropout=0.3, scale_out=float(z["out_proj_scale"]),
                                       verifier=lambda x: tok.exists_prefix(x))
    model.enable_generation = True
    model.inference_prefix_index = tok
    batch = bs.tokenized(z, device)
    want = model.generate_next_sem_id(batch, temperature=1, top_k=True, fused=True, sample=False)
    got = model.generate_next_sem_id(batch, temperature=1, top_k=True, fused=True, sample=False, incremental=True)
    assert model.training, "train mode restored"
    assert model.transformer.cached_enc_output is None, "encoder cache cleared"
    assert torch.equal(got.sem_ids, want.sem_ids)
    np.testing.assert_allclose(got.log_probas.cpu().numpy(), want.log_probas.cpu().numpy(), rtol=1e-5, atol=0)


def test_incremental_generation_sampled_properties(golden, device):
    z = golden("generation")
    tok = bs.corpus_tokenizer(golden("tokenizer"), device)
    tok.reference_batching = False
    model = bs.decoder_model(z, device, scale_out=float(z["out_proj_scale"]))
    model.enable_generation = True
    model.inference_prefix_index = tok
    kw = dict(temperature=1, top_k=True, fused=True, sample=True, incremental=True)
    torch.manual_seed(0)
    out = model.generate_next_sem_id(bs.tokenized(z, device), **kw)
    ids, lp = out.sem_ids.cpu(), out.log_probas.cpu()
    assert ids.shape == (3, 32, 4) and lp.shape == (3, 32)
    assert torch.all(lp[:, :-1] >= lp[:, 1:]), "beams sorted by cumulative log-probability"
    for b in range(3):
        assert len({tuple(r) for r in ids[b].tolist()}) == 32, "a beam's candidates are distinct"
    corpus = set(map(tuple, golden("tokenizer")["corpus_ids"].tolist()))
    ok = lp > -5000
    assert all(tuple(r) in corpus for r in ids[ok].tolist())
    torch.manual_seed(1)
    again = model.generate_next_sem_id(bs.tokenized(z, device), **kw)
    assert not torch.equal(again.sem_ids.cpu(), ids) or not ok.any(), "the draw follows torch's generator"
    assert model.training and model.transformer.cached_enc_output is None
