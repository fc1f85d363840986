"""Scoring caller-named candidates on the device: rq_score_paths against an fp64 log-softmax + gather + add, bitwise
against rq_beam_expand over a complete synthetic trie level, its ranks against a CPU stable ordering, its refusals;
then model.score_sem_ids / score_items against an fp64 teacher-forced loop over the model's own full forwards, their
agreement with recommend(), and the evaluator's sampled-negatives switch."""
import glob

import numpy as np
import pytest
import torch

import beam_support as bs

pytestmark = pytest.mark.gpu

_NINF = -float("inf")


# ------------------------------------------------------------------------------------------ kernel vs fp64
def _kernel_inputs(B, C, V, G, seed):
    """Logits 2 randn; tokens uniform in [0, V); about one candidate in six padding; about one present candidate in
    six with a token >= V or < 0; prev_lp negative with some -inf. Tokens live in a (B, C, 3) tensor: column 1."""
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(B * G, V, generator=g)
    tok3 = torch.randint(0, V, (B, C, 3), generator=g)
    present = torch.rand(B, C, generator=g) >= 1 / 6
    bad = present & (torch.rand(B, C, generator=g) < 1 / 6)
    off = torch.randint(0, 4, (B, C), generator=g)
    tok3[:, :, 1] = torch.where(bad, torch.where(off % 2 == 0, V + off, -1 - off), tok3[:, :, 1])
    prev = -(5.0 * torch.rand(B, C, generator=g)) - 0.1
    prev[torch.rand(B, C, generator=g) < 0.1] = _NINF
    return logits, tok3, present, bad, prev


def _score_reference(logits, tokens, present, prev, B, C, V, G, T):
    lp64 = bs.log_softmax64(logits, T).view(B, G, V).expand(B, C, V)
    ok = present & (tokens >= 0) & (tokens < V)
    want = lp64.gather(2, tokens.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    if prev is not None:
        want = want + prev.double()
    return torch.where(ok, want, torch.full_like(want, _NINF)), ok


def _assert_scores(lp, want, what=""):
    lp = lp.cpu()
    assert lp.dtype == torch.float32 and lp.shape == want.shape
    assert not torch.isnan(lp).any(), "never NaN"
    assert torch.equal(torch.isneginf(lp), torch.isneginf(want)), f"-inf exactly where the reference has it {what}"
    fin = torch.isfinite(want)
    if fin.any():
        print(f"{what} max rel err {float(((lp.double() - want).abs() / want.abs())[fin].max()):.3e}")
    np.testing.assert_allclose(lp.double()[fin].numpy(), want[fin].numpy(), rtol=1e-5, atol=0)


# C, V, G == C, T, strided tokens, prev_lp given
_KERNEL_CASES = [(1, 5, False, 1.0, False, False), (3, 12, False, 1.0, True, True), (64, 37, True, 1.0, False, True),
                 (65, 64, True, 1.0, True, True), (200, 65, True, 1.0, True, True), (1024, 256, False, 1.0, False, True),
                 (1024, 256, True, 1.0, False, True), (7, 300, True, 0.7, True, True),
                 (70, 1100, True, 1.0, True, True)]   # V > 1024: the 64-registers-per-lane instantiation


@pytest.mark.parametrize("C,V,per_cand,T,strided,with_prev", _KERNEL_CASES)
def test_score_paths_vs_fp64(device, C, V, per_cand, T, strided, with_prev):
    from rqvae_hip import ops
    B, G = 3, C if per_cand else 1
    logits, tok3, present, bad, prev = _kernel_inputs(B, C, V, G, seed=700 + 13 * C + V + G)
    if not with_prev:
        prev = None
    tokens = tok3[:, :, 1]
    want, ok = _score_reference(logits, tokens, present, prev, B, C, V, G, T)
    if C >= 64:
        assert (~present).any() and bad.any() and ok.any() and torch.isneginf(prev[ok]).any(), "every kind occurs"
    tdev = tok3.to(device)[:, :, 1]
    if not strided:
        tdev = tdev.contiguous()
    assert tdev.is_contiguous() == (not strided)
    lp, rank = ops.score_paths(logits.to(device), tdev, present=present.to(device),
                               prev_lp=bs.dev(prev, device), temperature=T)
    assert rank is None
    _assert_scores(lp, want, f"C={C} V={V} G={G} T={T}:")
    assert torch.isneginf(lp.cpu()[~present]).all(), "padding gives -inf"


def test_score_paths_dominant_and_underflow_rows(device):
    """Row 0: one logit 30 above the rest — its log-probability -log1p(39 e^-30) ~ -3.6e-12 keeps the relative
    tolerance (the log1p form). Row 1: a class 200 below the max has p == 0 in fp32 and gives exactly -inf."""
    from rqvae_hip import ops
    V = 40
    x = torch.zeros(2, V)
    x[0, 7] = 30.0
    x[1, 3] = -200.0
    tokens = torch.tensor([[7, 0], [3, 0]])
    lp = ops.score_paths(x.to(device), tokens.to(device))[0].cpu()
    want = bs.log_softmax64(x, 1.0).gather(1, tokens)
    assert -5e-12 < float(want[0, 0]) < -1e-12
    np.testing.assert_allclose(lp[0].double().numpy(), want[0].numpy(), rtol=1e-5, atol=0)
    assert lp[1, 0] == _NINF and torch.isfinite(want[1, 0]), "underflow: exactly -inf"
    np.testing.assert_allclose(float(lp[1, 1]), float(want[1, 1]), rtol=1e-5, atol=0)
    # the same rows as per-candidate rows (G == C == 1 is the shared-row form, so use C = 2 with a copy of each row)
    lp2 = ops.score_paths(x.repeat_interleave(2, 0).to(device), tokens.to(device))[0].cpu()
    assert torch.equal(lp2.view(torch.int32), lp.view(torch.int32)), "both forms give the same bits"


# ------------------------------------------------------------------------------------------ bitwise vs beam_expand
@pytest.mark.parametrize("kprev,V,with_parent", [(1, 256, True), (1, 37, False), (1, 300, True), (4, 12, True),
                                                 (32, 256, True), (1, 1100, True), (6, 1100, True)])
def test_score_paths_bitwise_equals_beam_expand(device, kprev, V, with_parent):
    """A complete trie level (every node has the children 0..V-1) and k = kprev V: beam_expand returns lp + parent_lp
    of every (beam, token). score_paths fed the same logits and prev_lp = parent_lp returns the same float bits."""
    from rqvae_hip import ops
    B = 2
    g = torch.Generator().manual_seed(800 + kprev + V)
    logits = (2.0 * torch.randn(B * kprev, V, generator=g)).to(device)
    child_off = (torch.arange(kprev + 1, dtype=torch.int32) * V).to(device)
    tok = torch.arange(V, dtype=torch.int32).repeat(kprev).to(device)
    beams = {}
    if with_parent:
        beams = dict(node=torch.arange(kprev, dtype=torch.int32).repeat(B, 1).to(device),
                     parents=torch.zeros(B, kprev, 1, dtype=torch.int64, device=device),
                     parent_lp=(-(5.0 * torch.rand(B, kprev, generator=g)) - 0.1).to(device))
    else:
        assert kprev == 1
    ids, lp, parent, _ = ops.beam_expand(logits, kprev * V, batch=B, child_off=child_off, tok=tok, **beams)
    assert (ids[:, :, -1] >= 0).all(), "every (beam, token) comes back"
    table = torch.empty(B, kprev, V, device=device)
    table[torch.arange(B, device=device).unsqueeze(1), parent.long(), ids[:, :, -1]] = lp
    plp = beams.get("parent_lp")
    if kprev == 1:   # G == 1: the tokens are a permutation of 0..V-1, every candidate continues the one parent
        tokens = torch.stack([torch.randperm(V, generator=g) for _ in range(B)]).to(device)
        # a call takes at most RANK_MAX_K candidates per user: a wider permutation goes in column chunks (views)
        got = torch.cat([ops.score_paths(logits, t, prev_lp=None if plp is None else
                                         plp.expand(B, t.shape[1]).contiguous())[0]
                         for t in tokens.split(ops.RANK_MAX_K, dim=1)], dim=1)
        want = table[:, 0].gather(1, tokens)
    else:            # G == C == kprev: one random token per row
        tokens = torch.randint(0, V, (B, kprev), generator=g).to(device)
        got = ops.score_paths(logits, tokens, prev_lp=plp)[0]
        want = table.gather(2, tokens.unsqueeze(-1)).squeeze(-1)
    assert torch.isfinite(want).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "float bits"


# ------------------------------------------------------------------------------------------ ranks
def _stable_rank(lp, present):
    """CPU: every candidate's place in the stable ordering by (present first, score descending, index ascending)."""
    B, C = lp.shape
    rank = torch.empty(B, C, dtype=torch.int32)
    for b in range(B):
        order = sorted(range(C), key=lambda c: (not bool(present[b, c]), -float(lp[b, c]), c))
        rank[b, torch.tensor(order)] = torch.arange(C, dtype=torch.int32)
    return rank


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 1000, 1024])
@pytest.mark.parametrize("per_cand", [False, True])
def test_score_paths_ranks(device, C, per_cand):
    """Scores on a coarse grid (a 4-class row of equal logits, prev_lp in quarters, duplicated candidates): plenty of
    exact ties, -inf candidates (a -inf prev_lp, a token >= V) and padding."""
    from evaluate.metrics import ranked_candidates
    from rqvae_hip import ops
    B, V, G = 3, 4, C if per_cand else 1
    g = torch.Generator().manual_seed(900 + C + per_cand)
    tokens = torch.randint(0, V, (B, C), generator=g)
    prev = -0.25 * torch.randint(1, 9, (B, C), generator=g).float()
    present = torch.ones(B, C, dtype=torch.bool)
    if C >= 63:
        present[torch.rand(B, C, generator=g) < 1 / 6] = False
        prev[torch.rand(B, C, generator=g) < 0.1] = _NINF
        tokens[torch.rand(B, C, generator=g) < 0.1] = V + 1
        present[:, :2] = True
        present[1, C // 2:] = False                           # a user whose second half is padding
    if C >= 2:
        tokens[:, 1], prev[:, 1] = tokens[:, 0], prev[:, 0]   # a duplicated candidate
    lp, rank = ops.score_paths(torch.zeros(B * G, V, device=device), tokens.to(device), present=present.to(device),
                               prev_lp=prev.to(device), want_rank=True)
    lp, rank_cpu = lp.cpu(), rank.cpu()
    assert rank.dtype == torch.int32 and rank.shape == (B, C)
    assert torch.equal(rank_cpu.sort(1).values, torch.arange(C, dtype=torch.int32).expand(B, C)), "a permutation"
    assert torch.equal(rank_cpu, _stable_rank(lp, present))
    if C >= 2:
        assert torch.equal(lp[:, 0].view(torch.int32), lp[:, 1].view(torch.int32))
        assert (rank_cpu[:, 1] == rank_cpu[:, 0] + 1).all(), "a tie goes to the lower index"
    if C >= 63:
        live = present & torch.isneginf(lp)
        assert live.any() and (~present).any()
        for b in range(B):
            n_pad = int((~present[b]).sum())
            assert (rank_cpu[b][~present[b]] >= C - n_pad).all(), "padding comes last, behind the real -inf candidates"
        assert len(set(lp[present & torch.isfinite(lp)].tolist())) < int(present.sum()) // 2, "many exact ties"
    items = torch.randint(0, 10 ** 6, (B, C), generator=g)
    listed = ranked_candidates(items, rank_cpu)
    assert torch.equal(ranked_candidates(items.to(device), rank).cpu(), listed)
    assert torch.equal(listed.gather(1, rank_cpu.long()), items)


# ------------------------------------------------------------------------------------------ refusals
def test_score_paths_refusals(device):
    from rqvae_hip import ops, RqHipError
    x = torch.zeros(6, 16, device=device)
    t = torch.zeros(2, 3, dtype=torch.int64, device=device)
    ok = dict(present=torch.ones(2, 3, dtype=torch.bool, device=device), prev_lp=torch.zeros(2, 3, device=device))
    lp, rank = ops.score_paths(x, t, **ok, want_rank=True)
    assert lp.shape == rank.shape == (2, 3) and rank.tolist() == [[0, 1, 2]] * 2
    assert ops.score_paths(x[:2], t, **ok)[0].shape == (2, 3)
    with pytest.raises(RqHipError, match="envelope"):   # C = 1025
        ops.score_paths(torch.zeros(1, 16, device=device), torch.zeros(1, 1025, dtype=torch.int64, device=device))
    with pytest.raises(RqHipError, match="envelope"):   # V = 4097
        ops.score_paths(torch.zeros(2, 4097, device=device), t)
    with pytest.raises(RqHipError, match="envelope"):   # 4 rows: G = 2 is neither 1 nor C
        ops.score_paths(x[:4], t)
    with pytest.raises(RqHipError, match="envelope"):   # B mismatch: 5 rows for 2 users
        ops.score_paths(x[:5], t)
    with pytest.raises(RqHipError, match="float32"):
        ops.score_paths(x.double(), t)
    with pytest.raises(RqHipError, match="int64"):
        ops.score_paths(x, t.int())
    with pytest.raises(RqHipError, match="present must be a contiguous torch.bool"):
        ops.score_paths(x, t, present=ok["present"].int())
    with pytest.raises(RqHipError, match="prev_lp must be a contiguous torch.float32"):
        ops.score_paths(x, t, prev_lp=ok["prev_lp"].double())
    with pytest.raises(RqHipError, match="prev_lp must have shape"):
        ops.score_paths(x, t, prev_lp=torch.zeros(3, 3, device=device))
    with pytest.raises(RqHipError, match="present must have shape"):
        ops.score_paths(x, t, present=torch.ones(2, 4, dtype=torch.bool, device=device))
    with pytest.raises(RqHipError, match="non-contiguous last dimension"):
        ops.score_paths(torch.zeros(6, 32, device=device)[:, ::2], t)
    with pytest.raises(RqHipError, match="prev_lp must be a contiguous"):
        ops.score_paths(x, t, prev_lp=torch.zeros(2, 6, device=device)[:, ::2])
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.score_paths(x.cpu(), t)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.score_paths(x, t.cpu())
    with pytest.raises(RqHipError, match="rc=-22.*temperature"):
        ops.score_paths(x, t, temperature=0.0)
    assert ops.score_paths(x[:0], t[:0])[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------ model vs fp64 loop
def _reference_scores(model, batch, sem, present, T=1.0):
    """The teacher-forced walk over the model's own full forwards (beam_support.walk_forwards, tokens clamped into
    [0, V)), fp64 log-softmax and gather on the CPU. sem (B, C, D), present (B, C) on the CPU."""
    B, C, D = sem.shape
    V = model.num_embeddings
    assert D == model.sem_id_dim

    def step(i, logits, lp):
        return (lp + _score_reference(logits, sem[:, :, i], present, None, B, C, V, 1 if i == 0 else C, T)[0],
                sem[:, :, :i + 1].clamp(0, V - 1))
    return bs.walk_forwards(model, batch, C, step, torch.zeros(B, C, dtype=torch.float64))


_SCORE = {}


def _score_case(golden, device, name, C):
    """Candidates of the generation fixture's three users over corpus `name`: the first items of recommend(k=10)
    (all ten for C = 40), a duplicate of the first, -1 padding, an index >= N, an item with a token >= V where the
    corpus holds one, random items. The fp64 reference is computed once and shared."""
    if (name, C) not in _SCORE:
        model, batch, corpus, _ = bs.generation_case(golden, device, name)
        V, n = model.num_embeddings, corpus.ids.shape[0]
        rec = model.recommend(batch, k=10).item_ids.cpu()
        g = torch.Generator().manual_seed(1100 + C + n)
        items = torch.randint(0, n, (3, C), generator=g)
        r = 10 if C >= 14 else 2
        items[:, :r] = rec[:, :r]
        items[:, r] = items[:, 0]
        items[:, r + 1] = -1
        items[:, r + 2] = n + 3
        over = [i for i, row in enumerate(corpus.rows) if max(row) >= V]
        if over:
            items[:, r + 3] = over[0]
        present = (items >= 0) & (items < n)
        sem = torch.where(present.unsqueeze(-1), corpus.ids[items.clamp(0, n - 1)], -1)
        _SCORE[(name, C)] = (model, batch, corpus, items, sem, present, bool(over),
                             _reference_scores(model, batch, sem, present))
    return _SCORE[(name, C)]


def _assert_untouched(model, rng):
    assert torch.equal(torch.cuda.get_rng_state(), rng), "no generator draw"
    assert model.training, "train mode restored"
    assert model.transformer.cached_enc_output is None, "encoder cache cleared"


@pytest.mark.parametrize("incremental", [True, False])
@pytest.mark.parametrize("C", [7, 40])
@pytest.mark.parametrize("name", ["c300", "c5"])
def test_score_items_vs_fp64_loop(golden, device, name, C, incremental):
    from modules.model import Scores
    model, batch, corpus, items, sem, present, over, want = _score_case(golden, device, name, C)
    assert torch.isfinite(want).any() and torch.isneginf(want[~present]).all()
    rng = torch.cuda.get_rng_state()
    got = model.score_items(batch, items.to(device), incremental=incremental)
    _assert_untouched(model, rng)
    assert isinstance(got, Scores) and got.rank.dtype == torch.int32 and got.rank.shape == (3, C)
    _assert_scores(got.log_probas, want, f"{name} C={C} incremental={incremental}:")
    lp, rank = got.log_probas.cpu(), got.rank.cpu()
    assert torch.equal(rank, _stable_rank(lp, present))
    r = 10 if C >= 14 else 2
    assert torch.equal(lp[:, r].view(torch.int32), lp[:, 0].view(torch.int32)), "a duplicated item scores the same"
    if over:
        assert torch.isneginf(lp[:, r + 3]).all(), "an item with a token >= V cannot be generated"
    by_row = model.score_sem_ids(batch, sem.to(device), incremental=incremental)
    _assert_untouched(model, rng)
    assert torch.equal(by_row.log_probas.view(torch.int32), got.log_probas.view(torch.int32))
    assert torch.equal(by_row.rank, got.rank)


@pytest.mark.parametrize("incremental", [True, False])
def test_score_sem_ids_row_outside_the_corpus(golden, device, incremental):
    """A tuple that is no corpus row is scored like any other: nothing depends on the trie."""
    model, batch, corpus, items, sem, present, _, _ = _score_case(golden, device, "c300", 7)
    V = model.num_embeddings
    rows = set(corpus.rows)
    alien = next(t for t in ((a, b, c, d) for a in range(V) for b in range(V) for c in range(V) for d in range(V))
                 if t not in rows)
    sem = sem.clone()
    sem[:, -1] = torch.tensor(alien)
    sem[:, -2] = torch.tensor([0, V, 0, 0])   # a class the model cannot generate
    sem[0, -3] = torch.tensor([1, 2, -5, 0])  # a negative token past the first: present, -inf
    present = sem[:, :, 0] >= 0
    want = _reference_scores(model, batch, sem, present)
    assert torch.isfinite(want[:, -1]).all() and torch.isneginf(want[:, -2]).all() and want[0, -3] == _NINF
    index, model.inference_prefix_index = model.inference_prefix_index, None
    try:
        rng = torch.cuda.get_rng_state()
        got = model.score_sem_ids(batch, sem.to(device), incremental=incremental)
        _assert_untouched(model, rng)
    finally:
        model.inference_prefix_index = index
    _assert_scores(got.log_probas, want, f"alien row incremental={incremental}:")
    assert torch.equal(got.rank.cpu(), _stable_rank(got.log_probas.cpu(), present))


@pytest.mark.parametrize("name", ["golden", "c300", "c5"])
def test_score_items_agrees_with_recommend(golden, device, name):
    """The separation precondition (asserted when the fixture's references are built) makes recommend's order well
    defined: its items come back with its log-probabilities and with the ranks 0..n_live-1 in order."""
    model, batch, corpus, refs = bs.generation_case(golden, device, name)
    want_node = refs[32][2][:, :10]
    rec = model.recommend(batch, k=10)
    got = model.score_items(batch, rec.item_ids)
    live = (rec.item_ids >= 0).cpu()
    assert torch.equal(live, want_node >= 0)
    want = rec.log_probas.cpu().double()
    assert torch.isneginf(want[~live]).all()
    _assert_scores(got.log_probas, want, f"{name}:")
    print(f"{name}: bitwise equal to recommend: "
          f"{torch.equal(got.log_probas.view(torch.int32), rec.log_probas.view(torch.int32))}")
    rank = got.rank.cpu()
    for b in range(3):
        n_live = int(live[b].sum())
        assert rank[b, :n_live].tolist() == list(range(n_live)), "recommend's order"
    full = model.score_items(batch, rec.item_ids, incremental=False)
    _assert_scores(full.log_probas, want, f"{name} full forwards:")
    assert torch.equal(full.rank, got.rank)


def test_score_items_refusals(golden, device):
    model, batch, corpus, _ = bs.generation_case(golden, device, "c5")
    items = torch.zeros(3, 4, dtype=torch.int64, device=device)
    with pytest.raises(ValueError, match="1 <= C <= 1024"):
        model.score_items(batch, torch.zeros(3, 1025, dtype=torch.int64, device=device))
    with pytest.raises(ValueError, match=r"\(B, C\) int64"):
        model.score_items(batch, items.int())
    with pytest.raises(ValueError, match="need 3 users"):
        model.score_items(batch, items[:2])
    with pytest.raises(ValueError, match="need 3 users and 4 tokens"):
        model.score_sem_ids(batch, torch.zeros(3, 4, 3, dtype=torch.int64, device=device))
    with pytest.raises(ValueError, match="must live on"):
        model.score_sem_ids(batch, torch.zeros(3, 4, 4, dtype=torch.int64))
    index = model.inference_prefix_index
    narrow = bs.hand_tokenizer(device, n=5)
    narrow.cached_ids = index.cached_ids[:, :3].contiguous()
    try:
        model.inference_prefix_index = narrow
        with pytest.raises(ValueError, match="the corpus rows hold 3 tokens, the model generates 4"):
            model.score_items(batch, items)
        model.inference_prefix_index = None
        with pytest.raises(ValueError, match="requires inference_prefix_index"):
            model.score_items(batch, items)
    finally:
        model.inference_prefix_index = index
    assert model.training and model.transformer.cached_enc_output is None


# ------------------------------------------------------------------------------------------ evaluator
def test_train_decoder_sampled_negatives(tmp_path, device, capsys, monkeypatch):
    """EVAL_SAMPLED_NEGATIVES = 5 adds the nine neg5_* keys to the full eval's output; everything else — the Hit@k
    values, the trained parameters, torch's global generators after the run — is what the default run gives, and the
    default run's keys are today's (test_exclude_gpu.test_train_decoder_item_metrics' pattern)."""
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
        return model, dict(train_decoder.LAST_RUN["eval"]), (torch.get_rng_state(), torch.cuda.get_rng_state())

    assert train_decoder.EVAL_SAMPLED_NEGATIVES == 0, "off by default"
    capsys.readouterr()
    m_on, ev, rng_on = run(EVAL_SAMPLED_NEGATIVES=5)
    printed = capsys.readouterr().out
    new = [f"neg5_{name}@{k}" for k in (1, 5, 10) for name in ("recall", "ndcg", "mrr")]
    hit = [f"h@{k}_{name}" for i in range(4) for name in (f"slice_:{i + 1}", f"pos_{i}") for k in (1, 5, 10)]
    assert set(ev) == set(new) | set(hit) | {"full_eval_iter"}
    assert all(0.0 <= ev[key] <= 1.0 for key in new) and "'neg5_recall@10'" in printed
    for name in ("recall", "ndcg", "mrr"):
        assert ev[f"neg5_{name}@1"] <= ev[f"neg5_{name}@5"] <= ev[f"neg5_{name}@10"]
    assert ev["neg5_recall@10"] == 1.0, "six candidates: the target always ranks below 10"
    assert m_on.training and not m_on.enable_generation and m_on.transformer.cached_enc_output is None
    m_off, ev_off, rng_off = run()
    assert set(ev_off) == set(hit) | {"full_eval_iter"}, "with the defaults the output keys are today's"
    assert all(ev_off[key] == ev[key] for key in ev_off), "the Hit@k values do not move"
    assert torch.equal(rng_on[0], rng_off[0]) and torch.equal(rng_on[1], rng_off[1]), "global generators untouched"
    on = dict(m_on.named_parameters())
    for n, p in m_off.named_parameters():
        assert torch.equal(p.detach(), on[n].detach()), f"{n}: the sampled-negatives evaluation perturbed training"
