"""Constrained beam decoding on the device: rq_beam_expand (one trie-walking launch per beam step) against an fp64
reference that enumerates the valid continuations from the corpus rows themselves, against the existing
beam_candidates + beam_select kernels, its tie / underflow / bad-table behaviour and argument refusals; then
generate_next_sem_id(constrained=True), recommend() and the Hit@k counters over beams with dead rows."""
import numpy as np
import pytest
import torch

import beam_support as bs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ kernel vs references
@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_beam_expand_vs_fp64(device, name, B, kprev, V, P, k, T):
    c = bs.case(device, name, B, kprev, V, P, k, T)
    want_ids, want_lp, want_parent, want_node, scores = c["ref"]
    if name == "c300" and P == 3:
        corpus = bs.tokenizer(name, device)[1]
        assert any(v >= V for kids in corpus.children[3].values() for v in kids), "dedup tokens >= V exist"
        assert any(len(s) < k for s in scores), "dead rows appear"
    ids, lp, parent, node = (t.cpu() for t in bs.expand(device, c["tok"], c, B, k, P, T))
    assert ids.shape == (B, k, P + 1) and ids.dtype == torch.int64 and lp.shape == (B, k) and lp.dtype == torch.float32
    assert parent.shape == node.shape == (B, k) and parent.dtype == node.dtype == torch.int32
    print(f"{name} B={B} kprev={kprev} V={V} P={P} k={k} T={T}: candidates per user {[len(s) for s in scores]}, "
          f"max rel lp err {float(((lp.double() - want_lp).abs() / want_lp.abs())[want_node >= 0].max()):.3e}")
    assert torch.equal(ids, want_ids), "out_ids"
    assert torch.equal(parent.long(), want_parent), "out_parent"
    assert torch.equal(node.long(), want_node), "out_node"
    np.testing.assert_allclose(lp.double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    bs.assert_dead_rows(ids, lp, parent, node)


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_beam_expand_vs_candidates_and_select(device, name, B, kprev, V, P, k, T):
    """beam_candidates over every class followed by beam_select's table search keeps the same valid candidates:
    equal ids and parents and bitwise equal log-probabilities on the rows that hold a valid candidate (all k of them
    where at least k exist; select fills the others with rejected candidates, expand with dead rows)."""
    from rqvae_hip import ops
    c = bs.case(device, name, B, kprev, V, P, k, T)
    n_valid = [min(k, len(s)) for s in c["ref"][4]]
    if (name, P) in (("c300", 0), ("c300", 1), ("c3000", 0), ("c3000", 1)):
        assert all(n == k for n in n_valid), "at least k valid candidates"
    ids, lp, parent, _ = bs.expand(device, c["tok"], c, B, k, P, T)
    keys, base = c["tok"].prefix_table(P + 1)
    cand_ids, cand_lp = ops.beam_candidates(c["logits"].to(device), V, T)
    s_ids, s_lp, s_parent = ops.beam_select(cand_ids, cand_lp, k, batch=B, keys=keys, base=base,
                                            parents=bs.dev(c["parents"], device),
                                            parent_lp=bs.dev(c["parent_lp"], device), return_parent=True)
    for b, n in enumerate(n_valid):
        assert torch.equal(ids[b, :n], s_ids[b, :n]) and torch.equal(parent[b, :n], s_parent[b, :n]), b
        assert torch.equal(lp[b, :n].view(torch.int32), s_lp[b, :n].view(torch.int32)), "out_lp bitwise"


# ------------------------------------------------------------------------------------------ ties, edge values
def test_beam_expand_ties_underflow_and_dead_rows(device):
    from rqvae_hip import ops
    tok, corpus = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    n3 = corpus.index[1][(3,)]
    # two beams on node (3,) with identical logits and equal parent_lp: children 0 and 1 of each, in (beam, token)
    # order; 4 candidates for k = 6
    node = torch.tensor([[n3, n3]], dtype=torch.int32, device=device)
    parents = torch.tensor([[[3], [3]]], device=device)
    plp = torch.full((1, 2), -0.5, device=device)
    ids, lp, parent, out_node = (t.cpu() for t in ops.beam_expand(
        torch.zeros(2, 16, device=device), 6, batch=1, child_off=trie.child_off[1], tok=trie.tok[2], node=node,
        parents=parents, parent_lp=plp))
    assert ids[0].tolist() == [[3, 0], [3, 1], [3, 0], [3, 1], [-1, -1], [-1, -1]]
    assert parent[0].tolist() == [0, 0, 1, 1, 0, 0]
    kids = [corpus.index[2][(3, 0)], corpus.index[2][(3, 1)]]
    assert out_node[0].tolist() == kids + kids + [-1, -1]
    np.testing.assert_allclose(lp[0, :4].numpy(), -0.5 - np.log(16.0), rtol=1e-6, atol=0)
    assert (lp[0, :4] == lp[0, 0]).all() and torch.isneginf(lp[0, 4:]).all()
    # an underflowing child (p == 0 in fp32) is kept with -inf: below every finite candidate, above the dead rows
    x = torch.full((1, 16), -200.0, device=device)
    x[0, 3] = 0.0
    ids, lp, parent, out_node = (t.cpu() for t in ops.beam_expand(x, 4, batch=1, child_off=trie.child_off[0],
                                                                   tok=trie.tok[1]))
    assert ids[0].tolist() == [[3], [0], [-1], [-1]]
    assert out_node[0].tolist() == [corpus.index[1][(3,)], corpus.index[1][(0,)], -1, -1] and parent[0].tolist() == [0] * 4
    assert lp[0, 0] == 0 and torch.isneginf(lp[0, 1:]).all()
    bs.assert_dead_rows(ids, lp, parent, out_node)


def test_beam_expand_bad_tables_stay_in_bounds(device):
    """Out-of-range node / child_off entries and tokens >= V or < 0 give no candidates (the result for a bad table is
    otherwise unspecified; every index the kernel forms from these values stays inside the buffers)."""
    from rqvae_hip import ops
    V, k = 8, 6
    tok = torch.tensor([0, 5, 40, 2, 7, -3], dtype=torch.int32, device=device)
    child_off = torch.tensor([-4, 3, 99, 4], dtype=torch.int32, device=device)   # node 0: [0, 3), 1: [3, 6), 2: [6, 4)
    node = torch.tensor([[0, 1, 2, 3, -1, 7]], dtype=torch.int32, device=device)
    g = torch.Generator().manual_seed(11)
    logits = 2.0 * torch.randn(6, V, generator=g)
    parents = torch.arange(6).reshape(1, 6, 1)
    plp = -torch.rand(1, 6, generator=g)
    ids, lp, parent, out_node = (t.cpu() for t in ops.beam_expand(
        logits.to(device), k, batch=1, child_off=child_off, tok=tok, node=node, parents=parents.to(device),
        parent_lp=plp.to(device)))
    lp64 = bs.log_softmax64(logits, 1.0)
    want = sorted([(float(lp64[j, v]) + float(plp[0, j]), j, v, c) for j, v, c in ((0, 0, 0), (0, 5, 1), (1, 2, 3), (1, 7, 4))],
                  key=lambda c: -c[0])
    assert ids[0, :4].tolist() == [[j, v] for _, j, v, _ in want]
    assert parent[0, :4].tolist() == [j for _, j, _, _ in want] and out_node[0, :4].tolist() == [c for *_, c in want]
    np.testing.assert_allclose(lp[0, :4].double().numpy(), [s for s, *_ in want], rtol=1e-5, atol=0)
    assert (ids[0, 4:] == -1).all() and torch.isneginf(lp[0, 4:]).all() and out_node[0, 4:].tolist() == [-1, -1]


def test_beam_expand_refuses_bad_arguments(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    x = torch.zeros(4, 16, device=device)
    lvl0 = dict(child_off=trie.child_off[0], tok=trie.tok[1])
    lvl1 = dict(child_off=trie.child_off[1], tok=trie.tok[2])
    beams = dict(node=torch.zeros(2, 2, dtype=torch.int32, device=device),
                 parents=torch.zeros(2, 2, 1, dtype=torch.int64, device=device), parent_lp=torch.zeros(2, 2, device=device))
    assert ops.beam_expand(x, 3, batch=2, **lvl1, **beams)[0].shape == (2, 3, 2)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand(x.cpu(), 3, batch=4, **lvl0)
    with pytest.raises(RqHipError, match="float32"):
        ops.beam_expand(x.double(), 3, batch=4, **lvl0)
    with pytest.raises(RqHipError, match=r"\(B \* kprev, V\)"):
        ops.beam_expand(x, 3, batch=3, **lvl0)
    with pytest.raises(RqHipError, match="go together"):
        ops.beam_expand(x, 3, batch=2, **lvl1, node=beams["node"])
    with pytest.raises(RqHipError, match="node must be a contiguous torch.int32"):
        ops.beam_expand(x, 3, batch=2, **lvl1, **{**beams, "node": beams["node"].long()})
    with pytest.raises(RqHipError, match="parent_lp must have shape"):
        ops.beam_expand(x, 3, batch=2, **lvl1, **{**beams, "parent_lp": torch.zeros(2, 3, device=device)})
    with pytest.raises(RqHipError, match="child_off must be a contiguous torch.int32"):
        ops.beam_expand(x, 3, batch=4, child_off=trie.child_off[0].long(), tok=trie.tok[1])
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand(torch.zeros(1, 5000, device=device), 3, batch=1, **lvl0)        # V > 4096
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand(torch.zeros(40, 256, device=device), 3, batch=1, **lvl0)        # kprev V > 8192
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand(x, 0, batch=4, **lvl0)
    with pytest.raises(RqHipError, match="rc=-22.*temperature"):
        ops.beam_expand(x, 3, batch=4, **lvl0, temperature=0.0)
    # the envelope's corner runs: V = 4096 with kprev = 2, and more beams asked for than candidates exist
    ids = ops.beam_expand(torch.zeros(2, 4096, device=device), 5, batch=1, **lvl1, node=beams["node"][:1],
                          parents=torch.full((1, 2, 1), 3, device=device), parent_lp=beams["parent_lp"][:1])[0]
    assert ids.shape == (1, 5, 2)
    assert ops.beam_expand(x[:0], 3, batch=0, **lvl0)[0].shape == (0, 3, 1)


# ------------------------------------------------------------------------------------------ generation
@pytest.mark.parametrize("name", ["golden", "c300"])
def test_constrained_generation_vs_fp64_loop(golden, device, name):
    model, batch, corpus, refs = bs.generation_case(golden, device, name)
    want_ids, want_lp, want_node = refs[32]
    assert (want_node >= 0).any()
    rng = torch.cuda.get_rng_state()
    kw = dict(temperature=1, top_k=True, fused=True, sample=False, constrained=True)
    got = model.generate_next_sem_id(batch, **kw)
    assert model.training, "train mode restored"
    assert model.transformer.cached_enc_output is None, "encoder cache cleared"
    assert torch.equal(torch.cuda.get_rng_state(), rng), "no generator draw"
    assert got.sem_ids.shape == (3, 32, 4) and got.log_probas.shape == (3, 32)
    assert torch.equal(got.sem_ids.cpu(), want_ids), "beams"
    np.testing.assert_allclose(got.log_probas.cpu().double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    again = model.generate_next_sem_id(batch, **kw)
    assert torch.equal(again.sem_ids, got.sem_ids)
    assert torch.equal(again.log_probas.view(torch.int32), got.log_probas.view(torch.int32)), "two calls bitwise equal"
    inc = model.generate_next_sem_id(batch, incremental=True, **kw)
    assert model.training and model.transformer.cached_enc_output is None
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    assert torch.equal(inc.sem_ids.cpu(), want_ids), "incremental beams"
    np.testing.assert_allclose(inc.log_probas.cpu().double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    rows = set(corpus.rows)
    dead = (got.sem_ids.cpu() == -1).all(-1)
    assert torch.equal(dead, want_node < 0) and torch.isneginf(got.log_probas.cpu()[dead]).all()
    assert all(tuple(r) in rows for r in got.sem_ids.cpu()[~dead].tolist()), "every live beam is a corpus row"


@pytest.mark.parametrize("incremental", [False, True])
def test_constrained_generation_greedy(golden, device, incremental):
    model, batch, corpus, refs = bs.generation_case(golden, device, "golden")
    want_ids, want_lp, _ = refs[1]
    got = model.generate_next_sem_id(batch, temperature=1, top_k=False, fused=True, sample=False, constrained=True,
                                     incremental=incremental)
    assert got.sem_ids.shape == (3, 4) and got.log_probas.shape == (3,)
    assert torch.equal(got.sem_ids.cpu(), want_ids[:, 0]), "the greedy valid path"
    np.testing.assert_allclose(got.log_probas.cpu().double().numpy(), want_lp[:, 0].numpy(), rtol=1e-5, atol=0)
    assert all(tuple(r) in set(corpus.rows) for r in got.sem_ids.cpu().tolist())


@pytest.mark.parametrize("name", ["golden", "c300", "c5"])
def test_recommend(golden, device, name):
    from modules.model import Recommendation
    model, batch, corpus, refs = bs.generation_case(golden, device, name)
    want_ids, want_lp, want_node = refs[32]
    rec = model.recommend(batch)
    assert isinstance(rec, Recommendation) and model.training and model.transformer.cached_enc_output is None
    assert rec.item_ids.shape == (3, 10) and rec.item_ids.dtype == torch.int64
    assert rec.sem_ids.shape == (3, 10, 4) and rec.log_probas.shape == (3, 10)
    assert torch.equal(rec.sem_ids.cpu(), want_ids[:, :10]), "the first 10 of the 32 beams"
    np.testing.assert_allclose(rec.log_probas.cpu().double().numpy(), want_lp[:, :10].numpy(), rtol=1e-5, atol=0)
    items, live = rec.item_ids.cpu(), want_node[:, :10] >= 0
    if name == "c5":
        assert (~live).any() and live.any(), "the 4 distinct rows leave dead beams"
    assert (items[~live] == -1).all() and (items[live] >= 0).all()
    assert torch.equal(corpus.ids[items[live]], rec.sem_ids.cpu()[live]), "cached_ids[item_ids] == sem_ids"
    assert items[live].tolist() == [corpus.first_row[tuple(r)] for r in rec.sem_ids.cpu()[live].tolist()], "lowest index"
    full = model.recommend(batch, k=32, incremental=False)
    assert torch.equal(full.sem_ids.cpu(), want_ids) and torch.equal(full.item_ids[:, :10], rec.item_ids)


# ------------------------------------------------------------------------------------------ Hit@k with dead rows
def test_topk_accumulator_counts_dead_rows_like_cpu(device):
    """Beams that end in dead rows (four steps of beam_expand over the 5-row corpus, k = 6 > its 4 distinct items):
    the device counters equal the CPU accumulator's, and a -1 row never matches a target."""
    from evaluate.metrics import TopKAccumulator
    from rqvae_hip import ops
    tok, corpus = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    B, k, V = 4, 6, 12
    g = torch.Generator().manual_seed(21)
    ids = lp = node = None
    for i in range(4):
        logits = 2.0 * torch.randn(B * (1 if i == 0 else k), V, generator=g)
        ids, lp, _, node = ops.beam_expand(logits.to(device), k, batch=B, child_off=trie.child_off[i], tok=trie.tok[i + 1],
                                           node=node, parents=ids, parent_lp=lp)
    beams = ids.cpu()
    assert (beams[:, :4] >= 0).all() and (beams[:, 4:] == -1).all(), "4 live beams and 2 dead rows per user"
    actual = torch.stack([beams[0, 0], beams[1, 2], torch.tensor([3, 1, 9, 0]), beams[3, 3]])
    ks = [1, 3, 6]
    cpu, gpu = TopKAccumulator(ks=ks), TopKAccumulator(ks=ks)
    cpu.accumulate(actual=actual, top_k=beams)
    gpu.accumulate(actual=actual.to(device), top_k=ids)
    assert torch.equal(gpu.counts.cpu(), cpu.counts) and gpu.reduce() == cpu.reduce()
    assert gpu.reduce()["h@6_slice_:4"] == 3 / 4 and gpu.reduce()["h@1_slice_:4"] == 1 / 4
