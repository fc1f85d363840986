"""Stochastic beam search on the device: rq_beam_expand_sampled against the fp64 reference step (picks exact, phi and
G within tolerance, dead rows, blocked children, underflow), its invariants, its distribution over 8192 users, and
sample_items against a loop of the model's own forwards with the fp64 step — exhaustion, exclusion, generators."""
import pytest
import torch

import beam_sampled_support as ss
import beam_support as bs

pytestmark = pytest.mark.gpu


def _check_against_reference(device, case_args, block=False):
    name, B, kprev, V, P, k, T = case_args
    c = ss.case(device, name, B, kprev, V, P, k, T, block)
    ref = c["ref"]
    ids, phi, g, parent, node = ss.expand(device, c, B, k, P, T)
    assert ids.shape == (B, k, P + 1) and ids.dtype == torch.int64
    assert phi.shape == g.shape == (B, k) and phi.dtype == g.dtype == torch.float32
    assert parent.shape == node.shape == (B, k) and parent.dtype == node.dtype == torch.int32
    assert torch.equal(ids, c["ref_ids"]), "out_ids"
    assert torch.equal(parent.long(), ref["parent"]), "out_parent"
    assert torch.equal(node.long(), c["ref_node"]), "out_node"
    err_phi, err_g = ss.max_error(phi, ref["phi"]), ss.max_error(g, ref["g"])
    print(f"{name} B={B} kprev={kprev} V={V} P={P} k={k} T={T} blocked={block}: live rows {ref['live'].sum(1).tolist()}, "
          f"max |phi err| {err_phi[0]:.3e} ({err_phi[1]:.3f} of the tolerance), max |G err| {err_g[0]:.3e} "
          f"({err_g[1]:.3f}), max |G| {float(ref['g'][ref['live']].abs().max()):.2f}")
    assert err_phi[1] <= 1 and err_g[1] <= 1
    bs.assert_dead_rows(ids, phi, parent, node)
    assert torch.isneginf(g[node < 0]).all()
    # invariants, on the same outputs
    assert not torch.isnan(phi).any() and not torch.isnan(g).any()
    assert (g[:, :-1] >= g[:, 1:]).all(), "out_g is non-increasing"
    live = node >= 0
    has = c["valid"].any(-1)   # the beams with a candidate
    if P:
        pg, pphi = c["parent_g"].gather(1, parent.long()), c["parent_phi"].gather(1, parent.long())
        assert (g <= pg)[live].all(), "never above the parent's perturbed score"
        assert (phi <= pphi + 1e-6)[live].all()
        best = torch.where(has, c["parent_g"], -float("inf")).max(1).values
    else:
        assert (g <= 0)[live].all() and (phi <= 1e-6)[live].all()
        best = torch.zeros(B)
    assert has.any(1).all() and torch.equal(g[:, 0], best), "the best beam hands its perturbed score to its best child"
    return c, (ids, phi, g, parent, node)


@pytest.mark.parametrize("case_args", ss.CASES, ids=lambda a: "-".join(map(str, a)))
def test_beam_expand_sampled_vs_fp64(device, case_args):
    c, _ = _check_against_reference(device, case_args)
    name, B, kprev, V, P, k, T = case_args
    if name == "c300" and P == 3:
        assert (~c["ref"]["live"]).any(), "precondition: dead rows appear"
        assert any(v >= V for kids in c["corpus"].children[3].values() for v in kids), "dedup tokens >= V exist"


def test_beam_expand_sampled_blocked_vs_fp64(device):
    name, B, kprev, V, P, k, T = ss.BLOCKED_CASE
    c, (ids, *_) = _check_against_reference(device, ss.BLOCKED_CASE, block=True)
    open_ref = ss.case(device, name, B, kprev, V, P, k, T)
    assert c["valid"].sum() < open_ref["valid"].sum(), "the filter removed candidates"
    for b in range(B):
        gone = {c["corpus"].rows[i][:P + 1] for i in c["excluded"][b]}
        assert not any(tuple(r) in gone for r in ids[b].tolist()), "no blocked child is returned"


def test_beam_expand_sampled_underflow_ranks_above_dead_rows(device):
    from rqvae_hip import ops
    tok, corpus = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    # the root's children are 0 and 3; the row's mass sits on class 5, 200 above them: p == 0 in fp32
    x = torch.full((1, 16), -200.0, device=device)
    x[0, 5] = 0.0
    noise = torch.empty(1, 16).exponential_(generator=torch.Generator().manual_seed(5)).to(device)
    ids, phi, g, parent, node = (t.cpu() for t in ops.beam_expand_sampled(
        x, 4, batch=1, child_off=trie.child_off[0], tok=trie.tok[1], noise=noise))
    assert ids[0].tolist() == [[0], [3], [-1], [-1]], "-inf candidates in token order, then the dead rows"
    assert node[0].tolist() == [corpus.index[1][(0,)], corpus.index[1][(3,)], -1, -1] and parent[0].tolist() == [0] * 4
    assert torch.isneginf(phi).all() and torch.isneginf(g).all()
    bs.assert_dead_rows(ids, phi, parent, node)
    # one such beam beside a healthy one: its children come after the healthy beam's, before the dead rows
    n0, n3 = corpus.index[1][(0,)], corpus.index[1][(3,)]
    x = torch.zeros(2, 16, device=device)
    x[0] = -200.0
    x[0, 7] = 0.0
    noise = torch.empty(2, 16).exponential_(generator=torch.Generator().manual_seed(6)).to(device)
    ids, phi, g, parent, node = (t.cpu() for t in ops.beam_expand_sampled(
        x, 6, batch=1, child_off=trie.child_off[1], tok=trie.tok[2], noise=noise,
        node=torch.tensor([[n3, n0]], dtype=torch.int32, device=device), parents=torch.tensor([[[3], [0]]], device=device),
        parent_phi=torch.tensor([[-0.5, -1.0]], device=device), parent_g=torch.tensor([[-0.25, -2.0]], device=device)))
    assert ids[0].tolist() == [[0, 2], [3, 0], [3, 1], [-1, -1], [-1, -1], [-1, -1]]
    assert phi[0, 0] == -1.0 and g[0, 0] == -2.0, "an only child keeps its parent's phi and G exactly"
    assert torch.isneginf(phi[0, 1:]).all() and torch.isneginf(g[0, 1:]).all() and node[0, 1] >= 0 and node[0, 2] >= 0
    bs.assert_dead_rows(ids, phi, parent, node)


def test_beam_expand_sampled_refuses_bad_arguments(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    x = torch.zeros(4, 16, device=device)
    e = torch.ones(4, 16, device=device)
    lvl0 = dict(child_off=trie.child_off[0], tok=trie.tok[1])
    lvl1 = dict(child_off=trie.child_off[1], tok=trie.tok[2])
    beams = dict(node=torch.zeros(2, 2, dtype=torch.int32, device=device),
                 parents=torch.zeros(2, 2, 1, dtype=torch.int64, device=device),
                 parent_phi=torch.zeros(2, 2, device=device), parent_g=torch.zeros(2, 2, device=device))
    assert ops.beam_expand_sampled(x, 3, batch=2, noise=e, **lvl1, **beams)[0].shape == (2, 3, 2)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand_sampled(x, 3, batch=4, noise=e.cpu(), **lvl0)
    with pytest.raises(RqHipError, match="noise must be a contiguous torch.float32"):
        ops.beam_expand_sampled(x, 3, batch=4, noise=e.double(), **lvl0)
    with pytest.raises(RqHipError, match="noise must have shape"):
        ops.beam_expand_sampled(x, 3, batch=4, noise=e[:, :8].contiguous(), **lvl0)
    with pytest.raises(RqHipError, match=r"\(B \* kprev, V\)"):
        ops.beam_expand_sampled(x, 3, batch=3, noise=e, **lvl0)
    with pytest.raises(RqHipError, match="go together"):
        ops.beam_expand_sampled(x, 3, batch=2, noise=e, **lvl1, **{**beams, "parent_g": None})
    with pytest.raises(RqHipError, match="go together"):
        ops.beam_expand_sampled(x, 3, batch=2, noise=e, **lvl1, node=beams["node"])
    with pytest.raises(RqHipError, match="parent_g must have shape"):
        ops.beam_expand_sampled(x, 3, batch=2, noise=e, **lvl1, **{**beams, "parent_g": torch.zeros(2, 3, device=device)})
    with pytest.raises(RqHipError, match="parent_phi must be a contiguous torch.float32"):
        ops.beam_expand_sampled(x, 3, batch=2, noise=e, **lvl1, **{**beams, "parent_phi": beams["parent_phi"].double()})
    with pytest.raises(RqHipError, match="envelope.*no wide form"):
        ops.beam_expand_sampled(torch.zeros(40, 256, device=device), 3, batch=1, noise=torch.ones(40, 256, device=device),
                                **lvl0)        # kprev V > 8192
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand_sampled(x, 0, batch=4, noise=e, **lvl0)
    with pytest.raises(RqHipError, match="rc=-22.*temperature"):
        ops.beam_expand_sampled(x, 3, batch=4, noise=e, **lvl0, temperature=0.0)
    assert ops.beam_expand_sampled(x[:0], 3, batch=0, noise=e[:0], **lvl0)[0].shape == (0, 3, 1)


# ------------------------------------------------------------------------------------------ the distribution
def test_beam_expand_sampled_distribution(device):
    """The host recipe through two launches: the kernel's picks are the fp64 reference's for every user that meets the
    separation rule, and its own picks pass both chi-square bounds."""
    from rqvae_hip import ops
    r = ss.recipe()
    B, k, V = r["B"], r["k"], r["V"]
    failing = float((~r["ok"]).double().mean())
    assert failing <= 0.01, "precondition: at most 1 % of the users fail the separation rule"
    trie = bs.ids_tokenizer(ss.ROWS.to(device), codebook_size=V).prefix_trie()
    ids0, phi0, g0, _, node0 = ops.beam_expand_sampled(r["logits0"].to(device), k, batch=B, child_off=trie.child_off[0],
                                                       tok=trie.tok[1], noise=r["e0"].to(device))
    logits1 = r["l1"].float().to(device)[ids0[:, :, 0]].reshape(B * k, V).contiguous()
    ids1, phi1, g1, _, node1 = ops.beam_expand_sampled(logits1, k, batch=B, child_off=trie.child_off[1], tok=trie.tok[2],
                                                       noise=r["e1"].reshape(B * k, V).to(device), node=node0,
                                                       parents=ids0, parent_phi=phi0, parent_g=g0)
    picks = ids1.cpu()
    ok = r["ok"]
    assert (node1.cpu() >= 0).all() and torch.equal(picks[ok], r["picks"][ok]), "the reference's picks"
    err_phi, err_g = ss.max_error(phi1.cpu()[ok], r["s1"]["phi"][ok]), ss.max_error(g1.cpu()[ok], r["s1"]["g"][ok])
    chi_first, chi_pair, _ = ss.chi_squares(picks, r["p"])
    print(f"users failing the rule {100 * failing:.3f} %, users whose picks differ "
          f"{int((picks != r['picks']).any(-1).any(-1).sum())}; chi-square first {chi_first:.2f}, pairs {chi_pair:.2f}; "
          f"max |phi err| {err_phi[0]:.3e}, max |G err| {err_g[0]:.3e}")
    assert err_phi[1] <= 1 and err_g[1] <= 1
    assert (g1[:, 0] == 0).all(), "the root's perturbed score reaches every user's first row"
    assert chi_first < ss.CHI2_FIRST
    assert chi_pair < ss.CHI2_PAIR


# ------------------------------------------------------------------------------------------ the model
def _reference_sample(model, batch, corpus, k, seed, T=1.0):
    """sample_items as a loop of the model's own forwards with the fp64 step; the noise comes from a device generator
    seeded like the call's, drawn in the documented order and shapes. Returns the last step's result, the rows
    (B, k, L1), the leaf nodes and the users that met the separation rule at every step."""
    B, V = batch.sem_ids.shape[0], model.num_embeddings
    dev = batch.sem_ids.device
    gen = torch.Generator(device=dev).manual_seed(seed)

    def step(i, logits, state):
        kprev = 1 if i == 0 else k
        noise = torch.empty(logits.shape, device=dev, dtype=torch.float32).exponential_(generator=gen).cpu()
        res, ids, _, ok = state or (None, None, None, torch.ones(B, dtype=torch.bool))
        prefixes = None if i == 0 else ids.tolist()
        live = [[True]] * B if i == 0 else res["live"].tolist()
        valid = ss.valid_mask(corpus, prefixes, live, B, kprev, V, i)
        res = ss.step64(logits, noise, valid, None if i == 0 else res["phi"], None if i == 0 else res["g"], T, k)
        ids, node = ss.assemble(corpus, prefixes, res, i)
        return (res, ids, node, ok & ss.separated(res["top"])), ids.clamp_min(0)
    return bs.walk_forwards(model, batch, k, step)


@pytest.mark.parametrize("incremental", [True, False])
def test_sample_items_vs_fp64_loop(golden, device, incremental):
    from modules.model import SampledItems
    model, batch, corpus, _ = bs.generation_case(golden, device, "golden")
    B, k, seed = batch.sem_ids.shape[0], 8, 77
    res, want_ids, want_node, ok = _reference_sample(model, batch, corpus, k, seed)
    assert ok.sum() * 10 >= 9 * B, "precondition: at most 1 user in 10 fails the separation rule"
    got = model.sample_items(batch, k=k, incremental=incremental, generator=torch.Generator(device=device).manual_seed(seed))
    assert isinstance(got, SampledItems) and model.training and model.transformer.cached_enc_output is None
    assert got.item_ids.shape == (B, k) and got.item_ids.dtype == torch.int64 and got.sem_ids.shape == (B, k, 4)
    assert got.log_probas.shape == got.perturbed.shape == (B, k) and got.log_probas.dtype == torch.float32
    items, ids, phi, g = got.item_ids.cpu(), got.sem_ids.cpu(), got.log_probas.cpu(), got.perturbed.cpu()
    assert torch.equal(ids[ok], want_ids[ok]), "the reference's rows"
    live = (ids >= 0).all(-1)
    assert torch.equal(live, (ids >= 0).any(-1)) and torch.equal(live[ok], res["live"][ok])
    err_phi, err_g = ss.max_error(phi[ok], res["phi"][ok]), ss.max_error(g[ok], res["g"][ok])
    print(f"incremental={incremental}: users compared {int(ok.sum())} of {B}, live rows {live.sum(1).tolist()}, "
          f"max |phi err| {err_phi[0]:.3e} ({err_phi[1]:.3f} of the tolerance), max |G err| {err_g[0]:.3e} ({err_g[1]:.3f})")
    assert err_phi[1] <= 1 and err_g[1] <= 1
    assert (g[:, 0] == 0).all(), "perturbed[:, 0] is exactly 0"
    assert (g[:, :-1] >= g[:, 1:]).all(), "rows in perturbed order"
    rows = set(corpus.rows)
    for b in range(B):
        mine = [tuple(r) for r in ids[b][live[b]].tolist()]
        assert all(r in rows for r in mine), "every live row is a corpus row"
        assert len(set(mine)) == len(mine), "rows are distinct"
        assert items[b][live[b]].tolist() == [corpus.first_row[r] for r in mine], "item_ids are the rows' leaf items"
    assert (items[~live] == -1).all() and torch.isneginf(phi[~live]).all() and torch.isneginf(g[~live]).all()


def test_sample_items_exhausts_a_small_corpus(golden, device):
    model, batch, corpus, _ = bs.generation_case(golden, device, "c5")
    B = batch.sem_ids.shape[0]
    got = model.sample_items(batch, k=8, generator=torch.Generator(device=device).manual_seed(3))
    ids, items = got.sem_ids.cpu(), got.item_ids.cpu()
    distinct = sorted(set(corpus.rows))
    assert len(distinct) == 4
    for b in range(B):
        assert sorted(tuple(r) for r in ids[b, :4].tolist()) == distinct, "each distinct row exactly once"
        assert sorted(items[b, :4].tolist()) == sorted(corpus.first_row[r] for r in distinct)
    assert (ids[:, 4:] == -1).all() and (items[:, 4:] == -1).all()
    assert torch.isneginf(got.log_probas.cpu()[:, 4:]).all() and torch.isneginf(got.perturbed.cpu()[:, 4:]).all()
    assert torch.isfinite(got.log_probas.cpu()[:, :4]).all()
    # the four probabilities of the renormalised distribution sum to 1
    assert torch.allclose(got.log_probas[:, :4].double().exp().sum(1).cpu(), torch.ones(B, dtype=torch.float64), atol=1e-5)


def test_sample_items_exclusion(golden, device):
    model, batch, corpus, _ = bs.generation_case(golden, device, "c300")
    first = model.sample_items(batch, k=6, generator=torch.Generator(device=device).manual_seed(11))
    assert (first.item_ids >= 0).all()
    second = model.sample_items(batch, k=6, exclude_items=first.item_ids,
                                generator=torch.Generator(device=device).manual_seed(11))
    assert (second.item_ids >= 0).all()
    for b in range(batch.sem_ids.shape[0]):
        gone = {tuple(r) for r in first.sem_ids[b].tolist()}
        assert not gone & {tuple(r) for r in second.sem_ids[b].tolist()}, "no excluded row (or duplicate of one) returns"
        assert not set(first.item_ids[b].tolist()) & set(second.item_ids[b].tolist())
    with pytest.raises(ValueError, match=r"exclude_items must be \(B, H\)"):
        model.sample_items(batch, k=6, exclude_items=first.item_ids[:1])


def test_sample_items_generators(golden, device):
    model, batch, _, _ = bs.generation_case(golden, device, "golden")
    params = [p.detach().clone() for p in model.parameters()]
    rng = torch.cuda.get_rng_state()
    a = model.sample_items(batch, k=8, generator=torch.Generator(device=device).manual_seed(5))
    b = model.sample_items(batch, k=8, generator=torch.Generator(device=device).manual_seed(5))
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                  y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert torch.equal(torch.cuda.get_rng_state(), rng), "a given generator leaves the default one alone"
    c = model.sample_items(batch, k=8, generator=torch.Generator(device=device).manual_seed(6))
    assert not torch.equal(c.sem_ids, a.sem_ids), "another seed, another draw"
    model.sample_items(batch, k=8)
    assert not torch.equal(torch.cuda.get_rng_state(), rng), "generator=None draws from the default generator"
    assert model.training and model.transformer.cached_enc_output is None
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params)), "parameters untouched"
