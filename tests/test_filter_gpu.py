"""Catalogue filters on the device: the expand entry points' allowed / group arguments (narrow, wide, sampled) against
the unfiltered kernels on the trie of the allowed rows alone — the sub-corpus the filtered search must equal, bit for bit — the group
rules, the equivalence with seen-item exclusion, the device table build against the CPU tables, and an fp64 cross-check."""
import numpy as np
import pytest
import torch

import beam_filter_support as fs
import beam_support as bs

pytestmark = pytest.mark.gpu

# corpus, B, kprev, V, P, k: bs.SHAPES' small cases
SMALL = [("c300", 2, 1, 12, 0, 5), ("c300", 3, 4, 12, 1, 8), ("c300", 3, 4, 12, 3, 8), ("c5", 2, 1, 37, 0, 8),
         ("c5", 2, 3, 37, 2, 8), ("c300", 2, 6, 12, 1, 8)]
WIDE = ("c3000", 2, 40, 256, 1, 40)   # kprev V > 8192: only the wide kernel takes it
KINDS = ["narrow", "wide", "sampled"]
NAMES = {"narrow": ("out_ids", "out_lp", "out_parent", None), "wide": ("out_ids", "out_lp", "out_parent", None),
         "sampled": ("out_ids", "out_phi", "out_g", "out_parent", None)}   # None: out_node, checked by its path


def _inputs(corpus, B, kprev, V, P, seed):
    """bs.wide_inputs plus what the sampled step reads: noise, and parent_g below parent_phi (= parent_lp)."""
    c = bs.wide_inputs(corpus, B, kprev, V, P, seed)
    g = torch.Generator().manual_seed(seed + 1)
    c["noise"] = torch.empty(B * kprev, V).exponential_(generator=g)
    c["parent_g"] = None
    if P:
        c["parent_g"] = torch.sort(c["parent_lp"] - torch.empty(B, kprev).exponential_(generator=g), dim=1,
                                   descending=True).values
    return c


def _run(device, kind, tok, c, B, k, P, T=1.0, **filt):
    from rqvae_hip import ops
    trie = tok.prefix_trie()
    common = dict(batch=B, child_off=trie.child_off[P], tok=trie.tok[P + 1], node=bs.dev(c["node"], device),
                  parents=bs.dev(c["parents"], device), temperature=T, **filt)
    if kind == "sampled":
        return ops.beam_expand_sampled(c["logits"].to(device), k, noise=c["noise"].to(device),
                                       parent_phi=bs.dev(c["parent_lp"], device),
                                       parent_g=bs.dev(c["parent_g"], device), **common)
    return ops.beam_expand(c["logits"].to(device), k, parent_lp=bs.dev(c["parent_lp"], device), wide=kind == "wide",
                           **common)


def _sub_run(device, kind, tok, corpus, c, allowed, B, kprev, k, P, T=1.0, excluded=None):
    """The existing kernel, user by user, on the trie of the rows each user's (N,) mask allowed[b] keeps; excluded:
    per user the items (full-corpus indices) of an exclusion list, handed over as the sub-corpus' blocked nodes."""
    outs = []
    for b in range(B):
        sub_tok, kept, sub = fs.sub_tokenizer(tok, allowed[b], device)
        sc = fs.sub_case(c, corpus, sub, b, kprev, P)
        sc["noise"] = c["noise"][b * kprev:(b + 1) * kprev]
        sc["parent_g"] = c["parent_g"][b:b + 1] if P else None
        filt = {}
        if excluded is not None:
            where = {int(i): at for at, i in enumerate(kept.tolist())}
            mine = [where[i] for i in excluded[b] if i in where]
            filt["blocked"] = sub_tok.blocked_nodes(bs.pad([mine]).to(device))[P].contiguous()
        outs.append(_run(device, kind, sub_tok, sc, 1, k, P, T, **filt))
    return tuple(torch.cat([o[i] for o in outs]) for i in range(len(outs[0])))


def _masks(corpus, G, seed):
    mask = fs.seeded_masks(len(corpus.rows), G, seed)
    mask[torch.arange(G), torch.arange(G) % len(corpus.rows)] = True   # no empty group here
    return mask


def _group(device, values):
    return torch.tensor(values, dtype=torch.int32, device=device)


def _check(got, want, corpus, kind, what):
    fs.assert_bitwise(got, want, NAMES[kind], what)
    fs.assert_nodes(corpus, got[0], got[-1], what)
    ids, node, parent = got[0].cpu(), got[-1].cpu(), got[-2].cpu()
    bs.assert_dead_rows(ids, got[1].cpu(), parent, node)


# ------------------------------------------------------------------------------------------ sub-corpus equality
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case_args", SMALL, ids=lambda a: "-".join(map(str, a)))
def test_filtered_step_equals_the_sub_corpus_step(device, case_args, kind):
    name, B, kprev, V, P, k = case_args
    tok, corpus = bs.tokenizer(name, device)
    c = _inputs(corpus, B, kprev, V, P, seed=100 + 7 * P + kprev)
    mask = _masks(corpus, B, seed=200 + P)
    filt = tok.item_filter(mask.to(device))
    for T in (1.0, 0.7):
        got = _run(device, kind, tok, c, B, k, P, T, allowed=filt.bits[P], group=_group(device, range(B)))
        want = _sub_run(device, kind, tok, corpus, c, mask, B, kprev, k, P, T)
        _check(got, want, corpus, kind, f"{case_args} {kind} T={T}: ")
    assert (got[-1] >= 0).any(), "precondition: the case has live rows"


def test_filtered_wide_step_40_beams(device):
    name, B, kprev, V, P, k = WIDE
    tok, corpus = bs.tokenizer(name, device)
    c = _inputs(corpus, B, kprev, V, P, seed=321)
    mask = _masks(corpus, B, seed=322)
    filt = tok.item_filter(mask.to(device))
    from rqvae_hip import ops, RqHipError
    got = _run(device, "wide", tok, c, B, k, P, allowed=filt.bits[P], group=_group(device, range(B)))
    want = _sub_run(device, "wide", tok, corpus, c, mask, B, kprev, k, P)
    _check(got, want, corpus, "wide", "wide 40: ")
    assert (got[-1] >= 0).all(), "precondition: 40 live rows per user"
    trie = tok.prefix_trie()
    args = dict(batch=B, child_off=trie.child_off[P], tok=trie.tok[P + 1], node=c["node"].to(device),
                parents=c["parents"].to(device), parent_lp=c["parent_lp"].to(device), allowed=filt.bits[P],
                group=_group(device, range(B)))
    auto = ops.beam_expand(c["logits"].to(device), k, wide=None, **args)   # what the model's search passes
    fs.assert_bitwise(auto, got, ("out_ids", "out_lp", "out_parent", "out_node"), "wide=None: ")
    with pytest.raises(RqHipError, match="outside the supported envelope"):
        ops.beam_expand(c["logits"].to(device), k, **args)


# ------------------------------------------------------------------------------------------ groups
@pytest.mark.parametrize("kind", KINDS)
def test_groups_and_unfiltered_users(device, kind):
    """G = 3 with group = [0, 2, -1]: users 0 and 1 read rows 0 and 2, user 2 is unfiltered; a group past the table
    (3) is unfiltered too."""
    name, B, kprev, V, P, k = "c300", 3, 4, 12, 1, 8
    tok, corpus = bs.tokenizer(name, device)
    c = _inputs(corpus, B, kprev, V, P, seed=41)
    mask = _masks(corpus, 3, seed=42)
    mask[1] = False
    filt = tok.item_filter(mask.to(device))
    plain = _run(device, kind, tok, c, B, k, P)
    everyone = torch.ones(len(corpus.rows), dtype=torch.bool)
    want = _sub_run(device, kind, tok, corpus, c, [mask[0], mask[2], everyone], B, kprev, k, P)
    for last in (-1, 3):
        got = _run(device, kind, tok, c, B, k, P, allowed=filt.bits[P], group=_group(device, [0, 2, last]))
        _check(got, want, corpus, kind, f"{kind} groups: ")
        for g, p in zip(got, plain):   # every output of the unfiltered user, out_node included
            assert torch.equal(fs.bits_of(g[2]), fs.bits_of(p[2])), "group outside [0, G): the unfiltered kernel"
    got = _run(device, kind, tok, c, B, k, P, allowed=filt.bits[P], group=_group(device, [1, 1, 1]))
    assert (got[0] == -1).all() and (got[-1] == -1).all() and (got[-2] == 0).all(), "nothing allowed: dead rows only"
    assert all(torch.isneginf(t).all() for t in got[1:-2])
    # an empty bitmap (n_words = 0) allows nothing and is never read
    empty = torch.zeros((3, 0), dtype=torch.int32, device=device)
    got = _run(device, kind, tok, c, B, k, P, allowed=empty, group=_group(device, [0, 2, -1]))
    assert (got[-1][:2] == -1).all()
    for g, p in zip(got, plain):
        assert torch.equal(fs.bits_of(g[2]), fs.bits_of(p[2]))
    # a bitmap cut short: the words past n_words read as "not allowed"
    n_words = filt.bits[P].shape[1]
    assert n_words >= 2
    cut = filt.bits[P][:, :1].contiguous()
    got = _run(device, kind, tok, c, B, k, P, allowed=cut, group=_group(device, [0, 2, -1]))
    low = mask.clone()
    anc = tok.trie_index().leaf_anc[P].cpu()[tok.trie_index().item_leaf.cpu().long()]
    low[:, anc >= 32] = False
    want = _sub_run(device, kind, tok, corpus, c, [low[0], low[2], everyone], B, kprev, k, P)
    _check(got, want, corpus, kind, f"{kind} short bitmap: ")


@pytest.mark.parametrize("kind", KINDS)
def test_one_item_group_returns_that_item(device, kind):
    """The last level, every user its own one-item group: that item's leaf, then dead rows."""
    name, B, kprev, V, P, k = "c300", 3, 4, 12, 3, 8
    tok, corpus = bs.tokenizer(name, device)
    c = _inputs(corpus, B, kprev, V, P, seed=51)
    items = []
    for b in range(B):   # the last item under user b's beam 0 (always live) whose row the model can name
        under = [i for i in bs.items_under(corpus, c["parents"][b, 0].tolist()) if corpus.rows[i][-1] < V]
        items.append(under[-1])
    mask = torch.zeros(B, len(corpus.rows), dtype=torch.bool)
    mask[torch.arange(B), torch.tensor(items)] = True
    filt = tok.item_filter(mask.to(device))
    got = _run(device, kind, tok, c, B, k, P, allowed=filt.bits[P], group=_group(device, range(B)))
    ids, node = got[0].cpu(), got[-1].cpu().long()
    for b in range(B):   # once per live beam on the item's prefix (user 0 has two on one node), then dead rows
        n = sum(nd >= 0 and p == c["parents"][b, 0].tolist()
                for p, nd in zip(c["parents"][b].tolist(), c["node"][b].tolist()))
        assert n == (2 if b == 0 else 1), "precondition"
        for r in range(n):
            assert tuple(ids[b, r].tolist()) == corpus.rows[items[b]]
            assert int(filt.leaf_item[b, node[b, r]]) == items[b]
        assert (node[b, n:] == -1).all() and (ids[b, n:] == -1).all()
    bs.assert_dead_rows(ids, got[1].cpu(), got[-2].cpu(), got[-1].cpu())
    want = _sub_run(device, kind, tok, corpus, c, mask, B, kprev, k, P)
    _check(got, want, corpus, kind, f"{kind} one item: ")


# ------------------------------------------------------------------------------------------ exclusion equivalence
def _excluded(corpus, c, B, V, P):
    """Per user the items under the first candidate of its beam 0: a whole level-(P + 1) subtree."""
    out = []
    for b in range(B):
        pre = tuple(c["parents"][b, 0].tolist()) if P else ()
        first = next(v for v in corpus.children[P][pre] if v < V)
        out.append(bs.items_under(corpus, pre + (first,)))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case_args", [("c300", 3, 4, 12, 1, 8), ("c5", 2, 3, 37, 2, 8), ("c300", 2, 1, 12, 0, 5)],
                         ids=lambda a: "-".join(map(str, a)))
def test_complement_of_an_exclusion_list(device, case_args, kind):
    """Per-user groups whose masks are the complement of an exclusion list (by row, as exclusion works) against the
    blocked argument on that list: every output bit for bit, out_node too. Both filters together: the sub-corpus
    with the union removed — exact here because the list is a whole subtree of the level the step selects from, so no
    node of that level has its allowed rows all excluded while other rows keep it unblocked."""
    name, B, kprev, V, P, k = case_args
    tok, corpus = bs.tokenizer(name, device)
    c = _inputs(corpus, B, kprev, V, P, seed=61 + P)
    excluded = _excluded(corpus, c, B, V, P)
    rows_left = fs.row_masks(corpus, excluded)
    blocked = tok.blocked_nodes(bs.pad(excluded).to(device))[P].contiguous()
    assert (blocked != bs.NONE).any(1).all(), "precondition: every user blocks a node"
    want = _run(device, kind, tok, c, B, k, P, blocked=blocked)
    filt = tok.item_filter(rows_left.to(device))
    got = _run(device, kind, tok, c, B, k, P, allowed=filt.bits[P], group=_group(device, range(B)))
    fs.assert_bitwise(got, want, [n or "out_node" for n in NAMES[kind]], f"{case_args} {kind} complement: ")
    mask =_masks(corpus, B, seed=71 + P)
    both = tok.item_filter(mask.to(device))
    got = _run(device, kind, tok, c, B, k, P, blocked=blocked, allowed=both.bits[P], group=_group(device, range(B)))
    want = _sub_run(device, kind, tok, corpus, c, mask & rows_left, B, kprev, k, P)
    _check(got, want, corpus, kind, f"{case_args} {kind} both: ")
    want = _sub_run(device, kind, tok, corpus, c, mask, B, kprev, k, P, excluded=excluded)
    _check(got, want, corpus, kind, f"{case_args} {kind} both, the sub-corpus' own blocked nodes: ")


# ------------------------------------------------------------------------------------------ table build
@pytest.mark.parametrize("name", ["five", "random", "straddle"])
def test_device_tables_equal_the_cpu_tables(device, name):
    ids = fs.corpus_ids(name)
    n = ids.shape[0]
    cpu_tok = bs.ids_tokenizer(ids.clone(), codebook_size=int(ids.max()) + 1)
    dev_tok = bs.ids_tokenizer(ids.clone().to(device), codebook_size=int(ids.max()) + 1)
    mask = fs.seeded_masks(n, 7, seed=13)
    mask[3] = False
    mask[4] = True
    if name == "straddle":
        mask[5] = ids[:, 0] == 31
        mask[6] = ~mask[5]
    want = cpu_tok.item_filter(mask)
    fs.assert_tables(want, ids, mask)
    got = dev_tok.item_filter(mask.to(device))
    assert got.leaf_item.device.type == "cuda" and all(b.device.type == "cuda" for b in got.bits)
    assert fs.same_filter(got, want)
    assert fs.same_filter(dev_tok.item_filter(mask.to(device)), got), "two runs, one result"
    one = dev_tok.item_filter(mask[1].to(device))
    assert one.groups == 1 and fs.same_filter(one, cpu_tok.item_filter(mask[1]))
    # a mask that does not start on a 4-byte boundary takes the byte loads
    odd = torch.zeros(7 * n + 1, dtype=torch.bool, device=device)
    odd[1:] = mask.flatten().to(device)
    assert fs.same_filter(dev_tok.item_filter(odd[1:].view(7, n)), want)


def test_table_build_refusals(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = bs.tokenizer("c5", device)
    idx = tok.trie_index()
    sizes = [c.numel() for c in idx.leaf_count]
    ok = torch.ones(2, 5, dtype=torch.bool, device=device)
    with pytest.raises(RqHipError, match="mask must be"):
        ops.trie_allowed_nodes(ok[0], idx.item_leaf, idx.leaf_anc, sizes)
    with pytest.raises(RqHipError, match="mask must be a contiguous torch.bool"):
        ops.trie_allowed_nodes(ok.int(), idx.item_leaf, idx.leaf_anc, sizes)
    with pytest.raises(RqHipError, match="item_leaf must have shape"):
        ops.trie_allowed_nodes(ok[:, :4].contiguous(), idx.item_leaf, idx.leaf_anc, sizes)
    with pytest.raises(RqHipError, match="D level sizes"):
        ops.trie_allowed_nodes(ok, idx.item_leaf, idx.leaf_anc, sizes[:2])
    trie = tok.prefix_trie()
    args = dict(batch=2, child_off=trie.child_off[0], tok=trie.tok[1])
    logits = torch.zeros(2, 37, device=device)
    bits = tok.item_filter(ok).bits[0]
    group = torch.zeros(2, dtype=torch.int32, device=device)
    for fn, extra in ((ops.beam_expand, {}), (ops.beam_expand_sampled, dict(noise=torch.ones(2, 37, device=device)))):
        with pytest.raises(RqHipError, match="allowed and group go together"):
            fn(logits, 4, allowed=bits, **args, **extra)
        with pytest.raises(RqHipError, match="allowed and group go together"):
            fn(logits, 4, group=group, **args, **extra)
        with pytest.raises(RqHipError, match="group must be a contiguous torch.int32"):
            fn(logits, 4, allowed=bits, group=group.long(), **args, **extra)
        with pytest.raises(RqHipError, match="group must have shape"):
            fn(logits, 4, allowed=bits, group=group[:1], **args, **extra)
        with pytest.raises(RqHipError, match="allowed must be"):
            fn(logits, 4, allowed=bits[0], group=group, **args, **extra)
        with pytest.raises(RqHipError, match="allowed must be a contiguous torch.int32"):
            fn(logits, 4, allowed=bits.long(), group=group, **args, **extra)


# ------------------------------------------------------------------------------------------ fp64 cross-check
def _separated_case(corpus, sub, B, kprev, V, P, k, T):
    """The first seed whose users all meet bs.separated on the sub-corpus, with its fp64 reference."""
    for seed in range(500, 540):
        c = _inputs(corpus, B, kprev, V, P, seed)
        pre = c["parents"].tolist() if P else None
        live = (c["node"] >= 0).tolist() if P else [[True] * kprev] * B
        ref = bs.expand_reference(sub, bs.log_softmax64(c["logits"], T), pre, live, c["parent_lp"], B, kprev, V, P, k)
        if all(bs.separated(s, k) for s in ref[4]):
            return c, ref
    return None, None


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("case_args", SMALL, ids=lambda a: "-".join(map(str, a)))
def test_filtered_step_vs_fp64(device, case_args, wide):
    name, B, kprev, V, P, k = case_args
    tok, corpus = bs.tokenizer(name, device)
    mask = _masks(corpus, 1, seed=81 + P)
    _, _, sub = fs.sub_tokenizer(tok, mask[0], "cpu")
    c, ref = _separated_case(corpus, sub, B, kprev, V, P, k, 1.0)
    assert c is not None, "no seed with separated scores: a skipped case is a failure"
    filt = tok.item_filter(mask.to(device))
    ids, lp, parent, node = _run(device, "wide" if wide else "narrow", tok, c, B, k, P, allowed=filt.bits[P],
                                 group=_group(device, [0] * B))
    want_ids, want_lp, want_parent = ref[:3]
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(parent.cpu().long(), want_parent)
    fs.assert_nodes(corpus, ids, node)
    fin = torch.isfinite(want_lp)
    assert torch.equal(torch.isneginf(lp.cpu()), ~fin)
    np.testing.assert_allclose(lp.cpu().double()[fin].numpy(), want_lp[fin].numpy(), rtol=1e-5, atol=0)
