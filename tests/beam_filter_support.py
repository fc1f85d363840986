"""What the catalogue-filter tests share (test_filter_*): the brute-force walk of the corpus rows that the ItemFilter
tables are compared against, a corpus whose level sizes straddle the 32-bit word boundaries, seeded item masks, the
tokenizer over the allowed rows alone (the sub-corpus the filtered search must equal) and one step's inputs restated
for it. CPU tensors throughout; nothing here touches a device at import."""
import torch

import beam_support as bs


# ------------------------------------------------------------------------------------------ the tables, by brute force
def brute_tables(ids, mask):
    """From the rows alone: per group g and level q = 1..D the set of level-q nodes (ranks among the sorted distinct
    length-q prefixes) with an allowed item below them, and per leaf the lowest allowed item (-1: none)."""
    rows = [tuple(r) for r in ids.tolist()]
    D = ids.shape[1]
    index = [{pre: i for i, pre in enumerate(sorted({r[:q] for r in rows}))} for q in range(D + 1)]
    nodes, leaf_item = [], []
    for g in range(mask.shape[0]):
        lvl = [set() for _ in range(D)]
        low = [-1] * len(index[D])
        for i, r in enumerate(rows):
            if not bool(mask[g, i]):
                continue
            for q in range(1, D + 1):
                lvl[q - 1].add(index[q][r[:q]])
            if low[index[D][r]] < 0:
                low[index[D][r]] = i
        nodes.append(lvl)
        leaf_item.append(low)
    return nodes, leaf_item, [len(ix) for ix in index[1:]]


def unpack(bits, n):
    """(G, n) bool from a (G, ceil(n / 32)) int32 bitmap; the padding bits of the last word must be clear."""
    words = bits.cpu().long() & 0xFFFFFFFF
    flat = ((words.unsqueeze(-1) >> torch.arange(32)) & 1).bool().reshape(bits.shape[0], -1)
    assert bits.dtype == torch.int32 and bits.shape[1] == (n + 31) // 32 and not flat[:, n:].any()
    return flat[:, :n]


def assert_tables(filt, ids, mask):
    """An ItemFilter against the brute-force walk; returns the unpacked per-level bool tables."""
    nodes, leaf_item, sizes = brute_tables(ids, mask)
    G = mask.shape[0]
    assert filt.groups == G and len(filt.bits) == ids.shape[1]
    assert filt.leaf_item.dtype == torch.int64 and filt.leaf_item.cpu().tolist() == leaf_item
    out = []
    for q, n_q in enumerate(sizes):
        got = unpack(filt.bits[q], n_q)
        for g in range(G):
            assert set(got[g].nonzero().flatten().tolist()) == nodes[g][q], f"group {g}, level {q + 1}"
        out.append(got)
    return out


def same_filter(a, b):
    return (a.groups == b.groups and len(a.bits) == len(b.bits) and
            all(x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()) for x, y in zip(a.bits, b.bits)) and
            a.leaf_item.dtype == b.leaf_item.dtype and torch.equal(a.leaf_item.cpu(), b.leaf_item.cpu()))


# ------------------------------------------------------------------------------------------ corpora and masks
def straddle_corpus():
    """72 rows of 4 tokens in [0, 32) whose levels hold exactly 32, 33, 65 and 70 nodes: nodes 31, 32, 63 and 64 sit on
    both sides of the bitmap's word boundaries. Rows 70 and 71 repeat rows 3 and 69."""
    rows = []
    for t in range(32):
        for u in ((0, 1) if t == 0 else (0,)):               # level 2: 33 nodes
            for w in ((0,) if t == 31 else (0, 1)):            # level 3: 2 * 32 + 1 = 65 nodes
                rows.append((t, u, w, 0))
    rows += [(t, 0, 0, 1) for t in range(5)]                   # level 4: 70 leaves
    ids = torch.tensor(rows + [rows[3], rows[69]])
    assert [len({tuple(r[:q]) for r in ids.tolist()}) for q in (1, 2, 3, 4)] == [32, 33, 65, 70]
    return ids


def corpus_ids(name):
    return {"five": bs.FIVE, "random": bs.random_corpus(), "straddle": straddle_corpus()}[name]


def seeded_masks(n, G, seed, density=(0.5, 0.2, 0.8)):
    """(G, n) bool: group g allows about density[g % 3] of the items."""
    g = torch.Generator().manual_seed(seed)
    p = torch.tensor([density[i % len(density)] for i in range(G)]).unsqueeze(1)
    return torch.rand(G, n, generator=g) < p


def row_masks(corpus, excluded):
    """(B, N) bool: user b may be shown every item whose row is not the row of an item on excluded[b] — the complement
    of an exclusion list, which works by row."""
    out = torch.ones(len(excluded), len(corpus.rows), dtype=torch.bool)
    for b, items in enumerate(excluded):
        gone = {corpus.rows[i] for i in items}
        out[b] = torch.tensor([r not in gone for r in corpus.rows])
    return out


# ------------------------------------------------------------------------------------------ the sub-corpus
def sub_tokenizer(tok, allowed, device):
    """(the tokenizer over the rows of `tok` that the (N,) bool `allowed` keeps, their corpus indices, its Corpus)."""
    kept = allowed.nonzero().flatten()
    ids = tok.cached_ids.cpu()[kept].clone()
    return bs.ids_tokenizer(ids.to(device), codebook_size=tok.codebook_size), kept, bs.Corpus(ids)


def sub_case(c, corpus, sub, b, kprev, P):
    """User b's slice of the step inputs c (bs.draw_beams over `corpus`) as a batch of one over the sub-corpus `sub`:
    the same logits, parents and parent scores, every beam's node looked up by its prefix in the sub-corpus — a beam
    whose prefix has no allowed row is dead there, as it has no candidate in the filtered search."""
    out = dict(logits=c["logits"][b * kprev:(b + 1) * kprev], node=None, parents=None, parent_lp=None)
    if P:
        out["parents"] = c["parents"][b:b + 1]
        out["parent_lp"] = c["parent_lp"][b:b + 1]
        out["node"] = torch.tensor([[sub.index[P].get(tuple(p), -1) if n >= 0 else -1
                                     for p, n in zip(c["parents"][b].tolist(), c["node"][b].tolist())]],
                                   dtype=torch.int32)
    return out


def assert_nodes(corpus, ids, node, what=""):
    """out_node by its path: every live row's node is the full trie's node of the row's ids, dead rows carry -1."""
    ids, node = ids.cpu(), node.cpu()
    depth = ids.shape[-1]
    for b in range(ids.shape[0]):
        for r in range(ids.shape[1]):
            path = tuple(ids[b, r].tolist())
            want = -1 if path[-1] < 0 else corpus.index[depth][path]
            assert int(node[b, r]) == want, f"{what}out_node[{b}][{r}]"


def bits_of(x):
    x = x.cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def assert_bitwise(got, want, names, what=""):
    for g, w, name in zip(got, want, names):
        if name is None:
            continue
        g, w = g.cpu(), w.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}{name}"
        assert torch.equal(bits_of(g), bits_of(w)), f"{what}{name}"
