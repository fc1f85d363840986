"""What the score-bias tests share (test_bias_*): the brute-force walk of the corpus rows that the ItemBias tables are
compared against, seeded bias tables (one with every awkward value), the fp64 biased beam step with its seeded,
separated cases, and the bitwise comparisons. CPU tensors throughout; nothing here touches a device at import."""
import math

import torch

import beam_support as bs

NINF = -float("inf")


# ------------------------------------------------------------------------------------------ the tables, by brute force
def clean(x):
    """A bias value as the kernels and the CPU tables read it: NaN and +inf are -inf, -0.0 is +0.0."""
    x = float(x)
    if math.isnan(x) or x == float("inf"):
        return NINF
    return 0.0 if x == 0.0 else x


def brute_tables(corpus, bias):
    """From the rows alone (a beam_support.Corpus): per group g and level q = 1..D every level-q node's bound — the
    max cleaned bias of the items below it, -inf with none — as fp32 tensors (G, n_q), and per leaf the lowest index
    among the items that attain the leaf's max (-1 at -inf), int64 (G, n_leaves)."""
    D = corpus.ids.shape[1]
    G = bias.shape[0]
    upper = [torch.full((G, len(corpus.index[q])), NINF) for q in range(1, D + 1)]
    leaf_item = torch.full((G, len(corpus.index[D])), -1, dtype=torch.int64)
    for g in range(G):
        vals = [clean(x) for x in bias[g].tolist()]
        for i, r in enumerate(corpus.rows):
            for q in range(1, D + 1):
                at = corpus.index[q][r[:q]]
                if vals[i] > float(upper[q - 1][g, at]):
                    upper[q - 1][g, at] = vals[i]
        for i, r in enumerate(corpus.rows):
            leaf = corpus.index[D][r]
            if vals[i] > NINF and vals[i] == float(upper[D - 1][g, leaf]) and int(leaf_item[g, leaf]) < 0:
                leaf_item[g, leaf] = i
    return upper, leaf_item


def bits_of(x):
    x = x.cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def assert_tables(got, want_upper, want_leaf_item, what=""):
    """An ItemBias against (upper, leaf_item), bit for bit."""
    assert got.groups == want_leaf_item.shape[0] and len(got.upper) == len(want_upper), what
    for q, (g, w) in enumerate(zip(got.upper, want_upper)):
        assert g.dtype == torch.float32 and g.shape == w.shape, f"{what}upper[{q}]"
        assert torch.equal(bits_of(g), bits_of(w)), f"{what}upper[{q}]"
    assert got.leaf_item.dtype == torch.int64 and torch.equal(got.leaf_item.cpu(), want_leaf_item), f"{what}leaf_item"


def awkward_bias(ids, seed=17):
    """(3, N) fp32 over the rows `ids`: row 0 2 randn with NaN, +inf, -0.0 and -inf planted, and every copy of a row
    that several items share given one bias value above its neighbours except the lowest copy (so the leaf's item is the
    max-bias one, then the lowest index: not simply the lowest); row 1 all -inf; row 2 2 randn with about 30 % -inf."""
    N = ids.shape[0]
    g = torch.Generator().manual_seed(seed)
    bias = 2.0 * torch.randn(3, N, generator=g)
    rows = {}
    for i, r in enumerate(ids.tolist()):
        rows.setdefault(tuple(r), []).append(i)
    for copies in rows.values():
        if len(copies) > 1:
            bias[0, copies[0]] = 1.0
            bias[0, copies[1:]] = 7.5   # two of a triple tie at the max: the lower of them is the leaf's item
    bias[0, 0], bias[0, 1 % N], bias[0, 2 % N], bias[0, 4 % N] = float("nan"), float("inf"), -0.0, NINF
    bias[1] = NINF
    bias[2][torch.rand(N, generator=g) < 0.3] = NINF
    return bias


TABLE_CORPORA = ("c300", "c5", "random")


def table_ids(name):
    """(N, 4) ids of a table test's corpus (CPU): the kernel tests' c300 and c5, random_corpus() with its triple row."""
    return bs.random_corpus() if name == "random" else bs.tokenizer(name, "cpu")[0].cached_ids.clone()


# ------------------------------------------------------------------------------------------ the fp64 biased step
def step_bias(corpus, seed):
    """(3, N) fp32 item bias of the kernel cases: 2 randn; 2 randn with about 30 % -inf; all zero."""
    N = corpus.ids.shape[0]
    g = torch.Generator().manual_seed(seed)
    bias = 2.0 * torch.randn(3, N, generator=g)
    bias[1][torch.rand(N, generator=g) < 0.3] = NINF
    bias[2] = 0.0
    return bias


_STEP_TABLES = {}


def step_tables(name, corpus):
    """The step_bias rows of corpus `name` as brute-force level tables, [q - 1] (3, n_q) fp32; built once."""
    if name not in _STEP_TABLES:
        _STEP_TABLES[name] = brute_tables(corpus, step_bias(corpus, 77))[0]
    return _STEP_TABLES[name]


def biased_reference(corpus, lp, prefixes, live, parent_lp, groups, table, B, kprev, V, P, k, blocked=None):
    """expand_reference with a bias: per batch element every (live beam j, valid child token v < V, node c not in
    blocked[b]) with, for a biased user (groups[b] in [0, G)), U = clean(table[g][c]) > -inf; lp_c = lp[b kprev + j][v]
    + parent_lp[b][j] and s_c = lp_c + U in fp64 (s_c = lp_c for an unbiased user); stable descending sort by s_c in
    (beam, token) order, the k best; dead rows (-1, -inf, -inf, parent 0, node -1) pad. table: the level-(P + 1) bounds
    (G, n_{P + 1}). Returns ids (B, k, P + 1), lp (B, k) fp64, scores (B, k) fp64, parent, node, and every user's
    sorted scores."""
    G = table.shape[0]
    tab = table.double().tolist()
    ids = torch.full((B, k, P + 1), -1, dtype=torch.int64)
    out_lp = torch.full((B, k), NINF, dtype=torch.float64)
    out_s = torch.full((B, k), NINF, dtype=torch.float64)
    parent = torch.zeros((B, k), dtype=torch.int64)
    node = torch.full((B, k), -1, dtype=torch.int64)
    all_scores = []
    for b in range(B):
        g = int(groups[b])
        biased = 0 <= g < G
        cands = []
        for j in range(kprev):
            if not live[b][j]:
                continue
            pre = tuple(prefixes[b][j]) if P else ()
            for v in corpus.children[P].get(pre, ()):
                if v >= V:
                    continue
                c = corpus.index[P + 1][pre + (v,)]
                if blocked is not None and c in blocked[b]:
                    continue
                u = clean(tab[g][c]) if biased else 0.0
                if u == NINF:
                    continue
                l = float(lp[b * kprev + j, v]) + (float(parent_lp[b][j]) if P else 0.0)
                cands.append((l + u if biased else l, l, j, v, pre, c))
        cands.sort(key=lambda t: -t[0])   # stable: equal scores stay in (beam, token) order
        all_scores.append([t[0] for t in cands])
        for r, (s, l, j, v, pre, c) in enumerate(cands[:k]):
            ids[b, r] = torch.tensor(pre + (v,))
            out_lp[b, r], out_s[b, r], parent[b, r], node[b, r] = l, s, j, c
    return ids, out_lp, out_s, parent, node, all_scores


_CASES = {}


def case(name, B, kprev, V, P, k, T=1.0):
    """Seeded inputs of one biased kernel case and their fp64 reference, built once (CPU): beam_support.draw_beams, the
    three step_bias rows as brute-force level tables, groups drawn from {-1, 0, 1, 2}; a user whose top k + 1 BIASED
    scores are not separated has its logits redrawn from the same stream. `redraws` counts them."""
    key = (name, B, kprev, V, P, k, T)
    if key in _CASES:
        return _CASES[key]
    _, corpus = bs.tokenizer(name, "cpu")
    g = torch.Generator().manual_seed(9000 + 97 * B + 31 * kprev + 7 * V + 3 * P + k + int(10 * T))
    c = bs.draw_beams(corpus, g, B, kprev, V, P)
    groups = torch.randint(-1, 3, (B,), generator=g).to(torch.int32)
    table = step_tables(name, corpus)[P]
    logits = c["logits"]
    pre = c["parents"].tolist() if P else None
    live = (c["node"] >= 0).tolist() if P else [[True] * kprev] * B
    redraws = 0
    for _ in range(200):
        ref = biased_reference(corpus, bs.log_softmax64(logits, T), pre, live, c["parent_lp"], groups, table, B, kprev,
                               V, P, k)
        bad = [b for b in range(B) if not bs.separated(ref[5][b], k)]
        if not bad:
            break
        redraws += len(bad)
        for b in bad:
            logits[b * kprev:(b + 1) * kprev] = 2.0 * torch.randn(kprev, V, generator=g)
    assert all(bs.separated(s, k) for s in ref[5]), "precondition: separated biased scores"
    _CASES[key] = dict(c, groups=groups, table=table, ref=ref, corpus=corpus, live=live, pre=pre, redraws=redraws)
    return _CASES[key]


def expand(device, tok, c, B, k, P, T=1.0, table=None, groups=None, **kw):
    """ops.beam_expand_biased over tok's trie level P on the CPU tensors of case c (its table and groups by default)."""
    from rqvae_hip import ops
    trie = tok.prefix_trie()
    table = c["table"] if table is None else table
    groups = c["groups"] if groups is None else groups
    return ops.beam_expand_biased(c["logits"].to(device), k, batch=B, child_off=trie.child_off[P], tok=trie.tok[P + 1],
                                  bias=table.to(device).contiguous(), bias_group=groups.to(device),
                                  node=bs.dev(c["node"], device), parents=bs.dev(c["parents"], device),
                                  parent_lp=bs.dev(c["parent_lp"], device), temperature=T, **kw)


NAMES = ("out_ids", "out_lp", "out_score", "out_parent", "out_node")


def assert_same(got, want, what=""):
    """The five outputs bit for bit."""
    for g, w, name in zip(got, want, NAMES):
        g, w = g.cpu(), w.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}{name}"
        assert torch.equal(bits_of(g), bits_of(w)), f"{what}{name}"
