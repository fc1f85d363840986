"""What the stochastic-beam-search tests share (test_beam_sampled_*): the fp64 reference step (the arithmetic of
rq_beam_expand_sampled, vectorised in torch), candidate masks and blocked children from the corpus rows, seeded kernel
cases, the separation rule, and the two-step sampler recipe with its chi-square figures. CPU tensors throughout;
nothing here touches a device at import."""
import torch

import beam_support as bs

FLT_MIN = float(torch.finfo(torch.float32).tiny)
SEP = 1e-4            # a user's top k + 1 fp64 perturbed scores must be this far apart for its picks to be compared
ATOL = RTOL = 1e-5    # phi and G against fp64 (test_beam_expand_gpu.py's tolerance; the measured maximum is in DESIGN)
NEG = -float("inf")


# ------------------------------------------------------------------------------------------ the fp64 step
def step64(logits, noise, valid, phi, g, T, k):
    """One stochastic-beam-search step in float64. logits / noise (B * kprev, V) fp32, valid (B, kprev, V) bool (the
    candidates: children of a live beam with a token < V, not blocked), phi / g (B, kprev) or None (0). Returns a dict:
    parent (B, k) and token (B, k) int64 (dead rows: 0 and -1), phi and g (B, k) float64 (dead rows -inf), live (B, k)
    bool, top (B, min(k + 1, kprev V)) the users' best perturbed scores in order (absent: -inf)."""
    B, kprev, V = valid.shape
    l = bs.log_softmax64(logits, T).view(B, kprev, V)                                            # 1
    zero = torch.zeros(B, kprev, dtype=torch.float64)
    phi_j = (zero if phi is None else phi.double()).unsqueeze(-1)
    g_j = (zero if g is None else g.double()).unsqueeze(-1)
    lm = torch.where(valid, l, NEG)
    lmax = lm.max(-1, keepdim=True).values
    safe = torch.where(torch.isneginf(lmax), 0.0, lmax)
    lam = lmax + torch.log(torch.exp(lm - safe).sum(-1, keepdim=True))                           # 2 (-inf: no mass)
    degenerate = torch.isneginf(l) | torch.isneginf(lam) | torch.isneginf(phi_j) | torch.isneginf(g_j)
    phi_c = torch.where(valid & ~degenerate, phi_j + (l - lam), NEG)                             # 3
    e = noise.double().view(B, kprev, V)
    e = torch.where((e > 0) & torch.isfinite(e), e, FLT_MIN)
    gt = phi_c - torch.log(e)                                                                    # 4
    z = gt.max(-1, keepdim=True).values                                                          # 5
    v = g_j - gt + torch.log1p(-torch.exp(gt - z))                                               # 6
    g_c = g_j - v.clamp_min(0) - torch.log1p(torch.exp(-v.abs()))                                # 7
    g_c = torch.where(torch.isneginf(phi_c), NEG, g_c).reshape(B, kprev * V)
    assert not torch.isnan(g_c).any()
    # larger G, then lower beam, then lower token; absent entries after every candidate
    absent = ~valid.reshape(B, kprev * V)
    first = torch.sort(g_c, dim=1, descending=True, stable=True).indices
    order = first.gather(1, torch.sort(absent.gather(1, first).int(), dim=1, stable=True).indices)
    n = min(k, kprev * V)
    sel = order[:, :n]
    live = torch.zeros(B, k, dtype=torch.bool)
    live[:, :n] = ~absent.gather(1, sel)
    parent = torch.zeros(B, k, dtype=torch.int64)
    token = torch.full((B, k), -1, dtype=torch.int64)
    out_phi = torch.full((B, k), NEG, dtype=torch.float64)
    out_g = torch.full((B, k), NEG, dtype=torch.float64)
    parent[:, :n] = sel // V
    token[:, :n] = sel % V
    out_phi[:, :n] = phi_c.reshape(B, kprev * V).gather(1, sel)
    out_g[:, :n] = g_c.gather(1, sel)
    parent[~live], token[~live], out_phi[~live], out_g[~live] = 0, -1, NEG, NEG
    top = torch.where(absent, NEG, g_c).gather(1, order[:, :k + 1])
    return dict(parent=parent, token=token, phi=out_phi, g=out_g, live=live, top=top)


def separated(top):
    """(B,) bool: the user's best k + 1 perturbed scores are pairwise >= SEP apart, so fp32 rounding cannot decide an
    order (two -inf entries tie exactly and are ordered by index in both)."""
    return ~((top[:, :-1] - top[:, 1:]) < SEP).any(1)


# ------------------------------------------------------------------------------------------ candidates from the rows
def blocked_children(corpus, excluded, P):
    """Per user the set of length-(P + 1) paths every one of whose rows is the row of a listed item."""
    out = []
    for items in excluded:
        rows = {corpus.rows[i] for i in items}
        out.append({path for path in corpus.index[P + 1] if all(r in rows for r in corpus.rows if r[:P + 1] == path)})
    return out


def valid_mask(corpus, prefixes, live, B, kprev, V, P, blocked=None):
    """(B, kprev, V) bool: class v is a candidate of beam (b, j)."""
    valid = torch.zeros(B, kprev, V, dtype=torch.bool)
    for b in range(B):
        for j in range(kprev):
            if not live[b][j]:
                continue
            pre = tuple(prefixes[b][j]) if P else ()
            for v in corpus.children[P].get(pre, ()):
                if v < V and not (blocked and pre + (v,) in blocked[b]):
                    valid[b, j, v] = True
    return valid


def assemble(corpus, prefixes, res, P):
    """ids (B, k, P + 1) and node (B, k) of a step64 result (dead rows -1)."""
    B, k = res["token"].shape
    ids = torch.full((B, k, P + 1), -1, dtype=torch.int64)
    node = torch.full((B, k), -1, dtype=torch.int64)
    for b in range(B):
        for r in range(k):
            if res["live"][b, r]:
                pre = tuple(prefixes[b][int(res["parent"][b, r])]) if P else ()
                path = pre + (int(res["token"][b, r]),)
                ids[b, r] = torch.tensor(path)
                node[b, r] = corpus.index[P + 1][path]
    return ids, node


# ------------------------------------------------------------------------------------------ kernel cases
# corpus, B, kprev, V, P, k, T
CASES = [("c300", 2, 1, 12, 0, 5, 1.0), ("c300", 2, 1, 12, 0, 5, 0.7),   # the first step: no node / parents / parent_*
         ("c300", 3, 4, 12, 1, 8, 1.0), ("c300", 3, 4, 12, 3, 8, 1.0), ("c300", 2, 6, 12, 1, 8, 1.0),
         ("c5", 2, 3, 37, 2, 8, 1.0), ("c3000", 2, 32, 256, 2, 32, 1.0)]
BLOCKED_CASE = ("c300", 3, 4, 12, 1, 8, 1.0)

_CASES = {}


def case(device, name, B, kprev, V, P, k, T, block=False):
    """Seeded inputs of one kernel case and their fp64 reference, built once: bs.draw_beams with parent_lp as
    parent_phi, parent_g = parent_phi minus Exponential(1) draws sorted descending per user, noise from the same CPU
    stream; a user whose top k + 1 perturbed scores are not separated has its noise redrawn. block: every user
    excludes the items under the first candidate of its beam 0 (the blocked row comes from the tokenizer on the
    device, the reference drops those children from the rows)."""
    key = (torch.device(device).type, name, B, kprev, V, P, k, T, block)
    if key in _CASES:
        return _CASES[key]
    tok, corpus = bs.tokenizer(name, device)
    gen = torch.Generator().manual_seed(7000 + 97 * B + 31 * kprev + 7 * V + 3 * P + k + int(10 * T) + 1000 * block)
    c = bs.draw_beams(corpus, gen, B, kprev, V, P)
    phi = g = None
    if P:
        phi = c["parent_lp"]
        g = torch.sort(phi - torch.empty(B, kprev).exponential_(generator=gen), dim=1, descending=True).values
    prefixes = c["parents"].tolist() if P else None
    live = (c["node"] >= 0).tolist() if P else [[True] * kprev] * B
    excluded = blocked = None
    if block:
        excluded = []
        for b in range(B):
            pre = tuple(prefixes[b][0]) if P else ()
            first = next(v for v in corpus.children[P][pre] if v < V)
            excluded.append(bs.items_under(corpus, pre + (first,)))
        blocked = blocked_children(corpus, excluded, P)
        assert all(blocked), "precondition: every user blocks a child"
    valid = valid_mask(corpus, prefixes, live, B, kprev, V, P, blocked)
    noise = torch.empty(B * kprev, V).exponential_(generator=gen)
    for _ in range(200):
        ref = step64(c["logits"], noise, valid, phi, g, T, k)
        bad = (~separated(ref["top"])).nonzero().flatten().tolist()
        if not bad:
            break
        for b in bad:
            noise[b * kprev:(b + 1) * kprev] = torch.empty(kprev, V).exponential_(generator=gen)
    assert separated(ref["top"]).all(), "precondition: separated perturbed scores"
    ids, node = assemble(corpus, prefixes, ref, P)
    _CASES[key] = dict(c, tok=tok, corpus=corpus, noise=noise, parent_phi=phi, parent_g=g, valid=valid, ref=ref,
                       ref_ids=ids, ref_node=node, excluded=excluded)
    return _CASES[key]


def expand(device, c, B, k, P, T=1.0):
    """ops.beam_expand_sampled over the case's trie level P; the five outputs on the CPU."""
    from rqvae_hip import ops
    trie = c["tok"].prefix_trie()
    blocked = None
    if c["excluded"] is not None:
        blocked = c["tok"].blocked_nodes(bs.pad(c["excluded"]).to(device))[P].contiguous()
    out = ops.beam_expand_sampled(c["logits"].to(device), k, batch=B, child_off=trie.child_off[P], tok=trie.tok[P + 1],
                                  noise=c["noise"].to(device), node=bs.dev(c["node"], device),
                                  parents=bs.dev(c["parents"], device), parent_phi=bs.dev(c["parent_phi"], device),
                                  parent_g=bs.dev(c["parent_g"], device), temperature=T, blocked=blocked)
    return tuple(t.cpu() for t in out)


def max_error(got, want):
    """The largest |got - want| over the finite entries of want, in units of the tolerance ATOL + RTOL |want|; the
    -inf entries must be -inf in both."""
    got, fin = got.double(), torch.isfinite(want)
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)) and not torch.isnan(got).any()
    if not fin.any():
        return 0.0, 0.0
    err = (got - want).abs()[fin]
    return float(err.max()), float((err / (ATOL + RTOL * want.abs()[fin])).max())


# ------------------------------------------------------------------------------------------ the sampler recipe
ROWS = torch.tensor([[0, 0], [0, 1], [0, 3], [2, 1], [3, 0], [3, 2]])
CHI2_FIRST, CHI2_PAIR = 35.888, 80.436   # chi-square tails 1e-6 at 5 and 29 degrees of freedom
_RECIPE = {}


def recipe():
    """The two-step recipe: 8192 identical users over ROWS, V = 4, k = 2, every draw from one seeded CPU generator in
    the documented order. Returns a dict with the logits, the noise, the child masks, the items' probabilities p
    (6,) fp64 under the renormalised trie distribution, and the fp64 reference's two steps, picks and rule."""
    if _RECIPE:
        return _RECIPE
    V, B, k = 4, 8192, 2
    gen = torch.Generator().manual_seed(1234)
    l0 = 1.5 * torch.randn(V, dtype=torch.float64, generator=gen)
    l1 = 1.5 * torch.randn(V, V, dtype=torch.float64, generator=gen)   # row = parent token
    e0 = torch.empty(B, V).exponential_(generator=gen)
    e1 = torch.empty(B, k, V).exponential_(generator=gen)
    kids = torch.zeros(V, V, dtype=torch.bool)
    kids[ROWS[:, 0], ROWS[:, 1]] = True
    roots = kids.any(1)
    # of the logits as both samplers see them: rounded to fp32
    p0 = torch.where(roots, torch.softmax(l0.float().double(), 0), 0.0)
    p1 = torch.where(kids, torch.softmax(l1.float().double(), 1), 0.0)
    p = (p0 / p0.sum())[ROWS[:, 0]] * (p1 / p1.sum(1, keepdim=True))[ROWS[:, 0], ROWS[:, 1]]
    assert abs(float(p.sum()) - 1) < 1e-12
    logits0 = l0.float().expand(B, V).contiguous()
    s0 = step64(logits0, e0, roots.expand(B, 1, V), None, None, 1.0, k)
    assert s0["live"].all()
    logits1 = l1.float()[s0["token"]].reshape(B * k, V).contiguous()
    s1 = step64(logits1, e1.reshape(B * k, V), kids[s0["token"]], s0["phi"], s0["g"], 1.0, k)
    assert s1["live"].all()
    picks = torch.stack([s0["token"].gather(1, s1["parent"]), s1["token"]], -1)   # (B, k, 2)
    _RECIPE.update(V=V, B=B, k=k, l0=l0, l1=l1, e0=e0, e1=e1, kids=kids, roots=roots, p=p, logits0=logits0, s0=s0, s1=s1,
                   picks=picks, ok=separated(s0["top"]) & separated(s1["top"]))
    return _RECIPE


def item_index(picks):
    """(B, k) the index in ROWS of every picked row."""
    code = ROWS[:, 0] * 4 + ROWS[:, 1]
    at = (picks[..., 0] * 4 + picks[..., 1]).unsqueeze(-1) == code
    assert at.any(-1).all(), "every pick is a corpus row"
    return at.int().argmax(-1)


def chi_squares(picks, p):
    """(first-row chi-square over the 6 items, ordered-pair chi-square over the 30 pairs, the smallest expected cell)
    of picks (B, 2, 2) against p and p_i p_j / (1 - p_i)."""
    B, n = picks.shape[0], p.numel()
    item = item_index(picks)
    assert (item[:, 0] != item[:, 1]).all(), "without replacement"
    first = torch.bincount(item[:, 0], minlength=n).double()
    chi_first = float(((first - B * p) ** 2 / (B * p)).sum())
    expect = B * p.unsqueeze(1) * p.unsqueeze(0) / (1 - p).unsqueeze(1)
    pair = torch.bincount(item[:, 0] * n + item[:, 1], minlength=n * n).double().view(n, n)
    off = ~torch.eye(n, dtype=torch.bool)
    chi_pair = float(((pair - expect) ** 2 / expect)[off].sum())
    return chi_first, chi_pair, float(expect[off].min())
