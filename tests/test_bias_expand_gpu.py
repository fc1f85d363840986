"""The biased beam step on the device: rq_beam_expand_biased / rq_beam_expand_wide_biased against an fp64 step that
enumerates the valid continuations from the corpus rows and adds the brute-force subtree bounds, against the plain
beam_expand where the bias is absent or zero, with blocked nodes, with bad values planted in a level table, narrow
against wide bit for bit, and one shape only the wide form takes against a chunk-merge of the narrow one."""
import numpy as np
import pytest
import torch

import beam_support as bs
import bias_support as bi

pytestmark = pytest.mark.gpu


def _check_vs_reference(got, ref, what=""):
    """ids, parent and node exact; out_lp and out_score to test_beam_expand_gpu's out_lp tolerance; dead rows."""
    ids, lp, score, parent, node = (t.cpu() for t in got)
    want_ids, want_lp, want_s, want_parent, want_node, _ = ref
    B, k = want_lp.shape
    assert ids.shape == want_ids.shape and ids.dtype == torch.int64
    assert lp.shape == score.shape == (B, k) and lp.dtype == score.dtype == torch.float32
    assert parent.shape == node.shape == (B, k) and parent.dtype == node.dtype == torch.int32
    live = want_node >= 0
    if live.any():
        print(f"{what}max rel err: lp {float(((lp.double() - want_lp).abs() / want_lp.abs())[live].max()):.3e}, "
              f"score {float(((score.double() - want_s).abs() / want_s.abs().clamp_min(1e-30))[live].max()):.3e}")
    assert torch.equal(ids, want_ids), f"{what}out_ids"
    assert torch.equal(parent.long(), want_parent), f"{what}out_parent"
    assert torch.equal(node.long(), want_node), f"{what}out_node"
    np.testing.assert_allclose(lp.double().numpy(), want_lp.numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(score.double().numpy(), want_s.numpy(), rtol=1e-5, atol=0)
    bs.assert_dead_rows(ids, lp, parent, node)
    assert torch.isneginf(score[node < 0]).all(), f"{what}dead rows carry out_score -inf"


# ------------------------------------------------------------------------------------------ kernel vs the fp64 step
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_biased_expand_vs_fp64(device, name, B, kprev, V, P, k, T, wide):
    c = bi.case(name, B, kprev, V, P, k, T)
    tok, _ = bs.tokenizer(name, device)
    print(f"{name} B={B} kprev={kprev} V={V} P={P} k={k} T={T}: groups {c['groups'].tolist()}, redraws {c['redraws']}, "
          f"candidates per user {[len(s) for s in c['ref'][5]]}")
    _check_vs_reference(bi.expand(device, tok, c, B, k, P, T, wide=wide), c["ref"])


def test_cases_cover_every_group():
    """The seeded groups of the nine shapes: unbiased users and every one of the three rows appear."""
    seen = set()
    for name, B, kprev, V, P, k in bs.SHAPES:
        seen |= set(bi.case(name, B, kprev, V, P, k, 1.0)["groups"].tolist())
    assert seen == {-1, 0, 1, 2}


@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_narrow_equals_wide_bitwise(device, name, B, kprev, V, P, k):
    c = bi.case(name, B, kprev, V, P, k, 1.0)
    tok, _ = bs.tokenizer(name, device)
    narrow = bi.expand(device, tok, c, B, k, P, wide=False)
    bi.assert_same(bi.expand(device, tok, c, B, k, P, wide=True), narrow)
    bi.assert_same(bi.expand(device, tok, c, B, k, P, wide=None), narrow, "wide=None is the narrow form here: ")


# ------------------------------------------------------------------------------------------ no bias, zero bias
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name,B,kprev,V,P,k", bs.SHAPES)
def test_unbiased_and_zero_row_equal_plain_expand(device, name, B, kprev, V, P, k, wide):
    """Group -1 (and any group outside [0, G)) and the all-zero row: ids, lp, parent and node are beam_expand's bits
    and out_score == out_lp."""
    c = bi.case(name, B, kprev, V, P, k, 1.0)
    tok, _ = bs.tokenizer(name, device)
    plain = bs.expand(device, tok, c, B, k, P, wide=wide)
    for groups in ([-1] * B, [2] * B, [3, -7, 99][:B], [-1, 2, -1][:B]):
        got = bi.expand(device, tok, c, B, k, P, wide=wide, groups=torch.tensor(groups, dtype=torch.int32))
        bs.assert_same((got[0], got[1], got[3], got[4]), plain, f"groups {groups}: ")
        assert torch.equal(got[2].view(torch.int32), got[1].view(torch.int32)), "out_score == out_lp"


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_all_minus_inf_user_has_only_dead_rows(device, wide):
    name, B, kprev, V, P, k = bs.SHAPES[1]
    c = bi.case(name, B, kprev, V, P, k, 1.0)
    tok, _ = bs.tokenizer(name, device)
    table = torch.cat([c["table"], torch.full_like(c["table"][:1], bi.NINF)])
    groups = torch.tensor([3, -1, 3], dtype=torch.int32)
    ids, lp, score, parent, node = (t.cpu() for t in bi.expand(device, tok, c, B, k, P, wide=wide, table=table,
                                                              groups=groups))
    for b in (0, 2):
        assert (ids[b] == -1).all() and torch.isneginf(lp[b]).all() and torch.isneginf(score[b]).all()
        assert (parent[b] == 0).all() and (node[b] == -1).all()
    plain = bs.expand(device, tok, c, B, k, P, wide=wide)
    assert torch.equal(ids[1], plain[0][1].cpu()) and (node[1] >= 0).any()


# ------------------------------------------------------------------------------------------ with blocked nodes
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name,B,kprev,V,P,k", [bs.SHAPES[2], bs.SHAPES[6], bs.SHAPES[8]])
def test_biased_with_blocked_vs_fp64(device, name, B, kprev, V, P, k, wide):
    """Every user's biased winners 0 and 2 are blocked: the result is the reference over the remaining candidates."""
    c = bi.case(name, B, kprev, V, P, k, 1.0)
    tok, _ = bs.tokenizer(name, device)
    want_node = c["ref"][4]
    gone = [sorted({int(want_node[b, r]) for r in (0, 2) if int(want_node[b, r]) >= 0}) for b in range(B)]
    assert all(gone), "every user has a winner to block"
    H = max(len(g) for g in gone)
    blocked = torch.tensor([g + [bs.NONE] * (H - len(g)) for g in gone], dtype=torch.int32)
    ref = bi.biased_reference(c["corpus"], bs.log_softmax64(c["logits"], 1.0), c["pre"], c["live"], c["parent_lp"],
                              c["groups"], c["table"], B, kprev, V, P, k, blocked=[set(g) for g in gone])
    got = bi.expand(device, tok, c, B, k, P, wide=wide, blocked=blocked.to(device))
    assert not any(int(n) in gone[b] for b in range(B) for n in got[4][b].tolist())
    assert all(bs.separated(s, k) for s in ref[5]), "precondition: the remaining scores are separated"
    _check_vs_reference(got, ref)


# ------------------------------------------------------------------------------------------ bad table values
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_nan_and_plus_inf_in_a_table_read_as_minus_inf(device, wide):
    name, B, kprev, V, P, k = bs.SHAPES[1]
    c = bi.case(name, B, kprev, V, P, k, 1.0)
    tok, _ = bs.tokenizer(name, device)
    groups = torch.tensor([0, 0, 1], dtype=torch.int32)
    base = bi.biased_reference(c["corpus"], bs.log_softmax64(c["logits"], 1.0), c["pre"], c["live"], c["parent_lp"],
                               groups, c["table"], B, kprev, V, P, k)
    hit = [int(base[4][b, 0]) for b in range(B)]   # every user's winner
    assert all(n >= 0 for n in hit)
    bad, hidden = c["table"].clone(), c["table"].clone()
    for b, val in zip(range(B), (float("nan"), float("inf"), float("nan"))):
        bad[int(groups[b]), hit[b]] = val
        hidden[int(groups[b]), hit[b]] = bi.NINF
    want = bi.expand(device, tok, c, B, k, P, wide=wide, table=hidden, groups=groups)
    got = bi.expand(device, tok, c, B, k, P, wide=wide, table=bad, groups=groups)
    bi.assert_same(got, want)
    assert not got[1].isnan().any() and not got[2].isnan().any()
    assert hit[0] not in got[4][0].tolist() and hit[2] not in got[4][2].tolist()
    # -0.0 is +0.0: the zero row negated gives plain beam_expand's bits
    neg = torch.cat([c["table"][:2], -c["table"][2:3]])
    assert (bi.bits_of(neg[2]) == -2 ** 31).all()
    zero = bi.expand(device, tok, c, B, k, P, wide=wide, table=neg, groups=torch.tensor([2] * B, dtype=torch.int32))
    plain = bs.expand(device, tok, c, B, k, P, wide=wide)
    bs.assert_same((zero[0], zero[1], zero[3], zero[4]), plain)
    assert torch.equal(zero[2].view(torch.int32), zero[1].view(torch.int32))


# ------------------------------------------------------------------------------------------ only the wide form
def test_wide_only_shape_equals_chunk_merge(device):
    """c3000, 128 beams in and out at P = 2 (kprev V = 32,768 keys): the exact 128 best by biased score of the narrow
    kernel's chunks of 32 beams, merged by (score descending, beam, token) — bit for bit, out_lp included."""
    name, B, kprev, V, P, k = "c3000", 2, 128, 256, 2, 128
    tok, corpus = bs.tokenizer(name, device)
    c = bs.wide_inputs(corpus, B, kprev, V, P, 5100)
    table = bi.step_tables(name, corpus)[P]
    groups = torch.tensor([1, 0], dtype=torch.int32)
    lp_of = {}

    def narrow(logits, node, parents, plp, batch, kp, kk):
        n_ch = batch // B
        out = tuple(t.cpu() for t in bi.expand(
            device, tok, dict(logits=logits, node=node, parents=parents, parent_lp=plp), batch, kk, P, table=table,
            groups=groups.repeat_interleave(n_ch), wide=False))
        ids, lp, score, parent, out_node = out
        for e in range(batch):
            for r in range(kk):
                if int(out_node[e, r]) >= 0:
                    lp_of[(e // n_ch, (e % n_ch) * kp + int(parent[e, r]), int(ids[e, r, P]))] = lp[e, r]
        return ids, score, parent, out_node   # chunk_merge orders by its second result: the biased score

    want_ids, want_s, want_parent, want_node = bs.chunk_merge(narrow, c, B, kprev, V, P, k)
    want_lp = torch.full((B, k), bi.NINF)
    for b in range(B):
        for r in range(k):
            if int(want_node[b, r]) >= 0:
                want_lp[b, r] = lp_of[(b, int(want_parent[b, r]), int(want_ids[b, r, P]))]
    assert (want_node >= 0).sum() > k, "live rows"
    got = bi.expand(device, tok, c, B, k, P, table=table, groups=groups, wide=True)
    bi.assert_same(got, (want_ids, want_lp, want_s, want_parent, want_node))
    bi.assert_same(bi.expand(device, tok, c, B, k, P, table=table, groups=groups, wide=None), got, "wide=None: ")
    plain = bs.expand(device, tok, c, B, k, P, wide=True)
    assert not torch.equal(plain[0], got[0]), "the bias changes the beams"


# ------------------------------------------------------------------------------------------ refusals
def test_biased_expand_refuses_bad_arguments(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = bs.tokenizer("c5", device)
    trie = tok.prefix_trie()
    x = torch.zeros(4, 16, device=device)
    lvl0 = dict(child_off=trie.child_off[0], tok=trie.tok[1])
    n1 = trie.tok[1].numel()
    ok = dict(bias=torch.zeros(2, n1, device=device), bias_group=torch.zeros(4, dtype=torch.int32, device=device))
    out = ops.beam_expand_biased(x, 3, batch=4, **lvl0, **ok)
    assert len(out) == 5 and out[0].shape == (4, 3, 1) and out[2].shape == (4, 3)
    with pytest.raises(RqHipError, match="bias must be .G, n_children"):
        ops.beam_expand_biased(x, 3, batch=4, **lvl0, **{**ok, "bias": torch.zeros(2, n1 + 1, device=device)})
    with pytest.raises(RqHipError, match="bias must be a contiguous torch.float32"):
        ops.beam_expand_biased(x, 3, batch=4, **lvl0, **{**ok, "bias": torch.zeros(2, n1, device=device).double()})
    with pytest.raises(RqHipError, match="bias_group must be a contiguous torch.int32"):
        ops.beam_expand_biased(x, 3, batch=4, **lvl0, **{**ok, "bias_group": torch.zeros(4, dtype=torch.int64, device=device)})
    with pytest.raises(RqHipError, match="bias_group must have shape"):
        ops.beam_expand_biased(x, 3, batch=4, **lvl0, **{**ok, "bias_group": torch.zeros(3, dtype=torch.int32, device=device)})
    with pytest.raises(RqHipError, match="are required"):
        ops.beam_expand_biased(x, 3, batch=4, **lvl0, bias=None, bias_group=None)
    with pytest.raises(RqHipError, match="envelope"):
        ops.beam_expand_biased(torch.zeros(40, 256, device=device), 3, batch=1, **lvl0,
                               bias=ok["bias"], bias_group=ok["bias_group"][:1])        # kprev V > 8192, narrow
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_expand_biased(x, 3, batch=4, **lvl0, **{**ok, "bias": ok["bias"].cpu()})
    # G == 0: nobody can be biased; plain beam_expand's result
    none = ops.beam_expand_biased(x, 3, batch=4, **lvl0, bias=torch.zeros(0, n1, device=device), bias_group=ok["bias_group"])
    plain = ops.beam_expand(x, 3, batch=4, **lvl0)
    bs.assert_same((none[0], none[1], none[3], none[4]), plain)
