"""rq_trie_bias_nodes on the device: the ItemBias tables of device tensors against the CPU tables and the brute-force
walk of the corpus rows, bit for bit, on the host tests' inputs; two runs give equal bits; odd group counts and sizes."""
import pytest
import torch

import beam_support as bs
import bias_support as bi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", bi.TABLE_CORPORA)
def test_device_tables_equal_cpu_tables_equal_brute_force(device, name):
    ids = bi.table_ids(name)
    corpus = bs.Corpus(ids)
    bias = bi.awkward_bias(ids)
    upper, leaf_item = bi.brute_tables(corpus, bias)
    cpu = bs.ids_tokenizer(ids.clone()).item_bias(bias)
    tok = bs.ids_tokenizer(ids.clone().to(device))
    got = tok.item_bias(bias.to(device))
    assert all(u.is_cuda for u in got.upper) and got.leaf_item.is_cuda
    bi.assert_tables(got, upper, leaf_item, "device vs brute force: ")
    bi.assert_tables(got, [u for u in cpu.upper], cpu.leaf_item, "device vs CPU: ")
    again = tok.item_bias(bias.to(device))
    bi.assert_tables(again, [u.cpu() for u in got.upper], got.leaf_item.cpu(), "two runs: ")
    one = tok.item_bias(bias[0].to(device))   # (N,): one group
    bi.assert_tables(one, [u[:1] for u in upper], leaf_item[:1], "1-D: ")


def test_many_groups_and_a_larger_corpus(device):
    """c3000 (more than one workgroup's worth of (group, item) pairs) with 5 groups, against the CPU tables; G == 0."""
    tok, corpus = bs.tokenizer("c3000", device)
    N = len(corpus.rows)
    g = torch.Generator().manual_seed(31)
    bias = 2.0 * torch.randn(5, N, generator=g)
    bias[3][torch.rand(N, generator=g) < 0.5] = bi.NINF
    bias[4] = bi.NINF
    cpu = bs.tokenizer("c3000", "cpu")[0].item_bias(bias)
    got = tok.item_bias(bias.to(device))
    bi.assert_tables(got, list(cpu.upper), cpu.leaf_item)
    assert (got.leaf_item[4] == -1).all() and torch.isneginf(got.upper[0][4]).all()
    # every level's bound is the max of its children's: the bounds never increase along a path
    trie = tok.prefix_trie()
    for q in range(1, trie.depth):
        off = trie.child_off[q].long()
        parent = torch.repeat_interleave(torch.arange(off.numel() - 1, device=device), off[1:] - off[:-1])
        assert (got.upper[q] <= got.upper[q - 1][:, parent]).all()
    empty = tok.item_bias(torch.zeros(0, N, device=device))
    assert empty.groups == 0 and empty.leaf_item.shape == (0, cpu.leaf_item.shape[1])


def test_refuses_bad_arguments(device):
    from rqvae_hip import ops, RqHipError
    tok, _ = bs.tokenizer("c5", device)
    idx = tok.trie_index()
    n_nodes = [c.numel() for c in idx.leaf_count]
    ok = torch.zeros(1, 5, device=device)
    assert len(ops.trie_bias_nodes(ok, idx.item_leaf, idx.leaf_anc, n_nodes)[0]) == 4
    with pytest.raises(RqHipError, match="bias must be .G, N."):
        ops.trie_bias_nodes(ok[0], idx.item_leaf, idx.leaf_anc, n_nodes)
    with pytest.raises(RqHipError, match="bias must be a contiguous torch.float32"):
        ops.trie_bias_nodes(ok.double(), idx.item_leaf, idx.leaf_anc, n_nodes)
    with pytest.raises(RqHipError, match="item_leaf must have shape"):
        ops.trie_bias_nodes(torch.zeros(1, 6, device=device), idx.item_leaf, idx.leaf_anc, n_nodes)
    with pytest.raises(RqHipError, match="envelope"):
        ops.trie_bias_nodes(ok, idx.item_leaf, idx.leaf_anc, n_nodes[:3])
    with pytest.raises(ValueError, match="must live on the corpus ids' device"):
        tok.item_bias(torch.zeros(5))
