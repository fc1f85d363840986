"""Incremental beam decoding, host side (CPU-only): the ancestor table that follows beams through re-ordering,
and the argument contracts of the new entry points."""
import pytest
import torch


def _walk(parents, widths, B):
    """Brute force: for every beam of the last level, follow its parent pointers back to the BOS row.
    parents[l] (B, widths[l + 1]) points from level l + 1 into level l; level l has widths[l] beams per user and
    beam (b, j) sits in row b * widths[l] + j of that level's buffer."""
    t = len(parents)
    rows = []
    for b in range(B):
        for j in range(widths[t]):
            chain, cur = [0] * t, j
            for s in range(t - 1, -1, -1):
                cur = int(parents[s][b][cur])
                chain[s] = b * widths[s] + cur
            rows.append(chain)
    return torch.tensor(rows, dtype=torch.int32).reshape(B * widths[t], t)


def test_beam_advance_ancestors_hand_tree():
    """B = 2, beams per user 1 -> 3 -> 3 -> 3. The second selection has two children of one parent and a parent
    left without children (user 0: parents 2, 2, 0; beam 1 dies), the third re-orders and duplicates again."""
    from rqvae_hip import ops
    B, widths = 2, [1, 3, 3, 3]
    parents = [torch.zeros(2, 3, dtype=torch.int32),
               torch.tensor([[2, 2, 0], [1, 0, 2]], dtype=torch.int32),
               torch.tensor([[1, 0, 1], [2, 2, 2]], dtype=torch.int32)]
    anc = None
    for t in range(1, 4):
        anc = ops.beam_advance_ancestors(anc, parents[t - 1], widths[t - 1])
        assert anc.dtype == torch.int32 and anc.shape == (B * widths[t], t)
        assert torch.equal(anc, _walk(parents[:t], widths, B)), t
    # spelled out: user 0's beams after the second selection continue rows 2, 2, 0 of step 1, all from BOS row 0
    want2 = torch.tensor([[0, 2], [0, 2], [0, 0], [1, 4], [1, 3], [1, 5]], dtype=torch.int32)
    assert torch.equal(ops.beam_advance_ancestors(ops.beam_advance_ancestors(None, parents[0], 1), parents[1], 3), want2)
    # and after the third: user 0 beam 0 continues step-2 beam 1 (row 1), whose own chain was (0, 2)
    assert anc[0].tolist() == [0, 2, 1] and anc[1].tolist() == [0, 2, 0] and anc[5].tolist() == [1, 5, 5]
    # int64 parents (as a torch reference would produce) give the same table
    assert torch.equal(ops.beam_advance_ancestors(None, parents[0].long(), 1),
                       ops.beam_advance_ancestors(None, parents[0], 1))


def test_new_beam_ops_refuse_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    q = torch.zeros(4, 32)
    qkv = torch.zeros(4, 96)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_self_attention(q, [(qkv[:, 32:64], qkv[:, 64:])], None, 2)
    ids = torch.zeros(2, 4, dtype=torch.int64)
    lp = torch.zeros(2, 4)
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.beam_select(ids, lp, 2, batch=2, valid=torch.ones(8, dtype=torch.bool), return_parent=True)


def test_incremental_requires_fused():
    from modules.model import EncoderDecoderRetrievalModel
    model = EncoderDecoderRetrievalModel(embedding_dim=8, attn_dim=16, dropout=0.0, num_heads=1, n_layers=2,
                                         num_embeddings=4, sem_id_dim=2, inference_verifier_fn=None, max_pos=8)
    model.enable_generation = True
    with pytest.raises(ValueError, match="requires fused=True"):
        model.generate_next_sem_id(None, top_k=True, fused=False, incremental=True)
    assert model.training and model.transformer.cached_enc_output is None
