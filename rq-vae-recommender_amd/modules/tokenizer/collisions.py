"""Collision-resolved corpus ids — an EXTENSION (the reference keeps colliding items apart only by the dedup column,
modules/tokenizer/semids.py:84-99, a token without semantic meaning whose vocabulary is as large as the most crowded
cell). `resolve` moves a colliding item to its next-best code path instead; the n-best paths per item come from the
beam encoder (RqVae.get_semantic_id_beams).

The rule, W rounds over paths (N, W, L), beams best first:

  * round 0: every item proposes paths[i, 0]; the lowest corpus index among equal tuples owns the tuple and is
    placed with choice 0;
  * round r = 1..W-1: every item not yet placed proposes paths[i, r]; a proposal is accepted iff no item owns that
    tuple and no lower-index item proposed it in this round; accepted items own the tuple, placed with choice r;
  * items still unplaced after the last round fall back to paths[i, 0] with choice 0 (they collide as before, and
    the dedup column separates them).

Deterministic, and a function of the paths alone: every data-parallel rank that runs it on the gathered paths gets
the same ids. Each round is one stable sort of packed tuple keys plus one binary search in the sorted owned keys —
no per-item Python loop; CPU and device tensors alike.
"""
import torch
from torch import Tensor


def _pack(cols: Tensor, base: int) -> Tensor:
    key = torch.zeros(cols.shape[:-1], dtype=torch.int64, device=cols.device)
    for j in range(cols.shape[-1]):
        key = key * base + cols[..., j].to(torch.int64)
    return key


@torch.no_grad()
def resolve(paths: Tensor, base: int):
    """paths (N, W, L) integer, every entry in [0, base) -> (ids (N, L) int64, choice (N,) int64): ids[i] =
    paths[i, choice[i]]."""
    if paths.dim() != 3:
        raise ValueError(f"resolve: paths must be (N, W, L), got {tuple(paths.shape)}")
    N, W, L = paths.shape
    if base < 1 or base ** L >= 1 << 63:
        raise ValueError(f"resolve: base ** L must fit a signed 64-bit key (base={base}, L={L})")
    dev = paths.device
    keys = _pack(paths, base)                                    # (N, W)
    placed = torch.zeros(N, dtype=torch.bool, device=dev)
    choice = torch.zeros(N, dtype=torch.int64, device=dev)
    owned = torch.zeros(0, dtype=torch.int64, device=dev)        # sorted keys of the owned tuples
    for r in range(W):
        idx = torch.nonzero(~placed).flatten()                   # the proposers, ascending corpus index
        if idx.numel() == 0:
            break
        sk, order = torch.sort(keys[idx, r], stable=True)        # equal tuples: lowest index first
        accept = torch.ones_like(sk, dtype=torch.bool)
        accept[1:] = sk[1:] != sk[:-1]
        if owned.numel() > 0:
            pos = torch.searchsorted(owned, sk).clamp_max(owned.numel() - 1)
            accept &= owned[pos] != sk
        win = idx[order[accept]]
        placed[win] = True
        choice[win] = r
        owned = torch.sort(torch.cat([owned, sk[accept]])).values
    ids = paths[torch.arange(N, device=dev), choice].to(torch.int64)
    return ids, choice
