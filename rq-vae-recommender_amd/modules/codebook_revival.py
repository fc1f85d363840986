"""Dead-code revival for the RQ-VAE codebooks — an EXTENSION (no counterpart in the reference, whose only
countermeasure against codebook collapse is the one-shot k-means init; its nearest relative is the
`codebook_usage_{l}` log at checkpoint time, train_rqvae.py:232-239).

A codeword that no item selects never receives a gradient, so it never moves: the level loses capacity and
collisions rise. `revive_` re-seats such codewords on encoder residuals of the data. The rule only copies and
zeroes, so the device kernel (rqvae_hip.ops.codebook_revive), the plain-torch CPU path below and every
data-parallel rank produce the same bits:

  * level l's dead codes are {k : counts[l][k] < min_count}, in ascending k;
  * the j-th dead code (0-based) takes donor row r = (s_l + j) mod B of res[l], with
    s_l = splitmix64(seed, l) mod B in unsigned 64-bit arithmetic (csrc/common.h splitmix64);
  * the codeword becomes a bit copy of res[l][r]; its rows of both AdamW moments become +0.0;
  * B >= K is required, so the donors of a level are distinct rows and nothing is capped.

Limits (ValueError outside them): 1 <= L <= 16, 1 <= K <= 2^20, D % 4 == 0, D <= 1024, min_count >= 0
(0: nothing is dead).
"""
import torch
import torch.distributed as dist

from rqvae_hip import ops as hip_ops

_M64 = (1 << 64) - 1


def splitmix64(seed: int, c: int) -> int:
    """SplitMix64 output of counter c under key seed (csrc/common.h splitmix64), mod 2^64."""
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def donor_start(seed: int, level: int, B: int) -> int:
    """s_l: the donor row of level `level`'s first dead code."""
    return splitmix64(int(seed) & _M64, level) % B


def _revive_cpu(weights, counts, res, min_count, seed, exp_avg, exp_avg_sq):
    L, (K, D), B = len(weights), weights[0].shape, res.shape[1]
    hip_ops.revive_check_args(L, K, D, B, min_count, "revive_")
    n_revived = torch.zeros(L, dtype=torch.int64)
    for l in range(L):
        dead = torch.nonzero(counts[l] < min_count).flatten()   # ascending k
        n_revived[l] = dead.numel()
        if dead.numel() == 0:
            continue
        rows = (donor_start(seed, l, B) + torch.arange(dead.numel())) % B
        weights[l].detach()[dead] = res[l][rows]
        if exp_avg is not None:
            exp_avg[l][dead] = 0.0
            exp_avg_sq[l][dead] = 0.0
    return n_revived


@torch.no_grad()
def revive_(weights, counts, res, *, min_count: int = 1, seed: int, exp_avg=None, exp_avg_sq=None, group=None):
    """Re-seat, IN PLACE, the codewords of every level whose usage count is below min_count -> n_revived (L,) int64.

    weights: the L levels' (K, D) fp32 codebook tensors; counts (L, K) int64 usage counters (RqVae.code_usage);
    res (L, B, D) fp32: each level's input residuals of B >= K data rows; exp_avg / exp_avg_sq: the weights' AdamW
    moments (both or neither). Device tensors run the HIP kernel; CPU tensors compute the same result, bit for bit,
    with plain torch. With torch.distributed initialised and more than one rank (in `group`): counts are first
    summed over the ranks, so every rank sees the same dead set and zeroes the same moment rows; each rank applies
    the rule to its own res; then the L weights are broadcast from the group's rank 0, whose donors therefore win.
    Ends with counts.zero_() — the next usage window starts here."""
    weights = list(weights)
    if (exp_avg is None) != (exp_avg_sq is None):
        raise ValueError("revive_: exp_avg and exp_avg_sq go together (both or neither)")
    exp_avg = None if exp_avg is None else list(exp_avg)
    exp_avg_sq = None if exp_avg_sq is None else list(exp_avg_sq)
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    if multi:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
    if res.is_cuda:
        _, n_revived = hip_ops.codebook_revive(weights, counts, res, min_count, seed, exp_avg, exp_avg_sq)
    else:
        if any(t.is_cuda for t in weights) or counts.is_cuda:
            raise hip_ops.RqHipError("revive_: weights, counts and res must be on one device")
        if res.dim() != 3 or res.shape[0] != len(weights) or tuple(res.shape[2:]) != tuple(weights[0].shape[1:]):
            raise ValueError(f"revive_: res must be (L, B, D), got {tuple(res.shape)}")
        n_revived = _revive_cpu(weights, counts, res, int(min_count), int(seed), exp_avg, exp_avg_sq)
    if multi:
        src = 0 if group is None else dist.get_global_rank(group, 0)
        for w in weights:
            dist.broadcast(w.detach(), src=src, group=group)
    counts.zero_()
    return n_revived
