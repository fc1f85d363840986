"""EMA-maintained codebooks for the RQ-VAE — an EXTENSION (the reference trains its codebooks with AdamW on the
codebook term of the loss and has no counterpart; this is the update rule of VQ-VAE's appendix, Sonnet's
VectorQuantizerEMA and vector-quantize-pytorch).

The rule (include/rqvae_hip.h, rq_codebook_ema_stats / rq_codebook_ema_apply), per level l and code k. One training
forward with level inputs res (L, B, D) fp32 and ids (B, L) int64 ACCUMULATES

    n[l][k]    += #{b : ids[b][l] == k}                                  exact, int64
    s[l][k][:]  = s[l][k][:] + sum_{b : ids[b][l] == k} res[l][b][:]     fp32, the batch sum formed first, added once

(ids outside [0, K) are skipped), so gradient-accumulation micro-batches and data-parallel shards add up; one update
with decay g and smoothing eps then reads the accumulated n, s, rewrites the fp32 state N (L, K), S (L, K, D) and the
codebooks, and zeroes n, s:

    N'[l][k] = g N[l][k] + (1 - g) n[l][k]          S'[l][k] = g S[l][k] + (1 - g) s[l][k]
    T[l]     = sum_k N'[l][k]                       N~[l][k] = (N'[l][k] + eps) / (T[l] + K eps) * T[l]
    W_l[k][:] = S'[l][k][:] / N~[l][k]

g and 1 - g are each rounded to fp32 once, from the Python floats. The state starts as N = 1, S = W.

Device tensors run the HIP kernels (rqvae_hip.ops.codebook_ema_stats / codebook_ema_apply); CPU tensors compute the
same rule with plain torch (summation orders differ, so the two agree within fp32 rounding, not bit for bit).
Data parallelism: n and s are summed over the ranks before the update; every rank then applies identical statistics
to identical state, so N, S and the codebooks stay bit-identical across ranks without a broadcast.

Limits (ValueError outside them): 1 <= L <= 16, 1 <= K <= 4096, D % 4 == 0, 4 <= D <= 1024, 0 <= decay < 1, eps > 0.
"""
import torch
import torch.distributed as dist

from rqvae_hip import ops as hip_ops


def _check_stats(res, ids, n, s, what):
    if res.dim() != 3 or ids.dim() != 2 or tuple(ids.shape) != (res.shape[1], res.shape[0]):
        raise ValueError(f"{what}: need res (L, B, D) and ids (B, L), got {tuple(res.shape)}, {tuple(ids.shape)}")
    L, _, D = res.shape
    if n.dim() != 2 or n.shape[0] != L or tuple(s.shape) != (L, n.shape[1], D):
        raise ValueError(f"{what}: need n (L, K) and s (L, K, D), got {tuple(n.shape)}, {tuple(s.shape)}")
    hip_ops.ema_check_args(L, n.shape[1], D, what=what)


@torch.no_grad()
def ema_stats_(res, ids, n, s):
    """Accumulate one forward's per-code counts and sums IN PLACE into n (L, K) int64 and s (L, K, D) fp32."""
    if res.is_cuda:
        hip_ops.codebook_ema_stats(res.detach().contiguous(), ids.contiguous(), n, s)
        return n, s
    what = "ema_stats_"
    if any(t.is_cuda for t in (ids, n, s)):
        raise hip_ops.RqHipError(f"{what}: res, ids, n and s must be on one device")
    _check_stats(res, ids, n, s, what)
    L, K = n.shape
    for l in range(L):
        col = ids[:, l]
        ok = (col >= 0) & (col < K)
        n[l] += torch.bincount(col[ok], minlength=K)
        s[l] += torch.zeros_like(s[l]).index_add_(0, col[ok], res[l].detach()[ok])
    return n, s


def _apply_cpu(weights, N, S, n, s, decay, eps):
    K = N.shape[1]
    g = torch.tensor(decay, dtype=torch.float64).to(torch.float32)
    omg = torch.tensor(1.0 - decay, dtype=torch.float64).to(torch.float32)
    e = torch.tensor(eps, dtype=torch.float64).to(torch.float32)
    ke = torch.tensor(K * eps, dtype=torch.float64).to(torch.float32)
    N.copy_(g * N + omg * n.to(torch.float32))
    S.copy_(g * S + omg * s)
    T = N.sum(1, keepdim=True)
    nt = (N + e) / (T + ke) * T
    for l, w in enumerate(weights):
        w.detach().copy_(S[l] / nt[l][:, None])
    n.zero_()
    s.zero_()


@torch.no_grad()
def ema_apply_(weights, N, S, n, s, *, decay: float = 0.99, eps: float = 1e-5, group=None):
    """One EMA update IN PLACE from the accumulated statistics: rewrites N, S and the L (K, D) weights, zeroes n, s.
    With torch.distributed initialised and more than one rank (in `group`), n and s are first summed over the ranks."""
    weights = list(weights)
    what = "ema_apply_"
    if not weights or weights[0].dim() != 2:
        raise ValueError(f"{what}: weights must be a non-empty list of (K, D) tensors")
    L, (K, D) = len(weights), weights[0].shape
    hip_ops.ema_check_args(L, K, D, float(decay), float(eps), what)
    if tuple(N.shape) != (L, K) or tuple(S.shape) != (L, K, D) or tuple(n.shape) != (L, K) or \
            tuple(s.shape) != (L, K, D):
        raise ValueError(f"{what}: need N, n ({L}, {K}) and S, s ({L}, {K}, {D})")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(n, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(s, op=dist.ReduceOp.SUM, group=group)
    if S.is_cuda:
        hip_ops.codebook_ema_apply(weights, N, S, n, s, float(decay), float(eps))
    else:
        if any(t.is_cuda for t in weights + [N, n, s]):
            raise hip_ops.RqHipError(f"{what}: weights, N, S, n and s must be on one device")
        _apply_cpu(weights, N, S, n, s, float(decay), float(eps))


def initial_state(weights):
    """(N, S, n, s) at the moment the feature is switched on: N = 1, S = W (so S / N is the codebook), n = s = 0."""
    weights = list(weights)
    S = torch.stack([w.detach() for w in weights]).to(torch.float32).clone().contiguous()
    N = torch.ones(S.shape[:2], dtype=torch.float32, device=S.device)
    return N, S, torch.zeros(S.shape[:2], dtype=torch.int64, device=S.device), torch.zeros_like(S)
