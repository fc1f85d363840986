"""Beam-searched residual quantization with torch ops — an EXTENSION (the reference encodes greedily,
modules/rqvae.py:114-138: one residual per item, one argmin per level). `beam_quantize_torch` restates the rule of
the device kernel (rqvae_hip.ops.rq_quantize_beam, include/rqvae_hip.h), the beam encoder of Faiss's
ResidualQuantizer (max_beam_size):

  * level 0 starts from one beam with residual x;
  * at level l, beam w (residual r_w) and code k have the key e(w, k) = (|r_w|^2 + |c_k|^2) - 2 r_w.c_k in fp32,
    the expression of the greedy path (modules/quantize.py:108-112);
  * the W candidates with the smallest (e, w, k), lexicographic, survive in that order — a STABLE sort of the keys
    flattened as w K + k, so ties fall to the lower beam, then the lower code;
  * a survivor's residual is r_w - c_k and its path is its parent's plus k.

It serves CPU tensors through RqVae.get_semantic_id_beams, and on the device it is the composite that
tools/beam_quantize_time.py times the kernel against. Integer-valued inputs give the kernel's bits; otherwise
the two agree wherever keys are further apart than the matmul's summation-order noise.
"""
import torch
from torch import Tensor

from rqvae_hip import ops as hip_ops


@torch.no_grad()
def beam_quantize_torch(x: Tensor, codebooks: Tensor, width: int):
    """x (B, D) fp32, codebooks (L, K, D) fp32 -> (paths (B, W, L) int64, err (B, W), residual (B, W, D))."""
    if x.dim() != 2 or codebooks.dim() != 3 or x.shape[1] != codebooks.shape[2]:
        raise ValueError(f"beam_quantize_torch: need x (B, D) and codebooks (L, K, D), got {tuple(x.shape)}, "
                         f"{tuple(codebooks.shape)}")
    (B, D), (L, K, _), W = x.shape, codebooks.shape, int(width)
    hip_ops.beam_quantize_check_args(D, K, L, W, "beam_quantize_torch")
    x, codebooks = x.to(torch.float32), codebooks.to(torch.float32)
    res = x.unsqueeze(1)                                                      # (B, 1, D)
    paths = torch.zeros((B, 1, 0), dtype=torch.int64, device=x.device)
    err = torch.zeros((B, 1), dtype=torch.float32, device=x.device)
    for l in range(L):
        cb = codebooks[l]
        n = res.shape[1]
        keys = ((res * res).sum(-1, keepdim=True) + (cb * cb).sum(-1)) - (2.0 * res) @ cb.T   # (B, n, K)
        flat = keys.reshape(B, n * K)
        err, order = torch.sort(flat, dim=1, stable=True)
        err, order = err[:, :W], order[:, :W]
        parent, code = torch.div(order, K, rounding_mode="floor"), order % K
        res = torch.gather(res, 1, parent.unsqueeze(-1).expand(B, W, D)) - cb[code]
        paths = torch.cat([torch.gather(paths, 1, parent.unsqueeze(-1).expand(B, W, l)), code.unsqueeze(-1)], 2)
    return paths, err, res
