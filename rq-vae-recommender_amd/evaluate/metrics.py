"""Hit@k accumulator — drop-in for reference evaluate/metrics.py (TopKAccumulator :6-31: same constructor,
reset / accumulate / reduce, same metric keys).

Per batch and per sem-ID column i the reference looks for the first beam whose columns 0..i equal the target's
(`h@{k}_slice_:{i+1}`) and the first beam equal in column i alone (`h@{k}_pos_{i}`), and counts the rows where
that beam's rank is below k. It reads each of its 2 * D * len(ks) counts back to the host per batch (`len(...)`
of a masked tensor). Here the counters are one int64 tensor (2, D, len(ks)):
  * device tensors: accumulate is one HIP launch (rqvae_hip.ops.topk_hits) into device counters, no host read;
    reduce() does the single read;
  * CPU tensors: the same counts with plain torch (module drop-in contract).
Under data parallelism reduce() sums the counters and the row total over the ranks with ONE all-reduce; ranks
may have accumulated different numbers of batches (also none).

RankAccumulator (this build's addition; the reference has only Hit@k): Recall@k, NDCG@k and MRR@k of a ranked list
against ONE relevant target per row, all derived from the histogram of the target's first-match rank — item ids
(model.recommend) or whole sem-ID tuples. Same split: one HIP launch per batch on the device
(rqvae_hip.ops.rank_hist), plain torch on the CPU, one host read and one all-reduce in reduce().

ranked_candidates turns the per-candidate ranks of model.score_items into the ranked list RankAccumulator(width=C)
takes (the sampled-negatives protocol: 1 positive + N negatives, the rank of the positive).
"""
import math

import torch
from torch import Tensor

_MAX_D = 64   # widest sem-ID tuple (the kernel's limit); the all-reduce buffer is laid out for it


def ranked_candidates(items: Tensor, rank: Tensor) -> Tensor:
    """(B, C): the candidates `items` (B, C) in rank order — out[b, rank[b, c]] = items[b, c] for `rank` (B, C), a
    permutation of 0..C-1 per row (model.score_items). One scatter; CPU or device tensors."""
    if items.dim() != 2 or items.shape != rank.shape:
        raise ValueError(f"need items (B, C) and rank (B, C), got {tuple(items.shape)}, {tuple(rank.shape)}")
    return torch.empty_like(items).scatter_(1, rank.to(torch.int64), items)


class TopKAccumulator:
    def __init__(self, ks=[1, 5, 10]):
        self.ks = ks
        self.reset()

    def reset(self):
        self.total = 0
        self.counts = None   # (2, D, len(ks)) int64: [0] slices, [1] positions

    def _cpu_counts(self, actual: Tensor, top_k: Tensor) -> Tensor:
        B, D = actual.shape
        k = top_k.shape[1]
        pos = actual.unsqueeze(1) == top_k                           # (B, k, D)
        ranks = torch.arange(k).view(1, k, 1)
        none = torch.iinfo(torch.int64).max

        def first(match):                                            # first matching rank per (row, column)
            return torch.where(match, ranks, torch.full_like(ranks, none)).min(dim=1).values   # (B, D)
        r = torch.stack([first(pos.long().cumprod(-1).bool()), first(pos)])                     # (2, B, D)
        ks = torch.tensor([int(v) for v in self.ks], dtype=torch.int64)
        return (r.unsqueeze(-1) < ks).sum(dim=1)                     # (2, D, n_ks)

    def accumulate(self, actual: Tensor, top_k: Tensor) -> None:
        B, D = actual.shape
        if D > _MAX_D:
            raise ValueError(f"sem-ID tuples wider than {_MAX_D} are not supported")
        if self.counts is None:
            self.counts = torch.zeros((2, D, len(self.ks)), dtype=torch.int64, device=actual.device)
        if actual.is_cuda:
            from rqvae_hip import ops as hip_ops
            hip_ops.topk_hits(actual.contiguous(), top_k.contiguous(), self.ks, self.counts)
        else:
            self.counts += self._cpu_counts(actual, top_k)
        self.total += B

    def reduce(self) -> dict:
        import torch.distributed as dist
        counts, total = self.counts, self.total
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            # one buffer: the counters padded to _MAX_D columns, the row total, and (D, 1) of the ranks that
            # saw a batch — a rank without one does not know D
            n_ks = len(self.ks)
            if counts is not None:
                dev = counts.device
            else:
                dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else "cpu"
            buf = torch.zeros(2 * _MAX_D * n_ks + 3, dtype=torch.int64, device=dev)
            if counts is not None:
                D = counts.shape[1]
                buf[:2 * _MAX_D * n_ks].view(2, _MAX_D, n_ks)[:, :D] = counts
                buf[-3:] = torch.tensor([total, D, 1], dtype=torch.int64).to(dev)
            dist.all_reduce(buf)
            host = buf.cpu()
            total, d_sum, seen = (int(v) for v in host[-3:])
            D = d_sum // seen if seen else 0
            counts = host[:2 * _MAX_D * n_ks].view(2, _MAX_D, n_ks)[:, :D]
        if counts is None:
            return {}
        c = counts.tolist()   # the one host read
        out = {}
        for i in range(len(c[0])):
            for t, name in ((0, f"slice_:{i + 1}"), (1, f"pos_{i}")):
                for j, k in enumerate(self.ks):
                    out[f"h@{k}_{name}"] = c[t][i][j] / total
        return out


class RankAccumulator:
    """First-match rank histogram -> recall@k / ndcg@k / mrr@k for k in `ks`.

    accumulate(actual, top_k): actual (B,) with top_k (B, k) item ids, or (B, D) with (B, k, D) tuples, k <= width.
    A row's rank is the index of its first beam equal to the target in every column; rows whose target starts with a
    negative id (no target) are skipped, a dead beam (-1) never equals a target. With one relevant item the ideal
    DCG is 1, so per row recall@k = [rank < k], ndcg@k = [rank < k] / log2(rank + 2), mrr@k = [rank < k] / (rank + 1).
    One int64 histogram (k + 1: ranks, then the misses) per distinct k seen, allocated on its first batch; reduce()
    folds them into the fixed (width + 1) vector (ranks 0..width-1, misses) that is all-reduced and read once."""

    def __init__(self, ks=[1, 5, 10], width: int = 32):
        self.ks = ks
        self.width = int(width)
        self.reset()

    def reset(self):
        self.hists = {}   # k -> (k + 1) int64

    @staticmethod
    def _cpu_hist(actual: Tensor, top_k: Tensor) -> Tensor:
        k = top_k.shape[1]
        match = (actual.unsqueeze(1) == top_k).all(-1)                                  # (B, k)
        ranks = torch.arange(k).view(1, k)
        rank = torch.where(match, ranks, torch.full_like(ranks, k)).min(dim=1).values    # k: no beam matched
        return torch.bincount(rank[actual[:, 0] >= 0], minlength=k + 1)

    def accumulate(self, actual: Tensor, top_k: Tensor) -> None:
        if actual.dim() == 1 and top_k.dim() == 2:
            actual, top_k = actual.unsqueeze(-1), top_k.unsqueeze(-1)
        if actual.dim() != 2 or top_k.dim() != 3 or top_k.shape[0] != actual.shape[0] or top_k.shape[2] != actual.shape[1]:
            raise ValueError(f"need actual (B,) / (B, D) and top_k (B, k) / (B, k, D), got {tuple(actual.shape)}, "
                             f"{tuple(top_k.shape)}")
        k = top_k.shape[1]
        if not 1 <= k <= self.width:
            raise ValueError(f"top_k holds {k} beams, the accumulator was built for 1..{self.width}")
        if actual.shape[1] > _MAX_D:
            raise ValueError(f"sem-ID tuples wider than {_MAX_D} are not supported")
        if k not in self.hists:
            self.hists[k] = torch.zeros(k + 1, dtype=torch.int64, device=actual.device)
        if actual.is_cuda:
            from rqvae_hip import ops as hip_ops
            hip_ops.rank_hist(actual.to(torch.int64).contiguous(), top_k.to(torch.int64).contiguous(), self.hists[k])
        else:
            self.hists[k] += self._cpu_hist(actual, top_k)

    def reduce(self) -> dict:
        import torch.distributed as dist
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if not self.hists and not multi:
            return {}
        if self.hists:
            dev = next(iter(self.hists.values())).device
        else:
            dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else "cpu"
        hist = torch.zeros(self.width + 1, dtype=torch.int64, device=dev)
        for k, h in self.hists.items():
            hist[:k] += h[:k]
            hist[self.width] += h[k]
        if multi:
            dist.all_reduce(hist)
        c = hist.tolist()   # the one host read
        total = sum(c)
        if total == 0:
            return {}
        out = {}
        for k in self.ks:
            top = c[:min(int(k), self.width)]
            out[f"recall@{k}"] = math.fsum(top) / total
            out[f"ndcg@{k}"] = math.fsum(n / math.log2(r + 2) for r, n in enumerate(top)) / total
            out[f"mrr@{k}"] = math.fsum(n / (r + 1) for r, n in enumerate(top)) / total
        return out
