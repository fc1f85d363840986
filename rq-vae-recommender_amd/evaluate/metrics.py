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
"""
import torch
from torch import Tensor

_MAX_D = 64   # widest sem-ID tuple (the kernel's limit); the all-reduce buffer is laid out for it


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
