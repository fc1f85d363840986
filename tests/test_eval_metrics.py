"""evaluate.metrics.TopKAccumulator on CPU tensors: the reference's results (tests/golden/topk_metrics.npz, recorded
from the reference's own class by tests/golden/make_golden_eval.py), a plain-loop brute force, and reduce() under
data parallelism (gloo, ranks that accumulated different numbers of batches)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from beam_support import free_port


def _batches(z):
    return [(torch.from_numpy(z["actual1"]), torch.from_numpy(z["topk1"])),
            (torch.from_numpy(z["actual2"]), torch.from_numpy(z["topk2"]))]


def brute_force_counts(actual, topk, ks):
    """{metric key: count} by plain loops over rows, columns and beams (the reference's definitions)."""
    actual, topk = np.asarray(actual), np.asarray(topk)
    B, D = actual.shape
    out = {}
    for i in range(D):
        for name, cols in ((f"slice_:{i + 1}", range(i + 1)), (f"pos_{i}", [i])):
            for k in ks:
                out.setdefault(f"h@{k}_{name}", 0)
            for b in range(B):
                rank = None
                for r in range(topk.shape[1]):
                    if all(topk[b, r, c] == actual[b, c] for c in cols):
                        rank = r
                        break
                for k in ks:
                    out[f"h@{k}_{name}"] += int(rank is not None and rank < k)
    return out


def test_matches_reference_fixture(golden):
    from evaluate.metrics import TopKAccumulator
    z = golden("topk_metrics")
    acc = TopKAccumulator(ks=[int(k) for k in z["ks"]])
    (a1, t1), (a2, t2) = _batches(z)
    acc.accumulate(actual=a1, top_k=t1)
    first = acc.reduce()
    assert list(first) == [str(k) for k in z["keys"]]
    assert list(first.values()) == z["values_first"].tolist()
    acc.accumulate(actual=a2, top_k=t2)   # k = 3 < max(ks)
    both = acc.reduce()
    assert list(both) == [str(k) for k in z["keys"]]
    assert list(both.values()) == z["values_both"].tolist()
    assert acc.total == 10
    acc.reset()
    acc.accumulate(actual=a2, top_k=t2)
    assert acc.total == 4 and acc.reduce()["h@1_slice_:4"] == 0.25


def test_matches_brute_force(golden):
    from evaluate.metrics import TopKAccumulator
    z = golden("topk_metrics")
    ks = [int(k) for k in z["ks"]]
    batches = _batches(z)
    g = torch.Generator().manual_seed(5)   # + a batch dense in chance matches: ids from {0, 1, 2}
    batches.append((torch.randint(0, 3, (17, 3), generator=g), torch.randint(0, 3, (17, 12, 3), generator=g)))
    for group in (batches[:2], batches[2:]):
        acc = TopKAccumulator(ks=ks)
        want, total = {}, 0
        for a, t in group:
            acc.accumulate(actual=a, top_k=t)
            for k_, v in brute_force_counts(a, t, ks).items():
                want[k_] = want.get(k_, 0) + v
            total += a.shape[0]
        got = acc.reduce()
        assert list(got) == list(want)
        assert got == {k_: v / total for k_, v in want.items()}


def test_planted_ranks(golden):
    """The fixture's planted cases, read off the counters: rows 0-4 match at ranks 0, 4, 5, 9, 10."""
    from evaluate.metrics import TopKAccumulator
    z = golden("topk_metrics")
    acc = TopKAccumulator(ks=[1, 5, 6, 10, 11, 21])
    acc.accumulate(*_batches(z)[0])
    m = acc.reduce()
    assert [round(m[f"h@{k}_slice_:4"] * 6) for k in acc.ks] == [1, 2, 3, 4, 5, 5]   # rank 20's copy never counts
    assert [round(m[f"h@{k}_slice_:2"] * 6) for k in (1, 5, 10)] == [1, 3, 4]        # ranks 0, 4, 5, 2 (row 3's prefix), 10
    assert round(m["h@10_pos_2"] * 6) == 5 and round(m["h@5_pos_2"] * 6) == 2        # row 5's column 2 at rank 7


def _dp_worker(rank, world, port, arrays, n_first, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        from evaluate.metrics import TopKAccumulator
        from rqvae_hip import dp
        dp.init_from_env(backend="gloo")
        batches = [(torch.from_numpy(a), torch.from_numpy(t)) for a, t in arrays]
        mine = batches[:n_first] if rank == 0 else batches[n_first:]
        acc = TopKAccumulator(ks=[1, 5, 10])
        for a, t in mine:
            acc.accumulate(actual=a, top_k=t)
        q.put((rank, acc.reduce()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("n_first", [1, 3])   # rank 0 / rank 1 batches: 1 / 2, and 3 / 0 (a rank without a batch)
def test_reduce_data_parallel(golden, n_first):
    from evaluate.metrics import TopKAccumulator
    z = golden("topk_metrics")
    arrays = [(z["actual1"], z["topk1"]), (z["actual2"], z["topk2"]), (z["actual1"][::-1].copy(), z["topk1"][:, :7].copy())]
    single = TopKAccumulator(ks=[1, 5, 10])
    for a, t in arrays:
        single.accumulate(actual=torch.from_numpy(a), top_k=torch.from_numpy(t))
    want = single.reduce()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, arrays, n_first, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0] == want and res[1] == want
    assert list(res[0]) == list(want)
