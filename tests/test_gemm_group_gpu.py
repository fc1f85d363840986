"""Grouped weight gradients (gemm_x3w_group_kernel, rq_gemm_bf16x3_group): the dW = g^T x problems of one
MLP chain in one wide-tile split-K launch, each member with its own split count over its share of the grid.

* small-integer operands (exact in bf16, every fp32 partial sum exact) give the fp64 product bit for bit
  for any partition: three members with edge tiles in M and in N, a half-empty tile, ragged last chunks
  and a leading dimension wider than the operand — the problem lookup, the per-problem tiles / split /
  chunk, the row clamps and the slab bases all show up exactly;
* with the split counts of the single-problem launches the grouped result equals theirs bitwise;
* two grouped runs agree bitwise (fixed summation order, no atomics);
* the fused chain's backward under grouping: within the split-bf16 bound of fp64 and of the ungrouped
  chain (RQ_GEMM_NO_GROUP), returned and direct-into-bucket gradients bitwise equal;
* rq_gemm_bf16x3_group_plan says what the run then does (the `gemm_group:` launches ops.TIMER records);
  nothing is grouped unless the caller asks (ops.group_wgrads() or explicit counts): the default path keeps every
  weight gradient's own partition and bits.

The shapes are the smallest at which the indexing can go wrong, not the workload's.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

K_RAGGED = 32 * 29
# (M, N, explicit S): 29 k steps in chunks of 10, 10, 9 / 8, 8, 8, 5 / 5 x 5 + 4 (x3_plan_s rounds S = 7 to 6 chunks)
MEMBERS = [(520, 256, 3), (256, 264, 4), (128, 256, 7)]


def _ops():
    from rqvae_hip import ops
    return ops


def _int_members(device, K=K_RAGGED, members=MEMBERS, pad=0):
    """(g, x) integer-valued operands per member; the first member's g is a column block of a wider buffer
    (ld != width) when pad > 0."""
    ops = _ops()
    gen = torch.Generator(device=device).manual_seed(11)
    out = []
    for i, (M, N, _) in enumerate(members):
        g = torch.randint(-8, 9, (K, M), generator=gen, device=device).float()
        x = torch.randint(-8, 9, (K, N), generator=gen, device=device).float()
        gs, xs = ops.split_bf16x3(g), ops.split_bf16x3(x)
        if i == 0 and pad:
            wide = [torch.zeros(K, M + pad, device=device, dtype=torch.bfloat16) for _ in range(2)]
            for w, pl in zip(wide, gs):
                w[:, :M] = pl
            gs = _Padded(wide[0], wide[1], M)
        out.append((g, x, gs, xs))
    return out


class _Padded:
    """Split planes whose rows are wider than the operand (leading dimension M + pad)."""

    def __init__(self, hi, lo, width):
        self.hi, self.lo, self.width = hi, lo, width


def _specs(ops, data, members, flags=0):
    specs = []
    for (g, x, gs, xs), (M, N, S) in zip(data, members):
        a = gs if not isinstance(gs, _Padded) else ops.Split(gs.hi, gs.lo)
        specs.append(dict(a=a, a_kcontig=False, b=xs, b_kcontig=False, M=M, N=N, K=g.shape[0],
                          flags=flags | ops.gemm_split(S)))
    return specs


def _group_keys(ops):
    return [k for k in ops.TIMER.events if k.startswith("gemm_group:")]


@pytest.fixture
def timer():
    ops = _ops()
    ops.TIMER.reset()
    ops.TIMER.enabled = True
    try:
        yield ops.TIMER
    finally:
        ops.TIMER.enabled = False
        ops.TIMER.reset()


def test_group_exact_on_integers(device):
    ops = _ops()
    data = _int_members(device, pad=24)
    assert data[0][2].hi.stride(0) == MEMBERS[0][0] + 24
    with ops.group_splits([s for _, _, s in MEMBERS]):
        plan = ops.gemm_group_choice([(m, n) for m, n, _ in MEMBERS], K_RAGGED)
    assert plan == [3, 4, 6], plan
    outs = ops.gemm_x3_group(_specs(ops, data, MEMBERS))
    for (g, x, _, _), out, (M, N, _) in zip(data, outs, MEMBERS):
        assert out.shape == (M, N)
        assert torch.equal(out.double(), g.double().t() @ x.double()), (M, N)


def test_group_same_partition_same_bits(device):
    """The single-problem wide launch and the grouped one with the same split counts: the same bits."""
    ops = _ops()
    K = 16384 + 32 * 5
    members = [(768, 512, 5), (512, 256, 9), (256, 512, 13)]
    gen = torch.Generator(device=device).manual_seed(12)
    data = []
    for M, N, _ in members:
        g = torch.randn(K, M, generator=gen, device=device)
        x = torch.randn(K, N, generator=gen, device=device)
        data.append((g, x, ops.split_bf16x3(g), ops.split_bf16x3(x)))
    with ops.group_splits([s for _, _, s in members]):
        assert all(s > 0 for s in ops.gemm_group_choice([(m, n) for m, n, _ in members], K))
    outs = ops.gemm_x3_group(_specs(ops, data, members))
    for (g, x, gs, xs), out, (M, N, S) in zip(data, outs, members):
        with ops.gemm_policy(ops.GEMM_FORCE_WIDE | ops.gemm_split(S)):
            assert ops.gemm_x3_choice(M, N, K, True, True, False, False)[0] == "wide"
            alone = ops.gemm_x3(gs, False, xs, False, M, N, K)
        assert torch.equal(out, alone), (M, N, S)
        ref = g.double().t() @ x.double()
        assert (out.double() - ref).abs().max() <= 1e-4 * ref.abs().max()


def test_group_repeatable(device):
    ops = _ops()
    gen = torch.Generator(device=device).manual_seed(13)
    data = []
    for M, N, _ in MEMBERS:
        g = torch.randn(K_RAGGED, M, generator=gen, device=device)
        x = torch.randn(K_RAGGED, N, generator=gen, device=device)
        data.append((g, x, ops.split_bf16x3(g), ops.split_bf16x3(x)))
    a = ops.gemm_x3_group(_specs(ops, data, MEMBERS))
    b = ops.gemm_x3_group(_specs(ops, data, MEMBERS))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


DIMS = [768, 512, 256, 128]
ROWS = 4096


def _chain_grads(ops, weights, x, gy, device):
    ws = [w.detach().clone().requires_grad_(True) for w in weights]
    xi = x.detach().clone().requires_grad_(True)
    ops.mlp_chain(xi, ws).backward(gy)
    return [w.grad for w in ws], xi.grad


@pytest.fixture
def split_input(monkeypatch):
    """The chain input split up front, as at the RQ-VAE batch (there _presplit_input says yes by itself): the
    first layer's weight gradient then has two split operands and can join the group."""
    monkeypatch.setattr(_ops(), "_presplit_input", lambda rows, weights, n: True)


def test_group_chain_backward(device, split_input, timer):
    ops = _ops()
    torch.set_float32_matmul_precision("high")
    try:
        gen = torch.Generator(device=device).manual_seed(14)
        weights = [torch.randn(o, i, generator=gen, device=device) / i ** 0.5 for i, o in zip(DIMS[:-1], DIMS[1:])]
        x = torch.randn(ROWS, DIMS[0], generator=gen, device=device)
        gy = torch.randn(ROWS, DIMS[-1], generator=gen, device=device)
        # the two layers whose g and input are both split planes (the last layer's g is fp32 here)
        shapes = [(256, 512), (512, 768)]
        with ops.group_splits(4):
            assert ops.gemm_group_choice(shapes, ROWS) == [4, 4]
            dws, dx = _chain_grads(ops, weights, x, gy, device)
            assert len(_group_keys(ops)) == 1 and len(timer.events[_group_keys(ops)[0]]) == 1
        timer.reset()
        with ops.gemm_policy(ops.GEMM_NO_GROUP):
            dws0, dx0 = _chain_grads(ops, weights, x, gy, device)
            assert not _group_keys(ops)
        assert torch.equal(dx, dx0)   # the data gradients do not depend on the grouping

        # fp64 chain
        wr = [w.double().requires_grad_(True) for w in weights]
        h = x.double()
        for j, w in enumerate(wr):
            h = h @ w.t()
            if j < len(wr) - 1:
                h = torch.nn.functional.silu(h)
        h.backward(gy.double())

        def close(a, b):
            return (a.double() - b).abs().max() <= 1e-4 * b.abs().max() + 1e-7
        for j in range(len(weights)):
            assert close(dws[j], wr[j].grad), j
            assert close(dws[j], dws0[j].double()), j
    finally:
        torch.set_float32_matmul_precision("highest")


class _Chain(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from modules.encoder import MLP
        self.mlp = MLP(DIMS[0], DIMS[1:-1], DIMS[-1])

    def forward(self, x):
        return self.mlp(x)


def test_group_direct_grad_equals_returned(device, split_input, timer):
    """Grouped weight gradients added into flat buckets (deferred reduction) and returned to autograd."""
    from rqvae_hip import dp
    ops = _ops()
    torch.set_float32_matmul_precision("high")
    try:
        torch.manual_seed(15)
        a = _Chain().to(device)
        b = copy.deepcopy(a)
        buckets = dp.GradBuckets(b.parameters(), overlap=False, flat_views=True)
        gen = torch.Generator(device=device).manual_seed(16)
        x = torch.randn(ROWS, DIMS[0], generator=gen, device=device)
        g = torch.randn(ROWS, DIMS[-1], generator=gen, device=device)
        with ops.group_splits(4):
            a(x).backward(g)
            assert len(_group_keys(ops)) == 1
            buckets.zero_grad()
            b(x).backward(g)
            buckets.synchronize()
            assert sum(len(timer.events[k]) for k in _group_keys(ops)) == 2
        for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(pa.grad, pb.grad), n
    finally:
        torch.set_float32_matmul_precision("highest")


def test_group_plan_twin(device, split_input, timer):
    """rq_gemm_bf16x3_group_plan against the run: no grouped launch by default nor when the model, asked with
    group_wgrads(), declines this chain at 4,096 rows; one under explicit counts; never under RQ_GEMM_NO_GROUP."""
    ops = _ops()
    torch.set_float32_matmul_precision("high")
    try:
        gen = torch.Generator(device=device).manual_seed(17)
        weights = [torch.randn(o, i, generator=gen, device=device) / i ** 0.5 for i, o in zip(DIMS[:-1], DIMS[1:])]
        x = torch.randn(ROWS, DIMS[0], generator=gen, device=device)
        gy = torch.randn(ROWS, DIMS[-1], generator=gen, device=device)
        shapes = [(256, 512), (512, 768)]
        for ctx, policy in ((ops.group_splits(None), 0), (ops.group_wgrads(), 0),
                            (ops.group_splits(6), 0), (ops.group_splits(6), ops.GEMM_NO_GROUP)):
            timer.reset()
            with ctx, ops.gemm_policy(policy):
                plan = ops.gemm_group_choice(shapes, ROWS)
                _chain_grads(ops, weights, x, gy, device)
                launches = sum(len(timer.events[k]) for k in _group_keys(ops))
            assert launches == (1 if any(plan) else 0), (plan, launches)
            if policy == ops.GEMM_NO_GROUP or ctx.key == "plan" or ctx.flags is None:
                assert not any(plan), plan
            else:
                assert plan == [6, 6], plan
        # the workload's chain at its batch: the model groups the three wide layers and leaves the 128 x 64
        # layer out; _mlp_backward takes that plan only inside group_wgrads()
        chain = [(768, 512), (512, 256), (256, 128), (128, 64)]
        assert ops.gemm_group_choice(chain, 65536)[3] == 0
        assert all(s > 1 for s in ops.gemm_group_choice(chain[:3], 65536))
        with ops.gemm_policy(ops.GEMM_NO_GROUP):
            assert not any(ops.gemm_group_choice(chain, 65536))
    finally:
        torch.set_float32_matmul_precision("highest")
