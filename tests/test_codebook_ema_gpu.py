"""EMA-maintained codebooks on the device: rq_codebook_ema_stats in every form the plan reports and
rq_codebook_ema_apply against the fp64 reference (codebook_ema_support: the rule, the case table, the bounds), and
RqVae.use_ema_codebooks through a training step — eager, with micro-batches, and captured."""
import numpy as np
import pytest
import torch

import codebook_ema_support as S

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def _stats(case, device, n0=None, s0=None):
    from rqvae_hip import ops
    n = _dev(case["n0"] if n0 is None else n0, device)
    s = _dev(case["s0"] if s0 is None else s0, device)
    ops.codebook_ema_stats(_dev(case["res"], device), _dev(case["ids"], device), n, s)
    return n.cpu().numpy(), s.cpu().numpy()


# ---------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", [c[0] for c in S.STATS_CASES])
def test_stats_match_reference_and_repeat_bitwise(name, device):
    case = S.stats_case(name)
    n1, s1 = _stats(case, device)
    S.check_stats(case, n1, s1)
    n2, s2 = _stats(case, device)
    assert np.array_equal(n1, n2) and s1.tobytes() == s2.tobytes()   # the same inputs give the same bits
    if name == "empty":
        assert s1.tobytes() == case["s0"].tobytes()


def test_case_table_reaches_every_form(device):
    from rqvae_hip import ops
    forms = {name: ops.codebook_ema_stats_plan(B, D, K, L).form for name, B, D, K, L, _ in S.STATS_CASES}
    assert set(forms.values()) == {0, 1, 2}   # RQ_EMA_STATS_NONE / LDS / TILED: every form the library has
    assert forms["ml32m"] == 1 and forms["tiled"] == 2 and forms["wide"] == 1 and forms["empty"] == 0
    p = ops.codebook_ema_stats_plan(2500, 512, 4096, 1)
    assert p.rows_per_chunk > 1024 and p.chunks == 2   # "subblocks": a workgroup walks several id sub-blocks


def test_two_calls_accumulate(device):
    a, b = S.stats_case("ml32m"), S.stats_case("second")
    n1, s1 = _stats(a, device)
    n2, s2 = _stats(b, device, n0=n1, s0=s1)
    S.check_stats(b, n2, s2, n0=n1, s0=s1)
    want = a["s0"].astype(np.float64) + a["s"] + b["s"]   # the fp64 sum of both batches
    bound = S.U * (a["n"][:, :, None] * a["a"] + b["n"][:, :, None] * b["a"] + np.abs(s1) + np.abs(want))
    assert np.array_equal(n2, a["n0"] + a["n"] + b["n"])
    assert (np.abs(s2.astype(np.float64) - want) <= bound).all()


@pytest.mark.parametrize("name", [c[0] for c in S.APPLY_CASES])
def test_apply_matches_reference(name, device):
    from rqvae_hip import ops
    c = S.apply_case(name)
    w = [torch.full((c["K"], c["D"]), float("nan"), device=device) for _ in range(c["L"])]
    N, Sx, n, s = (_dev(c[k], device) for k in ("N0", "S0", "n", "s"))
    ops.codebook_ema_apply(w, N, Sx, n, s, c["decay"], c["eps"])
    S.check_apply(c["N0"], c["S0"], c["n"], c["s"], c["decay"], c["eps"], N.cpu().numpy(), Sx.cpu().numpy(),
                  torch.stack(w).cpu().numpy(), n.cpu().numpy(), s.cpu().numpy())


def test_argument_errors(device):
    from rqvae_hip import ops
    w = [torch.zeros(4, 8, device=device)]
    st = (torch.ones(1, 4, device=device), torch.zeros(1, 4, 8, device=device),
          torch.zeros(1, 4, dtype=torch.int64, device=device), torch.zeros(1, 4, 8, device=device))
    for decay, eps in ((1.0, 1e-5), (-0.1, 1e-5), (0.5, 0.0)):
        with pytest.raises(ValueError):
            ops.codebook_ema_apply(w, *st, decay, eps)
    with pytest.raises(ValueError, match="res"):
        ops.codebook_ema_stats(torch.zeros(1, 3, 8, device=device), torch.zeros(2, 1, dtype=torch.int64, device=device),
                               st[2], st[3])


# ------------------------------------------------------------------------------------------ the model
_INP, _HID, _D, _K, _L, _B = 32, [32], 8, 16, 2, 256
MODES = ["STE", "ROTATION_TRICK"]


def _model(device, mode, ema=True, seed=0):
    from modules.quantize import QuantizeForwardMode
    from modules.rqvae import RqVae
    torch.manual_seed(seed)
    m = RqVae(input_dim=_INP, embed_dim=_D, hidden_dims=_HID, codebook_size=_K, codebook_kmeans_init=False,
              codebook_mode=QuantizeForwardMode[mode], n_layers=_L, n_cat_features=0).to(device).train()
    with torch.no_grad():   # codebooks at the scale of the encoder's outputs: several codes per level are in use
        for layer in m.layers:
            layer.embedding.weight.mul_(0.2)
    if ema:
        m.use_ema_codebooks(decay=0.9, eps=1e-5)
    return m


def _x(device, seed, rows=_B):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, _INP, generator=g).to(device)


def _batch(x):
    from data.schemas import SeqBatch
    return SeqBatch(None, None, None, x, None, None)


def _levels(m, x):
    """(res (L, B, D), ids (B, L)) a training forward of x sees under the current weights, as numpy."""
    with torch.no_grad():
        out = m.quantize_levels(m.encode(x), 0.2)
    return out[1].cpu().numpy(), out[2].cpu().numpy()


def _weights(m):
    return torch.stack([l.embedding.weight.detach() for l in m.layers]).cpu().numpy()


def _check_update(m, batches, W0, decay=0.9, eps=1e-5):
    """After forwards on `batches` (their (res, ids) given) and one ema_update from the initial state N = 1, S = W0:
    the accumulated statistics within the summation bound (taken before the update), then the rule."""
    res = np.concatenate([r for r, _ in batches], 1)
    ids = np.concatenate([i for _, i in batches], 0)
    n, s, a = S.stats_ref(res, ids, _K)
    n_got, s_got = m.ema["n"].cpu().numpy(), m.ema["s"].cpu().numpy()
    assert np.array_equal(n_got, n) and (n > 0).sum() > _L   # more than one code per level on average
    # one fp32 add per batch into the accumulator on top of the rows' sum
    assert (np.abs(s_got - s) <= n[:, :, None] * S.U * a + len(batches) * S.U * np.abs(s)).all()
    m.ema_update()
    e = m.ema
    S.check_apply(np.ones((_L, _K), np.float32), W0, n_got, s_got, decay, eps, e["N"].cpu().numpy(),
                  e["S"].cpu().numpy(), _weights(m), e["n"].cpu().numpy(), e["s"].cpu().numpy())


@pytest.mark.parametrize("mode", MODES)
def test_step_leaves_codebooks_to_the_ema_rule(mode, device):
    from rqvae_hip import optim as hip_optim
    m = _model(device, mode)
    opt = hip_optim.AdamW(m.parameters(), lr=1e-2, weight_decay=0.1)   # the codebooks included: it must skip them
    x = _x(device, 1)
    W0, enc0 = _weights(m), m.encoder.mlp[0].weight.detach().clone()
    levels = _levels(m, x)
    out = m(_batch(x), gumbel_t=0.2)
    out.loss.backward()
    assert all(l.embedding.weight.grad is None for l in m.layers)
    assert m.encoder.mlp[0].weight.grad is not None and torch.isfinite(out.rqvae_loss)
    opt.step()
    assert _weights(m).tobytes() == W0.tobytes()   # neither the update nor the weight decay touched them
    assert not torch.equal(m.encoder.mlp[0].weight.detach(), enc0)
    m.eval()
    with torch.no_grad():
        m(_batch(x), gumbel_t=0.2)   # eval forwards do not accumulate
    m.train()
    _check_update(m, [levels], W0)
    assert _weights(m).tobytes() != W0.tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_micro_batches_add_up_before_one_update(mode, device):
    """Two micro-batches before one ema_update() equal one update on their union: the fp64 rule on the concatenation
    of the (res, ids) the two forwards saw, within the bound."""
    m = _model(device, mode)
    x = _x(device, 2)
    W0 = _weights(m)
    halves = [x[:100], x[100:]]
    levels = [_levels(m, h) for h in halves]
    for h in halves:
        (m(_batch(h), gumbel_t=0.2).loss / 2).backward()
    _check_update(m, levels, W0)


@pytest.mark.parametrize("mode", MODES)
def test_captured_step_gives_the_eager_bits(mode, device):
    from rqvae_hip import dp
    from rqvae_hip import optim as hip_optim
    from rqvae_hip.graph import GraphedSteps
    xs = [_x(device, 10 + i) for i in range(4)]

    def run(graphed):
        m = _model(device, mode)
        params = [p for p in m.parameters() if p.requires_grad]
        buckets = dp.GradBuckets(params, overlap=False, flat_views=True)
        assert all(id(l.embedding.weight) not in {id(p) for p in buckets.params} for l in m.layers)
        opt = hip_optim.AdamW(params, lr=1e-2, weight_decay=0.01)
        gs = GraphedSteps(lambda x: m(_batch(x), gumbel_t=0.2).loss, lambda x: 0, buckets,
                          after_warmup=m.ema_discard_stats) if graphed else None
        trace = []
        for x in xs:
            if gs is not None:
                loss = gs(x).clone()
            else:
                buckets.zero_grad()
                loss = m(_batch(x), gumbel_t=0.2).loss
                loss.backward()
                loss = loss.detach()
            buckets.synchronize()
            opt.step()
            m.ema_update()
            trace.append((loss.cpu().numpy().tobytes(), _weights(m).tobytes(), m.ema["N"].cpu().numpy().tobytes(),
                          m.ema["S"].cpu().numpy().tobytes()))
        if gs is not None:
            assert len(gs.graphs) == 1 and gs.eager_steps == 1   # the statistics launches did not break the capture
        return trace

    eager, graphed = run(False), run(True)
    assert len({t[1] for t in eager}) == len(xs)   # the codebooks moved at every step
    for i, (e, g) in enumerate(zip(eager, graphed)):
        assert e == g, i


@pytest.mark.parametrize("mode", MODES)
def test_model_without_ema_is_untouched(mode, device, monkeypatch):
    """Without use_ema_codebooks() a step makes no EMA launch, keeps no EMA state and trains the codebooks by their
    gradient as before: the same seed gives the same bits whether or not the EMA ops could be called at all."""
    from rqvae_hip import ops
    from rqvae_hip import optim as hip_optim

    def step(m):
        opt = hip_optim.AdamW(m.parameters(), lr=1e-2, weight_decay=0.01)
        out = m(_batch(_x(device, 3)), gumbel_t=0.2)
        out.loss.backward()
        grads = [l.embedding.weight.grad.clone() for l in m.layers]
        opt.step()
        return out.loss.detach().cpu().numpy().tobytes(), _weights(m).tobytes(), grads

    first = step(_model(device, mode, ema=False))

    def refuse(*a, **k):
        raise AssertionError("an EMA op ran in a model without use_ema_codebooks()")
    monkeypatch.setattr(ops, "codebook_ema_stats", refuse)
    monkeypatch.setattr(ops, "codebook_ema_apply", refuse)
    m = _model(device, mode, ema=False)
    second = step(m)
    assert first[:2] == second[:2] and m.ema is None
    assert all(g is not None and bool(g.abs().sum() > 0) for g in second[2])
    assert all(l.embedding.weight.requires_grad for l in m.layers)
