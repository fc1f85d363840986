"""Every instantiated width and regime of the row-wise kernels (csrc/rowwise.hip) against the fp64 references of
tests/rowwise_support.py: the sixteen VPL instantiations of the nine width-switched families at two widths each (one
live lane in the last vector slot, the slot full), the 8- and 16-row regimes of the fork's backward, the fix kernel's
row-stride loop; the loss head on both sides of its staging limit, at K below, at and above a wave, with large logits,
a padded row stride, dead sequences and positions, single upstream gradients and an out-of-range target; the Gumbel
kernels at their largest K and D, below a wave of codes and on exact ties; rq_col_sum's order, bitwise; the narrow lane
groupings of rq_row_norms are in test_rowwise_stats_gpu.py.

Bounds are the existing tests' (test_rowwise_gpu.py, test_rmsnorm_fork_gpu.py, test_ce_loss_gpu.py,
test_gumbel_gpu.py), now against fp64; each test prints its figures before it asserts.
Largest errors measured on an MI355X, as a share of the scale in each bound:
  RMSNorm (single and fork)  y 1.4e-7, gx 9.7e-8 of the maximum, gw 2.0e-7 of sum_b |gy x rstd|      (bound 2e-5)
  l2norm + reconstruction    recon 1.8 % and g_pre 1.6 % of rtol 1e-5 / 1e-4 + atol; g_pre 2.7e-7 of the row maximum
  loss head                  dX 2.0e-7 of max |dX| (x40 case 1.8e-7); loss_d 9.3e-6 absolute at values near 100
  Gumbel                     emb 5.4e-5, loss 1.3e-5, grad_x 1.2e-4, grad_codebook 1.6e-4 of the maximum   (bound 3e-4)
  rq_col_sum                 6.0e-8 of sum|P| from fp64                                                  (bound 1e-6)"""
import numpy as np
import pytest
import torch

import rowwise_support as S

pytestmark = pytest.mark.gpu

_NAN = float("nan")


def _ops():
    from rqvae_hip import ops
    return ops


def _h(device):
    from rqvae_hip._lib import ptr, stream_handle
    return ptr, stream_handle(device)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _within(got, ref, scale, what, rel=2e-5, floor=1e-7):
    err = (got.double().cpu() - ref).abs()
    worst = float((err / (scale + 1e-300)).max())
    print(f"  {what}: max |err| {float(err.max()):.3e}, {worst:.2e} of its scale")
    assert bool((err <= rel * scale + floor).all()), (what, float(err.max()), worst)


# ------------------------------------------------------------------------------------------------ A. width sweep
def _rms_fwd(device, x, w, p=0.0, seed=0):
    ptr, s = _h(device)
    B, D = x.shape
    y, rstd = torch.full_like(x, _NAN), torch.full((B,), _NAN, device=device)
    _ops().call("rq_rmsnorm_dropout_fwd", ptr(x), ptr(w), B, D, S.RMS_EPS, p, seed, ptr(y), ptr(rstd), s)
    return y, rstd


def _rms_bwd(device, x, w, rstd, gy, gres, p=0.0, seed=0):
    ptr, s = _h(device)
    ops = _ops()
    B, D = x.shape
    nb = ops._lib.load().rq_rmsnorm_bwd_workspace(B, D)
    ws = torch.empty(nb, device=device, dtype=torch.uint8)
    gx, gw = torch.full_like(x, _NAN), torch.full((D,), _NAN, device=device)
    ops.call("rq_rmsnorm_dropout_bwd", ptr(x), ptr(w), ptr(rstd), ptr(gy), ptr(gres), B, D, p, seed, ptr(gx), ptr(gw), 0,
             0, None, ptr(ws), nb, s)
    return gx, gw


def _rms2_fwd(device, x, w1, w2, p1=0.0, seed1=0, p2=0.0, seed2=0):
    ptr, s = _h(device)
    B, D = x.shape
    y1, y2, rstd = torch.full_like(x, _NAN), torch.full_like(x, _NAN), torch.full((B,), _NAN, device=device)
    _ops().call("rq_rmsnorm2_dropout_fwd", ptr(x), ptr(w1), ptr(w2), B, D, S.RMS_EPS, p1, seed1, p2, seed2, ptr(y1),
                ptr(y2), ptr(rstd), s)
    return y1, y2, rstd


def _rms2_bwd(device, x, w1, w2, rstd, gy1, gy2, gres, p1=0.0, seed1=0, p2=0.0, seed2=0):
    ptr, s = _h(device)
    ops = _ops()
    B, D = x.shape
    nb = 2 * ops._lib.load().rq_rmsnorm_bwd_workspace(B, D)
    ws = torch.empty(nb, device=device, dtype=torch.uint8)
    gx, gw1, gw2 = torch.full_like(x, _NAN), torch.full((D,), _NAN, device=device), torch.full((D,), _NAN, device=device)
    ops.call("rq_rmsnorm2_dropout_bwd", ptr(x), ptr(w1), ptr(w2), ptr(rstd), ptr(gy1), ptr(gy2), ptr(gres), B, D, p1,
             seed1, p2, seed2, ptr(gx), ptr(gw1), ptr(gw2), 0, 0, None, ptr(ws), nb, s)
    return gx, gw1, gw2


def _sweep(device, B, D):
    d = S.sweep_inputs(B, D)
    return d, S.SweepData(*(t.to(device) for t in d))


@pytest.mark.parametrize("D", S.WIDTHS)
def test_rmsnorm_width_vs_fp64(device, D):
    """rmsnorm_fwd_kernel<VPL> / rmsnorm_bwd_kernel<VPL> at p = 0 with gres: y, gx within 2e-5 max|fp64| + 1e-7, gw
    within 2e-5 sum_b |gy x rstd| + 1e-7 (test_rmsnorm_fused_matches_fp64's bounds)."""
    print(f"\n[rms] D {D} VPL {S.vpl(D)}")
    d, g = _sweep(device, S.SWEEP_ROWS, D)
    ref = S.rmsnorm_ref64(d.x, [d.w1], S.RMS_EPS, [d.gy1], d.gres)
    y, rstd = _rms_fwd(device, g.x, g.w1)
    gx, gw = _rms_bwd(device, g.x, g.w1, rstd, g.gy1, g.gres)
    _within(y, ref.ys[0], ref.ys[0].abs().max(), "y")
    _within(gx, ref.gx, ref.gx.abs().max(), "gx")
    _within(gw, ref.gws[0], ref.gw_scales[0], "gw")


def _check_rms2(device, B, D):
    d, g = _sweep(device, B, D)
    ref = S.rmsnorm_ref64(d.x, [d.w1, d.w2], S.RMS_EPS, [d.gy1, d.gy2], d.gres)
    y1, y2, rstd = _rms2_fwd(device, g.x, g.w1, g.w2)
    gx, gw1, gw2 = _rms2_bwd(device, g.x, g.w1, g.w2, rstd, g.gy1, g.gy2, g.gres)
    _within(y1, ref.ys[0], ref.ys[0].abs().max(), "y1")
    _within(y2, ref.ys[1], ref.ys[1].abs().max(), "y2")
    _within(gx, ref.gx, ref.gx.abs().max(), "gx")
    _within(gw1, ref.gws[0], ref.gw_scales[0], "gw1")
    _within(gw2, ref.gws[1], ref.gw_scales[1], "gw2")
    # under dropout: bitwise the chained single-norm launches, gx = norm2'(g2) + (norm1'(g1) + gres)
    p1, s1, p2, s2 = 0.1, 1234, 0.5, 98765
    y1, y2, rstd = _rms2_fwd(device, g.x, g.w1, g.w2, p1, s1, p2, s2)
    gx, gw1, gw2 = _rms2_bwd(device, g.x, g.w1, g.w2, rstd, g.gy1, g.gy2, g.gres, p1, s1, p2, s2)
    c1, r1 = _rms_fwd(device, g.x, g.w1, p1, s1)
    c2, r2 = _rms_fwd(device, g.x, g.w2, p2, s2)
    cx1, cw1 = _rms_bwd(device, g.x, g.w1, r1, g.gy1, g.gres, p1, s1)
    cx, cw2 = _rms_bwd(device, g.x, g.w2, r2, g.gy2, cx1, p2, s2)
    for name, a, b in (("y1", y1, c1), ("y2", y2, c2), ("rstd", rstd, r1), ("rstd2", rstd, r2), ("gx", gx, cx),
                       ("gw1", gw1, cw1), ("gw2", gw2, cw2)):
        assert _same(a, b), f"{name}: the dual launch differs from the chained single-norm launches"
    if B * D >= 1024:    # the masks drew: about p of each output is zero
        assert 0.05 < float((y1 == 0).float().mean()) < 0.15 and 0.4 < float((y2 == 0).float().mean()) < 0.6


@pytest.mark.parametrize("D", S.WIDTHS)
def test_rmsnorm2_width_vs_fp64_and_chained(device, D):
    """rmsnorm2_fwd_kernel<VPL> / rmsnorm2_bwd_kernel<VPL>: at p = 0 the single norm's fp64 bounds for both outputs, the
    summed input gradient and both weight gradients; at (p1, p2) = (0.1, 0.5) every output bitwise the chained
    single-norm launches (test_rmsnorm_fork_dual_kernel_bitwise's claim, through the C ABI)."""
    print(f"\n[rms2] D {D} VPL {S.vpl(D)}")
    _check_rms2(device, S.SWEEP_ROWS, D)


@pytest.mark.parametrize("B,D", S.RMS2_REGIME_CASES)
def test_rmsnorm2_row_regimes(device, B, D):
    """The same two checks where the backward walks 8 and 16 rows per workgroup (two and four per wave)."""
    assert S.rms_rows(B) in (8, 16)
    assert _ops()._lib.load().rq_rmsnorm_bwd_workspace(B, D) == -(-B // S.rms_rows(B)) * D * 4
    print(f"\n[rms2] B {B} D {D} rows per workgroup {S.rms_rows(B)}")
    _check_rms2(device, B, D)


def _l2r_fwd(device, pre, x, gs=None):
    ptr, s = _h(device)
    B, C = pre.shape
    recon, norms = torch.full((B,), _NAN, device=device), torch.full((B,), _NAN, device=device)
    if gs is None:
        _ops().call("rq_l2norm_recon_fwd", ptr(pre), ptr(x), B, C, ptr(recon), ptr(norms), s)
        return recon, norms
    hi, lo = _planes(device, B, C)
    _ops().call("rq_l2norm_recon_fwd_grad", ptr(pre), ptr(x), B, C, ptr(recon), ptr(norms), gs, ptr(hi), ptr(lo), s)
    return recon, norms, hi, lo


_SENTINEL = -77.0


def _planes(device, B, C):
    return (torch.full((B, C), _SENTINEL, device=device, dtype=torch.bfloat16),
            torch.full((B, C), _SENTINEL, device=device, dtype=torch.bfloat16))


def _l2r_bwd_split(device, pre, x, norms, g):
    ptr, s = _h(device)
    B, C = pre.shape
    hi, lo = _planes(device, B, C)
    _ops().call("rq_l2norm_recon_bwd_split", ptr(pre), ptr(x), ptr(norms), ptr(g), B, C, ptr(hi), ptr(lo), s)
    return hi, lo


def _l2r_fix(device, pre, x, norms, g, stride, gs):
    ptr, s = _h(device)
    B, C = pre.shape
    hi, lo = _planes(device, B, C)
    _ops().call("rq_l2norm_recon_bwd_fix", ptr(pre), ptr(x), ptr(norms), ptr(g), stride, B, C, gs, ptr(hi), ptr(lo), s)
    return hi, lo


def _check_fix(device, pre, x, norms, g, gs):
    """rq_l2norm_recon_bwd_fix from sentinel planes: per-row g_recon with odd rows bitwise gs (kept) and the others
    recomputed; one shared value that matches (nothing written) and one that does not (every row rewritten)."""
    B, C = pre.shape
    alt = g.clone()
    alt[1::2] = gs
    want = _l2r_bwd_split(device, pre, x, norms, alt)
    got = _l2r_fix(device, pre, x, norms, alt, 1, gs)
    sent = _planes(device, B, C)
    for name, a, w, s0 in zip(("hi", "lo"), got, want, sent):
        assert _same(a[1::2], s0[1::2]), f"fix {name}: a row whose g_recon is gs was rewritten"
        assert _same(a[0::2], w[0::2]), f"fix {name}: a recomputed row differs from bwd_split"
    one = torch.tensor([gs], device=device)
    got = _l2r_fix(device, pre, x, norms, one, 0, gs)
    assert _same(got[0], sent[0]) and _same(got[1], sent[1]), "fix: g_stride 0 with a match wrote something"
    other = torch.tensor([0.625], device=device)
    got = _l2r_fix(device, pre, x, norms, other, 0, gs)
    want = _l2r_bwd_split(device, pre, x, norms, other.expand(B).contiguous())
    assert _same(got[0], want[0]) and _same(got[1], want[1]), "fix: g_stride 0 with a mismatch"
    assert not bool((_bits(want[0]) == _bits(sent[0])).all(dim=1).any())     # every row was written


@pytest.mark.parametrize("C", S.WIDTHS)
def test_l2norm_recon_width(device, C):
    """Every l2norm_recon kernel at VPL = ceil(C / 256), 9 rows, one all zero: forward and fp32 backward against fp64
    (recon rtol 1e-5 / atol 1e-6, g_pre rtol 1e-4 / atol 1e-7: test_l2norm_recon_ragged_vs_fp64's bounds); the split
    backward's planes bitwise split_bf16x3 of the fp32 backward; the forward with the speculative gradient bitwise the
    plain forward and the split backward for g_recon == gs; the fix kernel's three outcomes."""
    ops = _ops()
    ptr, s = _h(device)
    B = S.SWEEP_ROWS
    print(f"\n[l2r] C {C} VPL {S.vpl(C)}")
    d, g = _sweep(device, B, C)
    ref_recon, ref_g = S.l2norm_recon_ref64(d.pre, d.tgt, d.g_recon)
    recon, norms = _l2r_fwd(device, g.pre, g.tgt)
    g32 = torch.full_like(g.pre, _NAN)
    ops.call("rq_l2norm_recon_bwd", ptr(g.pre), ptr(g.tgt), ptr(norms), ptr(g.g_recon), B, C, ptr(g32), s)
    e_r = (recon.double().cpu() - ref_recon).abs()
    e_g = (g32.double().cpu() - ref_g).abs()
    print(f"  recon: max |err| / (1e-5 |ref| + 1e-6) {float((e_r / (1e-5 * ref_recon.abs() + 1e-6)).max()):.3f}; "
          f"g_pre: max |err| / (1e-4 |ref| + 1e-7) {float((e_g / (1e-4 * ref_g.abs() + 1e-7)).max()):.3f}, "
          f"max |err| / max |row| {float((e_g / ref_g.abs().amax(1, keepdim=True)).max()):.2e}")
    assert torch.allclose(recon.double().cpu(), ref_recon, rtol=1e-5, atol=1e-6)
    assert float(norms[B // 2]) == 0 and bool((norms[:B // 2] > 0).all())
    assert torch.allclose(g32.double().cpu(), ref_g, rtol=1e-4, atol=1e-7)
    hi, lo = _l2r_bwd_split(device, g.pre, g.tgt, norms, g.g_recon)
    sp = ops.split_bf16x3(g32)
    assert _same(hi, sp.hi) and _same(lo, sp.lo), "bwd_split planes != split_bf16x3(fp32 backward)"
    gs = float(np.float32(1.0 / B))
    r2, n2, fhi, flo = _l2r_fwd(device, g.pre, g.tgt, gs)
    assert _same(r2, recon) and _same(n2, norms), "fwd_grad: recon / norms differ from the plain forward"
    whi, wlo = _l2r_bwd_split(device, g.pre, g.tgt, norms, torch.full((B,), gs, device=device))
    assert _same(fhi, whi) and _same(flo, wlo), "fwd_grad planes != bwd_split for g_recon == gs"
    _check_fix(device, g.pre, g.tgt, norms, g.g_recon + 2.0, gs)


def test_l2norm_recon_fix_row_loop(device):
    """More rows than the fix kernel's 2,048 x 4 waves: the row-stride loop runs a second trip."""
    B, C = S.L2R_FIX_LOOP_CASE
    d, g = _sweep(device, B, C)
    recon, norms = _l2r_fwd(device, g.pre, g.tgt)
    _check_fix(device, g.pre, g.tgt, norms, g.g_recon + 2.0, float(np.float32(1.0 / B)))


# ------------------------------------------------------------------------------------------------ B. loss head
def _ce_run(device, case, d, which=(True, True, True), tgt=None):
    ops = _ops()
    rows = case.B * (case.npos + 1)
    buf = torch.full((rows, case.K + case.pad), 1e30, device=device)
    buf[:, :case.K] = d.X.to(device)
    X = buf[:, :case.K].detach().requires_grad_(True)
    t = (d.tgt if tgt is None else tgt).to(device)
    assert X.stride(0) == case.K + case.pad and ops.ce_loss_supported(X, t, case.B)
    loss, loss_d, logits = ops.cross_entropy_loss(X, t, case.B)
    total = 0
    if which[0]:
        total = total + loss * d.w_loss
    if which[1]:
        total = total + (loss_d * d.w_d.to(device)).sum()
    if which[2]:
        total = total + (logits * d.w_logits.to(device)).sum()
    total.backward()
    return loss.detach(), loss_d.detach(), logits.detach(), X.grad


def _ce_ref(case, d, which=(True, True, True), tgt=None):
    return S.ce_loss_ref64(d.X, d.tgt if tgt is None else tgt, case.B, d.w_loss if which[0] else None,
                           d.w_d if which[1] else None, d.w_logits if which[2] else None)


def _ce_check(case, got, ref, what):
    got = [t.double().cpu() for t in got]
    rel = 0.0 if case.atol_only else 1.0
    e_dx = float((got[3] - ref.dX).abs().max())
    m_dx = float(ref.dX.abs().max())
    print(f"\n[ce] {what}: loss {float(got[0]):.7g} (fp64 {float(ref.loss):.7g}), max |err| loss_d "
          f"{float((got[1] - ref.loss_d).abs().max()):.3e}, dX {e_dx:.3e} = {e_dx / max(m_dx, 1e-300):.3e} of max |dX|")
    torch.testing.assert_close(got[0], ref.loss, rtol=2e-6 * rel, atol=1e-6)
    torch.testing.assert_close(got[1], ref.loss_d, rtol=2e-6 * rel, atol=1e-6)
    assert torch.equal(got[2], ref.logits), "logits are a copy"
    if case == S.CE_X40:
        assert e_dx <= S.CE_X40_DX_BOUND * m_dx, (e_dx / m_dx, S.CE_X40_DX_BOUND)
    else:
        torch.testing.assert_close(got[3], ref.dX, rtol=1e-5 * rel, atol=1e-7)


@pytest.mark.parametrize("case", S.CE_CASES, ids=lambda c: c.id)
def test_ce_loss_regimes_vs_fp64(device, case):
    """ops.cross_entropy_loss with all three upstream gradients against ce_loss_ref64, test_ce_loss_matches_torch's
    bounds (loss, loss_d rtol 2e-6 / atol 1e-6; dX rtol 1e-5 / atol 1e-7; logits bitwise), and bitwise repeatable.
    The x40 case's dX is held to 4 x 1.14e-7 = 4.56e-7 of max |dX| instead: 1.14e-7 is the error of torch's fp32
    composite on the CPU against ce_loss_ref64 on the same inputs (test_rowwise_ref_host.py). Measured on an MI355X:
    1.8e-7; 3.7e-6 while the backward formed exp(x - L) from the saved, rounded L = m + log sum."""
    d = S.ce_inputs(case)
    got = _ce_run(device, case, d)
    again = _ce_run(device, case, d)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs differ"
    _ce_check(case, got, _ce_ref(case, d), case.id)
    if case.dead:    # a fully ignored sequence (7) and position (5): zero loss_d, dX = the logits gradient alone
        assert float(got[1][5]) == 0.0
        dX = got[3].view(case.B, case.npos + 1, case.K).cpu()
        wl = d.w_logits.view(case.B, case.npos, case.K)
        assert torch.equal(dX[7, :case.npos], wl[7]) and torch.equal(dX[:, 5], wl[:, 5])
        assert not dX[:, case.npos].any()


@pytest.mark.parametrize("which", [(True, False, False), (False, True, False), (False, False, True)],
                         ids=["loss", "loss_d", "logits"])
def test_ce_loss_single_upstream_gradient(device, which):
    """Only one of the three outputs has a gradient: the other two reach rq_ce_loss_bwd as NULL."""
    case = S.CE_SINGLE_GRAD_CASE
    d = S.ce_inputs(case)
    _ce_check(case, _ce_run(device, case, d, which), _ce_ref(case, d, which), f"{case.id} {which}")


def test_ce_loss_out_of_range_target(device):
    """One target equal to K: loss and that position's loss_d are NaN; every other loss_d entry and every dX row of
    another (b, j) is what the reference gives with that target ignored."""
    case = S.CE_BAD_TARGET_CASE
    d = S.ce_inputs(case)
    bad = d.tgt.clone()
    bad[1, 0] = case.K
    ign = d.tgt.clone()
    ign[1, 0] = -1
    got = [t.double().cpu() for t in _ce_run(device, case, d, tgt=bad)]
    ref = _ce_ref(case, d, tgt=ign)
    assert bool(torch.isnan(got[0])) and bool(torch.isnan(got[1][0]))
    torch.testing.assert_close(got[1][1:], ref.loss_d[1:], rtol=2e-6, atol=1e-6)
    keep = torch.ones(case.B * (case.npos + 1), dtype=torch.bool)
    keep[1 * (case.npos + 1) + 0] = False
    torch.testing.assert_close(got[3][keep], ref.dX[keep], rtol=1e-5, atol=1e-7)
    assert torch.equal(got[2], ref.logits)


# ------------------------------------------------------------------------------------------------ C. Gumbel edges
@pytest.mark.parametrize("B,D,K,T", S.GUMBEL_CASES)
def test_gumbel_edges_vs_fp64(device, monkeypatch, B, D, K, T):
    """test_gumbel_hip_vs_fp64's procedure and bounds (3e-4 max|fp64|, at most 5x the composite's error; ids exact on
    margin-safe rows, more than 0.9 of them) at K below a wave, at the largest K and D, and with one code."""
    import distributions.gumbel as gumbel
    import modules.quantize as mq
    from modules.quantize import Quantize, QuantizeForwardMode
    ops = _ops()
    x0, cb0, noise, g_emb = S.gumbel_inputs(B, D, K)
    launched = []
    real = ops.gumbel_softmax_quantize
    monkeypatch.setattr(ops, "gumbel_softmax_quantize", lambda *a: (launched.append(1), real(*a))[1])

    def run(hip):
        monkeypatch.setattr(gumbel, "sample_gumbel", lambda shape, device, eps=1e-20: noise.to(device).reshape(shape))
        monkeypatch.setattr(mq, "GUMBEL_HIP", hip)
        q = Quantize(D, K, do_kmeans_init=False, sim_vq=False, forward_mode=QuantizeForwardMode.GUMBEL_SOFTMAX).to(device)
        with torch.no_grad():
            q.embedding.weight.copy_(cb0)
        q.train(True)
        x = x0.clone().to(device).requires_grad_(True)
        o = q(x, temperature=T)
        ((o.embeddings * g_emb.to(device)).sum() + o.loss.sum()).backward()
        return (o.ids.cpu(), o.embeddings.detach().cpu().double(), o.loss.detach().cpu().double(),
                x.grad.cpu().double(), q.embedding.weight.grad.cpu().double())

    hip = run(True)
    assert launched == [1], "the HIP kernels did not run"
    comp = run(False)
    assert launched == [1]
    ref = S.gumbel_ref64(x0, cb0, None, noise, T, g_emb)
    safe = S.gumbel_safe_rows(ref[5])
    assert safe.float().mean() > 0.9
    assert torch.equal(hip[0][safe], ref[0][safe]) and torch.equal(comp[0][safe], ref[0][safe])
    print(f"\n[gumbel] {(B, D, K, T)}")
    for i, name in ((1, "emb"), (2, "loss"), (3, "grad_x"), (4, "grad_codebook")):
        m = ref[i].abs().max().item()
        e_hip = (hip[i] - ref[i]).abs().max().item()
        e_comp = (comp[i] - ref[i]).abs().max().item()
        print(f"  {name}: max |err| vs fp64 hip {e_hip:.3e}, composite {e_comp:.3e} (max |fp64| {m:.3e})")
        assert e_hip <= 3e-4 * m, (name, e_hip, m)
        assert e_hip <= 5 * e_comp + 1e-6 * m, (name, e_hip, e_comp)


def test_gumbel_lowest_index_on_ties(device):
    """Codebook rows 70 (the lane of row 6) and 100 (another lane) are copies of row 6, and the x rows lie next to
    that codeword: the three distances are the same arithmetic, bitwise equal, and ids must name 6 — within a lane
    the first minimum, across lanes the lowest index."""
    t = S.GUMBEL_TIE
    K, D, rows = t["K"], t["D"], t["rows"]
    gen = torch.Generator().manual_seed(5)
    cb = torch.randn(K, D, generator=gen) * 0.7
    cb[t["same_lane"]] = cb[t["base"]]
    cb[t["other_lane"]] = cb[t["base"]]
    x = cb[t["base"]][None, :] + 0.01 * torch.randn(rows, D, generator=gen)
    noise = torch.randn(rows, K, generator=gen)
    dist = (x.double()[:, None, :] - cb.double()[None, :, :]).pow(2).sum(-1)
    assert bool((dist.argmin(1) == t["base"]).all()) and bool((dist[:, t["base"]] == dist[:, t["other_lane"]]).all())
    emb, ids = _ops().gumbel_softmax_quantize(x.to(device), cb.to(device), noise.to(device), 0.5)
    assert ids.cpu().tolist() == [t["base"]] * rows, ids.cpu().tolist()


# ------------------------------------------------------------------------------------------------ D. rq_col_sum
@pytest.mark.parametrize("n", S.COL_SUM_N)
@pytest.mark.parametrize("S_", S.COL_SUM_S)
def test_col_sum_order(device, S_, n):
    """rq_col_sum at each boundary of strided_slab_sum (one partial per lane, one round of eight, a second round) and
    with idle column threads: bitwise col_sum_order, within 1e-6 sum|P| of fp64 (the accumulated form: of
    sum|P| + |out|), bitwise repeatable, with and without accumulation."""
    ptr, s = _h(device)
    P, base = S.col_sum_inputs(S_, n)
    Pd = P.to(device)
    p64 = P.double()
    for acc in (0, 1):
        outs = []
        for _ in range(2):
            out = base.to(device) if acc else torch.full((n,), _NAN, device=device)
            _ops().call("rq_col_sum", ptr(Pd), S_, n, ptr(out), acc, s)
            outs.append(out.cpu())
        assert _same(outs[0], outs[1]), "two runs differ"
        want = S.col_sum_order(P.numpy(), base.numpy() if acc else None)
        assert np.array_equal(outs[0].numpy().view(np.uint32), want.view(np.uint32)), f"order (accumulate {acc})"
        ref = p64.sum(0) + (base.double() if acc else 0)
        scale = p64.abs().sum(0) + (base.double().abs() if acc else 0)
        err = float(((outs[0].double() - ref).abs() / scale).max())
        print(f"\n[col_sum] S {S_} n {n} accumulate {acc}: {err:.2e} of sum|P|")
        assert err <= 1e-6
