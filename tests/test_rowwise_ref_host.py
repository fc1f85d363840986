"""The row-wise tests' fp64 references and case tables on the host, no GPU: every closed-form reference of
tests/rowwise_support.py against torch autograd in fp64 of the reference's own composition (F.normalize, RMSNorm's
formula, F.cross_entropy with ignore_index -1), col_sum_order against an fp64 sum, the case tables against the list of
instantiated forms and the row-count regimes, and the share of margin-safe rows of every Gumbel case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowwise_support as S


def _close(a, b, what):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-12 * scale, (what, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("D", S.WIDTHS)
def test_l2norm_recon_ref64_vs_autograd(D):
    d = S.sweep_inputs(S.SWEEP_ROWS, D)
    recon, g_pre = S.l2norm_recon_ref64(d.pre, d.tgt, d.g_recon)
    p = d.pre.double().requires_grad_(True)
    r = ((F.normalize(p, p=2, dim=-1, eps=1e-12) - d.tgt.double()) ** 2).sum(-1)
    (r * d.g_recon.double()).sum().backward()
    _close(recon, r.detach(), "recon")
    zero = S.SWEEP_ROWS // 2
    assert not d.pre[zero].any() and float(g_pre[zero].abs().max()) > 1e8       # the clamped branch: g_y / eps
    _close(g_pre, p.grad, "g_pre")


@pytest.mark.parametrize("B,D", [(S.SWEEP_ROWS, D) for D in S.WIDTHS] + list(S.RMS2_REGIME_CASES))
def test_rmsnorm_ref64_vs_autograd(B, D):
    d = S.sweep_inputs(B, D)
    for two in (False, True):
        ws, gys = ([d.w1, d.w2], [d.gy1, d.gy2]) if two else ([d.w1], [d.gy1])
        ref = S.rmsnorm_ref64(d.x, ws, S.RMS_EPS, gys, d.gres)
        x = d.x.double().requires_grad_(True)
        wl = [w.double().requires_grad_(True) for w in ws]
        ys = [x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + S.RMS_EPS) * w for w in wl]   # modules/normalize.py:22-32
        (sum((y * gy.double()).sum() for y, gy in zip(ys, gys)) + (x * d.gres.double()).sum()).backward()
        for a, b in zip(ref.ys, ys):
            _close(a, b.detach(), "y")
        _close(ref.gx, x.grad, "gx")
        for a, w, s in zip(ref.gws, wl, ref.gw_scales):
            _close(a, w.grad, "gw")
            assert bool((s >= a.abs()).all())
    none = S.rmsnorm_ref64(d.x, [d.w1], S.RMS_EPS, [d.gy1])
    _close(none.gx + d.gres.double(), S.rmsnorm_ref64(d.x, [d.w1], S.RMS_EPS, [d.gy1], d.gres).gx, "gres")


def _ce_autograd(d, B, dtype, w_loss, w_d, w_logits):
    X = d.X.to(dtype).clone().requires_grad_(True)
    K = X.shape[1]
    logits = X.view(B, -1, K)[:, :-1, :].flatten(end_dim=1)
    unred = F.cross_entropy(logits, d.tgt.flatten(), reduction="none", ignore_index=-1).view(B, -1)
    loss, loss_d = unred.sum(axis=1).mean(), unred.mean(axis=0)
    total = 0
    if w_loss is not None:
        total = total + loss * w_loss
    if w_d is not None:
        total = total + (loss_d * w_d.to(dtype)).sum()
    if w_logits is not None:
        total = total + (logits * w_logits.to(dtype)).sum()
    total.backward()
    return loss.detach(), loss_d.detach(), logits.detach(), X.grad


@pytest.mark.parametrize("case", S.CE_CASES, ids=lambda c: c.id)
def test_ce_loss_ref64_vs_autograd(case):
    d = S.ce_inputs(case)
    assert d.X.stride(0) == case.K + case.pad and int((d.tgt == -1).sum()) >= 2
    alone = ((d.w_loss, None, None), (None, d.w_d, None), (None, None, d.w_logits))
    for w_loss, w_d, w_logits in ((d.w_loss, d.w_d, d.w_logits),) + (alone if case == S.CE_SINGLE_GRAD_CASE else ()):
        ref = S.ce_loss_ref64(d.X, d.tgt, case.B, w_loss, w_d, w_logits)
        want = _ce_autograd(d, case.B, torch.float64, w_loss, w_d, w_logits)
        for name, a, b in zip(("loss", "loss_d", "logits", "dX"), ref, want):
            _close(a, b, name)
    if case.dead:
        ref = S.ce_loss_ref64(d.X, d.tgt, case.B, d.w_loss, d.w_d, d.w_logits)
        assert float(ref.loss_d[5]) == 0.0
        rows = ref.dX.view(case.B, case.npos + 1, case.K)
        assert torch.equal(rows[7, :case.npos], d.w_logits.double().view(case.B, case.npos, case.K)[7])
    if case.atol_only:
        ref = S.ce_loss_ref64(d.X, d.tgt, case.B, d.w_loss, d.w_d, None)
        assert float(ref.loss) == 0.0 and not ref.dX.any()


def test_ce_case_table_regimes():
    nu = sorted(c.B * c.npos for c in S.CE_CASES)
    assert S.CE_STAGE in nu and min(v for v in nu if v > S.CE_STAGE) == S.CE_STAGE + 4     # both sides of the limit
    assert any(c.B > 256 for c in S.CE_CASES) and {1, 63, 64, 65, 1024} <= {c.K for c in S.CE_CASES}
    assert S.CE_SINGLE_GRAD_CASE in S.CE_CASES and S.CE_BAD_TARGET_CASE in S.CE_CASES and S.CE_X40 in S.CE_CASES
    assert sum(c.dead for c in S.CE_CASES) == 1 and sum(c.pad > 0 for c in S.CE_CASES) == 1


def test_ce_x40_composite_error():
    """The fp32 CPU composite on the x40 case against ce_loss_ref64, dX as a share of max |dX|: the figure the
    kernel's bound (four times it) is taken from."""
    d = S.ce_inputs(S.CE_X40)
    ref = S.ce_loss_ref64(d.X, d.tgt, S.CE_X40.B, d.w_loss, d.w_d, d.w_logits)
    got = _ce_autograd(d, S.CE_X40.B, torch.float32, d.w_loss, d.w_d, d.w_logits)
    err = float((got[3].double() - ref.dX).abs().max() / ref.dX.abs().max())
    print(f"x40: fp32 composite dX error {err:.3e} of max |dX| (recorded {S.CE_X40_COMPOSITE_ERR:.3e})")
    assert float(d.X.abs().max()) > 120 and float(torch.logsumexp(d.X.double(), -1).max()) > 89   # exp overflows unshifted
    assert 0 < err <= S.CE_X40_DX_BOUND


@pytest.mark.parametrize("B,D,K,T", S.GUMBEL_CASES)
def test_gumbel_cases_keep_their_rows(B, D, K, T):
    """The share of margin-safe rows (test_gumbel_hip_vs_fp64's rule, which requires more than 0.9) of every new case."""
    x0, cb0, noise, g_emb = S.gumbel_inputs(B, D, K)
    dist = S.gumbel_ref64(x0, cb0, None, noise, T, g_emb)[5]
    share = float(S.gumbel_safe_rows(dist).float().mean())
    print(f"gumbel {(B, D, K, T)}: safe share {share:.3f}")
    assert share > 0.9


def test_gumbel_tie_rows_are_exact_ties():
    t = S.GUMBEL_TIE
    assert t["same_lane"] % 64 == t["base"] % 64 != t["other_lane"] % 64 and t["base"] < t["same_lane"] < t["other_lane"]


@pytest.mark.parametrize("n", S.COL_SUM_N)
@pytest.mark.parametrize("S_", S.COL_SUM_S)
def test_col_sum_order_vs_fp64(S_, n):
    P, base = S.col_sum_inputs(S_, n)
    got = S.col_sum_order(P.numpy())
    assert got.dtype == np.float32 and got.shape == (n,)
    ref = P.double().sum(0).numpy()
    assert bool((np.abs(got - ref) <= 1e-6 * P.double().abs().sum(0).numpy()).all())
    acc = S.col_sum_order(P.numpy(), base.numpy())
    assert np.array_equal(acc, base.numpy() + got)
    if S_ <= 64:      # one partial per lane: the tree alone
        tree = P.numpy().copy()
        tree = np.concatenate([tree, np.zeros((64 - S_, n), np.float32)])
        h = 32
        while h:
            tree = tree[:h] + tree[h:2 * h]
            h //= 2
        assert np.array_equal(got, tree[0])


def test_sweep_reaches_every_form():
    assert len(S.WIDTHS) == 32 and all(d % 4 == 0 and 4 <= d <= 4096 for d in S.WIDTHS)
    assert sorted({S.vpl(d) for d in S.WIDTHS}) == list(range(1, 17))
    for v in range(1, 17):
        assert 256 * (v - 1) + 4 in S.WIDTHS and 256 * v in S.WIDTHS
    reached = set()
    for d in S.WIDTHS:
        reached |= S.sweep_forms(d)
    assert reached == set(S.FORMS) and len(S.FORMS) == 9 * 16
    assert S.SWEEP_ROWS % 4 == 1


def test_rms_rows_regimes():
    for B, r in ((1, 4), (S.SWEEP_ROWS, 4), (2044, 4), (2045, 4), (4088, 4), (4089, 8), (8176, 8), (8177, 16), (65536, 16)):
        assert S.rms_rows(B) == r, (B, r)
    assert [S.rms_rows(B) for B, _ in S.RMS2_REGIME_CASES] == [8, 16]
    B, C = S.L2R_FIX_LOOP_CASE
    assert B > 2048 * 4 and S.vpl(C) == 1
