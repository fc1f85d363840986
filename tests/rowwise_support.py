"""Shared by tests/test_rowwise_ref_host.py, tests/test_rowwise_forms_gpu.py and tests/test_gumbel_gpu.py: fp64
references of the row-wise kernels (csrc/rowwise.hip) in torch on the CPU, a numpy restatement of rq_col_sum's
summation order, the launchers' form rule (row width -> template instantiation, row count -> rows per workgroup),
the list of instantiated forms and the case tables that reach each of them. No GPU needed to import or to run a
reference."""
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

RMS_EPS = 1e-6


# ------------------------------------------------------------------------------------------------ the form rule
def vpl(D: int) -> int:
    """float4 vectors per lane: the template argument every width switch of rowwise.hip selects (D <= 4096)."""
    return -(-D // 256)


def rms_rows(B: int) -> int:
    """rms_rows_per_blk: rows per workgroup of the RMSNorm backward — 16, halved while above 4 and fewer than 512
    workgroups would start. 4 up to 2,044 rows (and from 2,045 to 4,088), 8 for 4,089 to 8,176, 16 from 8,177."""
    r = 16
    while r > 4 and -(-B // r) < 512:
        r //= 2
    return r


# family -> the C entry point that launches it
FAMILIES = dict(rms_fwd="rq_rmsnorm_dropout_fwd", rms_bwd="rq_rmsnorm_dropout_bwd",
                rms2_fwd="rq_rmsnorm2_dropout_fwd", rms2_bwd="rq_rmsnorm2_dropout_bwd",
                l2r_fwd="rq_l2norm_recon_fwd", l2r_fwd_grad="rq_l2norm_recon_fwd_grad", l2r_bwd="rq_l2norm_recon_bwd",
                l2r_bwd_split="rq_l2norm_recon_bwd_split", l2r_fix="rq_l2norm_recon_bwd_fix")
FORMS = tuple((f, v) for f in FAMILIES for v in range(1, 17))

# Two widths per VPL: one live lane in the last vector slot, and the slot full.
WIDTHS = tuple(d for v in range(1, 17) for d in (256 * (v - 1) + 4, 256 * v))
SWEEP_ROWS = 9          # the last 4-row forward workgroup holds one row
# (B, D) of the fork's 8- and 16-row backward regimes, and (B, C) past the fix kernel's 2,048 x 4 row grid
RMS2_REGIME_CASES = ((4099, 8), (8181, 12))
L2R_FIX_LOOP_CASE = (8197, 8)


def sweep_forms(D: int):
    """The forms the width sweep's case D launches: every family at vpl(D)."""
    return {(f, vpl(D)) for f in FAMILIES}


class SweepData(NamedTuple):
    x: torch.Tensor        # (B, D) RMSNorm input
    w1: torch.Tensor
    w2: torch.Tensor
    gy1: torch.Tensor
    gy2: torch.Tensor
    gres: torch.Tensor
    pre: torch.Tensor      # (B, D) l2norm input, row B // 2 all zero
    tgt: torch.Tensor      # (B, D) unit rows
    g_recon: torch.Tensor  # (B,)


def sweep_inputs(B: int, D: int) -> SweepData:
    g = torch.Generator().manual_seed(1000 * B + D)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    x = r(B, D) * 3
    w1, w2 = 1 + 0.1 * r(D), 1 + 0.1 * r(D)
    gy1, gy2, gres = r(B, D), r(B, D), r(B, D)
    pre = r(B, D)
    pre[B // 2] = 0.0
    tgt = F.normalize(r(B, D), dim=-1)
    return SweepData(x, w1, w2, gy1, gy2, gres, pre, tgt, torch.rand(B, generator=g))


# ------------------------------------------------------------------------------------------------ fp64 references
def l2norm_recon_ref64(pre, x, g_recon):
    """(recon, g_pre) of recon_b = sum_c (pre_b / max(|pre_b|, 1e-12) - x_b)^2 (F.normalize eps 1e-12 and
    ReconstructionLoss) in fp64, closed form: g_y = 2 g_b (y - x_b); g_pre = (g_y - y (g_y . y)) / n where
    |pre_b| > eps, g_y / eps on clamped rows (the norm's gradient does not pass the clamp)."""
    p, t, g = pre.double(), x.double(), g_recon.double()
    raw = p.pow(2).sum(-1, keepdim=True).sqrt()
    n = raw.clamp_min(1e-12)
    y = p / n
    recon = (y - t).pow(2).sum(-1)
    gy = 2 * g[:, None] * (y - t)
    g_pre = torch.where(raw > 1e-12, (gy - y * (gy * y).sum(-1, keepdim=True)) / n, gy / n)
    return recon, g_pre


class RmsRef(NamedTuple):
    ys: list
    gx: torch.Tensor
    gws: list
    gw_scales: list     # sum_b |gy x rstd| per column: the scale of the fp32 row sums behind gw


def rmsnorm_ref64(x, ws, eps, gys, gres=None) -> RmsRef:
    """RMSNorm (t = x rsqrt(mean(x^2) + eps), y_i = t w_i) for one or two weights of the same rows, no dropout, in
    fp64, closed form: gx = r sum_i (w_i gy_i) - x (r^3 / D) sum_j (sum_i w_i gy_i x)_j (+ gres); gw_i = sum_b gy_i t."""
    x = x.double()
    D = x.shape[-1]
    rs = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    t = x * rs
    ys = [t * w.double() for w in ws]
    gt = sum(w.double() * gy.double() for w, gy in zip(ws, gys))
    gx = rs * gt - x * (rs.pow(3) / D) * (gt * x).sum(-1, keepdim=True)
    if gres is not None:
        gx = gx + gres.double()
    gws = [(gy.double() * t).sum(0) for gy in gys]
    scales = [(gy.double() * t).abs().sum(0) for gy in gys]
    return RmsRef(ys, gx, gws, scales)


class CeRef(NamedTuple):
    loss: torch.Tensor
    loss_d: torch.Tensor
    logits: torch.Tensor
    dX: torch.Tensor


def ce_loss_ref64(X, tgt, B, w_loss=None, w_d=None, w_logits=None) -> CeRef:
    """The decoder loss head in fp64, closed form: logits = X.view(B, npos_x, K)[:, :npos].flatten(0, 1), unred =
    cross_entropy(logits, tgt, reduction='none', ignore_index=-1), loss = unred.sum(1).mean(), loss_d =
    unred.mean(0); dX = d(w_loss loss + w_d . loss_d + sum(w_logits logits)) / dX, each weight possibly None.
    X (B * npos_x, K) may be a strided view. Targets must lie in [-1, K)."""
    K = X.shape[1]
    npos, npos_x = tgt.shape[1], X.shape[0] // B
    Xd = X.double().reshape(B, npos_x, K)
    lg = Xd[:, :npos]
    lse = torch.logsumexp(lg, dim=-1)
    live = tgt >= 0
    picked = lg.gather(-1, tgt.clamp_min(0)[..., None])[..., 0]
    u = torch.where(live, lse - picked, torch.zeros_like(lse))
    g = torch.zeros(B, npos, dtype=torch.float64)
    if w_loss is not None:
        g = g + float(w_loss)
    if w_d is not None:
        g = g + w_d.double()[None, :]
    g = torch.where(live, g / B, torch.zeros_like(g))
    onehot = F.one_hot(tgt.clamp_min(0), K).double()
    d = g[..., None] * (torch.exp(lg - lse[..., None]) - onehot)
    if w_logits is not None:
        d = d + w_logits.double().reshape(B, npos, K)
    dX = torch.zeros(B, npos_x, K, dtype=torch.float64)
    dX[:, :npos] = d
    return CeRef(u.sum(1).mean(), u.mean(0), lg.reshape(B * npos, K).clone(), dX.reshape(B * npos_x, K))


def gumbel_ref64(x0, cb0, proj, noise, T, g_emb, beta=0.25):
    """Reference Quantize.forward (modules/quantize.py:105-129,146 with distributions/gumbel.py:14-18 and
    modules/loss.py:34-42) in fp64: (ids, emb, loss, grad_x, grad_codebook, dist) of the same objective."""
    x = x0.double().requires_grad_(True)
    w = cb0.double().requires_grad_(True)
    codebook = w @ proj.double().t() if proj is not None else w
    dist = (x ** 2).sum(1, keepdim=True) + (codebook.t() ** 2).sum(0, keepdim=True) - 2 * x @ codebook.t()
    ids = dist.detach().min(1).indices
    weights = torch.softmax((-dist + noise.double()) / T, dim=-1)
    emb = weights @ codebook
    loss = ((x.detach() - emb) ** 2).sum(-1) + beta * ((x - emb.detach()) ** 2).sum(-1)
    ((emb * g_emb.double()).sum() + loss.sum()).backward()
    return ids, emb.detach(), loss.detach(), x.grad, w.grad, dist.detach()


def gumbel_inputs(B, D, K):
    """(x0, cb0, noise, g_emb) by the generator recipe of test_gumbel_gpu.py::test_gumbel_hip_vs_fp64."""
    gen = torch.Generator().manual_seed(B + K)
    x0 = torch.randn(B, D, generator=gen)
    cb0 = torch.randn(K, D, generator=gen) * 0.7
    u = torch.rand(B, K, generator=gen)
    noise = -torch.log(-torch.log(u + 1e-20) + 1e-20)
    g_emb = torch.randn(B, D, generator=gen)
    return x0, cb0, noise, g_emb


def gumbel_safe_rows(dist):
    """test_gumbel_hip_vs_fp64's rule: rows whose two smallest fp64 distances are more than 1e-4 (relative, at least
    absolute) apart; with one code there is no second distance and every row is safe."""
    if dist.shape[1] < 2:
        return torch.ones(dist.shape[0], dtype=torch.bool)
    top2 = dist.topk(2, dim=1, largest=False).values
    return (top2[:, 1] - top2[:, 0]) > 1e-4 * top2[:, 0].abs().clamp_min(1.0)


def col_sum_order(P, accumulate_into=None):
    """numpy fp32 restatement of rms_reduce_kernel's fixed order for P (S, n): row lane q of 64 sums partials q,
    q + 64, ... ascending from 0, then the halving tree red[q] += red[q + h], h = 32 .. 1; if accumulating,
    out + sum last."""
    P = np.asarray(P, np.float32)
    S, n = P.shape
    red = np.zeros((64, n), np.float32)
    for k in range(0, S, 64):
        m = min(64, S - k)
        red[:m] = red[:m] + P[k:k + m]
    h = 32
    while h > 0:
        red[:h] = red[:h] + red[h:2 * h]
        h //= 2
    out = red[0]
    if accumulate_into is not None:
        out = np.asarray(accumulate_into, np.float32) + out
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------ loss-head cases
class CeCase(NamedTuple):
    B: int
    npos: int
    K: int
    scale: float = 3.0
    pad: int = 0             # X = buf[:, :K] of a (rows, K + pad) buffer whose padding holds 1e30
    dead: bool = False       # also sequence 7 and position 5 fully ignored
    atol_only: bool = False  # K = 1: loss and gradients are zero

    @property
    def id(self):
        return f"{self.B}x{self.npos}x{self.K}" + ("-x40" if self.scale != 3.0 else "") + ("-ldx" if self.pad else "")


CE_STAGE = 8192   # kCeStage: u staged in LDS by ce_means_kernel when B * npos <= 8192
CE_CASES = (CeCase(2048, 4, 8), CeCase(2049, 4, 8), CeCase(300, 33, 4, dead=True), CeCase(257, 3, 1, atol_only=True),
            CeCase(5, 2, 63), CeCase(5, 2, 64), CeCase(5, 2, 65), CeCase(3, 2, 1024), CeCase(6, 5, 256, scale=40.0),
            CeCase(8, 5, 256, pad=8))
CE_SINGLE_GRAD_CASE = CeCase(5, 2, 65)     # run with each upstream gradient alone
CE_BAD_TARGET_CASE = CeCase(5, 2, 64)      # run with tgt[1, 0] = K
CE_X40 = CeCase(6, 5, 256, scale=40.0)
# dX of the x40 case, as a share of max |dX|: the rounding of the log-sum-exp (an ulp at ~150 is 1.5e-5) enters every
# probability. The fp32 CPU composite measures CE_X40_COMPOSITE_ERR against ce_loss_ref64 on these inputs
# (test_rowwise_ref_host.py::test_ce_x40_composite_error); the kernel's bound is four times that.
CE_X40_COMPOSITE_ERR = 1.14e-7
CE_X40_DX_BOUND = 4 * CE_X40_COMPOSITE_ERR


class CeData(NamedTuple):
    X: torch.Tensor          # (B * (npos + 1), K), a view with stride(0) = K + pad
    tgt: torch.Tensor        # (B, npos) int64
    w_loss: float
    w_d: torch.Tensor        # (npos,)
    w_logits: torch.Tensor   # (B * npos, K)


def ce_inputs(c: CeCase) -> CeData:
    g = torch.Generator().manual_seed(c.B * 7 + c.K + 31 * c.npos)
    rows = c.B * (c.npos + 1)
    vals = torch.randn(rows, c.K, generator=g) * c.scale
    buf = torch.full((rows, c.K + c.pad), 1e30)
    buf[:, :c.K] = vals
    tgt = torch.randint(0, c.K, (c.B, c.npos), generator=g)
    tgt[0, -1] = -1
    tgt[2, 0] = -1
    if c.dead:
        tgt[7, :] = -1
        tgt[:, 5] = -1
    w_d = torch.randn(c.npos, generator=g)
    w_logits = torch.randn(c.B * c.npos, c.K, generator=g) * 0.01
    return CeData(buf[:, :c.K], tgt, 0.7, w_d, w_logits)


# ------------------------------------------------------------------------------------------------ Gumbel / col-sum
GUMBEL_CASES = ((70, 4, 2, 1.0), (70, 256, 63, 0.5), (130, 68, 65, 0.05), (9, 256, 4096, 0.3), (5, 4, 1, 1.0))
GUMBEL_TIE = dict(K=130, D=16, base=6, same_lane=70, other_lane=100, rows=8)

COL_SUM_S = (1, 63, 64, 65, 512, 513, 1100)
COL_SUM_N = (4, 12, 2048)


def col_sum_inputs(S, n):
    g = torch.Generator().manual_seed(S * 10007 + n)
    return torch.randn(S, n, generator=g), torch.randn(n, generator=g)
