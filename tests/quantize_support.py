"""Shared by tests/test_quantize_ref_host.py and tests/test_quantize_forms_gpu.py: an fp64 reference of the residual
quantization chain that follows given ids, the checks against it, rq_quantize_{fwd,bwd}_plan through ctypes, the list
of kernel forms csrc/rq_quantize.hip instantiates and the case table that reaches each of them. No GPU needed to
import, to plan or to run the reference."""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

MODE_EVAL, MODE_STE, MODE_ROTATION = 0, 2, 3
MODES = (MODE_EVAL, MODE_STE, MODE_ROTATION)
IMPL_TILED, IMPL_REG, IMPL_SPLIT, IMPL_R16 = 1, 2, 3, 4
CB_NONE, CB_CHUNK, CB_SORT = 0, 1, 2
BETA = 0.25

# The project's contract (tests/test_quantize_gpu.py): 2e-5 on emb / res / qloss, 2e-4 on gradients.
RTOL_OUT, RTOL_GRAD = 2e-5, 2e-4


# ------------------------------------------------------------------------------------------------ the plan
class FwdForm(NamedTuple):
    impl: int
    d: int
    resident: int
    wpi: int
    nb: int
    norms_pass: int
    items: int
    grid: int
    lds_bytes: int


class BwdForm(NamedTuple):
    lpi: int
    epl: int
    route: int
    vpl: int
    chunks: int
    contrib: int
    seg_direct: int
    seg_split: int


def fwd_plan(B, D, K, L=2, mode=MODE_ROTATION, impl=0, with_norms=False):
    """(rc, FwdForm) of rq_quantize_fwd_plan; rc != 0 is a refusal (the form is then all zero)."""
    from rqvae_hip import _lib
    f = _lib.QuantizeFwdForm()
    rc = _lib.load().rq_quantize_fwd_plan(B, D, K, L, mode, impl, int(with_norms), ctypes.byref(f))
    return rc, FwdForm(*(getattr(f, n) for n in FwdForm._fields))


def bwd_plan(B, D, K, L=2, mode=MODE_ROTATION, has_g_qloss=True):
    """(rc, BwdForm) of rq_quantize_bwd_plan."""
    from rqvae_hip import _lib
    f = _lib.QuantizeBwdForm()
    rc = _lib.load().rq_quantize_bwd_plan(B, D, K, L, mode, int(has_g_qloss), ctypes.byref(f))
    return rc, BwdForm(*(getattr(f, n) for n in BwdForm._fields))


def last_error():
    from rqvae_hip import _lib
    return _lib.load().rq_last_error().decode(errors="replace")


def fwd_form_key(f: FwdForm):
    """The instantiation a forward plan names: ("tiled" | "split" | "r16", D) or ("reg", D, resident, wpi)."""
    if f.impl == IMPL_REG:
        return ("reg", f.d, f.resident, f.wpi)
    return ({IMPL_TILED: "tiled", IMPL_SPLIT: "split", IMPL_R16: "r16"}[f.impl], f.d)


def bwd_form_keys(f: BwdForm, ids, K):
    """The instantiations a backward call reaches: the rows kernel, then the chunk kernel or the sort route's
    branches. Which branch a codeword's segment takes (direct: at most seg_direct rows, heavy: more) is decided by
    the ids, so it is read from their counts."""
    if f.route == CB_NONE:
        return set()
    keys = {("rows", f.lpi, f.epl)}
    if f.route == CB_CHUNK:
        keys.add(("chunk", f.vpl))
        return keys
    form = "contrib" if f.contrib else "recompute"
    ids = np.asarray(ids)
    for l in range(ids.shape[1]):
        counts = np.bincount(ids[:, l], minlength=K)
        if (counts <= f.seg_direct).any():
            keys.add(("sort", "direct", form))
        if (counts > f.seg_direct).any():
            keys.add(("sort", "heavy", form))
    return keys


def smallest_streaming_K(D, B=131):
    """The smallest K whose register-kernel plan is not resident (the level codebook no longer fits one LDS image)."""
    lo, hi = 1, 1 << 14   # resident at lo, streamed at hi
    assert fwd_plan(B, D, lo, impl=IMPL_REG)[1].resident == 1 and fwd_plan(B, D, hi, impl=IMPL_REG)[1].resident == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fwd_plan(B, D, mid, impl=IMPL_REG)[1].resident:
            lo = mid
        else:
            hi = mid
    return hi


# every forward instantiation of csrc/rq_quantize.hip (rq_quantize_fwd's switches) ...
_ALL_D, _REG_D, _SPLIT_D = (8, 16, 32, 64, 128, 256, 512, 1024), (8, 16, 32, 64), (128, 256, 512, 1024)
FWD_FORMS = ({("tiled", d) for d in _ALL_D} | {("reg", d, r, w) for d in _REG_D for r in (1, 0) for w in (4, 2, 1)} |
             {("split", d) for d in _SPLIT_D} | {("r16", 64)})
# ... and every backward one (rq_quantize_bwd's switches; the sort route's kernel has one instantiation whose two
# branches and two forms are listed as forms, since each is code of its own)
BWD_FORMS = ({("rows", min(d // 4, 64), d // min(d // 4, 64)) for d in _ALL_D} | {("chunk", v) for v in (1, 2, 4)} |
             {("sort", b, f) for b in ("direct", "heavy") for f in ("recompute", "contrib")})
assert len(FWD_FORMS) == 8 + 24 + 4 + 1 and len(BWD_FORMS) == 8 + 3 + 4
# forms no case reaches, with the reason (none: every instantiation has a case)
FWD_FORMS_LEFT_OUT = set()
BWD_FORMS_LEFT_OUT = set()


class FwdCase(NamedTuple):
    """One forward launch: impl forced through the C ABI, L = 2, every mode. K = "stream": smallest_streaming_K(D)."""
    impl: int
    B: int
    D: int
    K: object
    norms: bool
    form: tuple

    @property
    def id(self):
        return f"{self.form[0]}-D{self.D}-B{self.B}-K{self.K}" + ("-norms" if self.norms else "")


def _fwd_cases():
    c = [FwdCase(IMPL_TILED, 131, d, 130, False, ("tiled", d)) for d in _ALL_D]
    c.append(FwdCase(IMPL_TILED, 131, 16, 1, False, ("tiled", 16)))
    for d in _REG_D:   # B = 131 / 8193 / 32769: 4 / 2 / 1 waves per 32-item tile
        for B, w in ((131, 4), (8193, 2), (32769, 1)):
            c.append(FwdCase(IMPL_REG, B, d, 40, False, ("reg", d, 1, w)))
            c.append(FwdCase(IMPL_REG, B, d, "stream", False, ("reg", d, 0, w)))
    c += [FwdCase(IMPL_SPLIT, 131, d, 130, False, ("split", d)) for d in _SPLIT_D]
    # 16x16: B one past a multiple of its 128 items per workgroup
    c += [FwdCase(IMPL_R16, 129, 64, 40, False, ("r16", 64)), FwdCase(IMPL_R16, 129, 64, 288, False, ("r16", 64)),
          FwdCase(IMPL_R16, 257, 64, 288, True, ("r16", 64))]
    return c


FWD_CASES = _fwd_cases()

ALL_G = ("g_emb", "g_emb_sum", "g_res", "g_qloss")


class BwdCase(NamedTuple):
    """One ops.rq_quantize forward + backward (impl auto): L levels, the named upstream gradients given, the others
    None. forms: what the case is meant to reach (checked against the plan and the ids)."""
    B: int
    D: int
    K: int
    L: int
    mode: int
    grads: tuple
    forms: tuple

    @property
    def id(self):
        g = "all" if self.grads == ALL_G else "+".join(self.grads)
        return f"B{self.B}-D{self.D}-K{self.K}-L{self.L}-m{self.mode}-{g}"


def _rows(d):
    lpi = min(d // 4, 64)
    return ("rows", lpi, d // lpi)


def _bwd_cases():
    c = []
    form = {MODE_EVAL: "contrib", MODE_STE: "recompute", MODE_ROTATION: "recompute"}
    for d in _ALL_D:   # each width x each mode, all four gradients (sort route, direct segments)
        for m in MODES:
            c.append(BwdCase(131, d, 40, 2, m, ALL_G, (_rows(d), ("sort", "direct", form[m]))))
    # each gradient alone: sub-wave item groups (D = 8), one wave per item with 4 / 8 / 16 elements per lane
    for d, modes in ((8, (MODE_ROTATION, MODE_EVAL)), (256, (MODE_ROTATION,)), (512, (MODE_ROTATION,)),
                     (1024, (MODE_ROTATION,))):
        for m in modes:
            for g in ALL_G:
                c.append(BwdCase(131, d, 40, 2, m, (g,), (_rows(d), ("sort", "direct", form[m]))))
    # chunk route: VPL 1 / 2 / 4, K < 16 (waves that own no codeword), B at the boundary, one row into a new chunk,
    # and a ragged last chunk
    for d, k in ((64, 256), (128, 128), (256, 64), (64, 5)):
        for B in (4096, 4097, 5000):
            m = MODE_STE if (d, B) == (64, 4097) else MODE_ROTATION
            c.append(BwdCase(B, d, k, 2, m, ALL_G, (_rows(d), ("chunk", d // 64))))
    c.append(BwdCase(4095, 64, 256, 2, MODE_ROTATION, ALL_G, (_rows(64), ("sort", "direct", "recompute"))))
    # heavy segments (about 1,500 rows on each of the two codewords that are not duplicates of a lower one)
    c.append(BwdCase(3000, 32, 4, 2, MODE_ROTATION, ALL_G, (_rows(32), ("sort", "heavy", "recompute"))))
    c.append(BwdCase(3000, 32, 4, 2, MODE_STE, ALL_G, (_rows(32), ("sort", "heavy", "recompute"))))
    c.append(BwdCase(3000, 32, 4, 2, MODE_EVAL, ALL_G, (_rows(32), ("sort", "heavy", "contrib"))))
    return c


BWD_CASES = _bwd_cases()


# ------------------------------------------------------------------------------------------------ inputs
def dup_pairs(K, extra=()):
    """(low, high) index pairs of bitwise-identical codewords: adjacent, across a 32 boundary, across a 128 boundary,
    `extra` (an LDS image boundary), with the last code; those that fit K, no index used twice."""
    used, out = set(), []
    for a, b in [(3, 4), (31, 32), (127, 128), *extra, (10 if K > 11 else 0, K - 1)]:
        if 0 <= a < b < K and a not in used and b not in used:
            used |= {a, b}
            out.append((a, b))
    return out


class Case(NamedTuple):
    x: np.ndarray
    cbs: np.ndarray
    pairs: list
    planted: int     # rows [0, planted) are the planted ones


def make_case(B, D, K, L, seed, extra_pairs=()):
    """randn / sqrt(D) inputs and codebooks with dup_pairs(K) duplicated at every level; row 0 all zero (a padding
    item), row 1 equal to a duplicated codeword of level 0 (to the only codeword when K has no pair), then for
    each pair one row near its codeword (0.4 of the distance to the nearest other codeword away, so the residual
    stays of the input's order) — so every pair is an exact tie for at least one row."""
    g = np.random.default_rng(1000003 * seed + 131 * D + K)
    x = (g.standard_normal((B, D)) / np.sqrt(D)).astype(np.float32)
    cbs = (g.standard_normal((L, K, D)) / np.sqrt(D)).astype(np.float32)
    pairs = dup_pairs(K, extra_pairs)
    for a, b in pairs:
        cbs[:, b] = cbs[:, a]
    planted = 0
    if B >= 2 + len(pairs):
        x[0] = 0.0
        x[1] = cbs[0, pairs[0][1] if pairs else 0]
        for i, (a, b) in enumerate(pairs):
            # 0.4 of the way to the nearest other codeword at most: a (= b) stays the nearest by a clear margin
            d = np.linalg.norm(cbs[0].astype(np.float64) - cbs[0, a].astype(np.float64), axis=1)
            step = 0.4 * d[d > 0].min() / max(float(np.linalg.norm(x[2 + i])), 1e-30)
            x[2 + i] = cbs[0, a] + np.float32(min(step, 0.5)) * x[2 + i]
        planted = 2 + len(pairs)
    return Case(x, cbs, pairs, planted)


def make_grads(B, D, L, names, seed):
    """Upstream gradients of emb (L,B,D), emb_sum (B,D), residuals (L,B,D), qloss (B,): those in `names`, else None."""
    g = np.random.default_rng(7 + seed)
    full = dict(g_emb=g.standard_normal((L, B, D)).astype(np.float32),
                g_emb_sum=g.standard_normal((B, D)).astype(np.float32),
                g_res=g.standard_normal((L, B, D)).astype(np.float32),
                g_qloss=g.random(B).astype(np.float32))
    return {k: (v if k in names else None) for k, v in full.items()}


# ------------------------------------------------------------------------------------------------ the reference
class Ref64(NamedTuple):
    emb: torch.Tensor        # (L,B,D) float64
    res: torch.Tensor        # (L,B,D)
    qloss: torch.Tensor      # (B,)
    emb_sum: torch.Tensor    # (B,D)
    grad_x: torch.Tensor     # (B,D)
    grad_codebooks: torch.Tensor   # (L,K,D)
    contrib_abs: torch.Tensor      # (L,K,D): sum over a codeword's rows of the row's contribution, its terms absolute
    d_sel: torch.Tensor      # (L,B): fp64 distance of the given code from the reference's level residual
    d_min: torch.Tensor      # (L,B): fp64 minimum over the level's codewords
    d_bound: torch.Tensor    # (L,B): the id rule's allowance for that row


def _t64(a):
    if a is None:
        return None
    if torch.is_tensor(a):
        return a.detach().cpu().double()
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def id_rule(res_l, cb_l, ids_l, chunk=4096):
    """fp64 distance of each row's given code, the fp64 minimum over the codewords, and the allowance
    2 (D + 3) 2^-24 (|r| + max_k |c_k|)^2: the worst-case error of two fp32 distances |r|^2 + |c|^2 - 2 r.c
    (D + 2 roundings each in the sums and the dot product, one more in the combination; loose, but far below the
    gap to any genuinely farther code)."""
    r, c = _t64(res_l), _t64(cb_l)
    D = r.shape[1]
    c2 = (c * c).sum(1)
    sel, mn = [], []
    for s in range(0, r.shape[0], chunk):
        rr = r[s:s + chunk]
        d = ((rr * rr).sum(1, keepdim=True) + c2[None, :]) - 2.0 * (rr @ c.T)
        sel.append(d.gather(1, ids_l[s:s + chunk, None])[:, 0])
        mn.append(d.min(1).values)
    empty = torch.zeros(0, dtype=torch.float64)
    bound = 2.0 * (D + 3) * 2.0 ** -24 * (r.norm(dim=1) + c.norm(dim=1).max()) ** 2
    return torch.cat(sel) if sel else empty, torch.cat(mn) if mn else empty, bound


def rq_ref64(x, codebooks, ids, mode, beta=BETA, g_emb=None, g_emb_sum=None, g_res=None, g_qloss=None) -> Ref64:
    """The reference chain — per level Quantize.forward (L2 distance, STE / rotation trick / eval output, QuantizeLoss)
    inside RqVae.get_semantic_ids' residual loop — in float64 with autograd, taking the level's code from `ids`
    (B,L) instead of an argmin. Rotation constants u = x / (|x| + 1e-8), q = e / (|e| + 1e-8),
    w = (u + q) / max(|u + q|, 1e-6), lam = |e| / (|x| + 1e-6) are detached, as oracle/quantize.py::rotation_fwd
    states them. Gradients are those of sum(g_emb emb) + sum(g_emb_sum emb_sum) + sum(g_res res) + sum(g_qloss qloss)
    wrt x and the codebooks (zero where no gradient is given)."""
    x64 = _t64(x).requires_grad_(True)
    cb = _t64(codebooks).requires_grad_(True)
    ids = torch.as_tensor(np.asarray(ids)).long()
    B, D = x64.shape
    L, K, _ = cb.shape
    res, qloss = x64, torch.zeros(B, dtype=torch.float64)
    embs, ress, picked, rule = [], [], [], []
    for l in range(L):
        ress.append(res)
        e = cb[l][ids[:, l]]
        picked.append(e)
        if l > 0:
            res.retain_grad()
        rule.append(id_rule(res, cb[l], ids[:, l]))
        if mode == MODE_ROTATION:
            xd, ed = res.detach(), e.detach()
            xn, en = xd.norm(dim=1, keepdim=True), ed.norm(dim=1, keepdim=True)
            u, q = xd / (xn + 1e-8), ed / (en + 1e-8)
            s = u + q
            w = s / s.norm(dim=1, keepdim=True).clamp_min(1e-6)
            lam = en / (xn + 1e-6)
            out = ((res - 2.0 * (res * w).sum(1, keepdim=True) * w) + 2.0 * (res * u).sum(1, keepdim=True) * q) * lam
        elif mode == MODE_STE:
            out = res + (e - res).detach()
        elif mode == MODE_EVAL:
            out = e
        else:
            raise ValueError(mode)
        qloss = qloss + ((res.detach() - e) ** 2).sum(1) + beta * ((res - e.detach()) ** 2).sum(1)
        embs.append(out)
        res = res - out
    emb, resv = torch.stack(embs), torch.stack(ress)
    emb_sum = emb.sum(0)
    total = None
    for g, v in ((g_emb, emb), (g_emb_sum, emb_sum), (g_res, resv), (g_qloss, qloss)):
        if g is not None:
            t = (_t64(g) * v).sum()
            total = t if total is None else total + t
    if total is not None and total.requires_grad and B > 0:
        total.backward()
    # a row's contribution to its codeword's gradient, term by term in absolute value: 2 gl e and 2 gl res (the loss)
    # and, in eval mode, the upstream gradients of the level's output (g_emb, g_emb_sum, the next residual's)
    gl = torch.zeros(B, 1, dtype=torch.float64) if g_qloss is None else _t64(g_qloss).abs()[:, None]
    contrib_abs = []
    for l, e in enumerate(picked):
        a = 2.0 * gl * (e.detach().abs() + ress[l].detach().abs())
        if mode == MODE_EVAL:
            for t in (None if g_emb is None else _t64(g_emb)[l], _t64(g_emb_sum), ress[l + 1].grad if l + 1 < L else None):
                if t is not None:
                    a = a + t.abs()
        contrib_abs.append(torch.zeros(K, D, dtype=torch.float64).index_add_(0, ids[:, l], a))
    contrib_abs = torch.stack(contrib_abs)
    return Ref64(emb.detach(), resv.detach(), qloss.detach(), emb_sum.detach(),
                 torch.zeros_like(x64) if x64.grad is None else x64.grad,
                 torch.zeros_like(cb) if cb.grad is None else cb.grad, contrib_abs,
                 *(torch.stack([r[i] for r in rule]) for i in range(3)))


# ------------------------------------------------------------------------------------------------ the checks
def check_ids(ids, res, cbs, pairs=(), what=""):
    """The id rule on the residuals the choice was made from, and the tie rule: a code that has a bitwise-identical
    codeword below it is never returned. Returns (largest excess of the chosen distance over the minimum as a share
    of the allowance, pairs of identical codewords some row of level 0 took, i.e. exact ties that were decided)."""
    ids = torch.as_tensor(np.asarray(ids)).long()
    cb32 = np.asarray(cbs, dtype=np.float32)
    L, K, _ = cb32.shape
    assert int(ids.min()) >= 0 and int(ids.max()) < K, f"{what}: ids outside [0, K)"
    worst, tied = 0.0, 0
    for l in range(L):
        sel, mn, bound = id_rule(res[l], cbs[l], ids[:, l])
        over = sel - mn
        bad = over > bound
        assert not bool(bad.any()), (f"{what}: level {l}: {int(bad.sum())} rows with a code farther than the fp64 minimum by "
                                     f"more than the fp32 allowance, worst {float((over / bound).max()):.3g} x")
        if over.numel():
            worst = max(worst, float((over / bound.clamp_min(1e-300)).max()))
        # lowest index among bitwise-identical codewords
        first = np.arange(K)
        _, inv = np.unique(cb32[l].view(np.uint32), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        lowest = np.full(inv.max() + 1, K)
        np.minimum.at(lowest, inv, first)
        want = lowest[inv][ids[:, l].numpy()]
        wrong = want != ids[:, l].numpy()
        assert not wrong.any(), f"{what}: level {l}: rows {np.nonzero(wrong)[0][:8]} took the higher of two identical codewords"
        if l == 0:
            tied = len({a for a, _ in pairs} & set(ids[:, 0].tolist()))
    return worst, tied


def collapsed_rows(ref: Ref64, mode):
    """(L,B) bool: (level, row) pairs whose reference input is not determined to the contract's accuracy. A rotation
    level's output depends on the direction of its input and, below |x| ~ 1e-6, on its length (lam = |e| / (|x| +
    1e-6)). Where the reference residual of a row collapses below the contract's own error on the operands it is the
    difference of (0 < max|res[l+1]| < 2e-5 max|res[l]|: the row equal to a codeword), fp32 rounding of res[l] - emb[l]
    decides that input, and no fp32 chain can follow the fp64 one from there. The criterion reads the reference only.
    Such a row keeps the id rule, the bitwise residual identities and qloss; its emb / res from that level on, its
    emb_sum and its grad_x are not compared. An exactly zero residual (the zero row; STE and eval on the codeword
    row) is exact in fp32 as well and is compared."""
    L, B, _ = ref.res.shape
    out = torch.zeros(L, B, dtype=torch.bool)
    if mode != MODE_ROTATION:
        return out
    m = ref.res.abs().amax(2)
    for l in range(1, L):
        out[l] = out[l - 1] | ((m[l] > 0) & (m[l] < RTOL_OUT * m[l - 1]))
    return out


def collapsed_downstream(skip, ids, K):
    """What else a collapsed row leaves undetermined when it collapses before the last level (never at L = 2): its
    qloss (B,) bool — the loss term of level l + 1 reads res[l] - emb[l] — and the codewords (L,K) bool that row takes
    at those levels, whose gradient holds 2 gl (e - res)."""
    L, B = skip.shape
    ids = torch.as_tensor(np.asarray(ids)).long()
    q = skip[L - 2].clone() if L >= 2 else torch.zeros(B, dtype=torch.bool)
    cw = torch.zeros(L, K, dtype=torch.bool)
    for l in range(1, L):
        cw[l, ids[skip[l - 1], l]] = True
    return q, cw


def _ulp32(m):
    return torch.from_numpy(np.spacing(m.numpy().astype(np.float32)).astype(np.float64))


def check_rows(got, ref, rtol, what, skip=None, ulp=True):
    """|got - ref| <= rtol max|ref| (+ one fp32 ulp of it) with the maximum over the row (the last axis; a vector is
    one value per row). Returns the largest error as a share of the row's maximum."""
    got, ref = _t64(got), _t64(ref)
    if ref.dim() == 1:
        got, ref = got[:, None], ref[:, None]
    err = (got - ref).abs().amax(-1)
    m = ref.abs().amax(-1)
    tol = rtol * m + (_ulp32(m) if ulp else 0.0)
    bad = err > tol
    if skip is not None:
        bad &= ~skip
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} rows off, worst {float((err / tol.clamp_min(1e-300))[bad].max()):.3g} x "
                                 f"the bound, first at {tuple(int(i) for i in torch.nonzero(bad)[0])}")
    keep = m > 0 if skip is None else (m > 0) & ~skip
    return float((err[keep] / m[keep]).max()) if bool(keep.any()) else 0.0


def check_grad_codebooks(got, ref: Ref64, what, skip_cw=None):
    """|got - ref| <= 2e-4 sum_b |c_b| of that codeword, level and column, the absolute contributions, so cancellation
    cannot fail a correct sum. A contribution c_b = 2 gl (e - res) (+ the output's upstream gradients in eval mode) is
    itself a difference, and res carries the fp32 rounding of the residual chain: |c_b| is taken term by term,
    2 |gl| (|e| + |res|) (+ |g_emb| + |g_emb_sum| + |g_res_next|), as test_rmsnorm_fused_matches_fp64 takes its products.
    With the difference's own absolute value a single-row codeword fails wherever e - res happens to cancel in a column
    (measured: 1 element of 10,240 at 1.4 x, D = 128, rotation). A codeword no row took gets an exact zero. Returns
    the largest error as a share of that sum."""
    got = _t64(got)
    err = (got - ref.grad_codebooks).abs()
    scale = ref.contrib_abs
    bad = err > RTOL_GRAD * scale
    keep = scale > 0
    if skip_cw is not None:
        bad &= ~skip_cw[:, :, None]
        keep &= ~skip_cw[:, :, None]
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements off, worst "
                                 f"{float((err / (RTOL_GRAD * scale).clamp_min(1e-300))[bad].max()):.3g} x the bound")
    return float((err[keep] / scale[keep]).max()) if bool(keep.any()) else 0.0


def check_forward(out, case: Case, mode, ref: Ref64, what, beta=BETA):
    """Every forward check of one launch: out = dict(ids, emb, res, qloss, emb_sum) as numpy / torch on the host.
    Returns the measured errors."""
    x, cbs = case.x, case.cbs
    res32, emb32 = np.asarray(out["res"], np.float32), np.asarray(out["emb"], np.float32)
    L = cbs.shape[0]
    over, tied = check_ids(out["ids"], res32, cbs, case.pairs, what)
    if case.planted:
        assert tied == len(case.pairs), f"{what}: only {tied} of {len(case.pairs)} duplicated codewords taken by a row"
    assert np.array_equal(res32[0].view(np.uint32), x.view(np.uint32)), f"{what}: res[0] != x"
    for l in range(L - 1):
        assert np.array_equal(res32[l + 1], (res32[l] - emb32[l]).astype(np.float32)), f"{what}: res[{l + 1}] != res - emb"
    skip = collapsed_rows(ref, mode)
    assert int(skip.any(0).sum()) <= 1, f"{what}: {int(skip.any(0).sum())} rows with a collapsed residual"
    skip_q, _ = collapsed_downstream(skip, out["ids"], cbs.shape[1])
    m = dict(ids=over,
             emb=check_rows(emb32, ref.emb, RTOL_OUT, f"{what} emb", skip),
             res=check_rows(res32, ref.res, RTOL_OUT, f"{what} res", skip),
             qloss=check_rows(out["qloss"], ref.qloss, RTOL_OUT, f"{what} qloss", skip_q),
             emb_sum=check_rows(out["emb_sum"], ref.emb_sum, RTOL_OUT, f"{what} emb_sum", skip.any(0)))
    return m
