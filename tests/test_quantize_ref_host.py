"""The quantize tests' fp64 reference and plan queries on the host, no GPU: rq_ref64 (tests/quantize_support.py)
against the pinned fp32 oracle (oracle/quantize.py) with the oracle's own ids, rq_quantize_{fwd,bwd}_plan at both
sides of every dispatch threshold, the refusals, and the case table against the list of instantiated forms."""
import numpy as np
import pytest
import torch

import quantize_support as S
from oracle import quantize as Q
from quantize_support import CB_CHUNK, CB_NONE, CB_SORT, IMPL_R16, IMPL_REG, IMPL_SPLIT, IMPL_TILED, MODE_EVAL, MODE_ROTATION, MODE_STE

# The oracle's own error against fp64 as the issue that asked for this file measured it (D in {8, 64, 256, 1024},
# L 2-3, every mode, one zero row): 6.1e-7 on emb / res relative to the maximum, 5e-7 on grad_x (per row) and
# grad_codebooks. The bounds here are four times those figures.
ORACLE_OUT, ORACLE_GRAD = 4 * 6.1e-7, 4 * 5e-7

# (B, D, K, L): the case table's shapes a numpy oracle handles in well under a second
_SHAPES = sorted({(c.B, c.D, c.K, 2) for c in S.FWD_CASES if c.B <= 257 and c.K != "stream"} |
                 {(c.B, c.D, c.K, c.L) for c in S.BWD_CASES if c.B * c.D <= 5000 * 64} | {(300, 64, 40, 3)})


@pytest.mark.parametrize("mode", S.MODES)
def test_ref64_vs_oracle(mode):
    """rq_ref64 fed the oracle's ids against oracle/quantize.py::rq_fwd / rq_bwd (all four upstream gradients, g_res
    through rq_bwd's new argument) on every CPU-sized shape of the case table, planted rows included: the id and tie
    rules hold for the oracle's ids, outputs within 4 x 6.1e-7 of the maximum, grad_x within 4 x 5e-7 of the row's
    maximum, grad_codebooks within 4 x 5e-7 of the maximum.
    Measured (largest over the shapes; eval / STE / rotation): emb 0 / 1.2e-7 / 6.9e-7, res 6.9e-8 / 6.9e-8 / 4.4e-7,
    qloss 1.4e-7 / 1.4e-7 / 2.7e-7, grad_x 1.5e-7 / 2.8e-7 / 7.8e-7, grad_codebooks 1.2e-6 / 1.1e-6 / 1.1e-6 (the
    oracle's serial fp32 index-add over up to 5,000 rows a codeword).
    The row equal to a codeword is the one collapsed row of every rotation case (quantize_support.collapsed_rows):
    the oracle's level-1 input there is fp32 rounding noise of about 1e-8 against the reference's 1e-17."""
    worst = dict(emb=0.0, res=0.0, qloss=0.0, grad_x=0.0, grad_codebooks=0.0)
    for B, D, K, L in _SHAPES:
        case = S.make_case(B, D, K, L, seed=1)
        g = S.make_grads(B, D, L, S.ALL_G, seed=B + D)
        f = Q.rq_fwd(case.x, case.cbs, mode, S.BETA)
        gx, gcb = Q.rq_bwd(f, case.cbs, mode, g_emb_sum=g["g_emb_sum"], g_emb=g["g_emb"], g_qloss=g["g_qloss"],
                           beta=S.BETA, g_res=g["g_res"])
        ref = S.rq_ref64(case.x, case.cbs, f["ids"], mode, S.BETA, **g)
        what = f"{(B, D, K, L)} mode {mode}"
        S.check_ids(f["ids"], f["res"], case.cbs, case.pairs, what)
        assert bool((ref.d_sel - ref.d_min <= ref.d_bound).all()), what
        skip = S.collapsed_rows(ref, mode)
        assert int(skip.any(0).sum()) <= 1
        keep = ~skip
        skip_q, skip_cw = S.collapsed_downstream(skip, f["ids"], K)
        for name, got, want in (("emb", f["emb"], ref.emb), ("res", f["res"], ref.res)):
            err = (torch.from_numpy(got).double() - want).abs().amax(-1)
            worst[name] = max(worst[name], float(err[keep].max() / want.abs().max()))
        worst["qloss"] = max(worst["qloss"], float((torch.from_numpy(f["qloss"]).double() - ref.qloss).abs()[~skip_q].max()
                                                   / ref.qloss.abs().max()))
        rows = ~skip.any(0)
        err = (torch.from_numpy(gx).double() - ref.grad_x).abs().amax(-1)
        m = ref.grad_x.abs().amax(-1)
        ok = rows & (m > 0)
        worst["grad_x"] = max(worst["grad_x"], float((err[ok] / m[ok]).max()))
        assert bool((err[rows & (m == 0)] == 0).all())
        worst["grad_codebooks"] = max(worst["grad_codebooks"], float(
            (torch.from_numpy(gcb).double() - ref.grad_codebooks).abs()[~skip_cw].max() / ref.grad_codebooks.abs().max()))
    print(f"mode {mode}: oracle vs fp64 " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["emb"] <= ORACLE_OUT and worst["res"] <= ORACLE_OUT and worst["qloss"] <= ORACLE_OUT, worst
    assert worst["grad_x"] <= ORACLE_GRAD and worst["grad_codebooks"] <= ORACLE_GRAD, worst


def test_ref64_gradient_inputs_are_separate():
    """Each upstream gradient alone, and none: the reference's gradients are linear in them (the sum of the four
    single-gradient results is the all-four result) and zero without any — so a dropped or doubled input shows."""
    case = S.make_case(64, 16, 12, 3, seed=2)
    ids = Q.rq_fwd(case.x, case.cbs, MODE_ROTATION, S.BETA)["ids"]
    g = S.make_grads(64, 16, 3, S.ALL_G, seed=5)
    full = S.rq_ref64(case.x, case.cbs, ids, MODE_ROTATION, S.BETA, **g)
    parts = [S.rq_ref64(case.x, case.cbs, ids, MODE_ROTATION, S.BETA, **{n: g[n]}) for n in S.ALL_G]
    for name in ("grad_x", "grad_codebooks"):
        total = sum(getattr(p, name) for p in parts)
        scale = max(float(getattr(p, name).abs().max()) for p in parts)   # the zero row's lam = |e| / 1e-6 sets it
        # every input reaches x; in rotation mode only the loss reaches the codebooks (u, q, w, lam are detached)
        live = [float(getattr(p, name).abs().max()) > 0 for p in parts]
        assert live == ([True] * 4 if name == "grad_x" else [False, False, False, True]), (name, live)
        assert float((total - getattr(full, name)).abs().max()) <= 1e-12 * scale, name
    none = S.rq_ref64(case.x, case.cbs, ids, MODE_ROTATION, S.BETA)
    assert float(none.grad_x.abs().max()) == 0 and float(none.grad_codebooks.abs().max()) == 0


def test_ref64_rejects_a_wrong_code_and_a_high_tie():
    """The id rule fails a code that is not the nearest, and the tie rule fails the higher of two identical codewords."""
    case = S.make_case(40, 16, 12, 2, seed=3)
    f = Q.rq_fwd(case.x, case.cbs, MODE_EVAL, S.BETA)
    S.check_ids(f["ids"], f["res"], case.cbs, case.pairs)
    ids = f["ids"].copy()
    ids[7, 0] = (ids[7, 0] + 5) % 12 if (ids[7, 0] + 5) % 12 not in (4, 11) else 6
    with pytest.raises(AssertionError, match="farther than the fp64 minimum"):
        S.check_ids(ids, f["res"], case.cbs, case.pairs)
    a, b = case.pairs[0]
    ids = f["ids"].copy()
    row = int(np.nonzero(ids[:, 0] == a)[0][0])
    ids[row, 0] = b
    with pytest.raises(AssertionError, match="higher of two identical codewords"):
        S.check_ids(ids, f["res"], case.cbs, case.pairs)


# ------------------------------------------------------------------------------------------------ the plan
def _fwd(B, D, K, impl=0, mode=MODE_ROTATION, norms=False, L=2):
    rc, f = S.fwd_plan(B, D, K, L, mode, impl, norms)
    assert rc == 0, S.last_error()
    return f


def _bwd(B, D, K, mode=MODE_ROTATION, gq=True, L=2):
    rc, f = S.bwd_plan(B, D, K, L, mode, gq)
    assert rc == 0, S.last_error()
    return f


def test_fwd_plan_boundaries():
    # auto: 16x16 from B = 32768 at D = 64, K <= 288; register for D <= 64; split where its scratch fits; else tiled
    assert S.fwd_form_key(_fwd(32767, 64, 256)) == ("reg", 64, 1, 2)
    assert S.fwd_form_key(_fwd(32768, 64, 256)) == ("r16", 64)
    assert S.fwd_form_key(_fwd(32769, 64, 288)) == ("r16", 64)
    assert S.fwd_form_key(_fwd(32769, 64, 289)) == ("reg", 64, 0, 1)
    assert S.fwd_form_key(_fwd(32769, 32, 256)) == ("reg", 32, 1, 1)
    assert S.fwd_form_key(_fwd(100, 128, 130)) == ("split", 128)
    assert S.fwd_form_key(_fwd(100, 128, 63 * 128)) == ("split", 128)        # 2 * 63 + 1 = 127 <= 128
    assert S.fwd_form_key(_fwd(100, 128, 63 * 128 + 1)) == ("tiled", 128)    # 64 blocks: 129 > 128
    # register: waves per 32-item tile by B
    for B, w in ((8192, 4), (8193, 2), (32767, 2), (32768, 2), (32769, 1)):
        f = _fwd(B, 32, 40, impl=IMPL_REG)
        assert (f.wpi, f.items, f.grid) == (w, 128 // w, -(-B // (128 // w))), (B, f)
    # register: K at and past each D's LDS fit (the codebook rounded up to 32 rows, D + 5 floats a row but for the
    # swizzled D = 64 image, in 75 KiB less 1 KiB)
    for D in (8, 16, 32, 64):
        fit = (75 * 1024 - 1024) // ((D + 5) * 4) // 32 * 32
        K = S.smallest_streaming_K(D)
        assert K == fit + 1, (D, K, fit)
        a, b = _fwd(131, D, K - 1, impl=IMPL_REG), _fwd(131, D, K, impl=IMPL_REG)
        assert (a.resident, a.nb) == (1, K - 1) and (b.resident, b.nb) == (0, fit)
        assert max(a.lds_bytes, b.lds_bytes) <= 75 * 1024
    # emb_norms: fused by the 16x16 kernel only
    assert _fwd(129, 64, 40, impl=IMPL_R16, norms=True).norms_pass == 0
    assert _fwd(129, 64, 40, impl=IMPL_REG, norms=True).norms_pass == 1
    assert _fwd(129, 64, 40, impl=IMPL_REG).norms_pass == 0
    f = _fwd(257, 64, 288, impl=IMPL_R16)
    assert (f.items, f.grid, f.lds_bytes) == (128, 3, 288 * 65 * 4)
    # the mode changes no launch; B == 0 launches nothing
    assert len({_fwd(131, 64, 40, mode=m) for m in S.MODES}) == 1
    assert _fwd(0, 64, 40) == S.FwdForm(*([0] * 9))


def test_bwd_plan_boundaries():
    chunk = lambda f: (f.route, f.vpl, f.chunks)   # noqa: E731
    assert chunk(_bwd(4095, 64, 256)) == (CB_SORT, 0, 0)
    assert chunk(_bwd(4096, 64, 256)) == (CB_CHUNK, 1, 4)
    assert chunk(_bwd(4097, 64, 256)) == (CB_CHUNK, 1, 5)
    assert chunk(_bwd(5000, 128, 128)) == (CB_CHUNK, 2, 5)          # K D = 16384
    assert chunk(_bwd(5000, 256, 64)) == (CB_CHUNK, 4, 5)
    assert chunk(_bwd(5000, 64, 257)) == (CB_SORT, 0, 0)            # K D = 16448
    assert chunk(_bwd(5000, 128, 129)) == (CB_SORT, 0, 0)
    assert chunk(_bwd(5000, 32, 256)) == (CB_SORT, 0, 0) and chunk(_bwd(5000, 512, 32)) == (CB_SORT, 0, 0)
    assert chunk(_bwd(5000, 64, 256, mode=MODE_STE)) == (CB_CHUNK, 1, 5)
    assert chunk(_bwd(5000, 64, 256, mode=MODE_EVAL)) == (CB_SORT, 0, 0)
    assert chunk(_bwd(5000, 64, 256, gq=False)) == (CB_SORT, 0, 0)
    assert _bwd(5000, 64, 256, mode=MODE_EVAL).contrib == 1 and _bwd(5000, 64, 256, gq=False).contrib == 0
    f = _bwd(100, 64, 256)
    assert (f.seg_direct, f.seg_split) == (256, 8)
    for D in (8, 16, 32, 64, 128, 256, 512, 1024):
        f = _bwd(100, D, 40)
        assert f.lpi * f.epl == D and f.lpi == min(D // 4, 64)
    assert _bwd(0, 64, 256) == S.BwdForm(*([0] * 8))
    assert _bwd(0, 64, 256).route == CB_NONE


def test_plan_refusals():
    for D in (0, 4, 12, 48, 100, 2048):
        assert S.fwd_plan(131, D, 40)[0] == -22 and "power of two in [8, 1024]" in S.last_error()
        assert S.bwd_plan(131, D, 40)[0] == -22 and "power of two in [8, 1024]" in S.last_error()
    assert S.fwd_plan(131, 64, 289, impl=IMPL_R16)[0] == -22 and "K <= 288" in S.last_error()
    assert S.fwd_plan(131, 64, 288, impl=IMPL_R16)[0] == 0
    assert S.fwd_plan(131, 32, 40, impl=IMPL_R16)[0] == -22
    assert S.fwd_plan(131, 128, 64 * 128, impl=IMPL_SPLIT)[0] == -22 and "2*ceil(K/128)+1 <= D" in S.last_error()
    assert S.fwd_plan(131, 128, 63 * 128, impl=IMPL_SPLIT)[0] == 0
    assert S.fwd_plan(131, 64, 40, impl=IMPL_SPLIT)[0] == -22
    assert S.fwd_plan(131, 128, 40, impl=IMPL_REG)[0] == -22 and "D <= 64" in S.last_error()
    assert S.fwd_plan(131, 64, 40, impl=5)[0] == -22 and S.fwd_plan(131, 64, 40, impl=-1)[0] == -22
    assert S.fwd_plan(131, 64, 0)[0] == -22 and S.fwd_plan(131, 64, 40, L=65)[0] == -22
    assert S.fwd_plan(131, 64, 40, mode=1)[0] == -22 and S.bwd_plan(131, 64, 40, mode=1)[0] == -22
    assert S.fwd_plan(-1, 64, 40)[0] == -22 and S.bwd_plan(1 << 31, 64, 40)[0] == -22
    assert S.bwd_plan(131, 64, 4097)[0] == -22
    from rqvae_hip import _lib
    assert _lib.load().rq_quantize_fwd_plan(131, 64, 40, 2, 3, 0, 0, None) == -22
    assert _lib.load().rq_quantize_bwd_plan(131, 64, 40, 2, 3, 1, None) == -22
    assert _lib.load().rq_abi_version() == 4


def test_case_table_names_every_form():
    """Every forward case plans to the form it names (the backward's sort branches depend on the ids: checked on the
    GPU), and the union over the table is the list of instantiated forms, nothing left out."""
    reached = set()
    for c in S.FWD_CASES:
        K = S.smallest_streaming_K(c.D, c.B) if c.K == "stream" else c.K
        for mode in S.MODES:
            f = _fwd(c.B, c.D, K, impl=c.impl, mode=mode, norms=c.norms)
            assert S.fwd_form_key(f) == c.form, (c, f)
        if c.impl == IMPL_R16:
            assert (c.B - 1) % f.items == 0
        reached.add(c.form)
    assert not S.FWD_FORMS_LEFT_OUT and reached == S.FWD_FORMS, sorted(S.FWD_FORMS ^ reached)
    named = set()
    for c in S.BWD_CASES:
        f = _bwd(c.B, c.D, c.K, mode=c.mode, gq="g_qloss" in c.grads, L=c.L)
        rows, cb = c.forms
        assert ("rows", f.lpi, f.epl) == rows, (c, f)
        assert (f.route == CB_CHUNK and cb == ("chunk", f.vpl)) or \
            (f.route == CB_SORT and cb[0] == "sort" and (cb[2] == "contrib") == bool(f.contrib)), (c, f)
        named |= set(c.forms)
    assert not S.BWD_FORMS_LEFT_OUT and named == S.BWD_FORMS, sorted(S.BWD_FORMS ^ named)
    assert all(impl in (IMPL_TILED, IMPL_REG, IMPL_SPLIT, IMPL_R16) for impl in {c.impl for c in S.FWD_CASES})
