"""Every kernel form of the residual-quantize path (csrc/rq_quantize.hip) and every upstream-gradient input against the
fp64 reference that follows the kernel's own ids (tests/quantize_support.py): no row is left out for a near-tie. The
form each case reaches is asked of rq_quantize_{fwd,bwd}_plan, not restated, and the union over the case table is the
list of instantiated forms.

Bounds: the project's contract (tests/test_quantize_gpu.py), per row — 2e-5 of the row's maximum (+ one fp32 ulp) on
emb / res / qloss / emb_sum, 2e-4 of the row's maximum on grad_x, 2e-4 of the codeword's summed absolute contributions
(each column's, taken term by term: quantize_support.check_grad_codebooks) on grad_codebooks. The fp32 oracle's own
error against the same reference (test_quantize_ref_host.py, relative to the maximum) is 6.9e-7 on the outputs, 7.8e-7
on grad_x and 1.2e-6 on grad_codebooks.
Largest errors measured on an MI355X, as a share of the scales above (every mode; rotation sets each of them):
  forward   tiled:    emb 7.0e-7, res 1.5e-6, qloss 4.2e-7, emb_sum 8.0e-7
            register: emb 1.3e-6, res 2.9e-6, qloss 1.2e-6, emb_sum 1.6e-6
            split:    emb 6.7e-7, res 1.5e-6, qloss 2.4e-7, emb_sum 6.4e-7
            16x16:    emb 7.3e-7, res 8.6e-7, qloss 3.5e-7, emb_sum 7.9e-7, emb_norms 7.5e-7
  backward  rows kernel: grad_x 8.4e-7; codebook gradient: sort route, direct 5.3e-5 (a codeword with one row, in a
            column where both e and res are a hundredth of the row's size: the rotation's error in res is relative to
            the row), heavy 1.5e-7; chunk route 3.0e-5
The id rule's excess (chosen fp64 distance over the fp64 minimum) stays below 5e-11 of its allowance: every row took
the fp64 nearest code or an exact tie's lowest index."""
import numpy as np
import pytest
import torch

import quantize_support as S

pytestmark = pytest.mark.gpu

_REACHED_BWD = {}


def _launch_fwd(device, data, K, mode, impl, norms):
    from rqvae_hip._lib import call, ptr, stream_handle
    B, D = data.x.shape
    L = data.cbs.shape[0]
    xt, ct = torch.from_numpy(data.x).to(device), torch.from_numpy(data.cbs).to(device)
    csq = torch.empty(L, K, device=device)
    s = stream_handle(device)
    call("rq_codebook_sqnorm", ptr(ct), L * K, D, ptr(csq), s)
    o = dict(ids=torch.full((B, L), -1, dtype=torch.int64, device=device),
             emb=torch.full((L, B, D), float("nan"), device=device), res=torch.full((L, B, D), float("nan"), device=device),
             qloss=torch.full((B,), float("nan"), device=device), emb_sum=torch.full((B, D), float("nan"), device=device))
    if norms:
        o["emb_norms"] = torch.full((L, B), float("nan"), device=device)
    call("rq_quantize_fwd", ptr(xt), B, D, ptr(ct), ptr(csq), K, L, mode, S.BETA, ptr(o["ids"]), ptr(o["emb"]),
         ptr(o["res"]), ptr(o["qloss"]), ptr(o["emb_sum"]), ptr(o.get("emb_norms")), impl, s)
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("case", S.FWD_CASES, ids=lambda c: c.id)
def test_forward_form_vs_fp64(device, case, mode):
    """One forced-impl launch of the form the case names (asked of the plan), L = 2: the id rule and the lowest index
    among identical codewords (planted exact ties: adjacent, across 32, across 128, across the streamed image's edge,
    with the last code), every output row against fp64, res[0] == x and res[l+1] == fp32(res[l] - emb[l]) bitwise."""
    K = S.smallest_streaming_K(case.D, case.B) if case.K == "stream" else case.K
    rc, form = S.fwd_plan(case.B, case.D, K, 2, mode, case.impl, case.norms)
    assert rc == 0 and S.fwd_form_key(form) == case.form, (rc, form)
    assert form.norms_pass == 0
    extra = ((form.nb - 1, form.nb),) if case.impl == S.IMPL_REG and not form.resident else ()
    data = S.make_case(case.B, case.D, K, 2, seed=11, extra_pairs=extra)
    assert not extra or extra[0] in data.pairs
    out = _launch_fwd(device, data, K, mode, case.impl, case.norms)
    ref = S.rq_ref64(data.x, data.cbs, out["ids"], mode, S.BETA)
    what = f"{case.id} mode {mode}"
    assert bool((ref.d_sel - ref.d_min <= ref.d_bound).all()), f"{what}: id rule on the reference's residuals"
    m = S.check_forward(out, data, mode, ref, what)
    if case.norms:
        skip = S.collapsed_rows(ref, mode)
        m["emb_norms"] = S.check_rows(out["emb_norms"].reshape(-1), ref.emb.norm(dim=2).reshape(-1), S.RTOL_OUT,
                                      f"{what} emb_norms", skip.reshape(-1))
    print(f"\n[fwd] {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))


def test_forward_norms_pass_changes_nothing(device):
    """emb_norms asked of a kernel that does not fuse them (the plan's norms_pass): same outputs bitwise, norms within
    the contract."""
    rc, form = S.fwd_plan(131, 32, 40, 2, S.MODE_ROTATION, S.IMPL_REG, True)
    assert rc == 0 and form.norms_pass == 1
    data = S.make_case(131, 32, 40, 2, seed=11)
    a = _launch_fwd(device, data, 40, S.MODE_ROTATION, S.IMPL_REG, False)
    b = _launch_fwd(device, data, 40, S.MODE_ROTATION, S.IMPL_REG, True)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    S.check_rows(b["emb_norms"].reshape(-1), torch.from_numpy(b["emb"]).double().norm(dim=2).reshape(-1), S.RTOL_OUT, "norms")


def _run_bwd(device, case, data, g):
    from rqvae_hip import ops
    xt = torch.from_numpy(data.x).to(device).requires_grad_(True)
    ct = torch.from_numpy(data.cbs).to(device).requires_grad_(True)
    emb, res, ids, ql, es = ops.rq_quantize(xt, ct, case.mode, S.BETA)
    outs = dict(g_emb=emb, g_emb_sum=es, g_res=res, g_qloss=ql)
    total = sum((outs[n] * torch.from_numpy(g[n]).to(device)).sum() for n in case.grads)   # the others arrive as None
    total.backward()
    return dict(ids=ids.cpu().numpy(), emb=emb.detach().cpu().numpy(), res=res.detach().cpu().numpy(),
                qloss=ql.detach().cpu().numpy(), emb_sum=es.detach().cpu().numpy(), grad_x=xt.grad.cpu().numpy(),
                grad_codebooks=ct.grad.cpu().numpy())


def _bwd_reached(case, ids):
    rc, form = S.bwd_plan(case.B, case.D, case.K, case.L, case.mode, "g_qloss" in case.grads)
    assert rc == 0, S.last_error()
    _REACHED_BWD[case] = S.bwd_form_keys(form, ids, case.K)
    return _REACHED_BWD[case]


@pytest.mark.parametrize("case", S.BWD_CASES, ids=lambda c: c.id)
def test_backward_form_vs_fp64(device, case):
    """ops.rq_quantize + autograd with the case's upstream gradients (the others None -> NULL), twice: bitwise equal
    runs, the forms the case names reached (plan + segment lengths of the ids), the forward checks of the auto-chosen
    kernel, grad_x per row and grad_codebooks per codeword against fp64."""
    data = S.make_case(case.B, case.D, case.K, case.L, seed=23)
    g = S.make_grads(case.B, case.D, case.L, case.grads, seed=case.B + case.D)
    a, b = _run_bwd(device, case, data, g), _run_bwd(device, case, data, g)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{case.id}: {k} differs between two runs"
    reached = _bwd_reached(case, a["ids"])
    assert set(case.forms) <= reached, (case.forms, reached)
    ref = S.rq_ref64(data.x, data.cbs, a["ids"], case.mode, S.BETA, **g)
    m = S.check_forward(a, data, case.mode, ref, case.id)
    skip = S.collapsed_rows(ref, case.mode)
    _, skip_cw = S.collapsed_downstream(skip, a["ids"], case.K)
    m["grad_x"] = S.check_rows(a["grad_x"], ref.grad_x, S.RTOL_GRAD, f"{case.id} grad_x", skip.any(0), ulp=False)
    m["grad_codebooks"] = S.check_grad_codebooks(a["grad_codebooks"], ref, f"{case.id} grad_codebooks", skip_cw)
    print(f"\n[bwd] {case.id} {sorted(reached)}: " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))


def test_backward_empty_batch(device):
    """B = 0 through ops.rq_quantize and autograd: empty grad_x, grad_codebooks written as zeros."""
    from rqvae_hip import ops
    xt = torch.zeros(0, 64, device=device, requires_grad=True)
    ct = torch.randn(2, 40, 64, device=device).requires_grad_(True)
    emb, res, ids, ql, es = ops.rq_quantize(xt, ct, S.MODE_ROTATION, S.BETA)
    assert emb.shape == (2, 0, 64) and ids.shape == (0, 2)
    (es.sum() + ql.sum() + emb.sum() + res.sum()).backward()
    assert xt.grad.shape == (0, 64) and ct.grad.shape == (2, 40, 64) and int(torch.count_nonzero(ct.grad)) == 0
    assert S.bwd_plan(0, 64, 40)[1].route == S.CB_NONE


def test_case_table_reaches_every_form(device):
    """The union of the forms the case table reaches — forward from the plan, backward from the plan and the ids of a
    forward run — is the list of instantiated forms; nothing is left out."""
    from rqvae_hip import ops
    fwd = set()
    for c in S.FWD_CASES:
        K = S.smallest_streaming_K(c.D, c.B) if c.K == "stream" else c.K
        rc, form = S.fwd_plan(c.B, c.D, K, 2, S.MODE_ROTATION, c.impl, c.norms)
        assert rc == 0 and S.fwd_form_key(form) == c.form
        fwd.add(c.form)
    assert fwd | S.FWD_FORMS_LEFT_OUT == S.FWD_FORMS and not fwd & S.FWD_FORMS_LEFT_OUT, sorted(S.FWD_FORMS ^ fwd)
    bwd = set()
    for c in S.BWD_CASES:
        if c not in _REACHED_BWD:
            data = S.make_case(c.B, c.D, c.K, c.L, seed=23)
            with torch.no_grad():
                ids = ops.rq_quantize(torch.from_numpy(data.x).to(device), torch.from_numpy(data.cbs).to(device),
                                      c.mode, S.BETA)[2]
            _bwd_reached(c, ids.cpu().numpy())
        assert set(c.forms) <= _REACHED_BWD[c], c
        bwd |= _REACHED_BWD[c]
    assert bwd | S.BWD_FORMS_LEFT_OUT == S.BWD_FORMS and not bwd & S.BWD_FORMS_LEFT_OUT, sorted(S.BWD_FORMS ^ bwd)
