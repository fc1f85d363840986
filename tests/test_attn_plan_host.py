"""varlen_attn_plan (csrc/attention_plan.h through the C ABI) on the host, no GPU: workspace sizes against the sizes
recorded from the library before the plan existed (golden/attn_ws_elems.json), workspace layouts, the launcher's
instantiation set, the DESIGN.md dispatch table at both sides of every threshold, and the launch sequences recorded
from that earlier library on an MI355X (golden/attn_launches.json)."""
import ctypes
import json
import os

import pytest

import attn_plan_support as S
from attn_plan_support import FEWQ_WG, LPT_SHORT, NO_DMA, NO_SPLIT, ORDER_GIVEN, QSPLIT, SPLIT_BF16, TWO_PASS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENS = [1, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 256, 257, 801]
HDS = [16, 32, 64, 128]
BH = [[1, 2], [3, 2], [8, 6], [64, 6], [4097, 1]]
FLAGS = [0, NO_DMA, TWO_PASS, NO_DMA | TWO_PASS, NO_SPLIT, SPLIT_BF16, FEWQ_WG, LPT_SHORT, LPT_SHORT | ORDER_GIVEN,
         QSPLIT(1), QSPLIT(4)]


def _pad4(n):
    return (n + 3) & ~3


def _layout_problem(backward, p, B, H, hd, mk, Tq, Tk, ws):
    """None, or what is wrong with the plan's workspace layout: offsets in layout order, 16-byte aligned where the
    layout pads (the order slot is pad4(B) floats), inside the floats provided, ending at the total."""
    order, part, kv = p.order_off, p.part_off, p.kvpart_off
    if ws < 0:
        return None if order == part == kv == -1 else "offsets without a workspace"
    if backward:
        part_size = (mk + 63) // 64 * Tq * H * hd
        segs = [(part, part_size), (order, _pad4(B)), (kv, 2 * p.qsplit * Tk * H * hd)]
    else:
        segs = [(order, _pad4(B)), (part, p.ws_total - _pad4(B)), (kv, 0)]
    end = 0
    for off, size in segs:
        if off < 0:
            continue
        if off % 4 or off < end or off + size > ws:
            return f"offset {off} (+{size}) misplaced after {end} in {ws} floats"
        end = off + size
    if kv >= 0 and not backward:
        return "dK / dV partials in a forward"
    if backward and kv >= 0 and end != p.ws_total:
        return f"layout ends at {end}, total {p.ws_total}"
    if backward and kv < 0 and (part >= 0 or order >= 0) and end != (p.ws_need or _pad4(B)):
        return f"layout ends at {end}, needs {p.ws_need}"
    if not backward and part >= 0 and end != p.ws_total:
        return f"layout ends at {end}, total {p.ws_total}"
    return None


@pytest.fixture(scope="module")
def sweep():
    """One pass over the whole grid: (problems, forms emitted). Every grid point is planned without a workspace and
    with one sized by *_ws_elems (the backward's with Tk = -1 and with Tk >= 0); Tq = B max_q, Tk = B max_k."""
    from rqvae_hip import _lib
    lib = _lib.load()
    gold = json.load(open(os.path.join(GOLDEN, "attn_ws_elems.json")))
    assert (gold["lens"], gold["hds"], gold["bh"], gold["flags"]) == (LENS, HDS, BH, FLAGS)
    p, n = _lib.AttnPlan(), ctypes.c_int64()
    pref, nref, size = ctypes.byref(p), ctypes.byref(n), ctypes.sizeof(_lib.AttnPlan)
    problems, emitted, seen = [], set(), set()
    for hd in HDS:
        for causal in (0, 1):
            for B, H in BH:
                for fl in FLAGS:
                    table = gold["tables"][f"{hd},{causal},{B},{H},{fl}"]
                    for i, mq in enumerate(LENS):
                        row = gold["rows"][table[i]]
                        for j, mk in enumerate(LENS):
                            Tq, Tk, at = B * mq, B * mk, (hd, causal, B, H, fl, mq, mk)
                            assert lib.varlen_attn_fwd_ws_elems(B, H, hd, mq, mk, Tq, causal, fl, nref) == 0
                            nf = n.value
                            assert lib.varlen_attn_bwd_ws_elems(B, H, hd, mq, mk, Tq, -1, fl, nref) == 0
                            nb0 = n.value
                            assert lib.varlen_attn_bwd_ws_elems(B, H, hd, mq, mk, Tq, Tk, fl, nref) == 0
                            nb = n.value
                            if [nf, nb0, nb] != row[3 * j:3 * j + 3]:
                                problems.append((at, "ws_elems", [nf, nb0, nb], row[3 * j:3 * j + 3]))
                            for backward, tk, ws, total in ((0, Tk, -1, nf), (0, Tk, nf, nf), (1, Tk, -1, nb), (1, Tk, nb0, nb),
                                                            (1, Tk, nb, nb), (1, -1, nb0, nb0)):
                                assert lib.varlen_attn_plan(backward, B, H, hd, mq, mk, Tq, tk, causal, fl, ws, pref) == 0
                                if p.ws_total != total:
                                    problems.append((at, backward, ws, "total", p.ws_total, total))
                                if ws >= 0 or p.order_off >= 0 or p.part_off >= 0 or p.kvpart_off >= 0:
                                    bad = _layout_problem(backward, p, B, H, hd, mk, Tq, tk, ws)
                                    if bad:
                                        problems.append((at, backward, ws, bad))
                                key = ctypes.string_at(ctypes.addressof(p), size)
                                if key not in seen:   # launch lists repeat: look into each distinct plan once
                                    seen.add(key)
                                    if not 0 <= p.n_launches <= 6:
                                        problems.append((at, backward, ws, "launches", p.n_launches))
                                    for l in p.launch[:max(0, min(p.n_launches, 6))]:
                                        emitted.add(S.Form(S.FAMILIES[l.family], l.hd, l.nw, l.r, l.x3))
    return problems, emitted


def test_grid_sizes_and_layouts(sweep):
    """The plan's total is what varlen_attn_{fwd,bwd}_ws_elems return, both are the recorded sizes, and every layout is
    ordered, aligned and ends at the total; no plan has more than six launches."""
    problems, _ = sweep
    assert not problems, (len(problems), problems[:5])


def test_grid_forms_are_instantiated(sweep):
    """Every (family, template arguments) a plan names is one the launcher builds, and the launcher builds nothing
    else but the split-key forward's unreachable 32-key blocks."""
    _, emitted = sweep
    assert emitted <= S.INSTANTIATED, sorted(emitted - S.INSTANTIATED)
    assert S.INSTANTIATED - emitted == S.UNREACHABLE


def test_form_cases_name_every_emitted_form(sweep):
    """The case table of test_every_launch_form_vs_oracle names exactly the forms the plan can emit over the grid,
    but for the one case left out because it misses the oracle bound with the earlier library too."""
    _, emitted = sweep
    named = {f for case in S.FORM_CASES for f in case[-1]}
    assert not named & S.FORM_CASES_LEFT_OUT
    assert named | S.FORM_CASES_LEFT_OUT == emitted, (sorted(emitted - named), sorted(named - emitted))


def _names(plan):
    return [S.kernel_name(f) for f in plan.forms]


# One line per row of DESIGN.md's dispatch table ("Attention dispatch"), at both sides of each threshold. B = 3, H = 2
# unless the line gives (B, H); Tq = B max_q, Tk = B max_k; workspace sized by *_ws_elems with Tk ("none": no
# workspace; "no_tk": sized with Tk = -1). The expected kernels are read from the predicates the dispatch had before
# the plan existed (short_plan, lpt_plan, split_plan, kvsplit_plan, dma_fwd_plan, dma_kv_plan, fewq_plan,
# short_fused_plan, fused_plan, fused_qsplit, waves_for, dma_rows_for, fewq_waves).
_FWD = [
    # key-split: non-causal, > 16 queries, > 256 keys, B H ceil(max_q / 64) <= 1024 workgroups, with a workspace
    (64, 17, 257, 0, 0, {}, ["attn_fwd_kvsplit_kernel<64, 4, 128, false>", "attn_fwd_combine_kernel<64, 128>"]),
    (64, 17, 257, 0, SPLIT_BF16, {}, ["attn_fwd_kvsplit_kernel<64, 4, 128, true>", "attn_fwd_combine_kernel<64, 128>"]),
    (64, 17, 256, 0, 0, {}, ["attn_order_kernel", "attn_fwd_kernel<64, 2, false>"]),
    (64, 17, 257, 1, 0, {}, ["attn_order_kernel", "attn_fwd_kernel<64, 2, false>"]),
    (64, 17, 257, 0, NO_SPLIT, {}, ["attn_order_kernel", "attn_fwd_kernel<64, 2, false>"]),
    (64, 17, 257, 0, 0, {"ws": "none"}, ["attn_fwd_kernel<64, 2, false>"]),
    (32, 17, 257, 0, 0, {}, ["attn_order_kernel", "attn_fwd_kernel<32, 2, false>"]),
    (64, 128, 257, 0, 0, {"bh": (64, 6)}, ["attn_fwd_kvsplit_kernel<64, 4, 128, false>", "attn_fwd_combine_kernel<64, 128>"]),
    (64, 129, 257, 0, 0, {"bh": (64, 6)}, ["attn_order_kernel", "attn_fwd_kernel<64, 4, false>"]),
    # split-key: non-causal, <= 16 queries, >= 129 keys; split-bf16 through the key-split kernel
    (64, 16, 129, 0, 0, {}, ["attn_fwd_split_kernel<64, 128>", "attn_fwd_combine_kernel<64, 128>"]),
    (64, 16, 129, 0, SPLIT_BF16, {}, ["attn_fwd_kvsplit_kernel<64, 4, 128, true>", "attn_fwd_combine_kernel<64, 128>"]),
    (64, 16, 128, 0, 0, {}, ["attn_fwd_fewq_kernel<4>"]),
    (64, 17, 129, 0, 0, {}, ["attn_order_kernel", "attn_fwd_kernel<64, 2, false>"]),
    (64, 16, 129, 1, 0, {}, ["attn_order_kernel", "attn_fwd_kernel<64, 1, false>"]),
    (64, 16, 129, 0, 0, {"ws": "none"}, ["attn_fwd_kernel<64, 1, false>"]),
    # few-query: <= 16 queries over <= 128 keys; 1 / 2 / 4 waves by the keys; never split-bf16
    (64, 16, 16, 0, 0, {}, ["attn_fwd_fewq_kernel<1>"]),
    (64, 16, 17, 0, 0, {}, ["attn_fwd_fewq_kernel<2>"]),
    (64, 16, 32, 1, 0, {}, ["attn_fwd_fewq_kernel<2>"]),
    (64, 16, 33, 0, SPLIT_BF16, {}, ["attn_fwd_fewq_kernel<4>"]),
    (64, 16, 33, 0, LPT_SHORT, {}, ["attn_order_kernel", "attn_fwd_fewq_kernel<4>"]),
    (64, 16, 33, 0, LPT_SHORT | ORDER_GIVEN, {}, ["attn_fwd_fewq_kernel<4>"]),
    (64, 16, 33, 0, LPT_SHORT, {"ws": "none"}, ["attn_fwd_fewq_kernel<4>"]),
    (64, 16, 33, 0, LPT_SHORT, {"bh": (1, 2)}, ["attn_fwd_fewq_kernel<4>"]),
    (32, 16, 16, 0, 0, {}, ["attn_fwd_kernel<32, 1, false>"]),
    # LDS-DMA short: > 16 queries over <= 128 keys, staged rows by the keys; split-bf16 only beyond 32 keys
    (64, 17, 32, 0, 0, {}, ["attn_fwd_dma_kernel<4, 32>"]),
    (64, 17, 33, 1, 0, {}, ["attn_fwd_dma_kernel<4, 64>"]),
    (64, 17, 64, 0, 0, {}, ["attn_fwd_dma_kernel<4, 64>"]),
    (64, 17, 65, 0, 0, {}, ["attn_fwd_dma_kernel<4, 96>"]),
    (64, 17, 96, 0, 0, {}, ["attn_fwd_dma_kernel<4, 96>"]),
    (64, 17, 97, 0, 0, {}, ["attn_fwd_dma_kernel<4, 128>"]),
    (64, 801, 128, 1, 0, {}, ["attn_fwd_dma_kernel<4, 128>"]),
    (64, 17, 32, 0, SPLIT_BF16, {}, ["attn_fwd_dma_kernel<4, 32>"]),
    (64, 17, 33, 0, SPLIT_BF16, {}, ["attn_fwd_short_x3_kernel<64>"]),
    (64, 17, 65, 0, SPLIT_BF16, {}, ["attn_fwd_short_x3_kernel<96>"]),
    (64, 17, 97, 0, SPLIT_BF16, {}, ["attn_fwd_short_x3_kernel<128>"]),
    (64, 17, 33, 0, LPT_SHORT, {}, ["attn_order_kernel", "attn_fwd_dma_kernel<4, 64>"]),   # the known useless order launch
    (64, 17, 33, 0, LPT_SHORT | SPLIT_BF16, {}, ["attn_order_kernel", "attn_fwd_short_x3_kernel<64>"]),
    # register-staged short (RQ_ATTN_NO_DMA): <= 128 queries over <= 32 keys
    (64, 16, 16, 0, NO_DMA, {}, ["attn_fwd_short_kernel<64, 1, 32>"]),
    (64, 17, 32, 0, NO_DMA, {}, ["attn_fwd_short_kernel<64, 4, 32>"]),
    (64, 128, 32, 1, NO_DMA, {}, ["attn_fwd_short_kernel<64, 4, 32>"]),
    (64, 129, 32, 0, NO_DMA, {}, ["attn_fwd_kernel<64, 4, false>"]),
    (64, 17, 33, 0, NO_DMA, {}, ["attn_fwd_kernel<64, 2, false>"]),
    (64, 16, 33, 0, NO_DMA | LPT_SHORT, {}, ["attn_fwd_kernel<64, 1, false>"]),
    (16, 17, 32, 0, NO_DMA, {}, ["attn_fwd_kernel<16, 2, false>"]),
    # chunked: 1 / 2 / 4 waves by the queries; split-bf16 at hd 64 with 4 waves; LPT order beyond 128 keys, 2 <= B <= 4096
    (16, 16, 16, 1, 0, {}, ["attn_fwd_kernel<16, 1, false>"]),
    (16, 17, 16, 0, 0, {}, ["attn_fwd_kernel<16, 2, false>"]),
    (128, 96, 128, 0, 0, {}, ["attn_fwd_kernel<128, 2, false>"]),
    (128, 97, 129, 0, SPLIT_BF16, {}, ["attn_order_kernel", "attn_fwd_kernel<128, 4, false>"]),
    (64, 97, 129, 1, SPLIT_BF16, {}, ["attn_order_kernel", "attn_fwd_kernel<64, 4, true>"]),
    (64, 96, 129, 1, SPLIT_BF16, {}, ["attn_order_kernel", "attn_fwd_kernel<64, 2, false>"]),
    (64, 97, 129, 1, ORDER_GIVEN, {}, ["attn_fwd_kernel<64, 4, false>"]),
    (64, 97, 129, 1, 0, {"bh": (1, 2)}, ["attn_fwd_kernel<64, 4, false>"]),
    (64, 97, 129, 1, 0, {"bh": (4096, 1)}, ["attn_order_kernel", "attn_fwd_kernel<64, 4, false>"]),
    (64, 97, 129, 1, 0, {"bh": (4097, 1)}, ["attn_fwd_kernel<64, 4, false>"]),
]
_FUSED = ["attn_delta_kernel<64>", "attn_bwd_fused_kernel<64, 4, 32>", "attn_dq_reduce_kernel<64, 64>"]
_BWD = [
    # long fused: >= 129 keys, hd 64, with a workspace; its own order (of cu_q) beyond 128 queries; query splits when sized with Tk
    (64, 17, 129, 0, 0, {}, _FUSED),
    (64, 16, 129, 1, 0, {}, _FUSED),
    (64, 127, 129, 0, 0, {}, _FUSED),
    (64, 17, 129, 0, SPLIT_BF16, {}, ["attn_delta_kernel<64>", "attn_bwd_fused_x3_kernel<4, 32>", "attn_dq_reduce_kernel<64, 64>"]),
    (64, 17, 129, 0, 0, {"ws": "none"}, ["attn_bwd_dq_kernel<64, 2>", "attn_bwd_dkdv_dma_kernel<4, 32>"]),
    (64, 17, 129, 0, TWO_PASS, {}, ["attn_bwd_dq_kernel<64, 2>", "attn_bwd_dkdv_dma_kernel<4, 32>"]),
    (32, 17, 129, 0, 0, {}, ["attn_bwd_dq_kernel<32, 2>", "attn_bwd_dkdv_kernel<32, 4>"]),
    (64, 129, 129, 0, 0, {}, ["attn_order_kernel", "attn_delta_kernel<64>", "attn_bwd_fused_kernel<64, 4, 32>",
                              "attn_kv_reduce_kernel<64>", "attn_dq_reduce_kernel<64, 64>"]),
    (64, 129, 129, 0, LPT_SHORT | ORDER_GIVEN, {"ws": "no_tk"}, ["attn_order_kernel"] + _FUSED),
    (64, 129, 129, 1, QSPLIT(1), {}, ["attn_order_kernel"] + _FUSED),
    (64, 129, 129, 0, 0, {"bh": (1, 2), "ws": "no_tk"}, _FUSED),
    # short one-pass: 17..128 queries over <= 128 keys; staged rows by the longer side, 2 waves at 32 rows
    (64, 17, 16, 0, 0, {}, ["attn_bwd_short_fused_kernel<2, 32>"]),
    (64, 32, 32, 1, 0, {}, ["attn_bwd_short_fused_kernel<2, 32>"]),
    (64, 33, 16, 0, 0, {}, ["attn_bwd_short_fused_kernel<4, 64>"]),
    (64, 64, 64, 0, 0, {}, ["attn_bwd_short_fused_kernel<4, 64>"]),
    (64, 65, 64, 0, 0, {}, ["attn_bwd_short_fused_kernel<4, 96>"]),
    (64, 17, 97, 0, 0, {}, ["attn_bwd_short_fused_kernel<4, 128>"]),
    (64, 128, 128, 1, SPLIT_BF16, {}, ["attn_bwd_short_fused_kernel<4, 128>"]),
    (64, 17, 16, 0, LPT_SHORT, {}, ["attn_order_kernel", "attn_bwd_short_fused_kernel<2, 32>"]),
    (64, 17, 16, 0, LPT_SHORT | ORDER_GIVEN, {}, ["attn_bwd_short_fused_kernel<2, 32>"]),
    (64, 17, 16, 0, LPT_SHORT, {"ws": "none"}, ["attn_bwd_short_fused_kernel<2, 32>"]),
    (64, 129, 128, 0, 0, {}, ["attn_bwd_dq_dma_kernel<4, 128>", "attn_bwd_dkdv_kernel<64, 4>"]),
    # few-query one-pass: <= 16 queries over <= 128 keys; the persistent walk beyond 32 keys unless RQ_ATTN_FEWQ_WG
    (64, 16, 16, 1, 0, {}, ["attn_bwd_fewq_fused_kernel<1>"]),
    (64, 16, 32, 0, 0, {}, ["attn_bwd_fewq_fused_kernel<2>"]),
    (64, 16, 33, 0, 0, {}, ["attn_bwd_fewq_stream_kernel<64>"]),
    (64, 16, 64, 0, 0, {}, ["attn_bwd_fewq_stream_kernel<64>"]),
    (64, 16, 65, 0, 0, {}, ["attn_bwd_fewq_stream_kernel<96>"]),
    (64, 16, 97, 0, 0, {}, ["attn_bwd_fewq_stream_kernel<128>"]),
    (64, 16, 128, 0, 0, {}, ["attn_bwd_fewq_stream_kernel<128>"]),
    (64, 16, 33, 0, FEWQ_WG, {}, ["attn_bwd_fewq_fused_kernel<4>"]),
    (64, 16, 33, 0, LPT_SHORT, {}, ["attn_order_kernel", "attn_bwd_fewq_stream_kernel<64>"]),
    # two-pass (RQ_ATTN_TWO_PASS): dQ few-query / LDS-DMA / register-staged short / chunked, then dK / dV likewise
    (64, 16, 16, 0, TWO_PASS, {}, ["attn_bwd_dq_fewq_kernel<1>", "attn_bwd_dkdv_short_kernel<64, 1, 32>"]),
    (64, 16, 17, 0, TWO_PASS, {}, ["attn_bwd_dq_fewq_kernel<2>", "attn_bwd_dkdv_dma_kernel<4, 32>"]),
    (64, 16, 33, 0, TWO_PASS, {}, ["attn_bwd_dq_fewq_kernel<4>", "attn_bwd_dkdv_dma_kernel<4, 32>"]),
    (64, 17, 32, 1, TWO_PASS, {}, ["attn_bwd_dq_dma_kernel<4, 32>", "attn_bwd_dkdv_dma_kernel<4, 32>"]),
    (64, 33, 33, 0, TWO_PASS, {}, ["attn_bwd_dq_dma_kernel<4, 64>", "attn_bwd_dkdv_dma_kernel<4, 64>"]),
    (64, 65, 65, 0, TWO_PASS, {}, ["attn_bwd_dq_dma_kernel<4, 96>", "attn_bwd_dkdv_dma_kernel<4, 96>"]),
    (64, 97, 97, 0, TWO_PASS, {}, ["attn_bwd_dq_dma_kernel<4, 128>", "attn_bwd_dkdv_dma_kernel<4, 128>"]),
    (64, 32, 16, 0, TWO_PASS, {}, ["attn_bwd_dq_dma_kernel<4, 32>", "attn_bwd_dkdv_short_kernel<64, 1, 32>"]),
    (64, 33, 16, 0, TWO_PASS, {}, ["attn_bwd_dq_dma_kernel<4, 32>", "attn_bwd_dkdv_kernel<64, 1>"]),
    (64, 128, 129, 0, TWO_PASS, {}, ["attn_bwd_dq_kernel<64, 4>", "attn_bwd_dkdv_dma_kernel<4, 128>"]),
    (64, 129, 129, 0, TWO_PASS, {}, ["attn_bwd_dq_kernel<64, 4>", "attn_bwd_dkdv_kernel<64, 4>"]),
    (64, 16, 16, 0, NO_DMA, {}, ["attn_bwd_dq_short_kernel<64, 1, 32>", "attn_bwd_dkdv_short_kernel<64, 1, 32>"]),
    (64, 17, 32, 0, NO_DMA | TWO_PASS, {}, ["attn_bwd_dq_short_kernel<64, 4, 32>", "attn_bwd_dkdv_short_kernel<64, 4, 32>"]),
    (64, 17, 33, 0, NO_DMA, {}, ["attn_bwd_dq_kernel<64, 2>", "attn_bwd_dkdv_short_kernel<64, 4, 32>"]),
    (64, 33, 17, 0, NO_DMA, {}, ["attn_bwd_dq_short_kernel<64, 4, 32>", "attn_bwd_dkdv_kernel<64, 2>"]),
    (64, 129, 32, 0, NO_DMA, {}, ["attn_bwd_dq_kernel<64, 4>", "attn_bwd_dkdv_kernel<64, 2>"]),
    (64, 16, 33, 0, NO_DMA | LPT_SHORT, {}, ["attn_bwd_dq_kernel<64, 1>", "attn_bwd_dkdv_short_kernel<64, 4, 32>"]),
    (16, 16, 97, 1, 0, {}, ["attn_bwd_dq_kernel<16, 1>", "attn_bwd_dkdv_kernel<16, 4>"]),
    (128, 97, 96, 0, 0, {}, ["attn_bwd_dq_kernel<128, 4>", "attn_bwd_dkdv_kernel<128, 2>"]),
]


@pytest.mark.parametrize("backward,table", [(0, _FWD), (1, _BWD)])
def test_dispatch_table(backward, table):
    for hd, mq, mk, causal, flags, opt, want in table:
        B, H = opt.get("bh", (3, 2))
        Tq, Tk = B * mq, B * mk
        ws = {"none": -1, "no_tk": S.ws_elems(backward, B, H, hd, mq, mk, Tq, -1, causal, flags),
              "tk": S.ws_elems(backward, B, H, hd, mq, mk, Tq, Tk, causal, flags)}[opt.get("ws", "tk")]
        got = S.plan(backward, B, H, hd, mq, mk, Tq, Tk, causal, flags, ws)
        assert _names(got) == want, (backward, hd, mq, mk, causal, flags, opt)


def test_plan_details():
    """What the table's kernel names do not show: order sources, query splits, grids, B == 0."""
    p = S.plan(0, 3, 2, 64, 16, 33, 48, 99, 0, LPT_SHORT | ORDER_GIVEN, 4)
    assert p.order_src == "given" and p.order_off == 0
    assert S.plan(0, 3, 2, 64, 16, 33, 48, 99, 0, LPT_SHORT, 4).order_src == "cu_k"
    assert S.plan(0, 3, 2, 64, 97, 129, 291, 387, 1, 0, 4).order_src == "cu_k"
    n = S.ws_elems(1, 3, 2, 64, 129, 129, 387, 387, 0, LPT_SHORT | ORDER_GIVEN)
    p = S.plan(1, 3, 2, 64, 129, 129, 387, 387, 0, LPT_SHORT | ORDER_GIVEN, n)
    assert p.order_src == "cu_q" and p.qsplit == 2 and p.order_off == 3 * 387 * 128 and p.kvpart_off == p.order_off + 4
    assert [l.grid for l in p.launches] == [(1, 1, 1), (49, 1, 1), (6, 2, 4), (49, 1, 1), (9, 2, 3)]
    # fewer floats than the Tk-sized total: one query split, no dK / dV partials
    p = S.plan(1, 3, 2, 64, 129, 129, 387, 387, 0, 0, n - 1)
    assert p.qsplit == 1 and p.kvpart_off == -1 and p.ws_need == n - 2 * 2 * 387 * 128
    # the short order needs B floats; a smaller workspace goes without
    assert S.plan(1, 3, 2, 64, 17, 16, 51, 48, 0, LPT_SHORT, 2).order_src == "none"
    assert S.plan(1, 3, 2, 64, 17, 16, 51, 48, 0, LPT_SHORT, 3).order_src == "cu_k"
    # the persistent few-query walk: one workgroup per (sequence, head) up to 2 (1 beyond 96 keys) per CU, 256 CUs
    assert S.plan(1, 64, 6, 64, 16, 96, 1024, 6144, 0, 0, -1).launches[0].grid == (384, 1, 1)
    assert S.plan(1, 4097, 1, 64, 16, 96, 65552, 393312, 0, 0, -1).launches[0].grid == (512, 1, 1)
    assert S.plan(1, 4097, 1, 64, 16, 97, 65552, 397409, 0, 0, -1).launches[0].grid == (256, 1, 1)
    for backward in (0, 1):
        p = S.plan(backward, 0, 2, 64, 17, 257, 0, 0, 0, 0, 100)
        assert p.launches == () and p.ws_total == 0


def _call_launches(hd, mq, mk, causal, flags, x3):
    """The launches of one ops.varlen_attention forward + backward of the recorded driver's case: B = 3 ragged lengths
    with an empty sequence on each side, H = 2, two tail rows; RQ_ATTN_LPT_SHORT | RQ_ATTN_ORDER_GIVEN as ops sets it
    (self-attention over offsets that carry their order, when the order is all the scratch the call needs)."""
    B, H = 3, 2
    lq, lk = [mq, 0, (mq + 1) // 2], [mk, (mk + 2) // 3, 0]
    given = flags == LPT_SHORT | ORDER_GIVEN
    Tq, Tk = sum(lq) + 2, (sum(lq) if given else sum(lk)) + 2
    base = (0 if given else flags) | (SPLIT_BF16 if x3 else 0)
    fwd, bwd = S.ops_call_plans(B, H, hd, mq, mk, Tq, Tk, causal, base, order_attached=given)
    return [[S.kernel_name(l.form), *l.grid, l.block] for l in fwd.launches + bwd.launches]


def test_plan_matches_recorded_launches():
    """golden/attn_launches.json: per case the (kernel, grid, workgroup size) sequence that the library from before
    the plan launched on an MI355X (kernel trace of forward + backward through ops.varlen_attention; matmul precision
    'high' recorded as RQ_ATTN_SPLIT_BF16). The plan's launch list equals it for every recorded case."""
    rec = json.load(open(os.path.join(GOLDEN, "attn_launches.json")))
    bad, n = [], 0
    for key, table in rec["tables"].items():
        hd, causal, flags, x3 = (int(x) for x in key.split(","))
        for i, mq in enumerate(rec["lens"]):
            for j, mk in enumerate(rec["lens"]):
                if table[i][j] < 0:
                    continue
                n += 1
                got, want = _call_launches(hd, mq, mk, causal, flags, x3), rec["lists"][table[i][j]]
                if got != want:
                    bad.append((key, mq, mk, got, want))
    assert n > 10000 and not bad, (len(bad), bad[:3])
