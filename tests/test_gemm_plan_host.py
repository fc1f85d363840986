"""The split-bf16 GEMM planner (csrc/gemm_plan.h through the C ABI) on the host, no GPU — so at the 256 CUs the
library assumes without a device, an MI355X's: every planning entry point against what the library from before the
header returned over the grid (golden/gemm_plans.json), rq_gemm_bf16x3_pair_resplit against the arithmetic
ops._bwd_pair did before it moved into the header, and the planned kernels against the built-form table."""
import ctypes
import json
import os

import pytest

import gemm_plan_support as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (load order: torch's HIP runtime first)
    from rqvae_hip import _lib
    return G.bind(ctypes.CDLL(_lib.LIB_PATH))


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "gemm_plans.json")))


@pytest.fixture(scope="module")
def recorded(lib):
    return G.record(lib)


def test_golden_is_the_grid(gold):
    assert (gold["dims"], gold["ks"]) == (G.DIMS, G.KS)
    assert len(gold["shapes"]) == len(G.DIMS) ** 2 * len(G.KS) and len(gold["pairs"]) == len(G.DIMS) ** 3
    assert all(len(t) == len(G.CODES) * len(G.EPIS) for t in gold["tables"])
    assert all(len(r) == 2 * len(G.FLAGS) for r in gold["rows"])
    n_pair = (len(G.PAIR_D) * len(G.PAIR_W) + len(G.FWD_O2) * len(G.FWD_CODES)) * len(G.PAIR_FLAGS)
    assert all(len(r) == n_pair for r in gold["pair_rows"])
    # the grid reaches every kernel, split and unsplit, and both answers of the pair and group planners
    seen = {(r[2 * i], r[2 * i + 1] > 1) for r in gold["rows"] for i in range(len(G.FLAGS))}
    assert {(k, s) for k in (0, 1, 2) for s in (False, True)} == seen   # every grid point is a valid call
    assert {c for r in gold["pair_rows"] for c in r} == {"0", "1"}
    assert {g[0] for v in gold["groups"].values() for gs in v.values() for g in gs} >= {0, 2, 3, 4}


def _expand(data):
    """(M, N, K, code, epilogue, flags) -> (return code, splits), and (M, N, K) -> workspace bytes."""
    plans, ws, it = {}, {}, iter(data["shapes"])
    for M in G.DIMS:
        for N in G.DIMS:
            for K in G.KS:
                ws[M, N, K], table = next(it)
                rows = iter(data["tables"][table])
                for code in G.CODES:
                    for epi in G.EPIS:
                        row = data["rows"][next(rows)]
                        for i, fl in enumerate(G.FLAGS):
                            plans[M, N, K, code, epi, fl] = (row[2 * i], row[2 * i + 1])
    return plans, ws


def test_plans_equal_the_recorded_ones(gold, recorded):
    want, want_ws = _expand(gold)
    got, got_ws = _expand(recorded)
    assert len(want) == 512000
    assert got_ws == want_ws
    diff = [(k, want[k], got[k]) for k in want if want[k] != got[k]]
    assert not diff, (len(diff), diff[:10])


def test_pair_plans_equal_the_recorded_ones(gold, recorded):
    want = [gold["pair_rows"][i] for i in gold["pairs"]]
    got = [recorded["pair_rows"][i] for i in recorded["pairs"]]
    diff = [i for i in range(len(want)) if want[i] != got[i]]
    assert not diff, (len(diff), diff[:10])


def test_group_plans_equal_the_recorded_ones(gold, recorded):
    assert recorded["groups"] == gold["groups"]
    assert set(gold["groups"]) == {str(k) for k in G.GROUP_KS}
    assert all(set(v) == set(G.GROUP_FLAGS) and all(len(g) == len(G.chains()) for g in v.values())
               for v in gold["groups"].values())


def _resplit_before(lib, dd, dw, cus=256):
    """ops._bwd_pair's arithmetic from before rq_gemm_bf16x3_pair_resplit existed, on the plans of the two
    descriptors (its two gemm_x3_choice calls), with 2 * multi_processor_count slots."""
    kd, sd = G.plan(lib, dd)
    kw, sw = G.plan(lib, dw)
    if not (G.KIND.get(kd) == "x3" and G.KIND.get(kw) == "x3" and sd == 1 and sw > 1):
        return 0
    slots = 2 * cus
    w1 = -(-dd.M // 128) * -(-dd.N // 128)
    t2 = -(-dw.M // 128) * -(-dw.N // 128)
    s_bal = -(-dw.K // dd.K)
    return s_bal if w1 < slots and 1 < s_bal < sw and w1 + t2 * s_bal > slots else 0


def test_pair_resplit_equals_the_python_rule(lib):
    lib.rq_gemm_bf16x3_pair_resplit.argtypes, lib.rq_gemm_bf16x3_pair_resplit.restype = [ctypes.c_void_p], ctypes.c_int
    n, hits, diff = 0, 0, []
    for R in G.DIMS:
        for O in G.DIMS:
            for I in G.DIMS:
                for code_d, epi, p in G.PAIR_D:
                    for code_w in G.PAIR_W:
                        for fl in (0, G.NO_GROUP):
                            dd, dw = G.desc(R, I, O, code_d, epi, fl, p), G.desc(O, I, R, code_w, G.EPI_STORE, fl)
                            got = lib.rq_gemm_bf16x3_pair_resplit((G.Desc * 2)(dd, dw))
                            want = _resplit_before(lib, dd, dw)
                            n += 1
                            hits += want > 0
                            if got != want:
                                diff.append((R, O, I, code_d, epi, code_w, fl, want, got))
    assert not diff, (len(diff), diff[:10])
    assert n == 70000 and hits > 100   # the rule fires on the grid (the decoder's 11,264-row layers are in it)
    # the decoder's qkv backward at 11,264 rows: dgrad 11264 x 512 x 1536 with wgrad 1536 x 512 x 11264
    dd, dw = G.desc(11264, 512, 1536, 18), G.desc(1536, 512, 11264, 2)
    assert lib.rq_gemm_bf16x3_pair_resplit((G.Desc * 2)(dd, dw)) == _resplit_before(lib, dd, dw)
    assert lib.rq_gemm_bf16x3_pair_resplit(None) == 0


def test_planned_kernel_is_a_built_form(gold):
    """The kernel planned under each flag is one the built-form table has for the call's layout and the epilogue the
    kernel itself runs (the plain store when it splits), whenever the table says some kernel can run the call. The
    128- and 64-tile kernels share one row of the table and take every shape, so that is: every (code, kernel
    epilogue) of TILE_FORMS, and every call planned onto the wide kernel. The one layout only the wide kernel has
    (code 14: m-contiguous split A x k-contiguous split B) plans onto a tile kernel where the wide one does not take
    the shape or the flag excludes it — as it did before the table existed — and the launcher refuses it."""
    plans, _ = _expand(gold)
    checked, wide_only, bad = 0, 0, []
    for (M, N, K, code, epi, fl), (rc, splits) in plans.items():
        if rc < 0:
            continue
        kind, epi_k = G.KIND[rc], (G.EPI_STORE if splits > 1 else epi)
        allowed = (code, epi_k) in G.BUILT[kind]
        if kind == "wide" or (code, epi_k) in G.TILE_FORMS:
            checked += 1
            if not allowed:
                bad.append((M, N, K, code, epi, fl, kind, splits))
        elif (code, epi_k) in G.WIDE_FORMS:
            wide_only += 1
            assert code == 14 and not allowed
    assert not bad, (len(bad), bad[:10])
    assert checked > 100000 and wide_only > 0
    # under FORCE_WIDE the wide-only layout runs wherever the wide kernel takes the shape
    assert plans[2048, 2048, 512, 14, G.EPI_STORE, G.FORCE_WIDE][0] == 1
