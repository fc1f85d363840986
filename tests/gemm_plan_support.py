"""Shared by tests/test_gemm_plan_host.py, tests/test_gemm_forms_gpu.py and tests/golden/make_gemm_plans_golden.py: the
rq_gemm_desc mirror, the planning grid and its recorder (the four host-only planning entry points of the split-bf16
GEMMs through ctypes), and the table of kernel forms csrc/linear.hip instantiates (csrc/gemm_plan.h: x3_form_built).
No GPU and no torch needed to import or to plan."""
import ctypes

ONLY_128, ONLY_64, FORCE_WIDE, NO_WIDE, MASKED, NO_PAIR, NO_GROUP = 1, 2, 4, 8, 16, 32, 64
EPI_STORE, EPI_SILU_FWD, EPI_SILU_BWD, EPI_ADD = 0, 1, 2, 3


def SPLIT(s):
    return s << 16


_P, _I64, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


class Desc(ctypes.Structure):   # rq_gemm_desc (include/rqvae_hip.h)
    _fields_ = [("A", _P), ("A_lo", _P), ("lda", _I64), ("a_kcontig", _I), ("B", _P), ("B_lo", _P), ("ldb", _I64),
                ("b_kcontig", _I), ("M", _I64), ("N", _I64), ("K", _I64), ("C", _P), ("ldc", _I64), ("epilogue", _I),
                ("Z", _P), ("H_hi", _P), ("H_lo", _P), ("ldh", _I64), ("p", ctypes.c_float), ("seed", ctypes.c_uint64),
                ("accumulate", _I), ("defer", _I), ("workspace", _P), ("ws_bytes", ctypes.c_size_t), ("flags", _I),
                ("reserved", _I)]


def code_of(a_kc, a_split, b_kc, b_split):
    """The layout code of csrc/gemm_plan.h: 16 a k-contiguous, 8 a split planes, 4 b k-contiguous, 2 b split planes."""
    return (16 if a_kc else 0) | (8 if a_split else 0) | (4 if b_kc else 0) | (2 if b_split else 0)


CODES = [code_of(ak, asp, bk, bsp) for ak in (0, 1) for asp in (0, 1) for bk in (0, 1) for bsp in (0, 1)]


def desc(M, N, K, code, epilogue=EPI_STORE, flags=0, p=0.0):
    """A planning descriptor (no real pointers) with minimal leading dimensions."""
    a_kc, b_kc = bool(code & 16), bool(code & 4)
    return Desc(A_lo=16 if code & 8 else None, lda=K if a_kc else M, a_kcontig=int(a_kc),
                B_lo=16 if code & 2 else None, ldb=K if b_kc else N, b_kcontig=int(b_kc), M=M, N=N, K=K, ldc=N,
                epilogue=epilogue, ldh=N, p=p, flags=flags)


# ---- the kernel forms linear.hip instantiates: kind -> {(layout code, kernel epilogue)}; dropout never selects a
# form that is not built (the plain store ignores it, every other built epilogue has both)
_FP32 = {0, 4, 16, 20}
_CHAIN_STORE = {30, 22, 26, 18, 10, 8, 2}
TILE_FORMS = ({(c, EPI_STORE) for c in _FP32 | _CHAIN_STORE} | {(c, e) for c in (22, 30) for e in (EPI_SILU_FWD, EPI_ADD)} |
              {(c, EPI_SILU_BWD) for c in (18, 26)})
WIDE_FORMS = {(c, EPI_STORE) for c in (10, 14, 26, 30)} | {(30, EPI_SILU_FWD), (26, EPI_SILU_BWD), (30, EPI_ADD)}
BUILT = {"x3": TILE_FORMS, "x3s": TILE_FORMS, "wide": WIDE_FORMS}
KIND = {0: "x3", 1: "wide", 2: "x3s"}   # rq_gemm_bf16x3_plan's return value
PAIR_DGRAD = {(18, EPI_STORE), (26, EPI_STORE), (18, EPI_SILU_BWD)}   # first problem of a (dgrad, wgrad) pair
PAIR_WGRAD = {(c, EPI_STORE) for c in (0, 2, 8, 10)}                  # its second problem
PAIR_FWD = {(22, EPI_STORE), (30, EPI_STORE)}                         # both problems of a (fwd, fwd) pair


# ---- the planning grid ----
DIMS = [8, 40, 64, 136, 256, 512, 1280, 2048, 11264, 65536]   # M and N
KS = [8, 32, 40, 128, 384, 512, 768, 4104, 11264, 65536]
EPIS = [EPI_STORE, EPI_SILU_FWD, EPI_SILU_BWD, EPI_ADD]
FLAGS = [0, ONLY_128, ONLY_64, FORCE_WIDE, NO_WIDE, MASKED, SPLIT(3), SPLIT(21)]
# pairs: a Linear's backward over R rows, O outputs, I inputs — dgrad (R, I, O) with wgrad (O, I, R) — and two forward
# projections (R, O, I), (R, O2, I) of different inputs; R, O, I run over DIMS
PAIR_D = [(18, EPI_STORE, 0.0), (26, EPI_STORE, 0.0), (18, EPI_SILU_BWD, 0.0), (18, EPI_SILU_BWD, 0.3),
          (26, EPI_SILU_BWD, 0.0), (22, EPI_STORE, 0.0), (16, EPI_STORE, 0.0)]
PAIR_W = [0, 2, 8, 10, 4]
PAIR_FLAGS = [0, ONLY_128, ONLY_64, NO_WIDE, NO_PAIR, SPLIT(3)]
FWD_O2 = [64, 512, 2048]
FWD_CODES = [(22, 22), (22, 30), (30, 22), (30, 30), (30, 18)]
# groups: every chain of 2 to 4 of these weight-gradient shapes (in this order), split m/n-contiguous operands
GROUP_POOL = [(512, 1280), (256, 512), (136, 256), (64, 256), (2048, 512), (40, 64), (1280, 1280)]
GROUP_KS = [11264, 32768, 65536]
# per-member flags of a chain, by position: no policy, forced counts, a forced first member only, NO_GROUP, a policy
GROUP_FLAGS = {"model": lambda i: 0, "split3": lambda i: SPLIT(3), "split21": lambda i: SPLIT(21),
               "first8": lambda i: SPLIT(8) if i == 0 else 0, "no_group": lambda i: NO_GROUP,
               "no_group21": lambda i: NO_GROUP | SPLIT(21), "only128": lambda i: ONLY_128}


def bind(lib):
    lib.rq_gemm_bf16x3_plan.argtypes, lib.rq_gemm_bf16x3_plan.restype = [_P, _P], _I
    lib.rq_gemm_bf16x3_pair_plan.argtypes, lib.rq_gemm_bf16x3_pair_plan.restype = [_P], _I
    lib.rq_gemm_bf16x3_group_plan.argtypes, lib.rq_gemm_bf16x3_group_plan.restype = [_P, _I, _P], _I
    lib.rq_gemm_bf16x3_workspace.argtypes, lib.rq_gemm_bf16x3_workspace.restype = [_I64] * 3, ctypes.c_size_t
    return lib


def plan(lib, d):
    s = ctypes.c_int(0)
    return lib.rq_gemm_bf16x3_plan(ctypes.byref(d), ctypes.byref(s)), s.value


def chains():
    from itertools import combinations
    return [c for n in (2, 3, 4) for c in combinations(range(len(GROUP_POOL)), n)]


def _dedup(store, index, row):
    key = tuple(row)
    if key not in index:
        index[key] = len(store)
        store.append(list(row))
    return index[key]


def record(lib):
    """What the four planning entry points return over the grid, deduplicated through indices:
    shapes[(M, N, K) in DIMS x DIMS x KS order] = [workspace bytes, table id]; a table holds one row id per
    (code, epilogue) in CODES x EPIS order; a row holds (return code, splits) per flag in FLAGS order, flattened.
    pairs[(R, O, I)] = row id into pair_rows: pair_plan's 0 / 1 per (PAIR_D x PAIR_W x PAIR_FLAGS), then per
    (FWD_O2 x FWD_CODES x PAIR_FLAGS), as a string. groups[K][variant] = per chain [n, splits...]."""
    bind(lib)
    rows, row_ix, tables, table_ix, shapes = [], {}, [], {}, []
    for M in DIMS:
        for N in DIMS:
            for K in KS:
                table = []
                for code in CODES:
                    for epi in EPIS:
                        row = []
                        for fl in FLAGS:
                            row += plan(lib, desc(M, N, K, code, epi, fl))
                        table.append(_dedup(rows, row_ix, row))
                shapes.append([int(lib.rq_gemm_bf16x3_workspace(M, N, K)), _dedup(tables, table_ix, table)])
    pair_rows, pair_ix, pairs = [], {}, []
    for R in DIMS:
        for O in DIMS:
            for I in DIMS:
                bits = []
                for code_d, epi, p in PAIR_D:
                    for code_w in PAIR_W:
                        for fl in PAIR_FLAGS:
                            arr = (Desc * 2)(desc(R, I, O, code_d, epi, fl, p), desc(O, I, R, code_w, EPI_STORE, fl))
                            bits.append(str(lib.rq_gemm_bf16x3_pair_plan(arr)))
                for O2 in FWD_O2:
                    for c1, c2 in FWD_CODES:
                        for fl in PAIR_FLAGS:
                            arr = (Desc * 2)(desc(R, O, I, c1, EPI_STORE, fl), desc(R, O2, I, c2, EPI_STORE, fl))
                            bits.append(str(lib.rq_gemm_bf16x3_pair_plan(arr)))
                key = "".join(bits)
                if key not in pair_ix:
                    pair_ix[key] = len(pair_rows)
                    pair_rows.append(key)
                pairs.append(pair_ix[key])
    groups = {}
    for K in GROUP_KS:
        groups[str(K)] = {}
        for name, fl in GROUP_FLAGS.items():
            out = []
            for chain in chains():
                n = len(chain)
                arr = (Desc * n)(*[desc(*GROUP_POOL[j], K, 10, EPI_STORE, fl(i)) for i, j in enumerate(chain)])
                splits = (ctypes.c_int * n)(*([-1] * n))
                out.append([lib.rq_gemm_bf16x3_group_plan(arr, n, splits)] + list(splits))
            groups[str(K)][name] = out
    return {"dims": DIMS, "ks": KS, "rows": rows, "tables": tables, "shapes": shapes, "pair_rows": pair_rows,
            "pairs": pairs, "groups": groups}
