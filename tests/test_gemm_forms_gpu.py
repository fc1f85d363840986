"""Every kernel form of the split-bf16 GEMM family, forced by policy flag: each kind (128-tile, 64-tile, their
split-K + reduce path, wide, the two paired families) runs every operand layout code x epilogue x dropout {0, 0.3} at
the smallest shape the kind admits. A case either matches the reference — operands in {1, 2, 3} / 4, exact in bf16 and in
every fp32 partial sum, so the plain product is the fp64 one bit for bit, the residual epilogue bitwise
Z + where(keep, product * scale, 0) with the host dropout mask (oracle/dropout.py), the SiLU epilogues within the
split-bf16 bound 3e-5 of fp64 with the host mask's zero pattern — or raises RqHipError "not built" (csrc/gemm_plan.h:
x3_form_built, checked before any launch). What ran, and on which kernel with how many k chunks, must equal
golden/gemm_forms.json, recorded on an MI355X with the library from before the planner header existed."""
import ctypes
import json
import os

import pytest
import torch

import gemm_plan_support as G
from oracle import dropout as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_forms.json")
SEED, PS = 12345, (0.0, 0.3)
# name: (policy flags, (M, N, K), split-K expected). (136, 72, 40): ragged tiles, a masked k tail, dims % 8;
# (64, 128, 4104): one or two tiles over a long ragged K, so split-K slabs and x3_reduce_kernel's epilogue
SINGLE = {"x3": (G.ONLY_128, (136, 72, 40), False), "x3s": (G.ONLY_64, (136, 72, 40), False),
          "x3_splitk": (G.ONLY_128, (64, 128, 4104), True), "x3s_splitk": (G.ONLY_64, (64, 128, 4104), True),
          "wide": (G.FORCE_WIDE, (2048, 2048, 64), False)}
# paired launches: the first problem (1280, 512, 512), the second (512, 512, 1280) — a Linear's backward over 1,280
# rows (data gradient with weight gradient), or two forward projections. One problem walks every layout code (the
# first also every epilogue x dropout) while the other keeps the family's own form (fixed codes below).
PAIR = {"pair_grad": (G.ONLY_128, 18, 10), "pair_grad_64": (G.ONLY_64, 18, 10),
        "pair_fwd": (G.ONLY_128, 30, 30), "pair_fwd_64": (G.ONLY_64, 30, 30)}
PAIR_SHAPES = ((1280, 512, 512), (512, 512, 1280))


def _q(r, c, gen, device):
    return torch.randint(1, 4, (r, c), generator=gen, device=device).float() / 4


class _Problem:
    """Operands of one (M, N, K) in every layout and form, their fp64 product, Z and the host masks; built once."""

    def __init__(self, ops, M, N, K, device):
        gen = torch.Generator(device=device).manual_seed(M + 3 * N + 7 * K)
        self.ops, self.shape, self.device = ops, (M, N, K), device
        A, B = _q(M, K, gen, device), _q(N, K, gen, device)
        self.prod = A.double() @ B.double().t()
        self.Z = _q(M, N, gen, device)
        self.a = {1: A, 0: A.t().contiguous()}   # by k-contiguity
        self.b = {1: B, 0: B.t().contiguous()}
        self.split = {}
        self.keep = {p: torch.from_numpy(D.keep_mask(SEED, (M, N), p)).to(device) if p else None for p in PS}

    def operand(self, which, kc, split):
        t = (self.a if which == "a" else self.b)[kc]
        if not split:
            return t
        key = (which, kc)
        if key not in self.split:
            self.split[key] = self.ops.split_bf16x3(t)
        return self.split[key]

    def spec(self, code, epi, p):
        M, N, K = self.shape
        return dict(a=self.operand("a", int(bool(code & 16)), bool(code & 8)), a_kcontig=bool(code & 16),
                    b=self.operand("b", int(bool(code & 4)), bool(code & 2)), b_kcontig=bool(code & 4), M=M, N=N, K=K,
                    epilogue=epi, Z=self.Z if epi in (G.EPI_SILU_BWD, G.EPI_ADD) else None, p=p, seed=SEED)

    def judge(self, epi, p, res, what):
        """The existing GEMM tests' judgement of one result (test_gemm_bf16x3: exact on exact operands;
        test_dropout_mask: the host mask, the residual add bitwise; test_gemm_splitk_epi: SiLU within 3e-5 of fp64)."""
        prod, Z = self.prod, self.Z
        if epi == G.EPI_STORE:   # the plain store draws no mask
            assert torch.equal(res.double(), prod), what
            return
        keep = self.keep[p] if p else torch.ones_like(Z, dtype=torch.bool)
        scale = _lib_scale(self.ops, p, self.device)
        if epi == G.EPI_ADD:
            assert torch.equal(res, Z + torch.where(keep, prod.float() * scale, torch.zeros_like(Z))), what
            return
        if epi == G.EPI_SILU_FWD:
            C, H = res
            assert torch.equal(C.double(), prod), what
            ref = torch.nn.functional.silu(prod) * keep * scale.double()
        else:
            H = res
            s = torch.sigmoid(Z.double())
            ref = s * (1 + Z.double() * (1 - s)) * prod * keep * scale.double()
        h = H.hi.float() + H.lo.float()
        assert torch.equal(h != 0, keep), what
        assert float((h.double() - ref).abs().max()) <= 3e-5 * float(ref.abs().max()), what


def _lib_scale(ops, p, device):
    thr, scale = ctypes.c_uint32(), ctypes.c_float()
    assert ops._lib.load().rq_dropout_params(ctypes.c_float(p), ctypes.byref(thr), ctypes.byref(scale)) == 0
    return torch.tensor(scale.value, dtype=torch.float32, device=device)


def _choice(ops, sp):
    """'kernel:splits' the library plans for the call under the current policy."""
    kind, S = ops.gemm_x3_choice(sp["M"], sp["N"], sp["K"], isinstance(sp["a"], ops.Split), isinstance(sp["b"], ops.Split),
                                 sp["a_kcontig"], sp["b_kcontig"], sp["epilogue"])
    return f"{kind}:{S}"


def _not_built(fn):
    """None after fn() ran, or 'not built' when the library refused the form."""
    from rqvae_hip._lib import RqHipError
    try:
        return fn()
    except RqHipError as e:
        assert "not built" in str(e), str(e)
        return "not built"


def run_single(ops, device, name):
    """{'code,epilogue,p': 'kernel:splits' | 'not built'} of one single-launch kind."""
    flags, shape, split = SINGLE[name]
    prob, ran = _Problem(ops, *shape, device), {}
    with ops.gemm_policy(flags):
        for code in G.CODES:
            for epi in G.EPIS:
                for p in PS:
                    sp = prob.spec(code, epi, p)
                    res = _not_built(lambda: ops.gemm_x3(**sp))
                    if not isinstance(res, str):
                        prob.judge(epi, p, res, (name, code, epi, p))
                        res = _choice(ops, sp)
                        assert (int(res.split(":")[1]) > 1) == split, (name, code, epi, res)
                    ran[f"{code},{epi},{p}"] = res
    torch.cuda.synchronize()
    return ran


def run_pair(ops, device, name):
    """{'1|2:code,epilogue,p': 'paired' | 'apart', kernel:splits of both | 'not built'}: problem 1 (2) walks the
    forms while problem 2 (1) keeps the family's own."""
    flags, code1, code2 = PAIR[name]
    probs, ran = [_Problem(ops, *s, device) for s in PAIR_SHAPES], {}
    Dt = ops._desc_type()
    walks = [(1, c, e, p) for c in G.CODES for e in G.EPIS for p in PS] + [(2, c, G.EPI_STORE, 0.0) for c in G.CODES]
    with ops.gemm_policy(flags):
        for which, code, epi, p in walks:
            sp1 = probs[0].spec(code if which == 1 else code1, epi if which == 1 else G.EPI_STORE, p)
            sp2 = probs[1].spec(code if which == 2 else code2, G.EPI_STORE, 0.0)
            res = _not_built(lambda: ops.gemm_x3_pair(sp1, sp2))
            if not isinstance(res, str):
                probs[0].judge(sp1["epilogue"], p, res[0], (name, which, code, epi, p, 1))
                probs[1].judge(G.EPI_STORE, 0.0, res[1], (name, which, code, epi, p, 2))
                descs = (Dt * 2)(Dt(*ops._x3_setup(**sp1).fields), Dt(*ops._x3_setup(**sp2).fields))
                paired = ops._lib.load().rq_gemm_bf16x3_pair_plan(descs)
                res = f"{'paired' if paired else 'apart'},{_choice(ops, sp1)},{_choice(ops, sp2)}"
            ran[f"{which}:{code},{epi},{p}"] = res
    torch.cuda.synchronize()
    return ran


@pytest.fixture(autouse=True)
def _epoch_zero(device):
    """The dropout epoch is device-global state (a captured step of an earlier test leaves it advanced)."""
    from rqvae_hip import ops
    ops.seed_epoch_set(0)


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_launch_forms(device, gold, name):
    from rqvae_hip import ops
    ran = run_single(ops, device, name)
    assert ran == gold[name], {k: (gold[name].get(k), v) for k, v in ran.items() if gold[name].get(k) != v}
    assert len(ran) == 128 and any(v != "not built" for v in ran.values()) and "not built" in ran.values()


@pytest.mark.parametrize("name", list(PAIR))
def test_paired_launch_forms(device, gold, name):
    from rqvae_hip import ops
    ran = run_pair(ops, device, name)
    assert ran == gold[name], {k: (gold[name].get(k), v) for k, v in ran.items() if gold[name].get(k) != v}
    assert len(ran) == 144 and any(v.startswith("paired") for v in ran.values())
