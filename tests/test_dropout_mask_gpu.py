"""Every kernel that draws a dropout mask draws exactly oracle/dropout.py's keep_mask(seed, shape, p, epoch):
the standalone kernels of dropout.hip (flat index), the RMSNorm + dropout kernels of rowwise.hip (index
r D + c) and the SiLU / SiLU' / residual epilogues of the split-bf16 GEMM in linear.hip (index m N + n), each
with its own copy of the dropout epoch.

The other dropout tests recover the mask from a kernel's output; here the mask is known beforehand, so a mask
shared between rows, swapped 32-bit words, an index built from a leading dimension, an off-by-one counter or a
stale epoch copy all fail. Inputs are nonzero, so an output is zero exactly where the element was dropped;
kept values are compared bitwise with the same kernel's p = 0 result times the library's fp32 scale. Mask and
value comparisons are exact; the RMSNorm gradients are checked against an fp64 formula under the host mask at
test_fused_decoder_gpu.test_rmsnorm_dropout's tolerances, with |gy| in [0.5, 2] so that one wrong mask bit
moves a gradient by orders of magnitude more than the tolerance. tests/test_dropout_mask_host.py checks the
restatement itself and the key schedule on the CPU.
"""
import ctypes

import pytest
import torch

from oracle import dropout as D

pytestmark = pytest.mark.gpu

PS = (0.1, 0.3, 0.5)
U64_MAX = (1 << 64) - 1
EPS = 1e-6


def _ops():
    from rqvae_hip import ops
    return ops


@pytest.fixture(autouse=True)
def _epoch_zero(device):
    """The dropout epoch is device-global state, and a captured train step of an earlier test in the same
    process leaves it advanced: every test here starts at epoch 0 (keys = the seeds)."""
    _ops().seed_epoch_set(0)


@pytest.fixture(scope="module")
def seeds(device):
    """0, 1, 2^63 - 1, one key as the model draws them (ops.next_seed) and 2^64 - 1 (the C ABI takes uint64)."""
    ops = _ops()
    with torch.random.fork_rng(devices=[device]):
        torch.manual_seed(20240)
        key = ops.next_seed()
    return (0, 1, (1 << 63) - 1, key, U64_MAX)


def _lib_scale(p, device):
    """The kernels' 1 / (1 - p) (fp32, computed by the library)."""
    thr, scale = ctypes.c_uint32(), ctypes.c_float()
    assert _ops()._lib.load().rq_dropout_params(ctypes.c_float(p), ctypes.byref(thr), ctypes.byref(scale)) == 0
    return torch.tensor(scale.value, dtype=torch.float32, device=device)


def _keep(seed, shape, p, device, epoch=0):
    return torch.from_numpy(D.keep_mask(seed, shape, p, epoch)).to(device)


def _nonzero_randn(shape, gen, device, mul=1.0):
    t = torch.randn(shape, generator=gen, device=device) * mul
    t[t == 0] = 1.0
    return t


def _grad_like(shape, gen, device):
    """|g| uniform in [0.5, 2], random sign."""
    mag = torch.rand(shape, generator=gen, device=device) * 1.5 + 0.5
    return torch.where(torch.rand(shape, generator=gen, device=device) < 0.5, -mag, mag)


def _same(out, want, what):
    bad = out != want
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


def _masked(keep, kept_values, what):
    """where(keep, kept_values, 0), after checking that no kept value is itself zero (a zero must mean dropped)."""
    assert bool((kept_values != 0).all()), what
    return torch.where(keep, kept_values, torch.zeros_like(kept_values))


# --------------------------------------------------------------------------- dropout.hip: flat index
def _silu_fwd(z, p, seed):
    ops = _ops()
    h = torch.empty_like(z)
    ops.call("rq_silu_dropout_fwd", ops.ptr(z), z.numel(), float(p), int(seed), ops.ptr(h), ops.stream_handle(z.device))
    return h


def _silu_bwd(g, z, p, seed):
    ops = _ops()
    gz = torch.empty_like(z)
    ops.call("rq_silu_dropout_bwd", ops.ptr(g), ops.ptr(z), z.numel(), float(p), int(seed), ops.ptr(gz),
             ops.stream_handle(z.device))
    return gz


def _dropout_add(h, y, p, seed):
    ops = _ops()
    out = torch.empty_like(h)
    ops.call("rq_dropout_add_fwd", ops.ptr(h), ops.ptr(y), h.numel(), float(p), int(seed), ops.ptr(out),
             ops.stream_handle(h.device))
    return out


def _dropout_bwd(g, p, seed):
    ops = _ops()
    gy = torch.empty_like(g)
    ops.call("rq_dropout_bwd", ops.ptr(g), g.numel(), float(p), int(seed), ops.ptr(gy), ops.stream_handle(g.device))
    return gy


# one float4; a partly filled workgroup; past ew_grid's cap of 4,096 workgroups: a second grid-stride pass with a
# ragged tail
FLAT_N = (4, 1020, 4 * (4096 * 256 + 257))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", FLAT_N)
def test_flat_kernels_draw_the_host_mask(device, seeds, n, p):
    gen = torch.Generator(device=device).manual_seed(n)
    z = _nonzero_randn(n, gen, device, 3.0)
    y = _grad_like(n, gen, device)
    g = _grad_like(n, gen, device)
    h = torch.randn(n, generator=gen, device=device)
    one = torch.ones(n, device=device)
    scale = _lib_scale(p, device)
    silu_kept = _silu_fwd(z, 0.0, 0) * scale
    silu_bwd_kept = _silu_bwd(g * scale, one, 0.0, 0)     # the backward mask, read at z = 1
    for seed in seeds:
        keep = _keep(seed, n, p, device)
        _same(_silu_fwd(z, p, seed), _masked(keep, silu_kept, "silu"), ("silu_dropout_fwd", n, p, seed))
        _same(_silu_bwd(g, one, p, seed), _masked(keep, silu_bwd_kept, "silu'"), ("silu_dropout_bwd", n, p, seed))
        _same(_dropout_bwd(g, p, seed), _masked(keep, g * scale, "g"), ("dropout_bwd", n, p, seed))
        _same(_dropout_add(h, y, p, seed), h + _masked(keep, y * scale, "y"), ("dropout_add_fwd", n, p, seed))


# ------------------------------------------------------------------------- rowwise.hip: index r D + c
def _rms_fwd(x, w, p, seed):
    ops = _ops()
    B, Dm = x.shape
    y, rstd = torch.empty_like(x), torch.empty(B, device=x.device)
    ops.call("rq_rmsnorm_dropout_fwd", ops.ptr(x), ops.ptr(w), B, Dm, EPS, float(p), int(seed), ops.ptr(y), ops.ptr(rstd),
             ops.stream_handle(x.device))
    return y, rstd


def _rms_bwd(x, w, rstd, gy, p, seed):
    ops = _ops()
    B, Dm = x.shape
    nb = ops._lib.load().rq_rmsnorm_bwd_workspace(B, Dm)
    ws = torch.empty(nb, device=x.device, dtype=torch.uint8)
    gx, gw = torch.empty_like(x), torch.empty(Dm, device=x.device)
    ops.call("rq_rmsnorm_dropout_bwd", ops.ptr(x), ops.ptr(w), ops.ptr(rstd), ops.ptr(gy), None, B, Dm, float(p), int(seed),
             ops.ptr(gx), ops.ptr(gw), 0, 0, None, ops.ptr(ws), nb, ops.stream_handle(x.device))
    return gx, gw


def _rms2_fwd(x, w1, w2, p1, s1, p2, s2):
    ops = _ops()
    B, Dm = x.shape
    y1, y2, rstd = torch.empty_like(x), torch.empty_like(x), torch.empty(B, device=x.device)
    ops.call("rq_rmsnorm2_dropout_fwd", ops.ptr(x), ops.ptr(w1), ops.ptr(w2), B, Dm, EPS, float(p1), int(s1), float(p2),
             int(s2), ops.ptr(y1), ops.ptr(y2), ops.ptr(rstd), ops.stream_handle(x.device))
    return y1, y2, rstd


def _rms2_bwd(x, w1, w2, rstd, g1, g2, p1, s1, p2, s2):
    ops = _ops()
    B, Dm = x.shape
    half = ops._lib.load().rq_rmsnorm_bwd_workspace(B, Dm)
    ws = torch.empty(2 * half, device=x.device, dtype=torch.uint8)
    gx, gw1, gw2 = torch.empty_like(x), torch.empty(Dm, device=x.device), torch.empty(Dm, device=x.device)
    ops.call("rq_rmsnorm2_dropout_bwd", ops.ptr(x), ops.ptr(w1), ops.ptr(w2), ops.ptr(rstd), ops.ptr(g1), ops.ptr(g2), None,
             B, Dm, float(p1), int(s1), float(p2), int(s2), ops.ptr(gx), ops.ptr(gw1), ops.ptr(gw2), 0, 0, None,
             ops.ptr(ws), 2 * half, ops.stream_handle(x.device))
    return gx, gw1, gw2


def _rms_ref64(x, ws, keeps, scales, gys):
    """fp64 (gx, [gw_i]) of sum_i <gy_i, Dropout_i(RMSNorm_{w_i}(x))> under the given masks."""
    xd = x.double().requires_grad_(True)
    wd = [w.double().requires_grad_(True) for w in ws]
    t = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + EPS)
    sum(((t * w) * k * s.double() * g.double()).sum() for w, k, s, g in zip(wd, keeps, scales, gys)).backward()
    return xd.grad, [w.grad for w in wd]


def _close(got, ref, what, atol):
    torch.testing.assert_close(got.double(), ref, rtol=2e-5, atol=atol, msg=lambda m: f"{what}: {m}")


def _rms_inputs(T, Dm, device):
    gen = torch.Generator(device=device).manual_seed(1000 * T + Dm)
    x = _nonzero_randn((T, Dm), gen, device)
    w = [torch.rand(Dm, generator=gen, device=device) + 0.5 for _ in range(2)]
    gy = [_grad_like((T, Dm), gen, device) for _ in range(2)]
    if T > 2048:
        # gw sums T terms. With random signs a column's sum can cancel to ~0 while its fp32 partial sums stay
        # ~sqrt(T): the absolute part of test_rmsnorm_dropout's gw tolerance (2e-5, set at 1,000 rows) is then
        # about the fp32 summation error itself (an fp32 sum in the kernel's order, emulated on the host, comes
        # within 0.8x of it at 8,181 rows). So here gy takes the sign of x: every term of gw is positive and the
        # relative part applies. gx is row-local and still sees every mask bit.
        gy = [g.abs() * torch.sign(x) for g in gy]
    return x, w, gy


# D: the smallest (4) and the largest (4,096) rmsnorm_supported accepts, 132 and 260 (a partial vector slot per
# lane, under and over one 256-wide slot). Rows: multiples of neither the forward's 4 rows per workgroup nor the
# backward's rows per workgroup (rms_rows_per_blk: 4 below 2,045 rows, 8 up to 8,176, 16 above); several workgroups.
RMS_SHAPES = ((1, 4), (5, 132), (3, 260), (1030, 512), (7, 4096), (4099, 8), (8181, 12))


@pytest.mark.parametrize("T,Dm", RMS_SHAPES)
def test_rmsnorm_dropout_draws_the_host_mask(device, seeds, T, Dm):
    ops = _ops()
    x, (w, _), (gy, _) = _rms_inputs(T, Dm, device)
    assert ops.rmsnorm_supported(x, w)
    plain, rstd0 = _rms_fwd(x, w, 0.0, 0)
    for p, seed in zip((0.1, 0.3, 0.5, 0.3, 0.3), seeds):
        keep, scale = _keep(seed, (T, Dm), p, device), _lib_scale(p, device)
        y, rstd = _rms_fwd(x, w, p, seed)
        _same(y, _masked(keep, plain * scale, "rmsnorm"), ("rmsnorm_dropout_fwd", T, Dm, p, seed))
        assert torch.equal(rstd, rstd0)
        if T > 1 and Dm >= 128:   # (equal by chance with probability < 0.82^128)
            assert not torch.equal(y[0] != 0, y[1] != 0), "two rows share a mask"
        gx, gw = _rms_bwd(x, w, rstd, gy, p, seed)
        rx, (rw,) = _rms_ref64(x, [w], [keep], [scale], [gy])
        _close(gx, rx, ("gx", T, Dm, p, seed), 2e-6)
        _close(gw, rw, ("gw", T, Dm, p, seed), 2e-5)


@pytest.mark.parametrize("T,Dm", [(5, 132), (1030, 512)])
def test_rmsnorm_fork_draws_each_host_mask(device, seeds, T, Dm):
    """rq_rmsnorm2_dropout_fwd / _bwd: each output under its own (p, seed); p2 = 0; equal seeds and p give the
    two norms one mask (the documented behaviour)."""
    x, (w1, w2), (g1, g2) = _rms_inputs(T, Dm, device)
    plain1, plain2 = _rms_fwd(x, w1, 0.0, 0)[0], _rms_fwd(x, w2, 0.0, 0)[0]
    for p1, s1, p2, s2 in ((0.3, seeds[3], 0.1, 7), (0.5, 1, 0.0, 99), (0.3, 5, 0.3, 5), (0.1, U64_MAX, 0.5, 0)):
        k1, k2 = _keep(s1, (T, Dm), p1, device), _keep(s2, (T, Dm), p2, device)
        c1, c2 = _lib_scale(p1, device), _lib_scale(p2, device)
        y1, y2, rstd = _rms2_fwd(x, w1, w2, p1, s1, p2, s2)
        _same(y1, _masked(k1, plain1 * c1, "norm 1"), ("rmsnorm2_fwd y1", T, Dm, p1, s1))
        _same(y2, _masked(k2, plain2 * c2, "norm 2"), ("rmsnorm2_fwd y2", T, Dm, p2, s2))
        assert torch.equal(y1 != 0, y2 != 0) == ((p1, s1) == (p2, s2))
        gx, gw1, gw2 = _rms2_bwd(x, w1, w2, rstd, g1, g2, p1, s1, p2, s2)
        rx, (r1, r2) = _rms_ref64(x, [w1, w2], [k1, k2], [c1, c2], [g1, g2])
        _close(gx, rx, ("gx", T, Dm, p1, s1, p2, s2), 2e-6)
        _close(gw1, r1, ("gw1", T, Dm, p1, s1), 2e-5)
        _close(gw2, r2, ("gw2", T, Dm, p2, s2), 2e-5)


# ------------------------------------------------------------ linear.hip: GEMM epilogues, index m N + n
def _gemm_problem(ops, epi, M, N, K, a_split, device):
    """Operands in {1, 2, 3} / 4: exact in bf16 and in every fp32 partial sum, and the product is never zero.
    (a, a_kcontig, b, b_kcontig, Z, product in fp64) in the layouts the fused MLP chain uses."""
    gen = torch.Generator(device=device).manual_seed(M + 3 * N + 7 * K + epi)

    def q(r, c):
        return torch.randint(1, 4, (r, c), generator=gen, device=device).float() / 4
    a = q(M, K)
    if epi == ops.EPI_SILU_BWD:   # g (rows, O) x W (O, I) -> (rows, I): B n-contiguous
        b, b_kc = q(K, N), False
        prod = a.double() @ b.double()
    else:                         # x (rows, I) x W (O, I)^T -> (rows, O): B k-contiguous
        b, b_kc = q(N, K), True
        prod = a.double() @ b.double().t()
    Z = None if epi == ops.EPI_SILU_FWD else q(M, N)
    return (ops.split_bf16x3(a) if a_split else a), True, ops.split_bf16x3(b), b_kc, Z, prod


def _check_epilogue(ops, epi, res, Z, prod, keep, scale, what):
    """The zero pattern of H.hi + H.lo (SiLU epilogues) or of C - Z (residual add) is the host mask; C of the
    SiLU forward is the exact product; the residual epilogue bitwise Z + where(keep, product * scale, 0)."""
    if epi == ops.EPI_SILU_FWD:
        C, H = res
        _same(C.double(), prod, what + ("z",))
    elif epi == ops.EPI_SILU_BWD:
        H = res
    else:
        _same(res, Z + _masked(keep, prod.float() * scale, what), what + ("C",))
        _same((res - Z) != 0, keep, what + ("C - Z",))
        return
    assert H.hi.is_contiguous() and H.hi.shape == keep.shape
    _same((H.hi.float() + H.lo.float()) != 0, keep, what + ("H",))


def _epis(ops):
    return {"silu_fwd": ops.EPI_SILU_FWD, "silu_bwd": ops.EPI_SILU_BWD, "add": ops.EPI_ADD}


# (family, policy flags, M, N, K, kernel reported, split-K, split A): the smallest shapes that select each kernel
# family with a dropout epilogue — M not a multiple of the tile, N a multiple of 4 (8 for an n-contiguous split
# B) but not of the tile, more than one tile each way. Split-K plans apply the epilogue in x3_reduce_kernel.
def _families(ops):
    return {"x3": (ops.GEMM_ONLY_128, 130, 136, 32, "x3", False, True),
            "x3s": (ops.GEMM_ONLY_64, 70, 72, 32, "x3s", False, False),
            "wide": (ops.GEMM_FORCE_WIDE, 2052, 2056, 32, "wide", False, True),
            "x3_splitk": (ops.GEMM_ONLY_128, 133, 264, 256, "x3", True, True),
            "x3s_splitk": (0, 40, 136, 512, "x3s", True, False)}


@pytest.mark.parametrize("epi_name", ["silu_fwd", "silu_bwd", "add"])
@pytest.mark.parametrize("family", ["x3", "x3s", "wide", "x3_splitk", "x3s_splitk"])
def test_gemm_epilogues_draw_the_host_mask(device, seeds, family, epi_name):
    ops = _ops()
    epi = _epis(ops)[epi_name]
    flags, M, N, K, kernel, split, a_split = _families(ops)[family]
    a, a_kc, b, b_kc, Z, prod = _gemm_problem(ops, epi, M, N, K, a_split, device)
    with ops.gemm_policy(flags):
        kern, S = ops.gemm_x3_choice(M, N, K, a_split, True, a_kc, b_kc, epi)
        assert kern == kernel and (S > 1) == split, (family, kern, S)
        for p, seed in zip((0.1, 0.3, 0.5, 0.3, 0.3), seeds):
            res = ops.gemm_x3(a, a_kc, b, b_kc, M, N, K, epi, Z=Z, p=p, seed=seed)
            _check_epilogue(ops, epi, res, Z, prod, _keep(seed, (M, N), p, device), _lib_scale(p, device),
                            (family, epi_name, p, seed))


def test_gemm_paired_launch_draws_the_host_mask(device, seeds):
    """The one paired instantiation that carries dropout: the SiLU' data gradient (fp32 g, split W) sharing a
    launch with its layer's weight gradient (gemm_x3_pair_kernel)."""
    ops = _ops()
    rows, I, O, p = 132, 136, 32, 0.3
    g, _, W, _, Z, prod = _gemm_problem(ops, ops.EPI_SILU_BWD, rows, I, O, False, device)
    x = torch.randn(rows, I, device=device)
    for flags in (ops.GEMM_ONLY_128, ops.GEMM_ONLY_64):
        with ops.gemm_policy(flags):
            for seed in seeds:
                dspec = dict(a=g, a_kcontig=True, b=W, b_kcontig=False, M=rows, N=I, K=O, epilogue=ops.EPI_SILU_BWD,
                             Z=Z, p=p, seed=seed)
                wspec = dict(a=g, a_kcontig=False, b=x, b_kcontig=False, M=O, N=I, K=rows)
                Dt = ops._desc_type()
                descs = (Dt * 2)(Dt(*ops._x3_setup(**dspec).fields), Dt(*ops._x3_setup(**wspec).fields))
                assert ops._lib.load().rq_gemm_bf16x3_pair_plan(descs) == 1, flags
                H, dW = ops.gemm_x3_pair(dspec, wspec)
                _check_epilogue(ops, ops.EPI_SILU_BWD, H, Z, prod, _keep(seed, (rows, I), p, device),
                                _lib_scale(p, device), ("pair", flags, seed))
                assert torch.equal(dW, ops.gemm_x3(**wspec))


@pytest.mark.parametrize("epi_name", ["silu_fwd", "silu_bwd"])
def test_gemm_mask_ignores_the_planes_leading_dim(device, seeds, epi_name):
    """H planes wider than N (ldh = N + 8): the mask index stays m N + n."""
    ops = _ops()
    epi = _epis(ops)[epi_name]
    M, N, K, p, seed, pad = 130, 136, 32, 0.3, seeds[3], 8
    a, a_kc, b, b_kc, Z, prod = _gemm_problem(ops, epi, M, N, K, True, device)
    with ops.gemm_policy(ops.GEMM_ONLY_128):
        c = ops._x3_setup(a, a_kc, b, b_kc, M, N, K, epi, Z, p, seed)
    hi = torch.zeros(M, N + pad, device=device, dtype=torch.bfloat16)
    lo = torch.zeros(M, N + pad, device=device, dtype=torch.bfloat16)
    f = list(c.fields)
    assert f[17] == N and f[15].value == c.H.hi.data_ptr()   # (H_hi, H_lo, ldh) of rq_gemm_desc
    f[15], f[16], f[17] = ops.ptr(hi), ops.ptr(lo), N + pad
    d = ops._desc_type()(*f)
    splits = ctypes.c_int(0)
    ops.call("rq_gemm_bf16x3_run", ctypes.byref(d), ctypes.byref(splits), ops.stream_handle(device))
    assert splits.value == 0
    merged = hi.float() + lo.float()
    _same(merged[:, :N] != 0, _keep(seed, (M, N), p, device), (epi_name, "ldh"))
    assert not bool(merged[:, N:].any())


# ----------------------------------------------------------------------------- p = 0 and p = 1
def test_p0_is_identity_and_p1_is_zero(device, seeds):
    ops = _ops()
    n = 1020
    gen = torch.Generator(device=device).manual_seed(3)
    z, y, h = _nonzero_randn(n, gen, device, 3.0), _grad_like(n, gen, device), torch.randn(n, generator=gen, device=device)
    one = torch.ones(n, device=device)
    x, (w1, w2), (g1, g2) = _rms_inputs(5, 132, device)
    plain1, rstd = _rms_fwd(x, w1, 0.0, 0)
    plain2 = _rms_fwd(x, w2, 0.0, 0)[0]
    M, N, K = 70, 72, 32
    gemm = {e: _gemm_problem(ops, e, M, N, K, False, device) for e in _epis(ops).values()}

    def run_gemm(e, p, seed):
        a, a_kc, b, b_kc, Z, _ = gemm[e]
        with ops.gemm_policy(ops.GEMM_ONLY_64):
            r = ops.gemm_x3(a, a_kc, b, b_kc, M, N, K, e, Z=Z, p=p, seed=seed)
        return r if e == ops.EPI_ADD else (r[1] if e == ops.EPI_SILU_FWD else r)

    def flat(t):
        return t if isinstance(t, torch.Tensor) else torch.cat([t.hi.float().reshape(-1), t.lo.float().reshape(-1)])
    runs = {"silu_fwd": lambda p, s: _silu_fwd(z, p, s), "silu_bwd": lambda p, s: _silu_bwd(y, z, p, s),
            "dropout_bwd": lambda p, s: _dropout_bwd(y, p, s), "dropout_add": lambda p, s: _dropout_add(h, y, p, s) - h,
            "rmsnorm_fwd": lambda p, s: _rms_fwd(x, w1, p, s)[0], "rmsnorm_bwd": lambda p, s: _rms_bwd(x, w1, rstd, g1, p, s)[0],
            "rmsnorm2_y1": lambda p, s: _rms2_fwd(x, w1, w2, p, s, 0.0, 0)[0],
            "rmsnorm2_y2": lambda p, s: _rms2_fwd(x, w1, w2, 0.0, 0, p, s)[1],
            "gemm_silu_fwd": lambda p, s: flat(run_gemm(ops.EPI_SILU_FWD, p, s)),
            "gemm_silu_bwd": lambda p, s: flat(run_gemm(ops.EPI_SILU_BWD, p, s)),
            "gemm_add": lambda p, s: run_gemm(ops.EPI_ADD, p, s) - gemm[ops.EPI_ADD][4]}
    for name, run in runs.items():
        base = run(0.0, 0)
        assert bool((base != 0).any()), name
        for seed in seeds:
            assert torch.equal(run(0.0, seed), base), (name, "p = 0", seed)
            out = run(1.0, seed)
            assert bool(torch.isfinite(out).all()) and not bool(out.any()), (name, "p = 1", seed)
    assert torch.equal(_dropout_bwd(y, 0.0, 5), y) and torch.equal(_dropout_add(h, y, 0.0, 5), h + y)
    assert torch.equal(_rms2_fwd(x, w1, w2, 0.0, 3, 0.0, 4)[1], plain2) and torch.equal(runs["rmsnorm_fwd"](0.0, 9), plain1)


# ------------------------------------------------------------------ the epoch, per translation unit
def _epoch_probes(ops, device, seed, p):
    """One kernel from each translation unit that holds a copy of the epoch word -> its kept set."""
    n, (T, Dm), (M, N, K) = 1020, (5, 132), (70, 72, 32)
    gen = torch.Generator(device=device).manual_seed(8)
    h, y = torch.zeros(n, device=device), _grad_like(n, gen, device)
    x, (w, _), _ = _rms_inputs(T, Dm, device)
    a, a_kc, b, b_kc, _, _ = _gemm_problem(ops, ops.EPI_SILU_FWD, M, N, K, False, device)

    def gemm():
        with ops.gemm_policy(ops.GEMM_ONLY_64):
            H = ops.gemm_x3(a, a_kc, b, b_kc, M, N, K, ops.EPI_SILU_FWD, p=p, seed=seed)[1]
        return (H.hi.float() + H.lo.float()) != 0
    return {"dropout.hip": ((n,), lambda: _dropout_add(h, y, p, seed) != 0),
            "rowwise.hip": ((T, Dm), lambda: _rms_fwd(x, w, p, seed)[0] != 0),
            "linear.hip": ((M, N), gemm)}


def test_epoch_reaches_every_translation_unit(device, seeds):
    ops = _ops()
    seed, p = seeds[3], 0.3
    probes = _epoch_probes(ops, device, seed, p)
    try:
        for epoch in (0, 1, (1 << 33) + 5):
            ops.seed_epoch_set(epoch)
            for unit, (shape, run) in probes.items():
                _same(run(), _keep(seed, shape, p, device, epoch), (unit, "epoch", epoch))
        ops.seed_epoch_set(5)
        ops.seed_epoch_advance()
        for unit, (shape, run) in probes.items():
            _same(run(), _keep(seed, shape, p, device, 6), (unit, "set 5, advance"))
    finally:
        ops.seed_epoch_set(0)
    for unit, (shape, run) in probes.items():
        _same(run(), _keep(seed, shape, p, device), (unit, "epoch restored"))
