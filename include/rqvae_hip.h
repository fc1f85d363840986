/* rqvae_hip.h — C ABI of the MI355X (gfx950) RQ-VAE training hot path.
 *
 * Library: rq-vae-recommender_amd/rqvae_hip/librqvae_hip.so (built by `make -C
 * rq-vae-recommender_amd/csrc`). Plain pointers and sizes only; no framework types.
 *
 * Conventions (every entry point):
 *   - All data pointers are DEVICE pointers owned by the caller; kernels never allocate/free.
 *   - `stream` is a hipStream_t (NULL = legacy default stream). Calls are asynchronous,
 *     stream-ordered, never synchronise the host, and are safe to capture in a hipGraph.
 *   - Return 0 on success, a hipError_t (> 0) on a launch/runtime failure, or a negative
 *     argument-check code (-22); rq_last_error() returns the message (thread-local).
 *   - Stateless and re-entrant (autograd may call backward from another host thread).
 *
 * The reference (AdamLTy/RQ-VAE-Recommender) has no FFI of its own: its hot path is Python
 * over ATen + one Triton kernel. Each entry point below names the reference function whose
 * semantics it implements; INTEGRATION.md shows the ctypes binding used by the drop-in
 * nn.Module / autograd.Function surface.
 */
#ifndef RQVAE_HIP_H_
#define RQVAE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library identification / errors. */
int rq_abi_version(void);
const char* rq_last_error(void);

/* Quantize modes (modules/quantize.py:16-20 QuantizeForwardMode; 0 = eval path :148-150). */
#define RQ_MODE_EVAL 0
#define RQ_MODE_STE 2
#define RQ_MODE_ROTATION 3

/* out[r] = sum_d rows[r][d]^2 for r < n — the (codebook.T**2).sum(0) term of the L2 distance
 * (modules/quantize.py:110). rows: (n, D) fp32. */
int rq_codebook_sqnorm(const float* rows, int64_t n, int64_t D, float* out, void* stream);

/* Fused L-level residual quantization forward = RqVae.get_semantic_ids' level loop
 * (modules/rqvae.py:114-138) over Quantize.forward (modules/quantize.py:99-156, L2 distance,
 * out_proj = Identity) with QuantizeLoss (modules/loss.py:34-42).
 *   x (B,D) fp32 encoder output; codebooks (L,K,D); cb_sqnorm (L,K) from rq_codebook_sqnorm.
 *   mode RQ_MODE_ROTATION / RQ_MODE_STE (training) or RQ_MODE_EVAL; beta = commitment weight.
 * Outputs: ids (B,L) int64; emb_out (L,B,D); residuals (L,B,D) with residuals[0] = x;
 *   qloss (B,) = sum_l loss_l; emb_sum (B,D) = sum_l emb_out_l, or NULL; emb_norms (L,B) =
 *   |emb_out[l][b]|_2, the embs_norm diagnostic of RqVae.forward (modules/rqvae.py:151), or NULL (the
 *   16x16 kernel writes them from its level epilogue; every other kernel adds one row-norm pass).
 * Requires D a power of two in [8, 1024], 1 <= K <= 2^20, 1 <= L <= 64. Ids are the lowest
 * index among equal minimum distances (torch.min semantics, quantize.py:121).
 * impl: the kernel (0 = auto: 4 for D == 64, K <= 288, B >= 32768; else 2 for D <= 64; else 3 when
 * allowed; else 1), 1 = fused LDS-tiled kernel (any D), 2 = register-resident 32x32x2 kernel (D <= 64),
 * 3 = split path for D >= 128 with 2*ceil(K/128)+1 <= D (per level: distance GEMM + partial argmin over
 * 128x128 tiles, then a row epilogue; emb_out doubles as the level's scratch before it is written),
 * 4 = register-resident 16x16x4 kernel (D == 64, K <= 288; 4 waves per SIMD). Every kernel gives the
 * same ids and the same outputs within fp32 summation order (kernel-vs-kernel tests). */
int rq_quantize_fwd(const float* x, int64_t B, int64_t D, const float* codebooks, const float* cb_sqnorm, int64_t K,
                    int64_t L, int mode, float beta, int64_t* ids, float* emb_out, float* residuals, float* qloss,
                    float* emb_sum, float* emb_norms, int impl, void* stream);

/* Backward of rq_quantize_fwd (the autograd graph of modules/quantize.py:99-156 chained by
 * modules/rqvae.py:129): grads of emb_out (g_emb, (L,B,D) or NULL), of sum_l emb_out
 * (g_emb_sum, (B,D) or NULL), of residuals (g_res, (L,B,D) or NULL) and of qloss (g_qloss,
 * (B,) or NULL). Writes grad_x (B,D) and grad_codebooks (L,K,D) (every element written).
 * The codebook gradient is reduced in ascending row order per codeword (stable counting
 * sort + segmented sum): bitwise deterministic. K <= 4096. An empty batch (B == 0) may come with NULL
 * residuals / ids / grad_x, as rq_quantize_fwd's may: grad_codebooks is zeroed.
 * workspace: device scratch of at least rq_quantize_bwd_workspace(B,D,K,L) bytes. */
size_t rq_quantize_bwd_workspace(int64_t B, int64_t D, int64_t K, int64_t L);
int rq_quantize_bwd(const float* residuals, const int64_t* ids, const float* codebooks, int64_t B, int64_t D, int64_t K,
                    int64_t L, int mode, float beta, const float* g_emb, const float* g_emb_sum, const float* g_res,
                    const float* g_qloss, float* grad_x, float* grad_codebooks, void* workspace, size_t ws_bytes,
                    void* stream);

/* The kernel form rq_quantize_fwd / rq_quantize_bwd launch for a shape: the same decision function the
 * launches go through, on the host, without a launch, an allocation or a device access. Tests use it to
 * ask which instantiation a shape reaches instead of restating the thresholds.
 * Forward: impl as rq_quantize_fwd's (0 = auto); with_norms != 0 stands for a non-NULL emb_norms. The
 * refusals are rq_quantize_fwd's shape refusals (D, K, L, B, mode, impl against D and K). B == 0: no launch,
 * every field 0. */
typedef struct rq_quantize_fwd_form {
  int impl;        /* the resolved kernel family: 1 tiled, 2 register, 3 split, 4 register 16x16; 0 = no launch */
  int d;           /* the family's D instantiation (16x16: 64) */
  int resident;    /* register: 1 = a level's codebook is one LDS image, 0 = streamed in images of nb rows */
  int wpi;         /* register: waves per 32-item tile (4, 2 or 1); 0 elsewhere */
  int nb;          /* register: codewords per LDS image; 0 elsewhere */
  int norms_pass;  /* 1 = emb_norms come from one rq_row_norms pass after the kernel (every family but 16x16) */
  int items;       /* items per workgroup of the (first) launch */
  unsigned grid;   /* its workgroups */
  int64_t lds_bytes;  /* its dynamic LDS */
} rq_quantize_fwd_form;
int rq_quantize_fwd_plan(int64_t B, int64_t D, int64_t K, int64_t L, int mode, int impl, int with_norms,
                         rq_quantize_fwd_form* form);
/* Backward: has_g_qloss != 0 stands for a non-NULL g_qloss. rq_bwd_rows_kernel<lpi, epl>, then the codebook
 * gradient by the chunk route (rq_cb_chunk_kernel<vpl> over chunks row chunks) or the sort route
 * (rq_cb_segsum_kernel: contrib = 1 sums the rows kernel's contributions (eval), 0 rebuilds 2 gl (e - x)
 * from the residuals; whether a codeword's segment is reduced directly or in partials depends on the ids). */
#define RQ_QUANTIZE_CB_NONE 0   /* B == 0: grad_codebooks zeroed, no kernel */
#define RQ_QUANTIZE_CB_CHUNK 1
#define RQ_QUANTIZE_CB_SORT 2
typedef struct rq_quantize_bwd_form {
  int lpi, epl;    /* rq_bwd_rows_kernel's lanes per item and elements per lane (0 when B == 0) */
  int route;       /* RQ_QUANTIZE_CB_* */
  int vpl;         /* chunk route: D / 64; 0 otherwise */
  int chunks;      /* chunk route: row chunks per level; 0 otherwise */
  int contrib;     /* sort route: 1 = contrib form, 0 = recompute form */
  int seg_direct;  /* sort route: the longest segment reduced by one workgroup */
  int seg_split;   /* sort route: partials of a longer one */
} rq_quantize_bwd_form;
int rq_quantize_bwd_plan(int64_t B, int64_t D, int64_t K, int64_t L, int mode, int has_g_qloss,
                         rq_quantize_bwd_form* form);

/* Deterministic segmented sum: out[k] = sum of rows[b] (B, D) over b with keys[b] == k (int64, in
 * [0, K)), reduced in a fixed order; counts[k] = #rows (or NULL). Used by the k-means codebook
 * init (init/kmeans.py:40-58 centroid means). D <= 1024, K <= 4096. */
size_t rq_segment_sum_workspace(int64_t B, int64_t K);
int rq_segment_sum(const float* rows, const int64_t* keys, int64_t B, int64_t D, int64_t K, float* out, int64_t* counts,
                   void* workspace, size_t ws_bytes, void* stream);

/* RMSNorm (modules/normalize.py:22-32): y = (x * rstd) * w, rstd = rsqrt(mean_j x^2 + eps) per row.
 * x, y: (B, D) fp32 rows, D % 4 == 0, D <= 4096; rstd (B,) saved for the backward. bwd: gx (B, D)
 * and gw (D,) = sum_b gy_b x_b rstd_b (fixed-order reduction; workspace >=
 * rq_rmsnorm_bwd_workspace(B, D) bytes). Replaces torch's pow/mean/rsqrt/mul chain (6 kernels fwd,
 * ~10 bwd) in the decoder (modules/model.py:54-55, modules/transformer/model.py:47-57). */
int rq_rmsnorm_fwd(const float* x, const float* w, int64_t B, int64_t D, float eps, float* y, float* rstd,
                   void* stream);
size_t rq_rmsnorm_bwd_workspace(int64_t B, int64_t D);
int rq_rmsnorm_bwd(const float* x, const float* w, const float* rstd, const float* gy, int64_t B, int64_t D,
                   float* gx, float* gw, void* workspace, size_t ws_bytes, void* stream);

/* RMSNorm followed by nn.Dropout(p) (modules/transformer/model.py:71,74 `self.do(self.attn_norm(x))`,
 * modules/model.py:128-129 `self.do(self.norm(...))`): y = keep * scale * rmsnorm(x), keep drawn from
 * a counter-based generator keyed by `seed` (element e of y keeps iff word e of SplitMix64(seed) >=
 * round(p 2^32); kept values scaled by 1/(1-p)), so the backward regenerates the mask from
 * (seed, e) instead of storing it. p = 0 is plain RMSNorm.
 * The generator, for every `seed` argument of this header: element e (row-major: r D + c here) takes 32-bit
 * word e & 1 (low word first) of mix(key + ((e >> 1) + 1) G), mix = SplitMix64's finaliser, G =
 * 0x9E3779B97F4A7C15, key = seed + epoch * 0xD6E8FEB86659FD93 (rq_seed_epoch_set). Raw seeds that differ by a
 * multiple of G therefore give the SAME mask shifted by two elements per multiple: pass mixed keys (a 64-bit
 * finaliser over whatever identifies the mask), as rqvae_hip.ops.next_seed does, never base + i. */
int rq_rmsnorm_dropout_fwd(const float* x, const float* w, int64_t B, int64_t D, float eps, float p, uint64_t seed,
                           float* y, float* rstd, void* stream);
/* Its backward, with two fusions and a deferral: gres (NULL or B x D) is added to gx — the gradient that
 * reaches x along the residual stream (modules/transformer/model.py:75-82: x feeds both the norm and the
 * residual add; autograd would sum the two in a separate pass) — and accumulate_gw = 1 adds the weight
 * gradient into gw instead of overwriting it (a flat data-parallel gradient bucket). defer = 1 leaves gw's
 * per-workgroup partials (*parts rows of D floats) at the start of the workspace and skips their reduction
 * (*parts = 0 when nothing was deferred); rq_reduce_partials (layout 1) later adds them into gw, batched
 * with other deferred reductions into one launch. workspace >= rq_rmsnorm_bwd_workspace(B, D) bytes. */
int rq_rmsnorm_dropout_bwd(const float* x, const float* w, const float* rstd, const float* gy, const float* gres,
                           int64_t B, int64_t D, float p, uint64_t seed, float* gx, float* gw, int accumulate_gw,
                           int defer, int* parts, void* workspace, size_t ws_bytes, void* stream);
/* Two RMSNorms of the same rows (the decoder block's attn_norm and cross_attn_norm of x,
 * modules/transformer/model.py:75-82), each with its own weight, dropout p and seed: one rstd, y1 and y2 —
 * bitwise two rq_rmsnorm_dropout_fwd calls, in one launch. The backward returns gx = norm2'(gy2) +
 * (norm1'(gy1) + gres) (the chained single-norm calls' roundings) and both weight gradients (accumulate /
 * defer as rq_rmsnorm_dropout_bwd; deferred: w1's partials at workspace, w2's at workspace +
 * rq_rmsnorm_bwd_workspace(B, D), *parts rows each). workspace >= 2 rq_rmsnorm_bwd_workspace(B, D) bytes. */
int rq_rmsnorm2_dropout_fwd(const float* x, const float* w1, const float* w2, int64_t B, int64_t D, float eps, float p1,
                            uint64_t seed1, float p2, uint64_t seed2, float* y1, float* y2, float* rstd, void* stream);
int rq_rmsnorm2_dropout_bwd(const float* x, const float* w1, const float* w2, const float* rstd, const float* gy1,
                            const float* gy2, const float* gres, int64_t B, int64_t D, float p1, uint64_t seed1, float p2,
                            uint64_t seed2, float* gx, float* gw1, float* gw2, int accumulate_gw, int defer, int* parts,
                            void* workspace, size_t ws_bytes, void* stream);
/* Elementwise dropout fusions over n fp32 elements (n % 4 == 0, 16-byte aligned), same mask
 * generator as above (element index = position in the buffer):
 *   rq_silu_dropout_fwd  h = Dropout(SiLU(z))         the MLP hidden layer (modules/encoder.py:20-28)
 *   rq_silu_dropout_bwd  gz = SiLU'(z) * keep * scale * g
 *   rq_dropout_add_fwd   out = h + Dropout(y)          the block output (modules/transformer/model.py:82)
 *   rq_dropout_bwd       gy = keep * scale * g         (grad of y; h's grad is g itself)
 * rq_dropout_params returns the (threshold, scale) pair the kernels use for p. Seeds: mixed keys, see
 * rq_rmsnorm_dropout_fwd (seeds a multiple of G apart give shifted copies of one mask). */
int rq_dropout_params(float p, uint32_t* thr, float* scale);
int rq_silu_dropout_fwd(const float* z, int64_t n, float p, uint64_t seed, float* h, void* stream);
int rq_silu_dropout_bwd(const float* g, const float* z, int64_t n, float p, uint64_t seed, float* gz, void* stream);
int rq_dropout_add_fwd(const float* h, const float* y, int64_t n, float p, uint64_t seed, float* out, void* stream);
int rq_dropout_bwd(const float* g, int64_t n, float p, uint64_t seed, float* gy, void* stream);

/* Dropout epoch: a device-side word mixed into every mask key of the functions above and of
 * rq_gemm_bf16x3_run (key = seed + epoch * C). 0 by default (keys = the host seeds). A train step
 * captured into a hipGraph ends with rq_seed_epoch_advance, so every replay draws fresh masks while
 * the forward and backward of one step share the epoch (replaces the per-step host RNG state that
 * torch.compile's cudagraphs trees manage for the reference's nn.Dropout, modules/model.py:247).
 * Both are stream-ordered kernel launches (capturable). */
int rq_seed_epoch_advance(void* stream);
int rq_seed_epoch_set(uint64_t value, void* stream);

/* Weight / bias gradient of a Linear layer over a large batch: dW (O,I) = g^T x, db (O,) = sum_b g
 * (or NULL). g: (Bn, O) rows of stride ldg, x: (Bn, I) rows of stride ldx, fp32, O, I, ld % 4 == 0,
 * 16-byte aligned. Replaces torch autograd's grad_weight = grad_out^T @ input for the nn.Linear
 * layers of modules/encoder.py:7-36 (RQ-VAE encoder/decoder MLPs): split-K over the batch with a
 * fixed-order reduction (deterministic). workspace >= rq_linear_wgrad_workspace(Bn, O, I) bytes. */
size_t rq_linear_wgrad_workspace(int64_t Bn, int64_t O, int64_t I);
int rq_linear_wgrad(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t Bn, int64_t O, int64_t I,
                    float* dW, float* db, void* workspace, size_t ws_bytes, void* stream);

/* fp32 GEMM at PyTorch's 'high' matmul precision, which the reference selects at import
 * (modules/rqvae.py:19, modules/model.py:27): each operand split as a = hi + lo in bf16, products
 * hi.hi + hi.lo + lo.hi accumulated in fp32 on bf16 MFMA (per-product relative error <= ~2^-17;
 * TF32's is 2^-11). Replaces the nn.Linear matmuls of modules/encoder.py:7-36 and
 * modules/transformer (forward x W^T, data grad g W, weight grad g^T x).
 *   C[m*ldc + n] = sum_k A(m,k) B(n,k),  A(m,k) = a_kcontig ? A[m*lda + k] : A[k*lda + m],
 *                                         B(n,k) = b_kcontig ? B[n*ldb + k] : B[k*ldb + n].
 * The contiguous axis of each operand (K for a k-contiguous one, else M or N) and lda, ldb % 4 == 0,
 * 16-byte aligned pointers. When the output tiles cannot fill the GPU, K is split across workgroups
 * with a fixed-order reduction (deterministic); that case needs ldc == N and workspace >=
 * rq_gemm_bf16x3_workspace(M, N, K) bytes (0 = the shape never splits). */
size_t rq_gemm_bf16x3_workspace(int64_t M, int64_t N, int64_t K);
int rq_gemm_bf16x3(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb, int b_kcontig, int64_t M,
                   int64_t N, int64_t K, float* C, int64_t ldc, void* workspace, size_t ws_bytes, void* stream);

/* Kernel policy of one call (rq_gemm_desc.flags; 0 = the time model picks per shape). For kernel-vs-kernel
 * tests and A/B measurements; every policy gives the same bits for the same split operands. */
#define RQ_GEMM_ONLY_128 1    /* the 128 x 128-tile kernel only (no wide kernel, no 64-tile form) */
#define RQ_GEMM_ONLY_64 2     /* the 64 x 64-tile form wherever the 128-tile kernel would run */
#define RQ_GEMM_FORCE_WIDE 4  /* the wide 256 x 256-tile kernel wherever it can run */
#define RQ_GEMM_NO_WIDE 8     /* never the wide kernel (128- / 64-tile chosen by the model) */
#define RQ_GEMM_MASKED 16     /* masked k staging even for whole 32-deep stages (bitwise the unmasked path) */
#define RQ_GEMM_NO_PAIR 32    /* rq_gemm_bf16x3_pair: two launches */
#define RQ_GEMM_NO_GROUP 64   /* rq_gemm_bf16x3_group: every member in its own launch */
/* flags | RQ_GEMM_SPLIT(S): split K into S chunks (1..4095; 0 = the planner's count) on the kernel the other
 * flags / the planner pick — a tuned plan for a known shape. S > 1 needs S x M x N fp32 of workspace (which
 * rq_gemm_bf16x3_workspace does not size for a forced S). Bits of a result depend on the chunking. */
#define RQ_GEMM_SPLIT_SHIFT 16
#define RQ_GEMM_SPLIT_MASK 0xFFF
#define RQ_GEMM_SPLIT(S) ((int)(S) << RQ_GEMM_SPLIT_SHIFT)

/* One general split-bf16 GEMM call (the fused MLP chain, modules/encoder.py:7-36 — Linear, SiLU,
 * [Dropout], ..., Linear — and every decoder Linear). An operand is fp32 (X_lo == NULL) or pre-split:
 * two bf16 planes (X = hi, X_lo = lo) of the operand's shape; split operands need their contiguous axis
 * and ld % 8 == 0. The epilogue turns the tile into:
 *   0  C = A B^T                                                  (accumulate = 1: C += A B^T)
 *   3  C = A B^T + Z                                              (a residual add after a projection);
 *      with p > 0: C = Z + Dropout_p(A B^T), the mask of rq_dropout_add_fwd (element m N + n), so
 *      rq_dropout_bwd regenerates it — the transformer block's h + Dropout(MLP(..)) in the MLP's last GEMM
 *   1  C = z = A B^T, and H = split(Dropout_p(SiLU(z)))          (a hidden layer's forward)
 *   2  H = split(SiLU'(Z) * Dropout_p(A B^T)), C unused          (its pre-activation grad)
 * H_hi / H_lo: bf16 planes (M, N) of row stride ldh; Z: (M, N) of stride ldc. The dropout mask is element
 * e = m N + n of the same counter-based mask as rq_silu_dropout_fwd (seed). Split-K applies to every
 * epilogue (partials in the workspace, a fixed-order reduction applies the epilogue). accumulate = 1
 * (plain epilogue only): C += A B^T — a weight gradient added straight into a flat data-parallel
 * gradient bucket (replaces autograd's AccumulateGrad add). defer = 1 (with accumulate): a split call
 * leaves its *splits partial slabs (M x N fp32 each) at the start of the workspace and does not reduce
 * them (*splits = 0: the call completed C itself); the caller adds them into C later with
 * rq_reduce_partials (layout 0), batched with other deferred reductions. */
typedef struct rq_gemm_desc {
  const void* A;
  const void* A_lo;
  int64_t lda;
  int a_kcontig;
  const void* B;
  const void* B_lo;
  int64_t ldb;
  int b_kcontig;
  int64_t M, N, K;
  float* C;
  int64_t ldc;
  int epilogue;
  const float* Z;
  uint16_t* H_hi;
  uint16_t* H_lo;
  int64_t ldh;
  float p;
  uint64_t seed;
  int accumulate;
  int defer;
  void* workspace;
  size_t ws_bytes;
  int flags;     /* RQ_GEMM_* kernel policy, 0 = automatic */
  int reserved;  /* 0 */
} rq_gemm_desc;
int rq_gemm_bf16x3_run(const rq_gemm_desc* d, int* splits, void* stream);
/* Two independent calls d[0], d[1] (splits[i] as rq_gemm_bf16x3_run's `splits`), results identical to the
 * two calls in a row; where both run on the 128- or 64-tile kernel with the same tile size and a paired
 * instantiation exists — a Linear's backward: d[0] the data gradient g W (SiLU'-with-dropout epilogue
 * allowed), d[1] the weight gradient g^T x (modules/encoder.py:7-36, modules/transformer: autograd's
 * grad_input / grad_weight of nn.Linear) — both problems' workgroups run in ONE launch (one launch instead
 * of two; together they fill the chip where each alone cannot). Also two forward projections of different
 * inputs (k-contiguous A, k-contiguous split B, plain store: the decoder block's self-attention qkv and
 * cross-attention q, modules/transformer/model.py:75-80); when both then use split-K, their slabs are
 * reduced in one launch (rq_reduce_partials' layout 0, bitwise the two reductions). RQ_GEMM_NO_PAIR in
 * either: two launches. */
int rq_gemm_bf16x3_pair(const rq_gemm_desc* d, int* splits, void* stream);
/* Host-only planning of a descriptor (pointers may be NULL): the kernel rq_gemm_bf16x3_run would launch —
 * 1 = the wide 256 x 256-tile kernel (both operands split, LDS-DMA staged, 8 waves), 0 = the 128 x 128-tile
 * kernel, 2 = its 64 x 64-tile form, -1 = empty shape / invalid — and *splits its split-K factor. */
int rq_gemm_bf16x3_plan(const rq_gemm_desc* d, int* splits);
/* 1 when rq_gemm_bf16x3_pair would run d[0], d[1] in one launch (host-only planning), else 0. */
int rq_gemm_bf16x3_pair_plan(const rq_gemm_desc* d);
/* Host-only planning for a Linear's backward pair, d[0] its data gradient and d[1] its weight gradient: the
 * split-K count that balances the weight gradient's workgroups with the data gradient's in the paired launch
 * (k chunks as long as the data gradient's K), which the caller adopts as RQ_GEMM_SPLIT(count) on d[1]; 0 = keep
 * the weight gradient's own plan. rq_gemm_bf16x3_pair never applies it itself: its results stay those of two
 * rq_gemm_bf16x3_run calls. */
int rq_gemm_bf16x3_pair_resplit(const rq_gemm_desc* d);
/* `count` (1..8) independent calls, the weight gradients dW = g^T x of one MLP chain (modules/encoder.py:7-36:
 * autograd's grad_weight of each nn.Linear). Members that carry an explicit split count (RQ_GEMM_SPLIT(S),
 * S >= 2) and have split m/n-contiguous operands, the plain epilogue, ldc == N, K % 32 == 0 and no other kernel
 * policy flag run in ONE wide-tile launch (gemm_x3w_group_kernel), each with its own split-K count over its
 * share of the grid; every other member runs as rq_gemm_bf16x3_run would run it, bit for bit. A grouped member
 * writes S slabs to its own workspace (S x M x N fp32) and is reduced in fixed order (rq_reduce_partials layout
 * 0), here in one launch or, with defer and accumulate, by the caller (splits[i] = S, as rq_gemm_bf16x3_run
 * reports); with the split count and chunk of its separate launch its bits are that launch's. RQ_GEMM_NO_GROUP
 * in any member: no grouped launch. */
int rq_gemm_bf16x3_group(const rq_gemm_desc* d, int count, int* splits, void* stream);
/* Host-only planning for rq_gemm_bf16x3_group (pointers may be NULL): the number of members that should share
 * the grouped launch (0: none) and splits[i] = member i's split-K count in it, 0 for a member left out.
 * Members with explicit counts: what the run does with them. Without: the time model's plan — one step budget
 * for all members, taken when it beats their separate plans (equal K of at least 32,768 rows) — which the
 * caller adopts by passing the counts as RQ_GEMM_SPLIT(splits[i]); they differ from the separate plans'
 * counts, so adopting them changes the fp32 summation order of those results. */
int rq_gemm_bf16x3_group_plan(const rq_gemm_desc* d, int count, int* splits);
/* Deferred partial reductions, up to 48 per launch: for each entry i, out_i[j] = (accumulate_i ? out_i[j] :
 * 0) + sum_{s < S_i} P_i[s n_i + j], j < n_i (n_i % 4 == 0, 16-B aligned pointers), in the order of the
 * reduction it replaces (layout 0: rq_gemm_bf16x3_run's slab reduction; layout 1: rq_rmsnorm_dropout_bwd's
 * weight-gradient partials) — bitwise the immediate result. Entries must not share an output. Host arrays. */
int rq_reduce_partials(int count, const float* const* P, float* const* out, const int64_t* n, const int* S,
                       const int* layout, const int* accumulate, void* stream);

/* rq_segment_sum over up to 16 sources at once (every embedding table of a decoder step: modules/model.py:59-63,
 * modules/embedding/id_embedder.py): source t's rows (n[t], D) with keys in [0, K[t]) (others and pad[t]
 * skipped) sum into rows [sum_{u<t} K[u], + K[t]) of out (sum K, D). One pack launch + one segmented-sum
 * chain instead of one chain per table; sum K <= 4096. */
size_t rq_segment_sum_multi_workspace(int count, const int64_t* n, const int64_t* K, int64_t D);
int rq_segment_sum_multi(int count, const float* const* rows, const int64_t* const* keys, const int64_t* n,
                         const int64_t* K, const int64_t* pad, int64_t D, float* out, void* workspace, size_t ws_bytes,
                         void* stream);
/* Decoder loss head (modules/model.py:137-143): X = out_proj output rows (B * npos_x, K), row stride ldx;
 * logits row r = b * npos + j is X row b * npos_x + j (the reference drops the last position);
 * u[r] = cross_entropy(logits[r], tgt[r], ignore_index=-1) (NaN for a target >= K), lse[r] = log sum_k
 * exp(x_k - max_k x_k) saved for the backward (which takes the row maximum again), logits = the contiguous
 * (B * npos, K) copy, loss = sum(u) / B, loss_d[j] = sum_b u[b][j] / B (fixed-order sums). K <= 1024. */
int rq_ce_loss_fwd(const float* X, int64_t ldx, int64_t K, const int64_t* tgt, int64_t B, int64_t npos, int64_t npos_x,
                   float* u, float* lse, float* logits, float* loss, float* loss_d, void* stream);
/* Its backward: dX (B * npos_x, K, contiguous) from g_loss (scalar), g_loss_d (npos) and g_logits
 * (B * npos, K), each optional (NULL = zero); rows of the dropped position and ignored targets get only
 * the g_logits part (or zeros). */
int rq_ce_loss_bwd(const float* X, int64_t ldx, int64_t K, const int64_t* tgt, const float* lse, int64_t B, int64_t npos,
                   int64_t npos_x, const float* g_loss, const float* g_loss_d, const float* g_logits, float* dX,
                   void* stream);
/* x (n fp32) -> hi = RN_bf16(x), lo = RN_bf16(x - hi) (bf16 bit patterns). */
int rq_split_bf16x3(const float* x, int64_t n, uint16_t* hi, uint16_t* lo, void* stream);
/* The same for count <= 48 tensors in one launch (x[t], n[t], hi[t], lo[t]: host arrays of device
 * pointers / element counts). */
int rq_split_bf16x3_multi(int count, const float* const* x, const int64_t* n, uint16_t* const* hi,
                          uint16_t* const* lo, void* stream);

/* Number of distinct L-tuples among the B rows of ids (B,L) -> *out_count (device int64).
 * p_unique_ids = count / B (modules/rqvae.py:152-157, which computes it in O(B^2 L)).
 * Requires K^L < 2^63. workspace >= rq_unique_workspace(B, L, K) bytes: where K^L <= 2^24 a byte map
 * of K^L bytes (counted in one pass, no scattered atomics), else a hash table of ~2B slots. */
size_t rq_unique_workspace(int64_t B, int64_t L, int64_t K);
int rq_unique_count(const int64_t* ids, int64_t B, int64_t L, int64_t K, int64_t* out_count, void* workspace,
                    size_t ws_bytes, void* stream);

/* p_unique_ids itself (modules/rqvae.py:152-157: the count / B the train step logs, as torch's true_divide by
 * the scalar B computes it, count * (1 / B) in fp32) -> *out_frac (device float), and the count -> *out_count
 * (either may be NULL, not both); B >= 1. Two launches where K^L <= 2^24 at large B: a bit map of the keys
 * (atomicOr) and one counting pass that also clears it — the workspace (>= rq_unique_fraction_workspace bytes)
 * must then be ALL ZERO on entry and is left all zero (keep one per stream; zero it once). Else the hash table
 * of rq_unique_count (self-initialising) and a division launch. */
size_t rq_unique_fraction_workspace(int64_t B, int64_t L, int64_t K);
int rq_unique_fraction(const int64_t* ids, int64_t B, int64_t L, int64_t K, int64_t* out_count, float* out_frac,
                       void* workspace, size_t ws_bytes, void* stream);

/* out[j] (+)= sum_{s < S} P[s * n + j] for j < n, in a fixed order (deterministic, no atomics):
 * the batch-sum gradient of a parameter broadcast over the batch — `pos + seq_emb` and
 * `bos_emb.repeat(B, 1, 1)` of EncoderDecoderRetrievalModel._predict (modules/model.py:91-95).
 * n % 4 == 0; P and out 16-byte aligned. accumulate != 0: out += sum. */
int rq_col_sum(const float* P, int64_t S, int64_t n, float* out, int accumulate, void* stream);

/* Fused decoder head of RqVae.forward (modules/rqvae.py:145-150): x_hat = l2norm(pre) (decoder MLP's
 * final L2NormalizationLayer, F.normalize eps 1e-12) and recon[b] = sum_c (x_hat - x)^2
 * (modules/loss.py:5-10). pre, x: (B, C) fp32, C % 4 == 0, C <= 4096. fwd writes recon (B,) and
 * norms (B,) = |pre_b| (saved for bwd); bwd writes g_pre (B, C) from g_recon (B,). */
int rq_l2norm_recon_fwd(const float* pre, const float* x, int64_t B, int64_t C, float* recon, float* norms,
                        void* stream);
int rq_l2norm_recon_bwd(const float* pre, const float* x, const float* norms, const float* g_recon, int64_t B,
                        int64_t C, float* g_pre, void* stream);
/* The same gradient emitted as split-bf16 planes (g = hi + lo, rq_split_bf16x3's form): the input of the
 * decoder MLP's last data-grad / weight-grad GEMMs at matmul precision 'high'. */
int rq_l2norm_recon_bwd_split(const float* pre, const float* x, const float* norms, const float* g_recon, int64_t B,
                              int64_t C, uint16_t* g_hi, uint16_t* g_lo, void* stream);
/* rq_l2norm_recon_fwd plus, in the same pass over pre and x, the split gradient rq_l2norm_recon_bwd_split
 * would write if g_recon[b] = gs for every row (the batch-mean loss, loss_means: gs = 1 / B) — speculative:
 * the backward then only checks g_recon (rq_l2norm_recon_bwd_fix) instead of reading pre and x again. */
int rq_l2norm_recon_fwd_grad(const float* pre, const float* x, int64_t B, int64_t C, float* recon, float* norms,
                             float gs, uint16_t* g_hi, uint16_t* g_lo, void* stream);
/* The backward after rq_l2norm_recon_fwd_grad: rows whose g_recon[b * g_stride] (g_stride 0: one value for
 * every row, 1: one per row) is bitwise gs keep the planes the forward wrote; every other row is recomputed
 * with rq_l2norm_recon_bwd_split's arithmetic (same bits as that call). */
int rq_l2norm_recon_bwd_fix(const float* pre, const float* x, const float* norms, const float* g_recon,
                            int64_t g_stride, int64_t B, int64_t C, float gs, uint16_t* g_hi, uint16_t* g_lo,
                            void* stream);

/* RqVae.forward statistics (modules/rqvae.py:151-162):
 *   rq_row_norms   out[r] = |x_r|_2 for rows (rows, D), D % 4 == 0 — embs_norm = emb.norm(dim=-1)
 *   rq_loss_means  out[3] = {mean(recon + qloss), mean(recon), mean(qloss)} over B rows, one
 *                  deterministic pass (the loss and the two logged components). */
int rq_row_norms(const float* x, int64_t rows, int64_t D, float* out, void* stream);
int rq_loss_means(const float* recon, const float* qloss, int64_t B, float* out, void* stream);
/* Its backward when only the total loss out[0] has a gradient g (device scalar): *out_scalar = g * (1 / B)
 * (torch: g / B), and out_vec[0..B) = the same value (the per-row qloss gradient) — one launch. */
int rq_loss_means_bwd(const float* g, int64_t B, float* out_scalar, float* out_vec, void* stream);

/* Gumbel-softmax quantize, training (replaces modules/quantize.py:107-112,121,124-129 with
 * distributions/gumbel.py:14-18 for GUMBEL_SOFTMAX + L2): per row b, dist_k = |x|^2 + |c_k|^2 - 2 x.c_k,
 * ids[b] = argmin_k dist (lowest index on ties), weights = softmax((noise - dist) / temperature) over the K
 * codes (noise: (B, K) Gumbel samples drawn by the caller, as the reference's sample_gumbel), emb = weights @
 * codebook. x (B, D), codebook (K, D), weights (B, K), emb (B, D), all contiguous fp32; D <= 256, K <= 4096.
 * rq_gumbel_softmax_bwd: g_emb (B, D) -> dx (B, D) and ddist (B, K) = d loss / d dist; the codebook gradient
 * weights^T g_emb + 2 colsum(ddist) (.) codebook - 2 ddist^T x is the caller's GEMMs. */
int rq_gumbel_softmax_fwd(const float* x, int64_t B, int64_t D, const float* codebook, int64_t K, const float* noise,
                          float temperature, float* weights, float* emb, int64_t* ids, void* stream);
int rq_gumbel_softmax_bwd(const float* x, const float* codebook, const float* weights, const float* g_emb, int64_t B,
                          int64_t D, int64_t K, float temperature, float* dx, float* ddist, void* stream);

/* Jagged (NJT) conversion — ops/triton/jagged.py. dtype: 0 fp32, 1 bf16, 2 fp16.
 * jagged_offsets: offsets (B+1) int64 = [0, cumsum(clamp(lengths, 0, N))]   (jagged.py:30-33)
 * jagged_from_padded: values[offsets[b]+t] = x[b,t] (+1-1 rounding when add_one_sub_one, as
 *   `target + 1 - 1` at jagged.py:65), x (B,N,D) contiguous            (jagged.py:11-66,92-125)
 * jagged_from_padded_rows: the same into a values buffer of alloc_rows (>= offsets[B]) rows whose tail
 *   rows [offsets[B], alloc_rows) are zero-filled on the device (a row-bucketed allocation: the
 *   caller never needs the valid total on the host, so the call is graph-capturable per bucket)
 * jagged_to_padded: x = zeros(B,N,D); x[b,t] = values[offsets[b]+t] for t < len_b (jagged.py:69-77)
 * B < 65535 per call. */
int jagged_offsets(const int64_t* lengths, int64_t B, int64_t N, int64_t* offsets, void* stream);
int jagged_from_padded(const void* x, int64_t B, int64_t N, int64_t D, const int64_t* offsets, void* values, int dtype,
                       int add_one_sub_one, void* stream);
int jagged_from_padded_rows(const void* x, int64_t B, int64_t N, int64_t D, const int64_t* offsets, void* values,
                            int64_t alloc_rows, int dtype, int add_one_sub_one, void* stream);
int jagged_to_padded(const void* values, const int64_t* offsets, int64_t B, int64_t N, int64_t D, void* x, int dtype,
                     void* stream);

/* Decoder input embeddings straight into the two jagged batches (reference modules/model.py:101-129
 * `_predict` up to padded_to_jagged_tensor, with modules/embedding/id_embedder.py:28-53 SemIdEmbedder /
 * UserIdEmbedder): context row 0 = user_w[user_ids[b] mod n_buckets]; context row 1 + j = wpe_w[j] +
 * sem_w[seq_mask ? type_ids * K + sem_ids : pad] for j < sum(seq_mask[b]); future row 0 = bos, future row
 * 1 + t = sem_w[type_ids_fut * K + sem_ids_fut] + tte_w[type_ids_fut]; every value through the jagged
 * gather's (v + 1) - 1 (ops/triton/jagged.py:65): bitwise the reference composition.
 *   ids (B, N) / (B, L) int64, seq_mask (B, N) bool, tables fp32 row-major with E columns (E % 4 == 0);
 *   ctx_values (ctx_alloc_rows, E): rows past ctx_offsets[B] zero; ctx_offsets (B+1) = [0, cumsum(sum(mask)+1)];
 *   fut_values (B * (L+1), E), fut_offsets (B+1) = b (L+1); keys (B, N+L) int64 = the context's sem-table rows
 *   then the future's (the backward's segmented-sum keys), uid_mod (B) int64; lpt_order (NULL or B int32, B <= 4096):
 *   the contexts longest-first (the ranking of the attention LPT order, for RQ_ATTN_ORDER_GIVEN). Two launches;
 *   graph-capturable. */
int rq_dec_prologue_fwd(const int64_t* user_ids, const int64_t* sem_ids, const int64_t* type_ids, const bool* seq_mask,
                        const int64_t* sem_ids_fut, const int64_t* type_ids_fut, int64_t B, int64_t N, int64_t L,
                        int64_t E, const float* user_w, int64_t n_buckets, const float* sem_w, int64_t n_sem_rows,
                        int64_t K, int64_t pad, const float* wpe_w, int64_t n_wpe_rows, const float* tte_w,
                        int64_t n_tte_rows, const float* bos, float* ctx_values, int64_t ctx_alloc_rows,
                        int64_t* ctx_offsets, float* fut_values, int64_t* fut_offsets, int64_t* keys, int64_t* uid_mod,
                        int* lpt_order, void* stream);

/* Varlen multi-head attention on packed rows = F.scaled_dot_product_attention on NJT q/k/v
 * (modules/transformer/attention.py:113-124), dropout 0, is_causal top-left.
 *   q[t][h][d] at q + t*sq + h*hd + d (likewise k, v, out, dout, dq, dk, dv with their strides);
 *   cu_q, cu_k (B+1) int64 offsets; max_q / max_k >= the longest segment (grid bound);
 *   lse (H, Tq) fp32 log-sum-exp per query (written by fwd, read by bwd). hd in {16, 32, 64, 128}.
 *   Tq / Tk: ALLOCATED rows of the q-side / kv-side buffers (>= cu_q[B] / cu_k[B]); rows past the
 *   last sequence get zero out / dq / dk / dv (written by the kernels: graph-capturable per bucket).
 *   ws / ws_elems: caller-provided fp32 scratch of at least varlen_attn_{fwd,bwd}_ws_elems(...) floats, or
 *   NULL / 0 (the forms that need none).
 *   flags: RQ_ATTN_* kernel policy, 0 = the measured-best forms (kernel-vs-kernel tests / A/B runs; every
 *   policy computes the same function within fp32 summation order).
 * Forward: with scratch, long ranges (max_k > 128, 2 <= B <= 4096) rank the sequences longest-first and
 * dispatch their workgroups in that order (no straggler tail); <= 16 queries per sequence over > 128 keys
 * (non-causal: the decoder's cross-attention) run split-key partials (one one-wave workgroup per 128-key
 * block) merged per query in block order (deterministic); many queries over long keys at low occupancy run
 * the key-split form. Backward is deterministic (no atomics): short ranges run one-pass forms (dQ, dK, dV
 * from S and dP formed once per tile pair); with scratch, longer ranges (hd == 64) run ONE fused launch
 * per key block (after a delta = rowsum(dO*O) pre-pass) whose dQ partials are summed in block order by a
 * reduction launch, and — when varlen_attn_bwd_ws_elems was given Tk >= 0 — may split each key block's
 * query range over up to 4 workgroups when the grid cannot fill the GPU (few long sequences per GPU),
 * their dK / dV partials summed in split order. Without scratch those ranges run the two-pass form (dQ per
 * query block, writing delta (H, Tq) to the caller's `delta`, then dK / dV per key block). */
#define RQ_ATTN_NO_DMA 1          /* register-staged short forms instead of the LDS-DMA ones */
#define RQ_ATTN_TWO_PASS 2        /* two-pass backward everywhere (no one-pass / fused forms) */
#define RQ_ATTN_NO_SPLIT 4        /* no split-key / key-split forward */
#define RQ_ATTN_SPLIT_BF16 8      /* matmul precision 'high': the hd-64 forwards over more than 32 keys with more
                                     than 16 queries per sequence (chunked, key-split and short forms) or with
                                     few queries over long key ranges (cross-attention, key-split form) multiply
                                     Q K^T and P V in split-bf16 (3 bf16 MFMA products, fp32 accumulate and
                                     softmax) instead of exact fp32; so does the fused long-range backward (S, dP,
                                     dV, dK and dQ products; P, dS fp32) */
#define RQ_ATTN_FEWQ_WG 16        /* few-query backward over 49..128 keys: one workgroup per (sequence, head) instead of
                                     the persistent walk with the next unit staged by LDS-DMA (same bits) */
#define RQ_ATTN_LPT_SHORT 32      /* the short / few-query forms (<= 128 keys) also dispatch their sequences longest-first
                                     (an order launch; the backward's scratch then holds B ints) */
#define RQ_ATTN_ORDER_GIVEN 64    /* ws[0, B) (as int32) already holds the longest-first order of cu_k's segments (e.g. from
                                     rq_dec_prologue_fwd): the forwards and the short backwards use it without an order
                                     launch (the fused long-range backward keeps its own) */
#define RQ_ATTN_QSPLIT_SHIFT 8
#define RQ_ATTN_QSPLIT(n) ((n) << RQ_ATTN_QSPLIT_SHIFT)   /* fused backward query splits forced to n (1..8; 1 = off) */
int varlen_attn_fwd_ws_elems(int64_t B, int64_t H, int64_t hd, int64_t max_q, int64_t max_k, int64_t Tq, int causal,
                             int flags, int64_t* elems);
int varlen_attn_fwd(const float* q, int64_t sq, const float* k, int64_t sk, const float* v, int64_t sv,
                    const int64_t* cu_q, const int64_t* cu_k, int64_t B, int64_t H, int64_t hd, int64_t max_q,
                    int64_t max_k, int causal, float scale, float* out, int64_t so, float* lse, int64_t Tq, float* ws,
                    int64_t ws_elems, int flags, void* stream);
/* Tk < 0: scratch without the query splits' dK / dV partials. */
int varlen_attn_bwd_ws_elems(int64_t B, int64_t H, int64_t hd, int64_t max_q, int64_t max_k, int64_t Tq, int64_t Tk,
                             int flags, int64_t* elems);
int varlen_attn_bwd(const float* q, int64_t sq, const float* k, int64_t sk, const float* v, int64_t sv, const float* out,
                    int64_t so, const float* dout, int64_t sdo, const float* lse, int64_t Tq, const int64_t* cu_q,
                    const int64_t* cu_k, int64_t B, int64_t H, int64_t hd, int64_t max_q, int64_t max_k, int causal,
                    float scale, float* dq, int64_t sdq, float* dk, int64_t sdk, float* dv, int64_t sdv, int64_t Tk,
                    float* delta, float* ws, int64_t ws_elems, int flags, void* stream);

/* Host-only planning of one varlen_attn_fwd (backward = 0) or varlen_attn_bwd (backward = 1) call: the
 * launches the call issues, in order, and how it lays out its workspace. The entry points above launch from
 * this same plan (csrc/attention_plan.h; DESIGN.md "Attention dispatch" tabulates the rules), so a test can
 * ask which kernel form a shape dispatches. No launch, no allocation; the only device access is the cached
 * CU-count query of the backward's query splits and persistent few-query walk (256, the MI355X count,
 * without a GPU: plans are the same on a machine without one).
 *   ws_elems: the floats of scratch the call would bring, < 0 for none (ws == NULL); Tk: as varlen_attn_bwd's,
 *   or < 0 as for varlen_attn_bwd_ws_elems (a plan without query splits); the forward ignores it.
 * One launch: the kernel family and the family's integer template arguments, 0 where it has none —
 *   hd (head dim), nw (waves per workgroup), r (staged rows R / chunk CH / key block KB), x3 (split-bf16
 *   products) — then grid and block. RQ_ATTN_K_BWD_FUSED with x3 = 1 is attn_bwd_fused_x3_kernel. */
enum {
  RQ_ATTN_K_ORDER = 1,        /* attn_order_kernel: longest-first ranking of order_src's segments */
  RQ_ATTN_K_FWD,              /* attn_fwd_kernel<hd, nw, x3>: the chunked forward */
  RQ_ATTN_K_FWD_SHORT,        /* attn_fwd_short_kernel<hd, nw, r> */
  RQ_ATTN_K_FWD_DMA,          /* attn_fwd_dma_kernel<nw, r> */
  RQ_ATTN_K_FWD_SHORT_X3,     /* attn_fwd_short_x3_kernel<r> */
  RQ_ATTN_K_FWD_FEWQ,         /* attn_fwd_fewq_kernel<nw> */
  RQ_ATTN_K_FWD_SPLIT,        /* attn_fwd_split_kernel<hd, r> */
  RQ_ATTN_K_FWD_KVSPLIT,      /* attn_fwd_kvsplit_kernel<hd, nw, r, x3> */
  RQ_ATTN_K_FWD_COMBINE,      /* attn_fwd_combine_kernel<hd, r> */
  RQ_ATTN_K_BWD_DQ,           /* attn_bwd_dq_kernel<hd, nw>: the chunked dQ pass */
  RQ_ATTN_K_BWD_DKDV,         /* attn_bwd_dkdv_kernel<hd, nw>: the chunked dK / dV pass */
  RQ_ATTN_K_BWD_DQ_SHORT,     /* attn_bwd_dq_short_kernel<hd, nw, r> */
  RQ_ATTN_K_BWD_DKDV_SHORT,   /* attn_bwd_dkdv_short_kernel<hd, nw, r> */
  RQ_ATTN_K_BWD_DQ_DMA,       /* attn_bwd_dq_dma_kernel<nw, r> */
  RQ_ATTN_K_BWD_DKDV_DMA,     /* attn_bwd_dkdv_dma_kernel<nw, r> */
  RQ_ATTN_K_BWD_DQ_FEWQ,      /* attn_bwd_dq_fewq_kernel<nw> */
  RQ_ATTN_K_BWD_FEWQ_FUSED,   /* attn_bwd_fewq_fused_kernel<nw> */
  RQ_ATTN_K_BWD_FEWQ_STREAM,  /* attn_bwd_fewq_stream_kernel<r> */
  RQ_ATTN_K_BWD_SHORT_FUSED,  /* attn_bwd_short_fused_kernel<nw, r> */
  RQ_ATTN_K_DELTA,            /* attn_delta_kernel<hd> */
  RQ_ATTN_K_BWD_FUSED,        /* attn_bwd_fused_kernel<hd, nw, r> / attn_bwd_fused_x3_kernel<nw, r> */
  RQ_ATTN_K_KV_REDUCE,        /* attn_kv_reduce_kernel<hd> */
  RQ_ATTN_K_DQ_REDUCE         /* attn_dq_reduce_kernel<hd, r> */
};
enum { RQ_ATTN_ORDER_SRC_NONE = 0, RQ_ATTN_ORDER_SRC_CU_Q, RQ_ATTN_ORDER_SRC_CU_K, RQ_ATTN_ORDER_SRC_GIVEN };
#define RQ_ATTN_MAX_LAUNCHES 6
typedef struct rq_attn_launch {
  int family;  /* RQ_ATTN_K_* */
  int hd, nw, r, x3;
  int block;
  unsigned grid[3];
} rq_attn_launch;
typedef struct rq_attn_plan {
  int n_launches;
  int qsplit;     /* query splits of the fused backward (1 = none) */
  int order_src;  /* RQ_ATTN_ORDER_SRC_*: the offsets array the order ranks, or GIVEN (RQ_ATTN_ORDER_GIVEN) */
  int reserved;   /* 0 */
  int64_t ws_total;  /* = varlen_attn_{fwd,bwd}_ws_elems(...) floats, whatever ws_elems is */
  int64_t ws_need;   /* a call that brings a workspace must bring this many floats (backward: ws_total
                        without the query splits' dK / dV partials) */
  /* float offsets into the workspace, -1 = absent: the order (B int32), the forward's split partials or
   * the fused backward's dQ partials, the query splits' dK / dV partials */
  int64_t order_off, part_off, kvpart_off;
  rq_attn_launch launch[RQ_ATTN_MAX_LAUNCHES];
} rq_attn_plan;
int varlen_attn_plan(int backward, int64_t B, int64_t H, int64_t hd, int64_t max_q, int64_t max_k, int64_t Tq,
                     int64_t Tk, int causal, int flags, int64_t ws_elems, rq_attn_plan* plan);

/* Decoder evaluation (csrc/beam.hip): one beam step of EncoderDecoderRetrievalModel.generate_next_sem_id
 * (modules/model.py:176-201) in two launches, and the Hit@k counters of TopKAccumulator.accumulate
 * (evaluate/metrics.py:15-28). No call allocates or synchronises; all are graph-capturable.
 *
 * rq_beam_candidates: per row of logits (R, V) fp32, p = softmax(logits / temperature) (model.py:177) and the
 *   score s_v = p_v / noise[r][v] (noise (R, V) fp32, or NULL: s_v = p_v). cand_ids (R, n_cand) int64 = the n_cand
 *   classes of largest score, descending, ties to the lower class; cand_lp (R, n_cand) fp32 = log p of each (-inf
 *   where p underflows to 0; otherwise formed as (z - max) - log1p(sum of the other exponentials), which is
 *   log p to fp32 relative precision also where one class takes nearly all the mass). With Exponential(1)
 *   noise the ids are distributed as torch.multinomial(p, n_cand, replacement=False) (model.py:178, the
 *   exponential-race form torch itself uses); without noise they are the n_cand most probable classes.
 *   1 <= n_cand <= V <= 4096, temperature > 0.
 * rq_beam_select: per batch element b the k best of its N = kprev * n_cand candidates (cand_ids / cand_lp viewed as
 *   (B, N); candidate e continues parent beam e / n_cand). parents (B, kprev, P) int64 and parent_lp (B, kprev) fp32
 *   are the beams so far (both NULL when P == 0, the first step). Validity of a candidate comes from exactly one of
 *   valid ((B, N) bool, the result of any inference_verifier_fn) and keys (n_keys sorted unique int64: the packed
 *   corpus prefixes of length P + 1, SemanticIdTokenizer.prefix_table; the kernel packs (parent prefix, candidate) in
 *   base `base`, every element required in [0, base), and binary-searches it; a global flat candidate index b N + e
 *   >= checked is invalid — the reference's exists_prefix skips its last partial batch of 16, semids.py:105-120;
 *   checked = B N switches that off). score = ((valid ? 0 : -10000) + cand_lp) + parent_lp (model.py:190-194, that
 *   fp32 order); out_lp (B, k) = the k largest scores, descending, ties to the lower e (a stable sort); out_ids
 *   (B, k, P + 1) = the parent's prefix followed by the candidate id. 1 <= k <= N <= 8192, P < 64.
 * rq_topk_hits: actual (B, D) int64 targets, topk (B, k, D) int64 beams, ks: HOST array of n_ks ints (copied into the
 *   kernel arguments). counts (2, D, n_ks) int64 is ACCUMULATED into (the caller zeroes it once):
 *   counts[0][i][j] += #rows whose first beam equal to the target in columns 0..i has rank < ks[j] (h@k_slice_:i+1),
 *   counts[1][i][j] the same for column i alone (h@k_pos_i). D <= 64, n_ks <= 8.
 * rq_beam_select_parent: rq_beam_select that also writes out_parent (B, k) int32 = each winner's parent beam index
 *   e / n_cand in [0, kprev) (NULL: not written; rq_beam_select is this call with NULL). out_ids / out_lp are the same.
 * rq_beam_self_attn: incremental decoding — the newest token's causal self-attention of R beams over their own
 *   ancestors. Step s = 0..t wrote a packed qkv buffer of R_s = rows[s] rows that stays where it is; k_steps[s] /
 *   v_steps[s] are its K / V column views (device pointers, row stride strides[s] floats, 16-byte aligned). The
 *   four step arrays are HOST arrays of t + 1 entries, copied into the kernel arguments (no device table, no
 *   copy). Entry t is the current step: beam r is its own key / value row and rows[t] == R. anc: DEVICE (R, t)
 *   int32, anc[r][s] = the row of step s's buffer that holds beam r's token s (NULL iff t == 0); beams that share
 *   an ancestor share its row, so re-ordering beams after a selection moves no K / V. The kernel does NOT check
 *   anc: entries in [0, rows[s]) are the caller's contract (out-of-range ones are clamped into the buffer and give
 *   an unspecified result). out[r, h] = sum_s softmax_s(scale q[r,h] . k_s[anc[r][s], h]) v_s[anc[r][s], h]: fp32
 *   scores, max subtracted, sums over s = 0..t in ascending order; at t == 0 out == v bitwise. q (R, H hd) with
 *   row stride sq, out row stride so; every stride >= H hd and a multiple of 4; hd in {16, 32, 64, 128};
 *   0 <= t < RQ_BEAM_MAX_T; R == 0 returns 0 without a launch.
 * rq_beam_expand: constrained decoding — one beam step against the corpus' prefix trie in ONE launch (no noise, no
 *   candidate lists, no table search). The trie is level-by-level CSR (SemanticIdTokenizer.prefix_trie): child_off
 *   (n_nodes + 1 int32) of level P and tok (n_children int32) of level P + 1; node i's children are
 *   [child_off[i], child_off[i + 1]), ascending by token. node (B, kprev) int32 is each beam's level-P node (NULL iff
 *   P == 0: every beam sits on the root, node 0); parents (B, kprev, P) int64 / parent_lp (B, kprev) fp32 as
 *   rq_beam_select (NULL iff P == 0). Candidates of batch element b: for every live beam j (node in [0, n_nodes)),
 *   every child c of its node with v = tok[c] in [0, V); score = lp(j, v) + parent_lp[b][j], lp the log-softmax of
 *   logits[b kprev + j] / temperature formed exactly as rq_beam_candidates forms cand_lp (bitwise equal). Outputs, k
 *   best in descending score order, ties to the lower beam then the lower token, NaN on top: out_ids (B, k, P + 1)
 *   int64 = parent prefix then token, out_lp (B, k) fp32, out_parent (B, k) int32 in [0, kprev), out_node (B, k)
 *   int32 = the winner's level-(P + 1) node c. With fewer than k candidates the remaining rows are DEAD: out_ids all
 *   -1, out_lp -inf, out_parent 0, out_node -1; a dead or out-of-range node entry contributes no candidates. The
 *   tables are the caller's contract, but a bad one never reads outside a buffer: child_off is clamped into
 *   [0, n_children], tokens outside [0, V) are skipped (an unsorted range gives an unspecified out_node or -1).
 *   V <= 4096, kprev V <= 8192, 1 <= k <= 8192, P < 64, temperature > 0; outside that -22, never a truncated result.
 *   The two optional filters come last, before the stream: blocked, n_blocked, allowed, n_words, G, group.
 *   blocked (seen-item exclusion; NULL with n_blocked == 0: no exclusion): (B, n_blocked) int32, row b holds the
 *   level-(P + 1) nodes that are not candidates for batch element b, ascending and padded with INT32_MAX (a slice of
 *   rq_trie_blocked_nodes' output); a child c found in row b is skipped, everything else is as without it (the same
 *   kernel body: scores, tie rule, dead rows, out_node, table clamping, limits). An unsorted row may filter the wrong
 *   children but is never read outside [0, n_blocked). 0 <= n_blocked <= 1024.
 *   group (catalogue filters, "only these items"; NULL: no catalogue filter, allowed / n_words / G are then not looked
 *   at): (B) int32, with allowed (G, n_words) int32 the level-(P + 1) slice of rq_trie_allowed_nodes' bitmaps: bit
 *   (c & 31) of word (c >> 5) in row g is set iff node c has an allowed item below it in group g. A child c of batch
 *   element b is a candidate iff it passes the blocked test AND (group[b] is outside [0, G) — that user is
 *   unfiltered, -1 is the documented spelling — OR bit c of row group[b] is set). A word index outside [0, n_words)
 *   reads as "not allowed" and is never read. Everything else is the unfiltered kernel body, bit for bit (log-softmax,
 *   tie rule, dead rows, out_node, table clamping, limits), so a filtered search is the unfiltered search over the
 *   corpus of the allowed rows. The rows are read from global memory: no LDS is added. With group given, allowed may
 *   be NULL only when G n_words == 0; n_words or G negative: -22. Both filters may be given: a candidate passes both.
 * rq_beam_expand_wide: rq_beam_expand (the same arguments, NULL meaning the same, one launch, one workgroup per batch
 *   element) for 1 <= kprev <= 1024 and 1 <= k <= 1024 with V <= 4096 and NO bound on kprev V: the candidates
 *   are enumerated from the trie, never stored, and the k best are found by an exact radix
 *   select over (score, beam, token). Wherever both accept a shape the four outputs are bit for bit the same — ids,
 *   out_lp, parents, nodes, the dead rows after the last candidate, the tie rule, the table clamping; a child range
 *   longer than V is searched for its first token >= V (a sorted range loses only skipped children), and duplicate
 *   (beam, token) pairs of a bad table give an unspecified choice among them, never an access outside a buffer.
 *   kprev > 1024 or k > 1024: -22.
 * rq_beam_expand_sampled: one step of stochastic beam search over the trie (Kool, van Hoof and Welling 2019, "Stochastic
 *   Beams and Where to Find Them", Algorithm 1; the reference has no counterpart — its generate_next_sem_id(sample=True),
 *   model.py:176-201, draws unconstrained classes and masks them afterwards): after the last level the k rows are k
 *   distinct corpus rows drawn without replacement from the trie's distribution, in ONE launch per step. The arguments
 *   are rq_beam_expand's (the filters included: blocked NULL with n_blocked == 0 and group NULL mean what they mean
 *   there) with noise (B kprev, V) fp32 Exponential(1)
 *   draws in rq_beam_candidates' layout, parent_phi / parent_g (B, kprev) fp32 in place of parent_lp (both NULL iff
 *   P == 0: taken as 0) and out_phi / out_g (B, k) fp32 in place of out_lp. A beam carries phi, its log-probability
 *   under the locally renormalised trie distribution, and G, its perturbed score. For a live beam j and its candidates
 *   C_j (the children rq_beam_expand scores: token in [0, V), not blocked, allowed), with l_c the full-V log-softmax
 *   rq_beam_expand forms (bitwise): Lam_j = log sum_{c in C_j} exp(l_c) (max subtracted; with a catalogue
 *   filter it runs over the candidates that remain); phi_c = phi_j + (l_c - Lam_j);
 *   Gt_c = phi_c - log(noise[b kprev + j][token_c]) (a noise value that is not a positive finite float is read as
 *   FLT_MIN; noise is read at candidates only); Z_j = max_c Gt_c; v = G_j - Gt_c + log(1 - exp(Gt_c - Z_j));
 *   G_c = G_j - max(v, 0) - log1p(exp(-|v|)), so the arg-max child keeps G_j exactly and every G_c <= G_j. l_c, Lam_j,
 *   phi_j or G_j at -inf gives phi_c = G_c = -inf: still a candidate, above the dead rows. The k candidates of largest
 *   G_c, ties to the lower beam then the lower token, descending: out_ids, out_parent, out_node and the dead rows as
 *   rq_beam_expand, out_g, and out_phi = the phi_c that the winner's Gt_c was formed from (dead rows: both -inf). No NaN
 *   is written for finite logits. V <= 4096, kprev V <= 8192, 1 <= k <= 8192, P < 64, 0 <= n_blocked <= 1024,
 *   temperature > 0, else -22 (there is no wide form of this step); B == 0 returns 0 without a launch. No allocation,
 *   no host read: capturable in a graph.
 * rq_trie_blocked_nodes: per user the trie nodes of every level 1..D whose leaves are ALL on the user's exclusion
 *   list, in ONE launch (one workgroup per user). items (B, H) int64 corpus indices, entries outside [0, n_items) are
 *   padding; item_leaf (n_items) int32 = each item's leaf (level-D node; items with equal rows share it, so
 *   exclusion is by row); leaf_anc[q - 1] (n_leaves) int32 = each leaf's level-q ancestor, leaf_count[q - 1]
 *   (n_nodes[q - 1]) int32 = each level-q node's number of leaves, q = 1..D (SemanticIdTokenizer.trie_index). The
 *   three level arrays are HOST arrays of D entries copied into the kernel arguments (no device table). out
 *   (D, B, H) int32: out[q - 1][b] = user b's blocked level-q nodes, ascending and distinct, then INT32_MAX. The
 *   ancestors of ascending leaves must be non-decreasing (a level's nodes are in key order). H <= 1024,
 *   D <= RQ_BEAM_MAX_T, else -22; B == 0 or H == 0 returns 0 without a launch.
 * rq_trie_allowed_nodes: the filter tables of an item mask, in TWO launches and no host read. mask (G, n_items) bool:
 *   mask[g][i] != 0 iff group g may be shown corpus item i. item_leaf (n_items) int32 and leaf_anc[q - 1] (n_leaves)
 *   int32, q = 1..D, as rq_trie_blocked_nodes takes them (leaf_anc, n_nodes and out_bits are HOST arrays of D entries
 *   copied into the kernel arguments). out_bits[q - 1]: (G, ceil(n_nodes[q - 1] / 32)) int32, the level-q bitmap of
 *   every group; out_leaf_item (G, n_leaves) int64: the lowest allowed item whose row is that leaf, -1 if it has none
 *   (filtering is by item: a row several items share stays reachable while one of them is allowed, and is reported
 *   under the lowest allowed one). ALL outputs must arrive ZEROED. The reductions are bit OR and index MIN: the result
 *   does not depend on the order, two runs give the same bits. A leaf outside [0, n_leaves) or an ancestor outside
 *   [0, n_nodes) is skipped. D <= RQ_BEAM_MAX_T, else -22; G == 0 or n_leaves == 0 returns 0 without a launch.
 * rq_trie_bias_nodes: the tables of a per-item score bias, in TWO launches and no host read (capturable in a graph).
 *   bias (G, n_items) fp32: bias[g][i] is what group g adds to corpus item i's score; it is read CLEANED: NaN and +inf
 *   as -inf (a bad value can only hide an item; -inf means "never show"), -0.0 as +0.0. item_leaf, leaf_anc, n_nodes
 *   as rq_trie_allowed_nodes takes them (leaf_anc, n_nodes and out_upper are HOST arrays of D entries copied into the
 *   kernel arguments). out_upper[q - 1]: (G, n_nodes[q - 1]) fp32, per group every level-q node's BOUND: the largest
 *   cleaned bias of an item below it, -inf if it has none — no completion of that prefix can gain more, and at the
 *   leaves it is the chosen item's own bias. out_leaf_item (G, n_leaves) int64: the lowest corpus index among the
 *   items on that leaf that attain the leaf's bound, -1 if the bound is -inf (ItemFilter.leaf_item's rule: a row that
 *   several items share is reported under one definite item). ALL outputs must arrive ZEROED; no workspace is needed
 *   (the reduction runs in the outputs: an integer max over the order-preserving image of the float per node, one
 *   64-bit max of (that image << 32 | ~item) per leaf, turned into floats / items in place by the second launch). No
 *   float atomic: the result does not depend on the order, two runs give the same bits. A leaf outside [0, n_leaves)
 *   or an ancestor outside [0, n_nodes) is skipped. n_items < 2^31; D <= RQ_BEAM_MAX_T, else -22; G == 0 or
 *   n_leaves == 0 returns 0 without a launch.
 * rq_beam_expand_biased: rq_beam_expand's step ranked by "log p + a bound on what the items below can still gain"
 *   (per-item score bias: promotions, de-biasing, priors, a second ranker's score), one launch. The arguments are
 *   rq_beam_expand's with out_score (B, k) fp32 after out_lp and, in place of allowed / n_words / G / group,
 *   bias (G, n_bias) fp32 — the level-(P + 1) slice of rq_trie_bias_nodes' out_upper — n_bias, G and group (B) int32:
 *   batch element b reads row group[b]; a group outside [0, G) (-1 is the documented spelling), or group == NULL,
 *   leaves it UNBIASED. blocked / n_blocked are rq_beam_expand's and compose. For child c (token v) of live beam j:
 *   it is a candidate iff rq_beam_expand would score it and, for a biased user, U = clean(bias[g][c]) > -inf (the
 *   cleaning of rq_trie_bias_nodes, applied again on the read: NaN and +inf are -inf); lp_c = rq_beam_expand's score,
 *   the same operations and bits; s_c = lp_c + U, one fp32 add (an unbiased user: s_c = lp_c). The k best by s_c
 *   descending, ties to the lower beam then the lower token: out_ids, out_parent, out_node as rq_beam_expand;
 *   out_score = s_c, the ranking key; out_lp = the winner's UNBIASED lp_c — what the next step takes as parent_lp, so
 *   no bound is ever accumulated: after the last level the bound is the item's own bias and out_score =
 *   log p(item) + bias[g][item]. Dead rows as rq_beam_expand, out_score -inf. With every group outside [0, G) or an
 *   all-zero table the first four outputs are rq_beam_expand's bit for bit and out_score == out_lp. Limits are
 *   rq_beam_expand's and kprev <= 1024 (the beams' softmax statistics stay in LDS for out_lp, three floats per beam);
 *   n_bias != n_children, n_bias or G negative, bias == NULL with G n_bias > 0: -22 before any launch; the kernel
 *   never indexes bias outside [0, n_bias). There is no catalogue bitmap here: write a filter into the bias as -inf.
 * rq_beam_expand_wide_biased: rq_beam_expand_biased in rq_beam_expand_wide's envelope (kprev, k <= 1024, any kprev V),
 *   the same arguments; where both accept a shape all five outputs are bit for bit the same. There is no biased form
 *   of rq_beam_expand_sampled: a draw in proportion to p e^bias needs a log-sum over every subtree, not a maximum.
 * rq_rank_hist: actual (B, D) int64 targets, topk (B, k, D) int64 beams; hist (k + 1) int64 is ACCUMULATED into:
 *   hist[r] += #rows whose first beam equal to the target in all D columns has rank r, hist[k] += #rows without one.
 *   Rows with actual[b][0] < 0 are skipped entirely. D <= 64, k <= 1024. D == 1 serves item ids.
 * rq_score_paths: teacher-forced scoring — one decoding step of log p(candidate | user) for C candidates per user that
 *   the CALLER names, one launch per step, one workgroup per user. logits (B G, V) fp32: G == 1 on step 0 (one BOS row
 *   per user, shared by its candidates), G == C afterwards (row b C + c belongs to candidate c). tokens: this step's
 *   token of every candidate, int64, element (b, c) at tokens[b tok_stride_b + c tok_stride_c] (strides in elements:
 *   a column of a (B, C, D) tensor is passed in place). present (B, C) bool: 0 marks PADDING (NULL: all present).
 *   prev_lp (B, C) fp32: the score so far (NULL on step 0: 0). out_lp[b][c] = lp + prev_lp[b][c] with lp the
 *   log-softmax of the candidate's row / temperature at its token, formed exactly as rq_beam_expand forms it (bitwise
 *   equal for the same row, token and parent score). A present candidate whose token is outside [0, V) — a class the
 *   model cannot generate — gets -inf (and keeps it on later steps); its row is not read. Padding gets -inf; its row
 *   is never read and its token never used. out_rank (B, C) int32 or NULL (give it on the last step): the number of
 *   the user's candidates that come before c in (score descending, index ascending) order, padding last and real
 *   -inf candidates before padding — every user's ranks are a permutation of 0..C-1. 1 <= V <= 4096, 1 <= C <= 1024,
 *   G in {1, C}, temperature > 0, strides >= 0, else -22; B == 0 returns 0 without a launch. */
#define RQ_BEAM_MAX_T 8 /* tokens per beam incl. BOS; sem_id_dim <= 8 as evaluate.metrics already assumes */
int rq_beam_candidates(const float* logits, const float* noise, int64_t R, int64_t V, int64_t n_cand,
                       float temperature, int64_t* cand_ids, float* cand_lp, void* stream);
int rq_beam_select(const int64_t* cand_ids, const float* cand_lp, const bool* valid, const int64_t* keys,
                   int64_t n_keys, int64_t base, int64_t checked, const int64_t* parents, const float* parent_lp,
                   int64_t B, int64_t kprev, int64_t n_cand, int64_t P, int64_t k, int64_t* out_ids, float* out_lp,
                   void* stream);
int rq_beam_select_parent(const int64_t* cand_ids, const float* cand_lp, const bool* valid, const int64_t* keys,
                          int64_t n_keys, int64_t base, int64_t checked, const int64_t* parents,
                          const float* parent_lp, int64_t B, int64_t kprev, int64_t n_cand, int64_t P, int64_t k,
                          int64_t* out_ids, float* out_lp, int32_t* out_parent, void* stream);
int rq_beam_self_attn(const float* q, int64_t sq, const float* const* k_steps, const float* const* v_steps,
                      const int64_t* strides, const int64_t* rows, const int32_t* anc, int64_t R, int64_t t,
                      int64_t H, int64_t hd, float scale, float* out, int64_t so, void* stream);
int rq_beam_expand(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                   int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                   const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k, int64_t* out_ids,
                   float* out_lp, int32_t* out_parent, int32_t* out_node, const int32_t* blocked, int64_t n_blocked,
                   const int32_t* allowed, int64_t n_words, int64_t G, const int32_t* group, void* stream);
int rq_topk_hits(const int64_t* actual, const int64_t* topk, int64_t B, int64_t k, int64_t D, const int* ks,
                 int64_t n_ks, int64_t* counts, void* stream);
int rq_beam_expand_wide(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                        int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                        const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k,
                        int64_t* out_ids, float* out_lp, int32_t* out_parent, int32_t* out_node,
                        const int32_t* blocked, int64_t n_blocked, const int32_t* allowed, int64_t n_words, int64_t G,
                        const int32_t* group, void* stream);
int rq_beam_expand_sampled(const float* logits, const float* noise, float temperature, const int32_t* node,
                           const int32_t* child_off, int64_t n_nodes, const int32_t* tok, int64_t n_children,
                           const int64_t* parents, const float* parent_phi, const float* parent_g, int64_t B,
                           int64_t kprev, int64_t V, int64_t P, int64_t k, int64_t* out_ids, float* out_phi,
                           float* out_g, int32_t* out_parent, int32_t* out_node, const int32_t* blocked,
                           int64_t n_blocked, const int32_t* allowed, int64_t n_words, int64_t G, const int32_t* group,
                           void* stream);
int rq_trie_blocked_nodes(const int64_t* items, int64_t B, int64_t H, const int32_t* item_leaf, int64_t n_items,
                          int64_t n_leaves, const int32_t* const* leaf_anc, const int32_t* const* leaf_count,
                          const int64_t* n_nodes, int64_t D, int32_t* out, void* stream);
int rq_trie_allowed_nodes(const bool* mask, int64_t G, int64_t n_items, const int32_t* item_leaf, int64_t n_leaves,
                          const int32_t* const* leaf_anc, const int64_t* n_nodes, int64_t D, int32_t* const* out_bits,
                          int64_t* out_leaf_item, void* stream);
int rq_trie_bias_nodes(const float* bias, int64_t G, int64_t n_items, const int32_t* item_leaf, int64_t n_leaves,
                       const int32_t* const* leaf_anc, const int64_t* n_nodes, int64_t D, float* const* out_upper,
                       int64_t* out_leaf_item, void* stream);
int rq_beam_expand_biased(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                          int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                          const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k,
                          int64_t* out_ids, float* out_lp, float* out_score, int32_t* out_parent, int32_t* out_node,
                          const int32_t* blocked, int64_t n_blocked, const float* bias, int64_t n_bias, int64_t G,
                          const int32_t* group, void* stream);
int rq_beam_expand_wide_biased(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                               int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                               const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k,
                               int64_t* out_ids, float* out_lp, float* out_score, int32_t* out_parent,
                               int32_t* out_node, const int32_t* blocked, int64_t n_blocked, const float* bias,
                               int64_t n_bias, int64_t G, const int32_t* group, void* stream);
int rq_rank_hist(const int64_t* actual, const int64_t* topk, int64_t B, int64_t k, int64_t D, int64_t* hist,
                 void* stream);
int rq_score_paths(const float* logits, float temperature, const int64_t* tokens, int64_t tok_stride_b,
                   int64_t tok_stride_c, const bool* present, const float* prev_lp, int64_t B, int64_t C, int64_t V,
                   int64_t G, float* out_lp, int32_t* out_rank, void* stream);

/* AdamW step (torch.optim.AdamW as stepped by train_rqvae.py:168-172 / train_decoder.py:203) over
 * every fp32 parameter of a group, one launch per 64 tensors. segs: HOST array of nseg records of 5
 * int64 {p, g, exp_avg, exp_avg_sq (device pointers), n}; it is copied into the kernel arguments, so
 * the call needs no device-side table and is graph-capturable. Per element (rq_adamw_chunk_elems()
 * elements per workgroup):
 *   p -= lr*wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= (lr/bc1) m / (sqrt(v)/bc2_sqrt + eps).
 * bias_correction1 = 1 - b1^step, bias_correction2_sqrt = sqrt(1 - b2^step) (caller-computed). */
int rq_adamw_step(const int64_t* segs, int64_t nseg, float lr, float beta1, float beta2, float eps,
                  float weight_decay, float bias_correction1, float bias_correction2_sqrt, void* stream);
size_t rq_adamw_chunk_elems(void);

/* Codebook usage and dead-code revival (csrc/codebook.hip). EXTENSIONS: the nearest reference counterpart is
 * the `codebook_usage_{l}` log at checkpoint time (train_rqvae.py:232-239); the reference never counts usage
 * during training and has no countermeasure against codebook collapse beyond its one-shot k-means init.
 *
 * rq_code_usage: counts[l][k] += #{b : ids[b][l] == k}. ids (B, L) int64 row-major; counts (L, K) int64,
 *   ACCUMULATED in place (the caller zeroes it). Ids outside [0, K) are skipped. B == 0 is a no-op. Integer
 *   atomics only (exact, order-free): the histogram is privatised in LDS while L K <= 8192 bins (one 64-bit
 *   global add per non-zero bin per workgroup), else global adds aggregated per wave. One launch, no workspace,
 *   no host sync, graph-capturable. L K < 2^31, B L <= 2^40.
 * rq_codebook_revive: re-seat dead codewords on data residuals. codebooks / exp_avg / exp_avg_sq: HOST arrays of
 *   L device pointers to (K, D) fp32, 16-byte aligned (the per-level parameters and their AdamW moments; the two
 *   moment arrays may be NULL together), copied into the kernel arguments. res (L, B, D) fp32 = each level's input
 *   residuals. The rule: for level l the dead codes are {k : counts[l][k] < min_count} in ascending k; the j-th
 *   (0-based) takes donor row r = (s_l + j) mod B, s_l = SplitMix64(seed, l) mod B (unsigned 64-bit; the mix of
 *   rq_rmsnorm_dropout_fwd's generator: counter l under key seed); codebook_l[k][:] becomes a bit copy of
 *   res[l][r][:], row k of both moments +0.0, revived[l][k] = 1 (else 0), n_revived[l] = the number of dead
 *   codes. revived (L, K) uint8 and n_revived (L) int64 are fully written; counts (L, K) int64 is only read.
 *   B >= K is required (-22 otherwise): the donors of a level are then distinct rows and nothing is capped.
 *   1 <= L <= 16, 1 <= K <= 2^20, D % 4 == 0, D <= 1024, min_count >= 0 (0: nothing is dead). Two launches
 *   (dead flags + 256-code chunk totals into the workspace; ranks from the chunk totals, one wave per dead code
 *   copying 16 bytes per lane); workspace >= rq_codebook_revive_workspace(L, K) bytes. */
int rq_code_usage(const int64_t* ids, int64_t B, int64_t L, int64_t K, int64_t* counts, void* stream);
size_t rq_codebook_revive_workspace(int64_t L, int64_t K);
int rq_codebook_revive(float* const* codebooks, float* const* exp_avg, float* const* exp_avg_sq, int64_t L, int64_t K,
                       int64_t D, const int64_t* counts, int64_t min_count, const float* res, int64_t B, uint64_t seed,
                       uint8_t* revived, int64_t* n_revived, void* workspace, size_t ws_bytes, void* stream);

/* EMA-maintained codebooks (csrc/codebook.hip). EXTENSIONS: the update rule of VQ-VAE / Sonnet's
 * VectorQuantizerEMA; the reference trains its codebooks with AdamW on the codebook term of the loss only.
 * The rule, per level l and code k, for residuals res (L, B, D) fp32 and ids (B, L) int64:
 *   n[l][k]   += #{b : ids[b][l] == k}                       exact, int64
 *   s[l][k][:] = s[l][k][:] + sum_{b : ids[b][l] == k} res[l][b][:]   fp32; the batch sum is formed first, in an
 *                order that depends on the shapes only (no float atomics: the same bits on every run), and added once
 *   ids outside [0, K) are skipped. Both are ACCUMULATED (micro-batches and data-parallel shards add up).
 * and, with decay g and smoothing eps, the update from the accumulated n, s:
 *   N'[l][k] = g N[l][k] + (1 - g) n[l][k];   S'[l][k] = g S[l][k] + (1 - g) s[l][k];   T[l] = sum_k N'[l][k]
 *   N~[l][k] = (N'[l][k] + eps) / (T[l] + K eps) * T[l];   codebook_l[k][:] = S'[l][k][:] / N~[l][k]
 * rq_codebook_ema_stats: 1 <= L <= 16, 1 <= K <= 4096, D % 4 == 0, 4 <= D <= 1024, B < 2^31 (-22 otherwise); B == 0
 *   is a no-op. res and s 16-byte aligned. Two launches whatever the form, no allocation, no host sync,
 *   graph-capturable; workspace >= rq_codebook_ema_stats_workspace(B, D, K, L) bytes. Launch 1: workgroups over
 *   (row chunk, level, code tile) sum their rows into an LDS image of the tile's codes — each of 16 waves owns a
 *   range of the codes and adds its matching rows in ascending row order — and write it as a partial; launch 2 adds
 *   the chunks' partials in chunk order into s and n. RQ_EMA_STATS_LDS: a level's K D image is one tile
 *   (K D <= RQ_EMA_STATS_LDS_ELEMS and K <= 2048, which holds for every D >= 8 under that bound);
 *   RQ_EMA_STATS_TILED: the codes are split into tiles of codes_per_tile = min(RQ_EMA_STATS_LDS_ELEMS / D, 2048),
 *   every tile's workgroups re-reading the chunk's ids. A chunk is rows_per_chunk rows (a multiple of 1024), chosen
 *   so that a level has at most 64 chunks and at most 2^22 / (K D) of them (at least one).
 * rq_codebook_ema_stats_plan: host-only; the form a shape takes (RQ_EMA_STATS_NONE for B == 0).
 * rq_codebook_ema_apply: codebooks: HOST array of L device pointers to (K, D) fp32, 16-byte aligned, copied into the
 *   kernel arguments. N (L, K), S (L, K, D) fp32 state, n (L, K) int64 and s (L, K, D) fp32 statistics; writes N, S
 *   and the codebooks, zeroes n and s. decay and 1 - decay are rounded to fp32 once each, from the doubles.
 *   0 <= decay < 1, eps > 0 (-22 otherwise). One launch, one workgroup per level (it rewrites N, which every code's
 *   N~ reads through T); T is summed in a fixed order. */
#define RQ_EMA_STATS_NONE 0
#define RQ_EMA_STATS_LDS 1
#define RQ_EMA_STATS_TILED 2
#define RQ_EMA_STATS_LDS_ELEMS 16384   /* floats of a level's K D image that one workgroup keeps in LDS */
typedef struct rq_codebook_ema_stats_form {
  int form;                /* RQ_EMA_STATS_* */
  int chunks;              /* row chunks per level */
  int tiles;               /* code tiles per level (1: RQ_EMA_STATS_LDS) */
  int codes_per_tile;
  int64_t rows_per_chunk;
  int64_t lds_bytes;       /* launch 1's dynamic LDS */
} rq_codebook_ema_stats_form;
int rq_codebook_ema_stats_plan(int64_t B, int64_t D, int64_t K, int64_t L, rq_codebook_ema_stats_form* form);
size_t rq_codebook_ema_stats_workspace(int64_t B, int64_t D, int64_t K, int64_t L);
int rq_codebook_ema_stats(const float* res, const int64_t* ids, int64_t B, int64_t D, int64_t K, int64_t L, int64_t* n,
                          float* s, void* workspace, size_t ws_bytes, void* stream);
int rq_codebook_ema_apply(float* const* codebooks, int64_t L, int64_t K, int64_t D, float* N, float* S, int64_t* n,
                          float* s, double decay, double eps, void* stream);

/* Beam-searched residual quantization (extension). The reference encodes greedily: its level loop
 * (modules/rqvae.py:114-138) keeps one residual per item and takes one argmin per level. This call generalises
 * that loop to the W best code paths per item, the beam encoder of Faiss's ResidualQuantizer (max_beam_size).
 * Arguments are rq_quantize_fwd's plus W: x (B, D) fp32; codebooks (L, K, D); cb_sqnorm (L, K) from
 * rq_codebook_sqnorm. Outputs: paths (B, W, L) int64; err (B, W); residual (B, W, D) or NULL.
 * The rule: level 0 starts from one beam with residual x. At level l, beam w (residual r_w) and code k have the
 *   key e(w, k) = (|r_w|^2 + |c_k|^2) - 2 r_w.c_k in fp32 (rq_quantize_fwd's distance expression; |r_w|^2 an
 *   fp32 sum over the residual, |c_k|^2 from cb_sqnorm, the dot product's summation order free). The W candidates
 *   with the smallest (e, w, k) in lexicographic order survive, stored in that order (beams are sorted, ties fall
 *   to the lower beam, then the lower code: deterministic). A survivor's residual is r_w - c_k elementwise in
 *   fp32 and its path is its parent's extended by k. err[b][w] is the last level's key, residual the last
 *   level's residual. W = 1 is the greedy rule.
 * Requires D a power of two in [8, 64] (wider rows are refused, not routed elsewhere), 1 <= K <= 4096,
 * 1 <= L <= 16, 1 <= W <= min(K, 32), B <= 2^25; x, codebooks and residual 16-byte aligned. One launch, no
 * allocation, no host sync, graph-capturable, the same bits on every run. workspace: at least
 * rq_quantize_beam_workspace(B, D, K, L, W) bytes; the present kernel keeps paths and candidate lists in LDS and
 * recomputes residuals from the paths, so the size is 0 and workspace may then be NULL. */
size_t rq_quantize_beam_workspace(int64_t B, int64_t D, int64_t K, int64_t L, int64_t W);
int rq_quantize_beam(const float* x, int64_t B, int64_t D, const float* codebooks, const float* cb_sqnorm, int64_t K,
                     int64_t L, int64_t W, int64_t* paths, float* err, float* residual, void* workspace, size_t ws_bytes,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RQVAE_HIP_H_ */
