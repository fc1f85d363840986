// Dispatch planning of the split-bf16 GEMM family (rq_gemm_bf16x3_run / _pair / _group) and of the exact-fp32
// weight gradient (rq_linear_wgrad): which kernel serves a call, its tiling, split-K count, grid, dynamic LDS
// and slab size; which two calls share a launch; which weight gradients share a grouped launch. Host-only C++17
// (no HIP include; the CU count is an argument), so the same code plans on a machine without a GPU, in the
// rq_gemm_bf16x3_*plan entry points and under a host sanitizer (tools/gemm_plan_check.cpp). linear.hip plans
// each call once (x3_call_plan) and launches from the plan; DESIGN.md ("GEMM dispatch") tabulates the rules.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "../../include/rqvae_hip.h"

namespace rqhip {

// ---------------------------------------------------------------------------------------------
// Exact-fp32 weight gradient (wgrad_partial_kernel + wgrad_reduce_kernel)
// ---------------------------------------------------------------------------------------------
constexpr int kWT = 128;    // output tile (o and i)
constexpr int kWBK = 32;    // rows per LDS stage

struct WgradPlan {
  int tiles_i, tiles, S, per;
  int64_t chunk;
  unsigned grid;     // whole XCD rounds of the tiles x S workgroups
  size_t ws_bytes;   // the partials [S][O][I] (+ [S][O])
};

static inline WgradPlan wgrad_plan(int64_t Bn, int64_t O, int64_t I, int cus) {
  WgradPlan p;
  p.tiles_i = (int)((I + kWT - 1) / kWT);
  p.tiles = (int)((O + kWT - 1) / kWT) * p.tiles_i;
  // one full round of resident workgroups (2 per CU, launch bounds): a partial second round would double the time
  int64_t S = 2 * cus / p.tiles;
  const int64_t max_s = (Bn + 4 * kWBK - 1) / (4 * kWBK);   // at least 4 stages per workgroup
  if (S > max_s) S = max_s;
  if (S < 1) S = 1;
  int64_t chunk = (Bn + S - 1) / S;
  chunk = (chunk + kWBK - 1) / kWBK * kWBK;
  if (chunk < kWBK) chunk = kWBK;
  p.chunk = chunk;
  p.S = (int)((Bn + chunk - 1) / chunk);
  if (p.S < 1) p.S = 1;
  p.per = (p.tiles * p.S + 7) / 8;
  p.grid = (unsigned)(p.per * 8);
  p.ws_bytes =(size_t)p.S * (size_t)(O * I + O) * sizeof(float);
  return p;
}

// ---------------------------------------------------------------------------------------------
// Split-bf16 GEMMs: tiles, epilogues, layout codes
// ---------------------------------------------------------------------------------------------
constexpr int kXT = 128;      // output tile (m and n) of the 128-tile kernel
constexpr int kXK = 32;       // k per LDS stage
constexpr int kXWG = 2;       // resident workgroups per CU
constexpr int kXWG64 = 4;     // resident workgroups per CU of the 64-tile form (128-B column-image rows, 32 KiB of LDS)
constexpr int kWT2 = 256;     // output tile (m and n) of the wide kernel
constexpr int kWK = 32;       // its k step
constexpr int kX3GroupMax = 8;   // problems of one grouped launch (gemm_x3w_group_kernel)

// Epilogues: what the accumulator tile becomes (all fp32 math; dropout mask = keep1(seed, m N + n),
// the convention of the standalone dropout kernels, dropout.hip).
enum X3Epi : int {
  kEpiStore = 0,     // C = A B^T (fp32; split-K slabs when S > 1)
  kEpiSiluFwd = 1,   // C = z = A B^T (fp32, kept for the backward); H = split(Dropout(SiLU(z)))
  kEpiSiluBwd = 2,   // H = split(SiLU'(Z) * Dropout(A B^T)): the pre-activation grad of a hidden layer
  kEpiAdd = 3,       // C = A B^T + Z (fp32; the residual add after an attention projection); with dropout
                     // C = Z + Dropout(A B^T) (the block output h + Dropout(MLP(.)))
};

// Layout code of a call's operands: 16 = A k-contiguous, 8 = A split planes, 4 = B k-contiguous, 2 = B split planes.
constexpr int kCodeAK = 16, kCodeAS = 8, kCodeBK = 4, kCodeBS = 2;

// The kernel that runs a call (the value rq_gemm_bf16x3_plan returns), then the roles of the two problems of
// a paired launch (gemm_x3_pair_kernel) — together the rows of the built-form table.
enum X3Kind : int { kX3Tile128 = 0, kX3Wide = 1, kX3Tile64 = 2, kX3PairDgrad = 3, kX3PairWgrad = 4, kX3PairFwd = 5 };

constexpr uint32_t x3_codes(std::initializer_list<int> codes) {
  uint32_t m = 0;
  for (int c : codes) m |= 1u << c;
  return m;
}
// THE table of instantiated forms: kX3Built[kind][kernel epilogue] = the layout codes built. The launchers'
// switch arms (x3_launch, x3_pair_launch in linear.hip) name exactly these; a new instantiation is one more code
// here and one more arm there. Dropout never decides whether a form exists: the plain store draws no mask and
// every other built form has both variants.
//   128- / 64-tile: every layout with fp32 operands (the generic entry point) and the fused MLP chain's (forward
//     of the last layer, data grads with split weights, weight grads) for the plain store; SiLU / residual-add
//     forwards on k-contiguous A x k-contiguous split B; SiLU' data grads on k-contiguous A x n-contiguous split B.
//   wide: both operands split planes; every layout for the plain store, the fused MLP chain's layouts otherwise.
//   pair: a data gradient g W (A fp32 or split k-contiguous, B split n-contiguous; plain, or SiLU' on fp32 A)
//     with a weight gradient g^T x (A, B fp32 or split, m/n-contiguous, plain); or two forward projections
//     (k-contiguous A fp32 / split x k-contiguous split B, plain).
constexpr uint32_t kX3TileStore = x3_codes({20, 16, 4, 0, 30, 22, 26, 18, 10, 8, 2});
constexpr uint32_t kX3Built[6][4] = {
    /* 128-tile   */ {kX3TileStore, x3_codes({22, 30}), x3_codes({18, 26}), x3_codes({22, 30})},
    /* wide       */ {x3_codes({10, 14, 26, 30}), x3_codes({30}), x3_codes({26}), x3_codes({30})},
    /* 64-tile    */ {kX3TileStore, x3_codes({22, 30}), x3_codes({18, 26}), x3_codes({22, 30})},
    /* pair dgrad */ {x3_codes({18, 26}), 0, x3_codes({18}), 0},
    /* pair wgrad */ {x3_codes({0, 2, 8, 10}), 0, 0, 0},
    /* pair fwd   */ {x3_codes({22, 30}), 0, 0, 0}};
static inline bool x3_form_built(int kind, int code, int epi) { return (kX3Built[kind][epi] >> code) & 1u; }

// What planning reads of one call (rq_gemm_desc without its pointers).
struct X3Shape {
  int64_t M, N, K, lda, ldb, ldc;
  int code, epilogue, flags;
  bool drop;   // the call draws a dropout mask (p > 0)
};
static inline X3Shape x3_shape(const rq_gemm_desc& d, bool drop = false) {
  return X3Shape{d.M, d.N, d.K, d.lda, d.ldb, d.ldc,
                 (d.a_kcontig ? kCodeAK : 0) | (d.A_lo ? kCodeAS : 0) | (d.b_kcontig ? kCodeBK : 0) | (d.B_lo ? kCodeBS : 0),
                 d.epilogue, d.flags, drop};
}

// The plan of one call: everything its launch and its slab reduction need.
struct X3Plan {
  int kind, ts;        // kX3Tile128 / kX3Wide / kX3Tile64, and its output tile: 128, 256 or 64
  int tiles_n, tiles, S, per;
  int64_t chunk;
  unsigned grid, block;
  bool slab;           // S > 1: the kernel stores split-K slabs, x3_reduce_kernel applies the epilogue
  size_t slab_bytes;   // S x M x N fp32 (0 unsplit)
  // of the call, not only the shape (x3_call_plan): the operand layout, the epilogue the GEMM kernel itself runs
  // (the plain store into slabs) and whether it draws a dropout mask; the 64-tile form's dynamic LDS (x3s_pad_lds);
  // kfull = whole 32-deep stages: unmasked staging (bitwise the masked path; RQ_GEMM_MASKED keeps the masked one)
  int code, epi_k, kfull;
  bool drop;
  unsigned lds_pad;
};

// ---------------------------------------------------------------------------------------------
// The planner's constants: split-K limits and the time model's measured rates.
// ---------------------------------------------------------------------------------------------
constexpr int kX3MaxSplit = 64;      // split-K: at most this many k chunks
constexpr int kX3MinStages = 2;      // split-K: k-stages per workgroup at least (fewer slabs to reduce)
constexpr int kX3SlabMB = 64;        // split-K: slab bytes (S x M x N fp32) allowed beyond kX3MaxSplit slabs
constexpr int kX3WMinSteps = 8;      // split-K of the wide kernel: k steps per workgroup at least
// Per-CU rates of the time model (x3_plan_time), M fp32-MAC / us:
constexpr double kX3Rate2 = 0.53;    // 128-tile kernel, its two workgroups per CU
constexpr double kX3Rate1 = 0.4;     // 128-tile kernel, a lone workgroup
constexpr double kX3WSpeed = 1.3;    // wide kernel: this multiple of kX3Rate2
constexpr double kX3SRate1 = 0.3;    // 64-tile kernel, one workgroup per CU
constexpr double kX3SRate2 = 0.35;   // 64-tile kernel, kXWG64 workgroups per CU
// Modelled cost (us) of the separate slab-reduction launch of a split-K call: the reduction kernel plus the
// gap it adds between launches in a replayed step (4 us measured best of 4 / 8 / 16 at both decoder
// configs in round 3 with whole rounds, profiles/r03/reduce_us_ab.txt; 3 with the fractional rounds, fitted
// on the round-5 plan sweeps: a back-to-back tiny launch costs ~2.7 us in a replayed graph).
constexpr double kX3ReduceUs = 3.0;
constexpr double kX3SlabBpus = 3.0e6;   // slab bytes per us (written + read back)

// Split-K count cap: kX3MaxSplit slabs, or more while the slabs stay within kX3SlabMB MiB — the
// small weight grads (e.g. 128 x 64 over 65,536 rows: one output tile) need hundreds of k chunks to
// cover the chip, and their slabs are tiny.
static inline int64_t x3_split_cap(int64_t M, int64_t N) {
  const int64_t by_bytes = ((int64_t)kX3SlabMB << 20) / (4 * M * N);
  return by_bytes > kX3MaxSplit ? by_bytes : kX3MaxSplit;
}

// The 64-tile form's compact LDS (32 KiB) lets 4 workgroups share a CU. A launch that fits in 2 per CU
// gets 32 KiB of padding LDS instead (dynamic, unused), so the dispatcher spreads it over every CU rather
// than packing them 4 per CU onto fewer CUs (measured: 1280 x 1536 x 512, 480 workgroups: 14.5 us spread,
// 24.8 us packed; 26,880 x 384 x 1152, 2,520 workgroups: 122.6 -> 109.1 us at 4 per CU).
static inline int x3s_resident(int64_t wgs, int cus) { return wgs > (int64_t)kXWG * cus ? kXWG64 : kXWG; }
static inline unsigned x3s_pad_lds(int64_t wgs, int cus) { return x3s_resident(wgs, cus) == kXWG ? 32768u : 0u; }

// Modelled time (us) of a plan, to choose the split-K factor and between the two kernels:
//  * MMA: rounds of resident workgroups (fractional: a partly filled last round costs its share — fitted
//    on measured plan sweeps, tools/plan_model_fit.py over profiles/r05/plan_sweep/; the whole-round count
//    it replaced mispriced the 64-tile form at 4 per CU, e.g. C4's 4,608 x 1,024 x 384 SiLU launches) x the
//    MACs a CU does per round, at the measured per-CU rates (128-tile kernel ~0.53 M fp32-MAC/us per
//    CU with its two workgroups, ~0.4 for a lone workgroup; wide kernel 1.3x) — the wide kernel's
//    256 x 256 tiles quantise into 4x coarser rounds (decoder context rows: a 1,536-wide projection is
//    270 wide tiles, two rounds, the second nearly empty);
//  * split-K: the slabs written by the GEMM and read back by the reduction, 2 S M N fp32 at ~3 TB/s (the
//    rate the batched deferred reductions reach), plus the reduce launch (kX3ReduceUs). Round 4 priced (S + 1) M N at
//    5 TB/s, which chose 256 x 256-tile plans with S = 21..30 for the decoder's 11k-row weight gradients:
//    ~64 MB of slabs per weight, 444 MB (C4) / 800 MB (Amazon) a step. Same-process A/B on MI355X: C4
//    2.766 -> 2.678 ms, Amazon 5.415 -> 5.355, RQ-VAE 1.957 -> 1.924 (half the rate, 1.5 TB/s, loses).
// Checked against tools/gemm_ab.py on MI355X (RQ-VAE and decoder shapes, both kernels forced).
static inline double x3_plan_time(const X3Plan& p, int cus) {
  const int64_t wgs = (int64_t)p.tiles * p.S;
  const bool wide = p.kind == kX3Wide, small = p.kind == kX3Tile64;
  const double tile = (double)p.ts * p.ts;
  const double rate = small ? kX3SRate2 : kX3Rate2 * (wide ? kX3WSpeed : 1.0);   // M MAC / us per CU
  double t;
  if (wgs <= cus) {   // at most one workgroup per CU
    t = tile * (double)p.chunk / ((wide ? rate : (small ? kX3SRate1 : kX3Rate1)) * 1e6);
  } else {
    const int per_cu = wide ? 1 : (small ? x3s_resident(wgs, cus) : kXWG);
    const int64_t slots = (int64_t)cus * per_cu;
    // a partly filled last round costs its share; one round at least
    const double rounds = wgs > slots ? (double)wgs / (double)slots : 1.0;
    t = rounds * per_cu * tile * (double)p.chunk / (rate * 1e6);
  }
  if (p.slab) t += 2.0 * (double)p.slab_bytes / kX3SlabBpus + kX3ReduceUs;
  return t;
}

// The plan of tile `ts` (128, 64, or kWT2: the wide kernel) at S k chunks (fewer when whole stages cover K sooner).
static inline X3Plan x3_plan_s(int64_t M, int64_t N, int64_t K, int64_t S, int ts = kXT) {
  X3Plan p{};
  const bool wide = ts == kWT2;
  const int KS = wide ? kWK : kXK;
  p.kind = wide ? kX3Wide : (ts == 64 ? kX3Tile64 : kX3Tile128);
  p.ts = ts;
  p.tiles_n = (int)((N + ts - 1) / ts);
  p.tiles = (int)((M + ts - 1) / ts) * p.tiles_n;
  int64_t chunk = (K + S - 1) / S;
  chunk = (chunk + KS - 1) / KS * KS;
  p.chunk = chunk;
  p.S = (int)((K + chunk - 1) / chunk);
  if (p.S < 1) p.S = 1;
  p.per = wide ? 0 : (p.tiles * p.S + 7) / 8;
  p.grid = wide ? (unsigned)(p.tiles * p.S) : (unsigned)(p.per * 8);   // 128- / 64-tile: whole XCD rounds
  p.block = wide ? 512 : 256;
  p.slab = p.S > 1;
  p.slab_bytes = p.slab ? (size_t)p.S * (size_t)(M * N) * sizeof(float) : 0;
  return p;
}

// Best split-K plan of one tile size: split K when the output tiles cannot fill the chip (weight
// gradients, the decoder's future rows) and the model says the slabs pay for themselves.
static inline X3Plan x3_plan_t(int64_t M, int64_t N, int64_t K, bool allow_split, int ts, int cus) {
  X3Plan p = x3_plan_s(M, N, K, 1, ts);
  const int64_t slots_t = (int64_t)cus * kXWG;   // split-K fills the 2-per-CU slots
  if (allow_split && p.tiles < slots_t / 2 && (M * N) % 4 == 0) {   // slab reduction reads float4
    int64_t S = slots_t / p.tiles;
    const int64_t max_s = (K + kX3MinStages * kXK - 1) / (kX3MinStages * kXK);   // min stages per workgroup
    if (S > max_s) S = max_s;
    if (S > x3_split_cap(M, N)) S = x3_split_cap(M, N);   // slab traffic of the reduction grows with S
    if (ts == 64) {   // small tiles: the best of S = 2, 4, ... up to the one-round heuristic
      for (int64_t s2 = 2; s2 < S; s2 *= 2) {
        const X3Plan q = x3_plan_s(M, N, K, s2, ts);
        if (x3_plan_time(q, cus) < x3_plan_time(p, cus)) p = q;
      }
    }
    if (S > 1) {
      const X3Plan q = x3_plan_s(M, N, K, S, ts);
      if (x3_plan_time(q, cus) < x3_plan_time(p, cus)) p = q;
    }
  }
  return p;
}

// 128-tile kernel, or its 64-tile form where the time model prefers it (the 128-tiles of a
// 1,280-row operand are 40 workgroups: split-K slabs and their reduction cost more than the GEMM).
// flags (the call's rq_gemm_desc.flags): RQ_GEMM_ONLY_128 / RQ_GEMM_ONLY_64 pin one tile size.
static inline X3Plan x3_plan(int64_t M, int64_t N, int64_t K, int flags, int epilogue, int cus) {
  // One row of 64-tiles (the C4 decoder's 40 future-token rows) over K <= 384 with a plain or residual
  // epilogue: unsplit. Measured per call (profiles/r05/plan_sweep2/sweep_c4.jsonl, hipGraph of 10 calls with
  // their reductions): 6.7-7.2 us unsplit vs 7.1-7.3 at the model's S = 6 plus a reduction launch per call
  // — the model underprices the short-K workgroups' fixed latency; the SiLU epilogues keep the model's split.
  const bool allow_split = !(!(flags & (RQ_GEMM_ONLY_128 | RQ_GEMM_ONLY_64)) && M <= 64 && K <= 384 &&
                             (epilogue == kEpiStore || epilogue == kEpiAdd));
  const X3Plan p = x3_plan_t(M, N, K, allow_split, kXT, cus);
  if (flags & RQ_GEMM_ONLY_128) return p;
  const X3Plan q = x3_plan_t(M, N, K, allow_split, 64, cus);
  if (flags & RQ_GEMM_ONLY_64) return q;
  // K <= 128 (at most four 32-deep stages): the 64-tile form, whose 4 resident workgroups per CU hide the
  // per-workgroup prologue / epilogue latency that such short k loops cannot — measured faster than the
  // 128-tile kernel for every short-K call of the three bench steps (plan_sweep2: RQ-VAE 65,536 x 128 x 64
  // SiLU' epilogue 27.6 -> 20.6 us, SiLU 23.4 -> 22.0; Amazon 11,520 x 512 x 128 14.6 -> 13.8)
  if (K <= 128) return q;
  return x3_plan_time(q, cus) < x3_plan_time(p, cus) ? q : p;
}

// Plan of the wide kernel, or false when the 128-tile kernel serves the shape better: k steps
// must be whole (K % 32), padding of a partial 256-row tile must stay small (R % 256 == 0 or
// R >= 2048), and the launch must cover at least a quarter of the CUs (split-K when allowed).
static inline bool x3w_plan(int64_t M, int64_t N, int64_t K, int cus, X3Plan* p) {
  if (K % kWK != 0 || K <= 0) return false;
  auto fits = [](int64_t R) { return R % kWT2 == 0 || R >= 2048; };
  if (!fits(M) || !fits(N)) return false;
  *p = x3_plan_s(M, N, K, 1, kWT2);
  if (p->tiles < cus / 2 && (M * N) % 4 == 0) {
    int64_t S = cus / p->tiles;
    const int64_t max_s = K / (kWK * kX3WMinSteps);
    if (S > max_s) S = max_s;
    if (S > x3_split_cap(M, N)) S = x3_split_cap(M, N);
    if (S > 1) {
      const X3Plan q = x3_plan_s(M, N, K, S, kWT2);
      if (x3_plan_time(q, cus) < x3_plan_time(*p, cus)) *p = q;
    }
  }
  return (int64_t)p->tiles * p->S >= cus / 4;
}

// Elements one wide workgroup's operand DMA spans from its descriptor base (32-bit byte offsets):
// 256 rows of a k-contiguous operand (+ K), or one k chunk of rows of an m/n-contiguous one (+ its rows).
static inline int64_t x3w_span(int64_t R, int64_t K, int64_t ld, bool kc, int64_t chunk) {
  return kc ? (int64_t)kWT2 * ld + K : (chunk + kWK) * ld + R;
}
// Both operands of a wide problem within the DMA's 32-bit byte offsets (the span at the largest chunk, K:
// a split only shortens it).
static inline bool x3w_spans_ok(const X3Shape& s) {
  return x3w_span(s.M, s.K, s.lda, s.code & kCodeAK, s.K) < (1ll << 30) &&
         x3w_span(s.N, s.K, s.ldb, s.code & kCodeBK, s.K) < (1ll << 30);
}
// The wide kernel (and the group kernel, which runs its body) can run the call as it stands: the form is
// built for the call's epilogue (both operands split planes) and the operands are within the DMA's reach.
static inline bool x3w_can_run(const X3Shape& s) { return x3_form_built(kX3Wide, s.code, s.epilogue) && x3w_spans_ok(s); }

// The wide kernel runs when it can run the call (x3w_can_run), the shape plans (x3w_plan) and the time model
// prefers it — or wherever it can run under RQ_GEMM_FORCE_WIDE; never under RQ_GEMM_NO_WIDE / RQ_GEMM_ONLY_128 /
// RQ_GEMM_ONLY_64.
static inline bool x3w_choose(const X3Shape& s, int cus, X3Plan* p) {
  if (s.flags & (RQ_GEMM_NO_WIDE | RQ_GEMM_ONLY_128 | RQ_GEMM_ONLY_64)) return false;
  if (!(x3w_can_run(s) && x3w_plan(s.M, s.N, s.K, cus, p))) return false;
  // priced against the 128-/64-tile plan this call would really get (same epilogue: the skinny-unsplit rule
  // applies to the store / add epilogues only)
  return (s.flags & RQ_GEMM_FORCE_WIDE) ||
         x3_plan_time(*p, cus) < x3_plan_time(x3_plan(s.M, s.N, s.K, s.flags, s.epilogue, cus), cus);
}

// The plan of one call (K > 0): the kernel the policy and the model pick, RQ_GEMM_SPLIT(S) forcing the split-K
// count on that kernel (a tuned plan), and the launch facts that follow. Plans forms that are not built, too:
// the launcher refuses those (x3_form_built), planning reports what the model would pick.
static inline X3Plan x3_call_plan(const X3Shape& s, int cus) {
  X3Plan pl = x3_plan(s.M, s.N, s.K, s.flags, s.epilogue, cus), pw;
  if (x3w_choose(s, cus, &pw)) pl = pw;
  const int forced_s = (s.flags >> RQ_GEMM_SPLIT_SHIFT) & RQ_GEMM_SPLIT_MASK;
  if (forced_s > 0) pl = x3_plan_s(s.M, s.N, s.K, forced_s, pl.ts);
  // slab path: split-K partials go to the workspace with the plain store, and x3_reduce_kernel applies
  // the real epilogue (and the accumulation); an unsplit accumulating call adds in the GEMM's epilogue
  pl.code = s.code;
  pl.epi_k = pl.slab ? (int)kEpiStore : s.epilogue;
  pl.drop = s.drop && pl.epi_k != kEpiStore;
  pl.lds_pad = pl.kind == kX3Tile64 ? x3s_pad_lds((int64_t)pl.tiles * pl.S, cus) : 0u;
  pl.kfull = !(s.flags & RQ_GEMM_MASKED) && s.K % kXK == 0 && pl.chunk % kXK == 0;
  return pl;
}

// Slab bytes of a shape: split-K slabs of whichever kernel may run for it (the largest of the 128-tile,
// 64-tile and wide plans, so one workspace serves every rq_gemm_desc.flags policy). An unsplit accumulating
// call adds in the GEMM's own epilogue: no slab.
static inline size_t x3_workspace_bytes(int64_t M, int64_t N, int64_t K, int cus) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  X3Plan pw;
  size_t b = std::max(x3_plan_t(M, N, K, true, kXT, cus).slab_bytes, x3_plan_t(M, N, K, true, 64, cus).slab_bytes);
  if (x3w_plan(M, N, K, cus, &pw)) b = std::max(b, pw.slab_bytes);
  return b;
}

// ---------------------------------------------------------------------------------------------
// Paired launches (gemm_x3_pair_kernel): two problems' workgroups in one grid.
// ---------------------------------------------------------------------------------------------
struct X3PairPlan {
  int kind;   // 0: two launches; kX3PairDgrad: (data gradient, weight gradient); kX3PairFwd: two forward projections
  unsigned grid, n1, lds_pad;   // n1: the first problem's workgroups
};

// The two problems can share a launch: both on the 128- / 64-tile kernel with one tile size, an instantiated
// form pair, and at least one of them leaving resident slots idle alone (the decoder's 40..11,332-row
// launches; two launches that each fill the chip already — the RQ-VAE's 65,536-row 64-tile layers — gain
// nothing and measured 4 us slower paired).
// The forward pair: two projections of different inputs (the decoder block's self-attention qkv of attn_norm(x)
// and cross-attention q of cross_attn_norm(x)).
static inline X3PairPlan x3_pair_plan(const X3Plan& p1, const X3Plan& p2, int cus) {
  X3PairPlan pp{};
  if (p1.kind == kX3Wide || p2.kind == kX3Wide || p1.ts != p2.ts) return pp;
  const bool fwd = x3_form_built(kX3PairFwd, p1.code, p1.epi_k) && x3_form_built(kX3PairFwd, p2.code, p2.epi_k);
  if (!fwd && !(x3_form_built(kX3PairDgrad, p1.code, p1.epi_k) && x3_form_built(kX3PairWgrad, p2.code, p2.epi_k)))
    return pp;
  const int64_t w1 = (int64_t)p1.tiles * p1.S, w2 = (int64_t)p2.tiles * p2.S;
  const bool t64 = p1.kind == kX3Tile64;
  const int64_t slots = (int64_t)(t64 ? x3s_resident(w1 + w2, cus) : kXWG) * cus;
  if (w1 >= slots && w2 >= slots) return pp;
  pp.kind = fwd ? kX3PairFwd : kX3PairDgrad;
  pp.n1 = p1.grid;
  pp.grid = p1.grid + p2.grid;
  pp.lds_pad = t64 ? x3s_pad_lds(w1 + w2, cus) : 0u;
  return pp;
}

// The weight gradient's split count chosen for the PAIR (the caller adopts it as RQ_GEMM_SPLIT; 0: keep its own
// plan): where the data gradient alone leaves resident slots idle (128-tile kernel, unsplit), the weight
// gradient's k chunks are sized like the data gradient's K (S = ceil(rows / K_d)) when that is fewer slabs than
// its own plan and the pair still spans more than one round of workgroups — equal-length workgroups instead of a
// tail of short ones, and fewer slabs (measured on the paired launches of the decoder's 11k-row qkv / MLP-up
// layers: 152 -> 127 and 93 -> 85 us, tools/pair_split_probe.py).
static inline int x3_pair_resplit(const X3Plan& pd, const X3Plan& pw, int64_t Kd, int64_t Kw, int cus) {
  if (pd.kind != kX3Tile128 || pw.kind != kX3Tile128 || pd.S != 1 || pw.S <= 1) return 0;
  const int64_t slots = (int64_t)kXWG * cus, s_bal = (Kw + Kd - 1) / Kd;
  return pd.tiles < slots && 1 < s_bal && s_bal < pw.S && pd.tiles + pw.tiles * s_bal > slots ? (int)s_bal : 0;
}

// ---------------------------------------------------------------------------------------------
// Grouped weight gradients (gemm_x3w_group_kernel): the dW = g^T x problems of one MLP chain share the batch
// as K and nothing in the backward waits for them, so they can share one launch in which each member takes
// its proportional share of the chip on the wide tile, instead of each filling 256 CUs alone (the big layer
// in many short chunks, the small ones on the 128- / 64-tile kernels at 2-4x the LDS fill per MFMA).
// The plan: one step budget T (k steps of 32 per workgroup) for every member, S_p = ceil(K / 32 T) chunks
// each, the whole group in one round of workgroups.
// ---------------------------------------------------------------------------------------------
// k steps per grouped workgroup at least: the wide loop's prologue and epilogue cost about 20 steps' worth
// (profiles/r06/gemm_diag/wgrad_policy.jsonl: 512 x 256 x 65,536 at S = 128, 16 steps per workgroup, 65.9 us
// against 62.4 us on the 128-tile kernel; at 49 steps the wide tile wins), so a budget under 32 steps is
// mostly ramp. Never below the wide kernel's own kX3WMinSteps.
constexpr int kX3GMinSteps = 32;
static_assert(kX3GMinSteps >= kX3WMinSteps, "the group's step budget respects the wide kernel's minimum");
// Rows (K) from which the model may group. Measured at the RQ-VAE's 65,536 rows only (profiles/r07/group_wgrad);
// the decoder's 40..11,332-row chains pair each weight gradient with its data gradient (gemm_x3_pair_kernel),
// which a grouped member gives up and the model does not price: they stay ungrouped until measured.
constexpr int64_t kX3GMinK = 32768;

struct X3GroupPlan {
  int n;                       // members sharing the launch (0: no group)
  bool in[kX3GroupMax];
  X3Plan pl[kX3GroupMax];      // a member's wide plan (tiles, S, chunk, slab bytes)
};

// A problem the group kernel can run: split m/n-contiguous operands, plain store to a dense output, whole k
// steps, no kernel policy of its own, and the wide kernel's operand conditions (dims % 8; x3w_can_run).
static inline bool x3_group_member(const X3Shape& s) {
  return s.K > 0 && s.code == (kCodeAS | kCodeBS) && s.epilogue == kEpiStore && (s.flags & 0xFFFF) == 0 &&
         s.K % kWK == 0 && s.M % 8 == 0 && s.N % 8 == 0 && s.ldc == s.N && x3w_can_run(s);
}

// Modelled time (us) of the members `in` at step budget T, with x3_plan_time's constants: one round of wide
// workgroups of at most T steps each, every member's slabs written and read back, one reduction launch.
// < 0: the group does not fit one round.
static inline double x3_group_time(const X3Shape* s, int count, const bool* in, int64_t T, int cus, X3Plan* pl) {
  int64_t wgs = 0, steps = 0;
  double slab = 0;
  for (int i = 0; i < count; ++i) {
    if (!in[i]) continue;
    const int64_t nk = s[i].K / kWK;
    pl[i] = x3_plan_s(s[i].M, s[i].N, s[i].K, (nk + T - 1) / T, kWT2);
    wgs += pl[i].grid;
    steps = std::max(steps, pl[i].chunk / kWK);
    slab += (double)(2 * pl[i].S) * (double)(s[i].M * s[i].N) * 4.0;
  }
  if (wgs > cus) return -1.0;
  return (double)kWT2 * kWT2 * kWK * (double)steps / (kX3Rate2 * kX3WSpeed * 1e6) + slab / kX3SlabBpus + kX3ReduceUs;
}

// Best budget for the members `in`: the modelled saving (us) against their separate plans `own`, <= 0 when
// grouping them does not pay or cannot run in one round.
static inline double x3_group_gain(const X3Shape* s, const X3Plan* own, int count, const bool* in, int cus,
                                   X3Plan* best) {
  int n = 0;
  int64_t K = -1;
  double apart = 0;
  for (int i = 0; i < count; ++i) {
    if (!in[i]) continue;
    if (K >= 0 && s[i].K != K) return 0;
    K = s[i].K;
    apart += x3_plan_time(own[i], cus);
    ++n;
  }
  if (n < 2 || K < kX3GMinK) return 0;
  double tbest = -1;
  X3Plan pl[kX3GroupMax] = {};
  for (int64_t T = kX3GMinSteps; T <= K / kWK; ++T) {
    const double t = x3_group_time(s, count, in, T, cus, pl);
    if (t >= 0 && (tbest < 0 || t < tbest)) {
      tbest = t;
      for (int i = 0; i < count; ++i)
        if (in[i]) best[i] = pl[i];
    }
  }
  return tbest < 0 ? 0 : apart - tbest;
}

// Which of the problems share one grouped launch. Members that carry an explicit split count (RQ_GEMM_SPLIT)
// are grouped as told: the only way rq_gemm_bf16x3_group itself groups (model = false). The model's common
// step budget gives the members other split counts than their separate plans, which changes the fp32
// summation order of their results (RQ-VAE step: 5.7 % faster, loss after 25 steps 1.1e-4 off the ungrouped
// run's, profiles/r07/group_wgrad), so taking its plan is the caller's decision: rq_gemm_bf16x3_group_plan
// reports it (model = true) and the caller passes the counts back as explicit ones. The model drops one
// member at a time while that raises the modelled saving (a mostly empty tile, 128 x 64, costs the group a
// whole tile's steps and stays in its own launch), and groups only when the rest beats its separate plans.
static inline X3GroupPlan x3_group_plan(const X3Shape* s, const X3Plan* own, int count, bool model, int cus) {
  X3GroupPlan g{};
  if (count < 2 || count > kX3GroupMax) return g;
  bool el[kX3GroupMax] = {}, forced = false;
  auto forced_s = [&](int i) { return (s[i].flags >> RQ_GEMM_SPLIT_SHIFT) & RQ_GEMM_SPLIT_MASK; };
  for (int i = 0; i < count; ++i) {
    if (s[i].flags & RQ_GEMM_NO_GROUP) return g;
    el[i] = x3_group_member(s[i]);
    forced = forced || forced_s(i) > 0;
  }
  if (forced) {
    for (int i = 0; i < count; ++i) {
      if (!el[i] || forced_s(i) < 2) continue;
      const X3Plan p = x3_plan_s(s[i].M, s[i].N, s[i].K, forced_s(i), kWT2);
      if (p.S < 2) continue;
      g.in[i] = true;
      g.pl[i] = p;
      ++g.n;
    }
  } else if (model) {
    double gain = x3_group_gain(s, own, count, el, cus, g.pl);
    for (;;) {
      int drop = -1;
      X3Plan pl[kX3GroupMax] = {};
      for (int j = 0; j < count; ++j) {
        if (!el[j]) continue;
        el[j] = false;
        const double gj = x3_group_gain(s, own, count, el, cus, pl);
        el[j] = true;
        if (gj > gain) {
          gain = gj;
          drop = j;
        }
      }
      if (drop < 0) break;
      el[drop] = false;
      gain = x3_group_gain(s, own, count, el, cus, g.pl);
    }
    if (gain > 0)
      for (int i = 0; i < count; ++i) {
        g.in[i] = el[i] && g.pl[i].S >= 2;
        g.n += g.in[i];
      }
    if (g.n != (int)std::count(el, el + count, true)) g.n = 0;   // an unsplit member: the plan does not hold
  }
  if (g.n < 2) {
    g.n = 0;
    for (int i = 0; i < count; ++i) g.in[i] = false;
  }
  return g;
}

}  // namespace rqhip
