// Dispatch planning of varlen_attn_fwd / varlen_attn_bwd: which kernel families serve a call, with which
// template arguments, grids and workspace layout. Host-only C++17 (no HIP include; the CU count is an
// argument), so the same code plans on a machine without a GPU, in varlen_attn_plan and under a host
// sanitizer (tools/attn_plan_check.cpp). attention.hip computes one plan per call and launches from it;
// DESIGN.md ("Attention dispatch") tabulates the rules below.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "../../include/rqvae_hip.h"

namespace rqhip {

constexpr int kAttnOrderMax = 4096;   // sequences attn_order_kernel ranks (attention.hip's kOrderMax)

constexpr int kShortMaxStaged = 32;   // longest staged range served by the short forms (A/B: 32 / 128); the
                                      // launcher instantiates the short kernels for CH == 32 only: raising
                                      // this needs the CH 64 / 96 / 128 arms back (attn_run_* in attention.hip)
constexpr int kShortMax = 128;   // longest staged range of the short forms

// waves of a short-form launch whose tiles run over `rows` (queries for fwd / dQ, keys for dK/dV) against
// a staged range of `staged` rows (always one 32-row chunk); 0 when the chunked kernels serve it
static inline int short_plan(int64_t rows, int64_t staged) {
  if (rows > kShortMax || staged > kShortMax) return 0;
  // Measured on MI355X (decoder Amazon step, rocprofv3): the short forms win where the staged range
  // is one 32-row chunk (decoder self-attention 5 x 5: fwd 11.6 -> 6.4 us, dQ 15.6 -> 8.9 us; the
  // cross-attention dK/dV over 5 staged queries 41 -> 24 us) and lose at 96 staged rows (encoder
  // self-attention, n <= 81: fwd 35 -> 39 us, dQ 54 -> 59 us, dK/dV 41 -> 64 us: 52 KB of LDS per
  // workgroup leaves 3 workgroups per CU, and a one-wave workgroup would hold it alone), so longer
  // staged ranges keep the chunked kernels.
  if (staged > kShortMaxStaged) return 0;
  return rows <= 16 ? 1 : 4;
}

// Waves per workgroup by the longest row count: 16 rows per wave; short sequences (the Amazon
// decoder's contexts <= 81 tokens, its 5-6 future tokens) use narrow workgroups so few waves idle
// on padding, long ones (ML-32M <= 801, C5 <= 1281) share each staged 64-row chunk between 4 waves.
static inline int waves_for(int64_t rows) { return rows <= 16 ? 1 : (rows <= 96 ? 2 : 4); }

// LPT order where a workgroup's run time varies enough with the sequence to leave a straggler tail
static inline bool lpt_plan(int64_t B, int64_t max_len) { return B >= 2 && B <= kAttnOrderMax && max_len > 128; }

// split-key forward: one query tile per sequence (<= 16 queries), non-causal, long key ranges (cross-attention)
constexpr int kSplitMinK = 129;   // key ranges from here use the split-key forward (A/B: at the Amazon
                                  // contexts, <= 81 keys in 32-key blocks, it ties the chunked form)
// The kernel policy of one call, from its `flags` argument (RQ_ATTN_* in include/rqvae_hip.h; 0 = the
// measured-best forms): LDS-DMA short forms, one-pass backwards, split-key / key-split forwards, and the
// fused backward's query splits (0 = automatic).
struct AttnPolicy {
  bool dma, fused, split;
  int qsplit;
  bool x3;   // RQ_ATTN_SPLIT_BF16: the long-range forwards multiply in split-bf16 (matmul precision 'high')
  bool lpt_short;   // RQ_ATTN_LPT_SHORT: longest-first sequence order for the short / few-query forms too
  bool order_given;   // RQ_ATTN_ORDER_GIVEN: ws[0, B) already holds the LPT order of cu_k (no order launch)
  bool fewq_stream;   // !RQ_ATTN_FEWQ_WG: the 4-wave few-query backward as the persistent LDS-DMA-staged walk
};
static inline AttnPolicy attn_policy(int flags) {
  return AttnPolicy{!(flags & RQ_ATTN_NO_DMA), !(flags & RQ_ATTN_TWO_PASS), !(flags & RQ_ATTN_NO_SPLIT),
                    (flags >> RQ_ATTN_QSPLIT_SHIFT) & 15, (flags & RQ_ATTN_SPLIT_BF16) != 0,
                    (flags & RQ_ATTN_LPT_SHORT) != 0, (flags & RQ_ATTN_ORDER_GIVEN) != 0,
                    !(flags & RQ_ATTN_FEWQ_WG)};
}

static inline int split_kb(int64_t max_k) { return max_k <= 128 ? 32 : 128; }   // 32: for a kSplitMinK <= 128
// key-split forward for many queries over long keys at low occupancy (attn_fwd_kvsplit_kernel): the C4
// per-rank config (8 sequences x 6 heads x <= 13 query blocks); RQ_ATTN_NO_SPLIT disables it (A/B)
constexpr int kKvSplitMaxWg = 1024;   // unsplit workgroups (B x H x 64-query blocks) up to which it applies
constexpr int kKvSplitKB = 128;

// staged rows of the LDS-DMA short forms (attn_fwd_dma_kernel and its backward passes)
static inline int dma_rows_for(int64_t n) { return n <= 32 ? 32 : (n <= 64 ? 64 : (n <= 96 ? 96 : 128)); }
static inline int fewq_waves(int64_t max_k) { return max_k <= 16 ? 1 : (max_k <= 32 ? 2 : 4); }

// Fused backward (one launch for dQ, dK, dV: attn_bwd_fused_kernel) where the two-pass form would use the
// chunked dK/dV kernel; the short forms keep the decoder's 5-token self- and cross-attention.
constexpr int kFusedNW = 4;           // waves per workgroup = key block / 16
constexpr int kFusedCH = 32;          // staged query rows per LDS round trip (A/B on MI355X: 32 beats 64 by 4-5 %)
constexpr int kFusedMinK = 129;       // shorter key ranges keep the two-pass form (Amazon n <= 81: 0.25 vs 0.30 ms)
constexpr int kFusedMinKFewq = 129;   // the same threshold for <= 16 queries per sequence (cross-attention;
                                      // A/B from 33 keys: Amazon decoder step 6.53 -> 6.60 ms, fewq_ab.txt)
constexpr int kFusedKB = 16 * kFusedNW;

// Query splits of the fused backward: when (sequences x heads x key blocks) workgroups cannot fill the
// chip twice over (ML-32M at 8 sequences per GPU: ~300 workgroups, each walking up to 801 queries), each
// key block's query range is split over up to 4 workgroups (whole 32-query chunks, >= 2 per split);
// their dK / dV partials are summed by attn_kv_reduce_kernel. A call's RQ_ATTN_QSPLIT(n) forces n (1 = off).
static inline int fused_qsplit(int64_t B, int64_t H, int64_t max_q, int64_t max_k, const AttnPolicy& pol, int cus) {
  const int forced = pol.qsplit;
  if (max_q <= 16) return 1;
  const int64_t max_by_len = std::max<int64_t>(1, max_q / (2 * kFusedCH));
  if (forced > 0) return (int)std::min<int64_t>(std::min(forced, 8), max_by_len);
  const int64_t wgs = B * H * ((max_k + kFusedKB - 1) / kFusedKB);
  const int64_t want = (6 * (int64_t)cus + wgs - 1) / std::max<int64_t>(1, wgs);   // ~2 rounds of 3 per CU
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, 4), max_by_len));
}

// The shape of one call and the scratch it brings (ws_elems < 0: none, the entry points' ws == NULL)
struct AttnShape {
  int64_t B, H, hd, max_q, max_k, Tq, Tk;
  int causal, flags;
  int64_t ws_elems;
};

static inline int64_t attn_pad4(int64_t n) { return (n + 3) & ~(int64_t)3; }   // B ints of order in 16-B padded float slots

static inline void attn_push(rq_attn_plan* p, int family, int hd, int nw, int r, int x3, int64_t gx, int64_t gy,
                             int64_t gz, int block) {
  rq_attn_launch& l = p->launch[p->n_launches++];
  l = rq_attn_launch{family, hd, nw, r, x3, block, {(unsigned)gx, (unsigned)gy, (unsigned)gz}};
}
// the order launch (unless the caller's workspace already holds it) and the plan's record of its source
static inline void attn_push_order(rq_attn_plan* p, int src, bool given, int64_t off) {
  p->order_off = off;
  p->order_src = given ? RQ_ATTN_ORDER_SRC_GIVEN : src;
  if (!given) attn_push(p, RQ_ATTN_K_ORDER, 0, 0, 0, 0, 1, 1, 1, 1024);
}
static inline rq_attn_plan attn_plan_empty() {
  rq_attn_plan p = {};
  p.qsplit = 1;
  p.order_off = p.part_off = p.kvpart_off = -1;
  return p;
}

// Forward. Workspace: [order: pad4(B)] [split-key / key-split partials: nsplit x Tq x H x (hd + 2)].
// Without a workspace: natural sequence order, no split-key / key-split form.
static inline rq_attn_plan attn_plan_fwd(const AttnShape& s) {
  const AttnPolicy pol = attn_policy(s.flags);
  const int64_t B = s.B, H = s.H, max_q = s.max_q, max_k = s.max_k;
  const bool hd64 = s.hd == 64, have_ws = s.ws_elems >= 0;
  rq_attn_plan p = attn_plan_empty();
  // key-split: many queries over long keys at low occupancy; split-key: one query tile over long keys
  const bool kvsplit = pol.split && hd64 && !s.causal && max_q > 16 && max_k > 2 * kKvSplitKB &&
                       B * H * ((max_q + 63) / 64) <= kKvSplitMaxWg;
  const bool split = pol.split && hd64 && !s.causal && max_q <= 16 && max_k >= kSplitMinK;
  const int kb = kvsplit ? kKvSplitKB : split_kb(max_k);
  const int64_t nsplit = (max_k + kb - 1) / kb;
  const int64_t ob = attn_pad4(B), sp = (kvsplit || split) ? nsplit * s.Tq * H * (s.hd + 2) : 0;
  p.ws_total = p.ws_need = ob + sp;
  if (have_ws && sp > 0) p.part_off = ob;
  if (B == 0) return p;
  const int64_t tail = B + 1;   // + the grid slice that zeroes the rows past the last sequence
  if (p.part_off >= 0) {
    const int64_t gc = std::max<int64_t>(1, (max_q + 15) / 16);   // combine: 256 / (hd / 4) = 16 rows per block
    if (kvsplit || (pol.x3 && kb == kKvSplitKB))   // split-bf16 split-key: the key-split form (4 waves stage each 128-key block)
      attn_push(&p, RQ_ATTN_K_FWD_KVSPLIT, 64, 4, kKvSplitKB, pol.x3, (kvsplit ? (max_q + 63) / 64 : 1) * nsplit, H, B, 256);
    else
      attn_push(&p, RQ_ATTN_K_FWD_SPLIT, 64, 0, kb, 0, nsplit, H, B, 64);
    attn_push(&p, RQ_ATTN_K_FWD_COMBINE, 64, 0, kb, 0, gc, H, tail, 256);
    return p;
  }
  // LDS-DMA short forms (attn_fwd_dma_kernel): self-attention style launches (more than one query tile)
  // whose key range fits 128 staged rows; RQ_ATTN_NO_DMA keeps the register-staged kernels (A/B).
  const bool dma = pol.dma && hd64 && max_q > 16 && max_k <= 128;
  // one query tile over <= 128 keys (cross-attention, the decoder's short causal self-attention): the key
  // tiles split over the waves (attn_fwd_fewq_kernel)
  const bool fewq = pol.dma && hd64 && max_q <= 16 && max_k <= 128;
  // LPT order of the short / few-query forms (by key length: their work per workgroup grows with it)
  if (have_ws && pol.lpt_short && B >= 2 && B <= kAttnOrderMax && (fewq || dma))
    attn_push_order(&p, RQ_ATTN_ORDER_SRC_CU_K, pol.order_given, 0);
  if (fewq) {
    const int nw = fewq_waves(max_k);
    attn_push(&p, RQ_ATTN_K_FWD_FEWQ, 0, nw, 0, 0, 1, H, tail, 64 * nw);
  } else if (dma && pol.x3 && max_k > 32) {   // split-bf16 form at matmul 'high'
    attn_push(&p, RQ_ATTN_K_FWD_SHORT_X3, 0, 0, dma_rows_for(max_k), 1, 1, H, tail, 256);
  } else if (dma) {
    attn_push(&p, RQ_ATTN_K_FWD_DMA, 0, 4, dma_rows_for(max_k), 0, 1, H, tail, 256);
  } else if (const int nw = hd64 ? short_plan(max_q, max_k) : 0) {
    attn_push(&p, RQ_ATTN_K_FWD_SHORT, 64, nw, 32, 0, 1, H, tail, 64 * nw);
  } else {
    if (have_ws && lpt_plan(B, max_k)) attn_push_order(&p, RQ_ATTN_ORDER_SRC_CU_K, pol.order_given, 0);
    const int cw = waves_for(max_q);
    attn_push(&p, RQ_ATTN_K_FWD, (int)s.hd, cw, 0, pol.x3 && hd64 && cw == 4, std::max<int64_t>(1, (max_q + 16 * cw - 1) / (16 * cw)),
              H, tail, 64 * cw);
  }
  return p;
}

// Backward. Workspace of the long fused form: [dQ partials: nkb x Tq x H x hd when nkb > 1] [order: pad4(B),
// under lpt_plan(B, max_q)] [dK / dV partials of the query splits: 2 x qsplit x Tk x H x hd]; of the one-pass
// short / few-query forms under RQ_ATTN_LPT_SHORT: [order: pad4(B)]; every other form uses none.
static inline rq_attn_plan attn_plan_bwd(const AttnShape& s, int cus) {
  const AttnPolicy pol = attn_policy(s.flags);
  const int64_t B = s.B, H = s.H, max_q = s.max_q, max_k = s.max_k, Tq = s.Tq, Tk = s.Tk;
  const bool hd64 = s.hd == 64, have_ws = s.ws_elems >= 0;
  rq_attn_plan p = attn_plan_empty();
  const bool dma_dq = pol.dma && hd64 && max_q > 16 && max_k <= 128;   // as the forward's LDS-DMA form
  const bool dma_kv = pol.dma && hd64 && max_k > 16 && max_q <= 128;   // dK / dV: queries staged
  const bool fewq = pol.dma && hd64 && max_q <= 16 && max_k <= 128;
  // one-pass backward of the self-attention style short launches (attn_bwd_short_fused_kernel) and of the
  // few-query launches (attn_bwd_fewq_fused_kernel); RQ_ATTN_TWO_PASS keeps the two-pass dQ + dK/dV kernels
  const bool short_fused = dma_dq && pol.fused && max_q <= 128;
  const bool fewq_fused = fewq && pol.fused;
  // the long fused form: few queries (cross-attention) have their own threshold
  const bool fused_shape = pol.fused && hd64 &&
                           (max_q <= 16 ? max_k >= kFusedMinKFewq : (max_k >= kFusedMinK && !short_plan(max_k, max_q)));
  const int64_t nkb = (max_k + kFusedKB - 1) / kFusedKB, ob = attn_pad4(B);
  const int64_t part = fused_shape && nkb > 1 ? nkb * Tq * H * s.hd : 0;
  const int64_t base = fused_shape ? part + (lpt_plan(B, max_q) ? ob : 0) : 0;   // without the dK / dV partials
  int qs = fused_shape ? fused_qsplit(B, H, max_q, max_k, pol, cus) : 1;
  const int64_t with_kv = base + (Tk >= 0 && qs > 1 ? 2 * qs * Tk * H * s.hd : 0);
  // the one-pass short / few-query backwards in LPT order (scratch: B ints)
  const bool short_lpt = pol.lpt_short && B >= 2 && B <= kAttnOrderMax && !fused_shape && (short_fused || fewq_fused);
  p.ws_total = fused_shape ? with_kv : (short_lpt ? ob : 0);
  // the fused long-range form needs its scratch; a call without one (ws NULL) runs the two-pass form there
  const bool fused = fused_shape && have_ws;
  p.ws_need = fused ? base : 0;
  if (B == 0) return p;
  const int64_t tail = B + 1;   // + the grid slice that zeroes the rows past the last sequence
  if (fused) {
    if (part > 0) p.part_off = 0;
    if (lpt_plan(B, max_q)) attn_push_order(&p, RQ_ATTN_ORDER_SRC_CU_Q, false, part);   // always its own order launch
    if (Tq * H > 0) attn_push(&p, RQ_ATTN_K_DELTA, 64, 0, 0, 0, (Tq * H * 16 + 255) / 256, 1, 1, 256);
    // query splits only when the caller sized the workspace for them (varlen_attn_bwd_ws_elems with Tk)
    if (qs > 1 && (Tk < 0 || s.ws_elems < with_kv)) qs = 1;
    p.qsplit = qs;
    if (qs > 1) p.kvpart_off = base;
    attn_push(&p, RQ_ATTN_K_BWD_FUSED, 64, kFusedNW, kFusedCH, pol.x3, std::max<int64_t>(1, nkb) * qs, H, tail, 64 * kFusedNW);
    if (qs > 1 && Tk > 0) attn_push(&p, RQ_ATTN_K_KV_REDUCE, 64, 0, 0, 0, (Tk * H * 16 + 255) / 256, 1, 1, 256);
    if (nkb > 1 && max_q > 0) attn_push(&p, RQ_ATTN_K_DQ_REDUCE, 64, 0, kFusedKB, 0, (max_q + 15) / 16, H, B, 256);
    return p;
  }
  if (have_ws && s.ws_elems >= B && short_lpt) attn_push_order(&p, RQ_ATTN_ORDER_SRC_CU_K, pol.order_given, 0);
  if (short_fused) {
    // 4 waves with up to two key tiles each (one key tile per wave, R / 16 waves, measured slower on the
    // Amazon step: 6.20-6.22 vs 6.10-6.15 ms, profiles/r03/short_tpw_ab.txt — more waves idle on short
    // sequences)
    const int r = dma_rows_for(std::max(max_q, max_k)), nw = r == 32 ? 2 : 4;
    attn_push(&p, RQ_ATTN_K_BWD_SHORT_FUSED, 0, nw, r, 0, 1, H, tail, 64 * nw);
    return p;
  }
  if (fewq_fused) {
    const int nw = fewq_waves(max_k);
    if (nw == 4 && pol.fewq_stream && Tq > 0 && Tk > 0) {   // persistent workgroups, the next unit staged by LDS-DMA
      const int64_t slots = (int64_t)cus * (max_k <= 96 ? 2 : 1);
      attn_push(&p, RQ_ATTN_K_BWD_FEWQ_STREAM, 0, 0, max_k <= 64 ? 64 : dma_rows_for(max_k), 0,
                std::max<int64_t>(1, std::min<int64_t>(B * H, slots)), 1, 1, 256);
    } else {
      attn_push(&p, RQ_ATTN_K_BWD_FEWQ_FUSED, 0, nw, 0, 0, 1, H, tail, 64 * nw);
    }
    return p;
  }
  // two passes. dQ first: it also writes delta_q = dO.O, which the dK/dV pass reads per query chunk
  if (fewq) {
    const int nw = fewq_waves(max_k);
    attn_push(&p, RQ_ATTN_K_BWD_DQ_FEWQ, 0, nw, 0, 0, 1, H, tail, 64 * nw);
  } else if (dma_dq) {
    attn_push(&p, RQ_ATTN_K_BWD_DQ_DMA, 0, 4, dma_rows_for(max_k), 0, 1, H, tail, 256);
  } else if (const int nw = hd64 ? short_plan(max_q, max_k) : 0) {
    attn_push(&p, RQ_ATTN_K_BWD_DQ_SHORT, 64, nw, 32, 0, 1, H, tail, 64 * nw);
  } else {
    const int cw = waves_for(max_q);
    attn_push(&p, RQ_ATTN_K_BWD_DQ, (int)s.hd, cw, 0, 0, std::max<int64_t>(1, (max_q + 16 * cw - 1) / (16 * cw)), H, tail, 64 * cw);
  }
  if (dma_kv) {
    attn_push(&p, RQ_ATTN_K_BWD_DKDV_DMA, 0, 4, dma_rows_for(max_q), 0, 1, H, tail, 256);
  } else if (const int nw = hd64 ? short_plan(max_k, max_q) : 0) {
    attn_push(&p, RQ_ATTN_K_BWD_DKDV_SHORT, 64, nw, 32, 0, 1, H, tail, 64 * nw);
  } else {
    const int cw = waves_for(max_k);
    attn_push(&p, RQ_ATTN_K_BWD_DKDV, (int)s.hd, cw, 0, 0, std::max<int64_t>(1, (max_k + 16 * cw - 1) / (16 * cw)), H, tail, 64 * cw);
  }
  return p;
}

}  // namespace rqhip
