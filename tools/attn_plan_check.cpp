// Stand-alone host check of csrc/attention_plan.h (plain C++17, no HIP): enumerates the dispatch grid of
// tests/test_attn_plan_host.py and checks every plan's invariants. Meant to run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/attn_plan_check.cpp -o /tmp/attn_plan_check
//   /tmp/attn_plan_check
#include <stdio.h>

#include "../rq-vae-recommender_amd/csrc/attention_plan.h"

using namespace rqhip;

static long long g_plans = 0, g_launches = 0;

static bool check(const rq_attn_plan& p, const AttnShape& s, bool backward) {
  bool ok = p.n_launches >= 0 && p.n_launches <= RQ_ATTN_MAX_LAUNCHES && p.ws_need <= p.ws_total && p.qsplit >= 1 &&
            p.qsplit <= 8 && (s.B > 0 || p.n_launches == 0);
  for (int i = 0; ok && i < p.n_launches; ++i) {
    const rq_attn_launch& l = p.launch[i];
    ok = l.family >= RQ_ATTN_K_ORDER && l.family <= RQ_ATTN_K_DQ_REDUCE && l.block >= 64 && l.block <= 1024 &&
         l.block % 64 == 0 && l.grid[0] >= 1 && l.grid[1] >= 1 && l.grid[2] >= 1 && l.grid[1] <= 65535 && l.grid[2] <= 65535;
    ++g_launches;
  }
  // offsets: only with a workspace, 16-byte aligned, in layout order, inside the provided floats
  const int64_t offs[3] = {backward ? p.part_off : p.order_off, backward ? p.order_off : p.part_off, p.kvpart_off};
  int64_t prev = -1;
  for (int64_t o : offs) {
    if (o < 0) continue;
    ok = ok && s.ws_elems >= 0 && o % 4 == 0 && o >= prev && o <= s.ws_elems;
    prev = o;
  }
  if (!ok)
    fprintf(stderr, "bad plan: backward=%d B=%lld H=%lld hd=%lld max_q=%lld max_k=%lld causal=%d flags=%d ws=%lld\n", backward,
            (long long)s.B, (long long)s.H, (long long)s.hd, (long long)s.max_q, (long long)s.max_k, s.causal, s.flags,
            (long long)s.ws_elems);
  ++g_plans;
  return ok;
}

int main() {
  const int64_t lens[] = {1, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 256, 257, 801};
  const int64_t hds[] = {16, 32, 64, 128};
  const int64_t bh[][2] = {{1, 2}, {3, 2}, {8, 6}, {64, 6}, {4097, 1}};
  const int flags[] = {0,
                       RQ_ATTN_NO_DMA,
                       RQ_ATTN_TWO_PASS,
                       RQ_ATTN_NO_DMA | RQ_ATTN_TWO_PASS,
                       RQ_ATTN_NO_SPLIT,
                       RQ_ATTN_SPLIT_BF16,
                       RQ_ATTN_FEWQ_WG,
                       RQ_ATTN_LPT_SHORT,
                       RQ_ATTN_LPT_SHORT | RQ_ATTN_ORDER_GIVEN,
                       RQ_ATTN_QSPLIT(1),
                       RQ_ATTN_QSPLIT(4)};
  bool ok = true;
  for (int64_t hd : hds)
    for (int causal = 0; causal < 2; ++causal)
      for (auto& b : bh)
        for (int fl : flags)
          for (int64_t mq : lens)
            for (int64_t mk : lens) {
              const int64_t B = b[0], H = b[1], Tq = B * mq, Tk = B * mk;
              AttnShape s{B, H, hd, mq, mk, Tq, Tk, causal, fl, -1};
              const int64_t fwd_total = attn_plan_fwd(s).ws_total;
              const int64_t bwd_total = attn_plan_bwd(s, 256).ws_total;
              s.Tk = -1;
              const int64_t bwd_base = attn_plan_bwd(s, 256).ws_total;
              ok = ok && bwd_base <= bwd_total;
              s.Tk = Tk;
              for (int64_t ws : {(int64_t)-1, fwd_total}) {   // workspace absent / as sized
                s.ws_elems = ws;
                const rq_attn_plan p = attn_plan_fwd(s);
                ok = check(p, s, false) && p.ws_total == fwd_total && ok;
              }
              for (int64_t ws : {(int64_t)-1, bwd_base, bwd_total}) {   // absent / sized without Tk / with Tk
                s.ws_elems = ws;
                const rq_attn_plan p = attn_plan_bwd(s, 256);
                ok = check(p, s, true) && p.ws_total == bwd_total && ok;
                // the dK / dV partials end the layout at the total
                if (p.kvpart_off >= 0) ok = ok && p.kvpart_off + 2 * p.qsplit * Tk * H * hd == bwd_total && ws == bwd_total;
              }
            }
  printf("%lld plans, %lld launches: %s\n", g_plans, g_launches, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
