// Stand-alone host check of csrc/gemm_plan.h (plain C++17, no HIP): enumerates the planning grid of
// tests/gemm_plan_support.py at 256 CUs and checks every plan's invariants. Meant to run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_check.cpp -o /tmp/gemm_plan_check
//   /tmp/gemm_plan_check
#include <stdio.h>

#include "../rq-vae-recommender_amd/csrc/gemm_plan.h"

using namespace rqhip;

static long long g_plans = 0, g_pairs = 0, g_groups = 0;
constexpr int kCus = 256;

static X3Shape shape(int64_t M, int64_t N, int64_t K, int code, int epi, int flags) {   // minimal leading dimensions
  return X3Shape{M, N, K, (code & kCodeAK) ? K : M, (code & kCodeBK) ? K : N, N, code, epi, flags, epi != kEpiStore};
}

// S >= 1, whole k stages, every chunk starts inside K, a grid, slabs as counted
static bool plan_ok(const X3Plan& p, int64_t M, int64_t N, int64_t K) {
  const int ks = p.kind == kX3Wide ? kWK : kXK;
  return p.S >= 1 && p.chunk > 0 && p.chunk % ks == 0 && (int64_t)(p.S - 1) * p.chunk < K && p.grid >= 1 &&
         (int64_t)p.grid >= (int64_t)p.tiles * p.S && p.slab == (p.S > 1) &&
         p.slab_bytes == (p.slab ? (size_t)p.S * (size_t)(M * N) * 4 : 0) &&
         p.ts == (p.kind == kX3Wide ? kWT2 : (p.kind == kX3Tile64 ? 64 : kXT));
}

static bool check_call(const X3Shape& s) {
  const X3Plan p = x3_call_plan(s, kCus);
  const bool forced = ((s.flags >> RQ_GEMM_SPLIT_SHIFT) & RQ_GEMM_SPLIT_MASK) > 0;
  bool ok = plan_ok(p, s.M, s.N, s.K) && p.code == s.code && p.epi_k == (p.slab ? (int)kEpiStore : s.epilogue) &&
            (p.lds_pad == 0 || p.kind == kX3Tile64) && (!p.kfull || (s.K % kXK == 0 && !(s.flags & RQ_GEMM_MASKED)));
  // the planner's own split counts fit the workspace the library sizes for the shape
  if (!forced) ok = ok && p.slab_bytes <= x3_workspace_bytes(s.M, s.N, s.K, kCus);
  // a wide plan: the operands within the DMA's reach, the form built, never against the policy
  if (p.kind == kX3Wide)
    ok = ok && x3w_spans_ok(s) && x3_form_built(kX3Wide, s.code, s.epilogue) && x3_form_built(kX3Wide, p.code, p.epi_k) &&
         !(s.flags & (RQ_GEMM_NO_WIDE | RQ_GEMM_ONLY_128 | RQ_GEMM_ONLY_64));
  if ((s.flags & RQ_GEMM_ONLY_128) && p.kind != kX3Tile128) ok = false;
  if ((s.flags & RQ_GEMM_ONLY_64) && p.kind != kX3Tile64) ok = false;
  if (!ok)
    fprintf(stderr, "bad plan: M=%lld N=%lld K=%lld code=%d epilogue=%d flags=%#x\n", (long long)s.M, (long long)s.N,
            (long long)s.K, s.code, s.epilogue, s.flags);
  ++g_plans;
  return ok;
}

static bool check_pair(const X3Shape& s1, const X3Shape& s2) {
  const X3Plan p1 = x3_call_plan(s1, kCus), p2 = x3_call_plan(s2, kCus);
  const X3PairPlan pp = x3_pair_plan(p1, p2, kCus);
  bool ok = true;
  if (pp.kind)
    ok = (pp.kind == kX3PairDgrad || pp.kind == kX3PairFwd) && p1.kind == p2.kind && p1.kind != kX3Wide &&
         pp.n1 == p1.grid && pp.grid == p1.grid + p2.grid && (pp.lds_pad == 0 || p1.kind == kX3Tile64) &&
         (pp.kind == kX3PairFwd ? x3_form_built(kX3PairFwd, p1.code, p1.epi_k) && x3_form_built(kX3PairFwd, p2.code, p2.epi_k)
                                : x3_form_built(kX3PairDgrad, p1.code, p1.epi_k) && x3_form_built(kX3PairWgrad, p2.code, p2.epi_k));
  const int rs = x3_pair_resplit(p1, p2, s1.K, s2.K, kCus);
  ok = ok && rs >= 0 && (rs == 0 || (rs > 1 && rs < p2.S));
  if (!ok)
    fprintf(stderr, "bad pair: (%lld, %lld, %lld, code %d) + (%lld, %lld, %lld, code %d) flags=%#x\n", (long long)s1.M,
            (long long)s1.N, (long long)s1.K, s1.code, (long long)s2.M, (long long)s2.N, (long long)s2.K, s2.code, s1.flags);
  ++g_pairs;
  return ok;
}

static bool check_group(const X3Shape* s, int count, bool model) {
  X3Plan own[kX3GroupMax];
  for (int i = 0; i < count; ++i) own[i] = x3_call_plan(s[i], kCus);
  const X3GroupPlan g = x3_group_plan(s, own, count, model, kCus);
  bool ok = g.n == 0 || g.n >= 2;
  int64_t wgs = 0;
  int n = 0;
  for (int i = 0; i < count; ++i) {
    if (!g.in[i]) continue;
    ++n;
    wgs += g.pl[i].grid;
    ok = ok && plan_ok(g.pl[i], s[i].M, s[i].N, s[i].K) && g.pl[i].kind == kX3Wide && g.pl[i].S >= 2 && x3_group_member(s[i]);
  }
  ok = ok && n == g.n;
  bool forced = false;
  for (int i = 0; i < count; ++i) forced = forced || ((s[i].flags >> RQ_GEMM_SPLIT_SHIFT) & RQ_GEMM_SPLIT_MASK) > 0;
  if (!forced) ok = ok && (model || g.n == 0) && wgs <= kCus;   // only the model groups by itself: into one round of wide workgroups
  if (!ok) fprintf(stderr, "bad group: %d members over K=%lld flags=%#x\n", count, (long long)s[0].K, s[0].flags);
  ++g_groups;
  return ok;
}

int main() {
  const int64_t dims[] = {8, 40, 64, 136, 256, 512, 1280, 2048, 11264, 65536};
  const int64_t ks[] = {8, 32, 40, 128, 384, 512, 768, 4104, 11264, 65536};
  const int flags[] = {0, RQ_GEMM_ONLY_128, RQ_GEMM_ONLY_64, RQ_GEMM_FORCE_WIDE, RQ_GEMM_NO_WIDE, RQ_GEMM_MASKED,
                       RQ_GEMM_SPLIT(3), RQ_GEMM_SPLIT(21)};
  bool ok = true;
  for (int64_t M : dims)
    for (int64_t N : dims)
      for (int64_t K : ks) {
        for (int code = 0; code < 32; code += 2)
          for (int epi = 0; epi < 4; ++epi)
            for (int fl : flags) ok = check_call(shape(M, N, K, code, epi, fl)) && ok;
        // a Linear's backward over M rows, K outputs, N inputs; two forward projections of M rows
        for (int fl : {0, (int)RQ_GEMM_ONLY_128, (int)RQ_GEMM_ONLY_64, (int)RQ_GEMM_NO_WIDE, RQ_GEMM_SPLIT(3)}) {
          for (int cd : {18, 26, 22, 16})
            for (int epi : {(int)kEpiStore, (int)kEpiSiluBwd})
              for (int cw : {0, 2, 8, 10, 4}) ok = check_pair(shape(M, N, K, cd, epi, fl), shape(K, N, M, cw, kEpiStore, fl)) && ok;
          for (int c2 : {22, 30, 18}) ok = check_pair(shape(M, N, K, 30, kEpiStore, fl), shape(M, 512, K, c2, kEpiStore, fl)) && ok;
        }
      }
  // chains of 2 to 4 weight gradients (split m/n-contiguous operands) over the batch as K
  const int64_t pool[][2] = {{512, 1280}, {256, 512}, {136, 256}, {64, 256}, {2048, 512}, {40, 64}, {1280, 1280}};
  const int member_flags[] = {0, RQ_GEMM_SPLIT(3), RQ_GEMM_SPLIT(21), RQ_GEMM_SPLIT(4095), RQ_GEMM_NO_GROUP, RQ_GEMM_ONLY_128};
  for (int64_t K : {(int64_t)11264, (int64_t)32768, (int64_t)65536})
    for (int fl : member_flags)
      for (int mask = 0; mask < (1 << 7); ++mask) {
        X3Shape s[kX3GroupMax];
        int n = 0;
        for (int j = 0; j < 7; ++j)
          if (mask >> j & 1) {   // SPLIT(21): on the first member only
            s[n] = shape(pool[j][0], pool[j][1], K, kCodeAS | kCodeBS, kEpiStore, n == 0 || fl != RQ_GEMM_SPLIT(21) ? fl : 0);
            ++n;
          }
        if (n < 2 || n > 4) continue;
        ok = check_group(s, n, true) && ok;
        ok = check_group(s, n, false) && ok;
      }
  printf("%lld plans, %lld pairs, %lld groups: %s\n", g_plans, g_pairs, g_groups, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
