// Beam-searched residual quantization: the W best code paths per item instead of the greedy one.
// gfx950 / wave64 / fp32 MFMA. An extension: the reference only has the greedy level loop
// (modules/rqvae.py:114-138, res_{l+1} = res_l - emb_l with one argmin per level), which this call
// generalises the way Faiss's ResidualQuantizer does with max_beam_size: W partial paths survive each
// level, all W K extensions are ranked.
//
// The rule (also modules/beam_quantize.py and the fp64 restatement of the tests):
//   level 0 starts from one beam with residual x. At level l beam w (residual r_w) and code k have the
//   key e(w, k) = (|r_w|^2 + |c_k|^2) - 2 r_w.c_k in fp32 (the greedy kernels' expression); the W
//   candidates with the smallest (e, w, k), lexicographic, survive in that order; a survivor's residual
//   is r_w - c_k elementwise and its path is its parent's plus k.
//
// One workgroup = 4 waves = 128 (item, beam) rows = floor(128 / W) items, all L levels inside the launch.
//   * distances: the rows are the lane axis of v_mfma_f32_32x32x2_f32 (B operand = the row's residual,
//     half a row per lane, in registers), the codewords its row axis (A operand from an LDS chunk of 128
//     codewords, padded rows, ds_read_b128) - rq_fwd_reg_kernel's arrangement with beams as extra items;
//   * a row's residual is never stored: x minus the codewords of its path, subtracted in level order, is
//     bit for bit the chained r_w - c_k, and a path is at most 16 small integers in LDS;
//   * selection in two stages: every lane keeps the W smallest (e, k) of the codewords it sees (its half
//     of each 32-codeword tile) as W unsorted 64-bit keys in LDS - order-preserving bits of e, then k, so
//     one unsigned compare is the rule's order and W-dependent state costs no registers; a new key
//     replaces the largest and a scan of W independent reads, eight in flight, finds the next largest (a
//     sorted insertion's dependent LDS chain made the whole call 2.2x slower at W >= 16). Then a group of >= 2 W lanes per item pops the W
//     smallest offers of the item's 2 W lists (keys widened by the beam: e, then w, then k; one
//     min-butterfly per survivor). Every member of the global top W is in its own parent's top W.
#include "common.h"

namespace rqhip {

constexpr int kBqRows = 128;    // (item, beam) rows per workgroup
constexpr int kBqNB = 128;      // codewords per LDS chunk
constexpr int kBqMaxW = 32, kBqMaxL = 16, kBqMaxK = 4096;

// fp32 -> uint32 whose unsigned order is the float order (a positive NaN sorts past +inf: still a valid code)
__device__ __forceinline__ uint32_t bq_ordered(float e) {
  const uint32_t u = __float_as_uint(e);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bq_unordered(uint32_t o) {
  return __uint_as_float((o >> 31) ? (o & 0x7FFFFFFFu) : ~o);
}

template <int D>
__global__ void __launch_bounds__(256)
beam_quantize_kernel(const float* __restrict__ x, int B, const float* __restrict__ cbs, const float* __restrict__ csq,
                     int K, int L, int W, int IPB, int G, int64_t* __restrict__ paths, float* __restrict__ err,
                     float* __restrict__ residual) {
  constexpr int H2 = D / 2, LD = D + 4;
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  float* A_s = dsm;                        // [kBqNB][LD] codeword chunk
  float* cs_s = A_s + kBqNB * LD;          // [kBqNB]     |c|^2 (+inf past the chunk)
  uint64_t* lkey = reinterpret_cast<uint64_t*>(cs_s + kBqNB);   // [W][256] per-lane candidate keys (8-B aligned)
  float* serr = reinterpret_cast<float*>(lkey + W * 256);       // [kBqRows] the survivors' keys
  unsigned short* pcur = reinterpret_cast<unsigned short*>(serr + kBqRows);   // [kBqRows][L] paths of the current beams
  unsigned short* pnext = pcur + kBqRows * L;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5;
  const int rr = wave * 32 + (lane & 31);            // this lane's row: item rr / W, beam rr % W
  const int it = rr / W, w = rr - it * W;
  const int64_t b = (int64_t)blockIdx.x * IPB + it;
  const bool item_ok = it < IPB && b < B;
  const float* xr = x + (item_ok ? b : 0) * D + h * H2;

  for (int i = tid; i < 2 * kBqRows * L; i += 256) pcur[i] = 0;   // rows never written hold valid codes
  __syncthreads();

  for (int l = 0; l <= L; ++l) {
    // the row's residual: x minus its path's codewords in level order
    float xv[H2];
#pragma unroll
    for (int k = 0; k < H2; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(xr + k);
      xv[k] = v.x; xv[k + 1] = v.y; xv[k + 2] = v.z; xv[k + 3] = v.w;
    }
    for (int lp = 0; lp < l; ++lp) {
      const int code = min((int)pcur[rr * L + lp], K - 1);
      const float* cr = cbs + ((int64_t)lp * K + code) * D + h * H2;
#pragma unroll
      for (int k = 0; k < H2; k += 4) {
        const float4 c = *reinterpret_cast<const float4*>(cr + k);
        xv[k] -= c.x; xv[k + 1] -= c.y; xv[k + 2] -= c.z; xv[k + 3] -= c.w;
      }
    }
    if (l == L) {
      if (residual != nullptr && item_ok) {
        float* dst = residual + (b * W + w) * D + h * H2;
#pragma unroll
        for (int k = 0; k < H2; k += 4)
          *reinterpret_cast<float4*>(dst + k) = make_float4(xv[k], xv[k + 1], xv[k + 2], xv[k + 3]);
      }
      break;
    }
    float xs = 0.f;
#pragma unroll
    for (int k = 0; k < H2; ++k) xs = __builtin_fmaf(xv[k], xv[k], xs);
    xs += __shfl_xor(xs, 32, 64);
    const bool live = item_ok && (l > 0 || w == 0);   // level 0 has one beam

    // this lane's W smallest keys so far, unsorted; (maxkey, maxpos) = the largest of them and its slot.
    // A key is the order-preserving bits of e, then the code: one unsigned compare is the (e, k) order.
    for (int s = 0; s < W; ++s) lkey[s * 256 + tid] = ~0ull;
    uint64_t maxkey = ~0ull;
    int maxpos = 0;
    const float* cb = cbs + (int64_t)l * K * D;

    for (int n0 = 0; n0 < K; n0 += kBqNB) {
      const int nrows = min(kBqNB, K - n0);
      __syncthreads();   // the previous chunk is consumed
      for (int f = tid; f < nrows * (D / 4); f += 256) {
        const int r = f / (D / 4), c = (f % (D / 4)) * 4;
        *reinterpret_cast<float4*>(A_s + r * LD + c) = *reinterpret_cast<const float4*>(cb + (int64_t)(n0 + r) * D + c);
      }
      if (tid < kBqNB) cs_s[tid] = tid < nrows ? csq[(int64_t)l * K + n0 + tid] : INFINITY;
      __syncthreads();
      for (int t0 = 0; t0 < nrows; t0 += 32) {
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // lane half h supplies dims [h H2, (h + 1) H2) of both operands: the same permutation of the
        // summation index on both sides. Rows past nrows read stale LDS; their keys are dropped below.
        const float* ap = A_s + (t0 + (lane & 31)) * LD + h * H2;
#pragma unroll
        for (int s4 = 0; s4 < H2; s4 += 4) {
          const float4 a = *reinterpret_cast<const float4*>(ap + s4);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xv[s4], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xv[s4 + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xv[s4 + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xv[s4 + 3], acc, 0, 0, 0);
        }
        // C map: register r of lane (j, h) = codeword t0 + (r & 3) + 8 (r >> 2) + 4 h of row j, ascending in r
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int il = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
          // (|r|^2 + |c|^2) - 2 r.c: 2 r.c is exact, so the fma rounds like the reference expression; + 0 makes -0 +0
          const float d = __builtin_fmaf(-2.f, acc[r], xs + cs_s[il]) + 0.f;
          const uint64_t key = ((uint64_t)bq_ordered(d) << 16) | (uint32_t)(n0 + il);
          if (live && il < nrows && key < maxkey) {
            // replace the largest, then find the new largest: independent reads, eight in flight (slots past
            // W re-read the last one), no dependent chain
            lkey[maxpos * 256 + tid] = key;
            maxkey = 0;
            maxpos = 0;
            for (int s0 = 0; s0 < W; s0 += 8) {
              uint64_t v[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) v[u] = lkey[min(s0 + u, W - 1) * 256 + tid];
#pragma unroll
              for (int u = 0; u < 8; ++u)
                if (v[u] > maxkey) { maxkey = v[u]; maxpos = min(s0 + u, W - 1); }
            }
          }
        }
      }
    }
    __syncthreads();   // every lane's list is complete

    // merge: G >= 2 W lanes per item, lane g owns list (beam g >> 1, half g & 1) and offers its smallest key
    // not yet taken (a scan of the W unsorted slots); the group's minimum survives, its owner offers its next
    {
      const int g = tid & (G - 1), grp = tid / G, ngrp = 256 / G;
      for (int base = 0; base < IPB; base += ngrp) {
        const int it2 = base + grp;
        const bool act = it2 < IPB;
        const bool has = act && g < 2 * W;
        const int mw = g >> 1, mrr = has ? it2 * W + mw : 0;
        const int mt = (mrr >> 5) * 64 + (g & 1) * 32 + (mrr & 31);
        bool taken = false;
        uint64_t last = 0;
        // the list's smallest key above `last`, as a group-wide key: bits of e, then beam, then code
        auto head = [&]() -> uint64_t {
          uint64_t best = ~0ull;
          if (has)
            for (int s0 = 0; s0 < W; s0 += 8) {
              uint64_t v[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) v[u] = lkey[min(s0 + u, W - 1) * 256 + mt];
#pragma unroll
              for (int u = 0; u < 8; ++u)
                if ((!taken || v[u] > last) && v[u] < best) best = v[u];
            }
          return best;
        };
        uint64_t own = head();
        for (int s = 0; s < W; ++s) {
          const uint64_t hd = own == ~0ull ? ~0ull : ((own >> 16) << 32) | ((uint64_t)mw << 16) | (own & 0xFFFFu);
          uint64_t m = hd;
          for (int o = G >> 1; o >= 1; o >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)m, o, 64);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(m >> 32), o, 64);
            const uint64_t other = ((uint64_t)hi << 32) | lo;
            m = other < m ? other : m;
          }
          if (hd == m && m != ~0ull) {
            taken = true;
            last = own;
            own = head();
          }
          int sw = (int)(((uint32_t)m >> 16) & 0xFFFFu), sk = (int)((uint32_t)m & 0xFFFFu);
          if (sk >= K || sw >= W) { sw = 0; sk = 0; }   // fewer than W keys (cannot happen for W <= K): stay in bounds
          if (act) {
            for (int lp = g; lp < l; lp += G) pnext[(it2 * W + s) * L + lp] = pcur[(it2 * W + sw) * L + lp];
            if (g == 0) {
              pnext[(it2 * W + s) * L + l] = (unsigned short)sk;
              serr[it2 * W + s] = bq_unordered((uint32_t)(m >> 32));
            }
          }
        }
      }
    }
    __syncthreads();   // the new paths are complete; the lists are free
    unsigned short* t = pcur; pcur = pnext; pnext = t;
  }

  // rows of this workgroup are contiguous in the outputs
  const int64_t row0 = (int64_t)blockIdx.x * IPB * W, nrow = (int64_t)B * W;
  for (int i = tid; i < IPB * W * L; i += 256)
    if (row0 + i / L < nrow) paths[row0 * L + i] = (int64_t)pcur[i];
  for (int i = tid; i < IPB * W; i += 256)
    if (row0 + i < nrow) err[row0 + i] = serr[i];
}

static size_t bq_lds_bytes(int D, int L, int W) {
  return (size_t)(kBqNB * (D + 4) + kBqNB + kBqRows) * sizeof(float) + (size_t)W * 256 * sizeof(uint64_t) +
         (size_t)(2 * kBqRows * L) * sizeof(unsigned short);
}

}  // namespace rqhip

using namespace rqhip;

extern "C" {

size_t rq_quantize_beam_workspace(int64_t B, int64_t D, int64_t K, int64_t L, int64_t W) {
  (void)B; (void)D; (void)K; (void)L; (void)W;
  return 0;   // paths and candidate lists live in LDS, residuals are recomputed from the paths
}

int rq_quantize_beam(const float* x, int64_t B, int64_t D, const float* codebooks, const float* cb_sqnorm, int64_t K,
                     int64_t L, int64_t W, int64_t* paths, float* err, float* residual, void* workspace,
                     size_t ws_bytes, void* stream) {
  RQ_CHECK_ARG(D == 8 || D == 16 || D == 32 || D == 64,
               "rq_quantize_beam: D must be a power of two in [8, 64] (D=%lld); wider rows are not supported",
               (long long)D);
  RQ_CHECK_ARG(K >= 1 && K <= kBqMaxK, "rq_quantize_beam: need 1 <= K <= %d (K=%lld)", kBqMaxK, (long long)K);
  RQ_CHECK_ARG(L >= 1 && L <= kBqMaxL, "rq_quantize_beam: need 1 <= L <= %d (L=%lld)", kBqMaxL, (long long)L);
  RQ_CHECK_ARG(W >= 1 && W <= std::min<int64_t>(K, kBqMaxW), "rq_quantize_beam: need 1 <= W <= min(K, %d) (W=%lld, K=%lld)",
               kBqMaxW, (long long)W, (long long)K);
  RQ_CHECK_ARG(B >= 0 && B <= (1ll << 31) / 64, "rq_quantize_beam: need 0 <= B <= 2^25 (B=%lld)", (long long)B);
  if (B == 0) return 0;
  RQ_CHECK_ARG(x && codebooks && cb_sqnorm && paths && err, "rq_quantize_beam: null pointer");
  RQ_CHECK_ARG(((uintptr_t)x | (uintptr_t)codebooks | (uintptr_t)residual) % 16 == 0,
               "rq_quantize_beam: x, codebooks and residual must be 16-byte aligned");
  const size_t need = rq_quantize_beam_workspace(B, D, K, L, W);
  RQ_CHECK_ARG(need == 0 || (workspace != nullptr && ws_bytes >= need),
               "rq_quantize_beam: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  const int w = (int)W, ipb = kBqRows / w;
  int g = 2;
  while (g < 2 * w) g <<= 1;
  const dim3 grid((unsigned)((B + ipb - 1) / ipb));
  const size_t lds = bq_lds_bytes((int)D, (int)L, w);
  hipStream_t s = (hipStream_t)stream;
#define RQ_BQ_LAUNCH(DD)                                                                                              \
  hipLaunchKernelGGL(beam_quantize_kernel<DD>, grid, dim3(256), lds, s, x, (int)B, codebooks, cb_sqnorm, (int)K,     \
                     (int)L, w, ipb, g, paths, err, residual)
  switch (D) {
    case 8: RQ_BQ_LAUNCH(8); break;
    case 16: RQ_BQ_LAUNCH(16); break;
    case 32: RQ_BQ_LAUNCH(32); break;
    default: RQ_BQ_LAUNCH(64); break;
  }
#undef RQ_BQ_LAUNCH
  RQ_LAUNCH_CHECK("rq_quantize_beam");
  return 0;
}

}  // extern "C"
