// Weight gradient of a Linear layer over a large batch: dW = g^T x, db = sum_b g  (fp32 MFMA).
//
// Reference: every nn.Linear in modules/encoder.py:7-36 (the RQ-VAE encoder / decoder MLPs) and
// modules/transformer/* — torch autograd computes grad_weight = grad_out^T @ input. At the RQ-VAE
// batch (B = 65,536 rows) that product has a tiny output (O x I <= 768 x 512) and a huge
// reduction axis, which the library GEMM tiles poorly (5-29 TFLOP/s measured on gfx950, where
// forward / data-grad GEMMs of the same layers reach 100-128). Here the reduction axis is split
// across workgroups (split-K) so a launch covers every CU:
//
//   pass 1  wgrad_partial_kernel: workgroup (s, tile) computes the 128 x 128 output tile over
//           rows [s*chunk, (s+1)*chunk) on v_mfma_f32_32x32x2_f32, operands staged through a
//           double-buffered LDS ring (rows stay in their HBM layout: b-major, coalesced float4
//           loads; one conflict-free ds_read_b64 per operand feeds two MFMA tiles).
//           Tile-column-0 workgroups also sum g over their rows for db. Partials go to a
//           workspace [S][O][I] (+ [S][O]).
//   pass 2  wgrad_reduce_kernel: fixed-order sum over s — deterministic, no atomics.
//
// Workgroups that share a row chunk are placed on the same XCD (blockIdx % 8 selects the XCD)
// so the tiles re-reading the same g / x rows hit one L2.
#include "common.h"
#include "gemm_plan.h"   // the tile constants (kWT, kWBK, kXT, kXK, kWT2, ...), the epilogue codes and every plan

namespace rqhip {

constexpr int kWLD = 128;   // LDS row stride in floats (float2 operand reads: 32 lanes x 8 B = all 64 banks)

// Operand mapping: a wave owns a 64 (o) x 64 (i) block as 2 x 2 MFMA tiles, interleaved so that
// one ds_read_b64 feeds both tiles of a pair: tile p's MFMA row m is o = 2m + p (and tile q's
// column n is i = 2n + q). The MFMA k index is the lane half (rows b = 2kp, 2kp+1 of the stage).
__global__ void __launch_bounds__(256, 2)
wgrad_partial_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ x, int64_t ldx, int64_t Bn,
                     int O, int I, int tiles_i, int tiles, int S, int64_t chunk, int per, float* __restrict__ P,
                     float* __restrict__ Pb) {
  __shared__ __attribute__((aligned(16))) float As[2][kWBK][kWLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][kWBK][kWLD];
  const int bid = blockIdx.x;
  const int lw = (bid & 7) * per + (bid >> 3);   // XCD-major order: consecutive lw share an XCD
  if (lw >= tiles * S) return;
  const int s = lw / tiles, t = lw % tiles;
  const int o0 = (t / tiles_i) * kWT, i0 = (t % tiles_i) * kWT;
  const int64_t b_lo = (int64_t)s * chunk;
  const int64_t b_hi = b_lo + chunk < Bn ? b_lo + chunk : Bn;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c32 = lane & 31;
  const int wo = wave >> 1, wi = wave & 1;
  const bool do_bias = Pb != nullptr && (t % tiles_i) == 0 && wi == 0;

  constexpr int kF = kWBK * kWT / 4 / 256;   // float4 per thread per operand per stage
  float4 ra[kF], rb[kF];
  bool okm[kF];
  // Branch-free staging: every load is issued (a guarded load compiles to a branch around it and
  // a vmcnt(0) per element). Rows past the chunk read row b_lo and are zeroed by a select (they
  // would add into valid outputs); columns past O / I are clamped in range and left as they are —
  // they only feed output rows / columns >= O / I, which are never written.
  const int scol = (tid & 31) * 4;
  const int64_t gcol = min(o0 + scol, O - 4), xcol = min(i0 + scol, I - 4);
  auto load = [&](int64_t b0) {
#pragma unroll
    for (int j = 0; j < kF; ++j) {
      const int r = (tid >> 5) + 8 * j;
      const int64_t b = b0 + r;
      const bool okb = b < b_hi;
      const int64_t bb = okb ? b : b_lo;
      ra[j] = *reinterpret_cast<const float4*>(g + bb * ldg + gcol);
      rb[j] = *reinterpret_cast<const float4*>(x + bb * ldx + xcol);
      okm[j] = okb;
    }
  };
  // The zero-select happens here, after the loads have landed (a select right after the load
  // would wait for it); per component, since a whole-float4 select lowers through scratch.
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < kF; ++j) {
      const int f = tid + 256 * j, r = f >> 5, c = (f & 31) * 4;
      const bool k = okm[j];
      const float4 a = make_float4(k ? ra[j].x : 0.f, k ? ra[j].y : 0.f, k ? ra[j].z : 0.f, k ? ra[j].w : 0.f);
      const float4 v = make_float4(k ? rb[j].x : 0.f, k ? rb[j].y : 0.f, k ? rb[j].z : 0.f, k ? rb[j].w : 0.f);
      *reinterpret_cast<float4*>(&As[buf][r][c]) = a;
      *reinterpret_cast<float4*>(&Bs[buf][r][c]) = v;
    }
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[p][q][r] = 0.f;
  float bsum = 0.f;

  const int nst = (int)((b_hi - b_lo + kWBK - 1) / kWBK);
  load(b_lo);
  stash(0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    if (st + 1 < nst) load(b_lo + (int64_t)(st + 1) * kWBK);   // in flight during the MFMAs
    // LDS operand pipeline: the two reads for k-pair kp+1 are issued ahead of k-pair kp's four
    // MFMAs (sched_group_barrier pins that order), so no MFMA group waits on its own ds_read.
    // A[o][k] = g[b][o], B[k][i] = x[b][i].
    float2 a = *reinterpret_cast<const float2*>(&As[buf][h][wo * 64 + 2 * c32]);
    float2 v = *reinterpret_cast<const float2*>(&Bs[buf][h][wi * 64 + 2 * c32]);
#pragma unroll
    for (int kp = 0; kp < kWBK / 2; ++kp) {
      float2 an = a, vn = v;
      if (kp + 1 < kWBK / 2) {
        const int k = 2 * (kp + 1) + h;
        an = *reinterpret_cast<const float2*>(&As[buf][k][wo * 64 + 2 * c32]);
        vn = *reinterpret_cast<const float2*>(&Bs[buf][k][wi * 64 + 2 * c32]);
      }
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, v.x, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, v.y, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, v.x, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, v.y, acc[1][1], 0, 0, 0);
      a = an;
      v = vn;
    }
#pragma unroll
    for (int kp = 0; kp < kWBK / 2; ++kp) {
      if (kp + 1 < kWBK / 2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // next k-pair's reads
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                          // this k-pair's MFMAs
    }
    if (do_bias) {
#pragma unroll
      for (int k = 0; k < kWBK; ++k) bsum += As[buf][k][wo * 64 + lane];
    }
    if (st + 1 < nst) stash(buf ^ 1);
    __syncthreads();
  }

  // C/D map: MFMA row m = (r&3) + 8(r>>2) + 4h, column n = lane&31; o = 2m + p, i = 2n + q.
  float* Ps = P + (int64_t)s * O * I;
  const int i = i0 + wi * 64 + 2 * c32;
  if (i < I) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + wo * 64 + 2 * ((r & 3) + 8 * (r >> 2) + 4 * h) + p;
        if (o < O) *reinterpret_cast<float2*>(Ps + (int64_t)o * I + i) = make_float2(acc[p][0][r], acc[p][1][r]);
      }
  }
  if (do_bias) {
    const int o = o0 + wo * 64 + lane;
    if (o < O) Pb[(int64_t)s * O + o] = bsum;
  }
}

// out[j] = sum_{s=0}^{S-1} P[s*n + j] in a fixed order (n % 4 == 0): workgroup = 64 float4
// columns x 4 waves; wave w sums s = w, w+4, ... (strided_slab_sum), then
// the four wave partials are added in wave order through LDS. Deterministic, no atomics.
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ P, int S, int64_t n,
                                                           float* __restrict__ out) {
  __shared__ float4 part[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t j = ((int64_t)blockIdx.x * 64 + lane) * 4;
  const bool ok = j < n;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) a = strided_slab_sum(P, S, n, j, wave, 4);
  part[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && ok) {
    float4 r = part[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 v = part[w][lane];
      r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    }
    *reinterpret_cast<float4*>(out + j) = r;
  }
}

// CUs of the current device, queried once: the one machine fact every plan of gemm_plan.h takes as an argument.
// 256 (an MI355X) when no device answers, so planning works on a machine without a GPU.
static int x3_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}


// ---------------------------------------------------------------------------------------------
// Split-bf16 ("bf16x3") GEMM: the fp32 matmul at torch.set_float32_matmul_precision('high'),
// which the reference selects at import (modules/rqvae.py:19, modules/model.py:27). PyTorch
// defines 'high' as TF32 or "each float32 as the sum of two bfloat16 numbers"; gfx950 has no
// xf32 MFMA, so this is the second form on v_mfma_f32_32x32x16_bf16: a = a_hi + a_lo with
// a_hi = RN_bf16(a), a_lo = RN_bf16(a - a_hi) (the subtraction is exact), and
//   a.b ~ a_hi.b_hi + a_hi.b_lo + a_lo.b_hi        (fp32 accumulation; a_lo.b_lo dropped)
// — per-product relative error <= ~2^-17 (TF32: 2^-11), at 3 bf16 MFMAs per product = 5.3x the
// f32-MFMA rate. 'highest' keeps the exact-f32 path (library GEMM + wgrad_partial_kernel).
//
//   C[m][n] = sum_k A(m, k) B(n, k)
//   A(m, k) = A[m*lda + k] (a_kc: k-contiguous) or A[k*lda + m] (m-contiguous); B likewise.
//   forward  y = x W^T : A = x (k-contig),  B = W (k-contig)
//   dgrad   dx = g W   : A = g (k-contig),  B(n=i, k=o) = W[o][i] (n-contig)
//   wgrad   dW = g^T x : A(m=o, k=b) = g[b][o], B(n=i, k=b) = x[b][i] (both m/n-contig), split-K
//
// Tile 128 x 128 x 32 per workgroup (4 waves, 64 x 64 each = 2 x 2 MFMA tiles). Operands are
// converted to (hi, lo) bf16 planes while staged into LDS (register staging, double-buffered):
//   k-contig operand -> "row image" [128 rows][32 k] (64-B rows, 16-B chunk c stored at
//                       c ^ ((row >> 2) & 3)): fragments by conflict-free ds_read_b128;
//   m/n-contig       -> "column image" [32 k][128 rows] (256-B rows, chunk XOR
//                       ((k & 3) << 2 | (k >> 2) & 3)): fragments by ds_read_b64_tr_b16 (the
//                       hardware transpose read), conflict-free per 32-lane half.
// Both images come from coalesced float4 loads in the operand's HBM layout.
// ---------------------------------------------------------------------------------------------

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));

constexpr int kXCPR = kXK / 8;                 // 16-byte bf16 chunks per row of the row image
constexpr int kXPlane = kXT * kXK * 2;         // bytes of one bf16 plane (8 KiB)
constexpr int kXOp = 2 * kXPlane;              // hi + lo planes of one operand
constexpr int kXBuf = 2 * kXOp;                // A + B
constexpr int kXLds = 2 * kXBuf;               // double buffer: 64 KiB (the 64-tile form: half)
static_assert(kXLds == 65536, "LDS of the 128-tile form");
static_assert(kXT == 128 && kXK == 32 && kXLds / 2 == 32768,
              "gemm_plan.h: x3s_pad_lds pads a 64-tile launch by that form's own 32 KiB, to two workgroups per CU");

__device__ __forceinline__ int col_swz(int k) { return ((k & 3) << 2) | ((k >> 2) & 3); }
// Byte offset of 16-B chunk `c` of k-row kr in a column image of TR columns: 256-B rows with col_swz
// for TR = 128 (and the wide kernel); for TR = 64 128-B rows with a swizzle over the 8 chunks,
// s = 2 ((kr >> 1) & 1) + 4 ((kr >> 3) & 1): a ds_read_b64_tr_b16 half-wave touches k-rows {4u..4u+3,
// 4u+8..4u+11} (+16), chunk pairs (c0, c0 + 1) with c0 even — the even rows land on banks 0-31 and the
// odd rows on 32-63, each row's pair at a distinct s: conflict-free; the staging stores write whole
// 128-B rows per 8- / 16-lane group.
template <int TR>
__device__ __forceinline__ int col_off(int kr, int c) {
  if constexpr (TR == 64) return 128 * kr + ((c ^ ((((kr >> 1) & 1) << 1) | (((kr >> 3) & 1) << 2))) << 4);
  else return 256 * kr + ((c ^ col_swz(kr)) << 4);
}
// Row image: row rr of 2 kXK bytes, 16-B chunk c stored at c ^ row_swz(rr). A fragment read of the
// 16x16x32 MFMA (xfrag16) is a ds_read_b128 whose lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31} (+32) touch rows {0-3, 12-15} at chunk c and rows 4-11 at chunk c ^ 1: the
// swizzle (rr >> 2) & 2 puts the four rows of equal rr % 4 on four distinct 16-B bank slots (the
// wide kernel's image; (rr >> 2) & 3, designed for the retired 32x32x16 reads, was 2-way conflicted here:
// SQ_LDS_BANK_CONFLICT 2.6 cycles per LDS instruction). Staging writes (ds_write_b128, 8-lane
// groups over 2 rows) stay conflict-free.
__device__ __forceinline__ int row_swz(int rr) { return (rr >> 2) & 2; }
__device__ __forceinline__ int row_off(int rr, int c) { return rr * (2 * kXK) + ((c ^ row_swz(rr)) << 4); }

// One operand's staging registers (a TR x 32 tile per stage, 256 threads; TR = 128 or 64 rows of m / n).
// Operand formats:
//   fp32  (SP = false): TR / 32 float4 per thread, split into (hi, lo) bf16 while written to LDS;
//   split (SP = true):  two bf16 planes (hi, lo) of the operand's shape, produced once upstream
//                       (rq_split_bf16x3, or a GEMM epilogue): TR / 64 + TR / 64 16-byte chunks per
//                       thread, copied to LDS as they are.
// The LDS images do not depend on TR (a 64-row tile uses the first 64 rows of a row image and the
// first 64 columns of a column image's 256-B rows, with the same swizzles).
// KF ("k full"): every stage of the launch lies inside [k_lo, k_hi) (K and the split-K chunk multiples of
// the stage depth), so no k mask, masked address or zeroing select is emitted.
template <bool KC, bool SP, int TR = 128, bool KF = false>
struct XStage {
  static_assert(TR == 128 || TR == 64, "tile rows");
  // fp32, k-contig: float4 per thread (two per 16-B bf16 chunk of the row image)
  static constexpr int NJ_FK = 2 * TR * kXCPR / 256;
  // fp32, m/n-contig: CT threads across the TR columns (4 each), KR k-rows per pass
  static constexpr int CT_F = TR / 4, KR_F = 256 / CT_F, NJ_FM = kXK / KR_F;
  // split, k-contig: hi + lo 16-B chunks per thread
  static constexpr int NJ_SK = TR * kXCPR / 256;
  // split, m/n-contig: CT threads across the TR columns (8 each), KR k-rows per pass
  static constexpr int CT_S = TR / 8, KR_S = 256 / CT_S, NJ_SM = kXK / KR_S;
  uint4 v[4];
  bool ok[4];   // k of the loaded vector < k_hi (else it read k_lo and is zeroed at store time)

  // rows [r0, r0 + TR) of the operand (clamped to R - 1: they feed only outputs >= R, never
  // written); k in [kb, kb + 32), positions >= k_hi read k_lo and are zeroed at store time. Every
  // load is unconditional and its address branch-free (a select), so the compiler can count the
  // loads in flight statically: with separate full-stage / masked-stage load paths it merged the
  // paths' counts and waited vmcnt(0) at the top of every k iteration, draining the prefetch.
  __device__ __forceinline__ void load(const void* __restrict__ Xv, const void* __restrict__ Xlv, int64_t ld, int r0,
                                       int R, int64_t kb, int64_t k_lo, int64_t k_hi, int tid) {
    if constexpr (!SP) {
      const float* __restrict__ X = static_cast<const float*>(Xv);
      if constexpr (KC) {   // thread: chunk tid % CPR of rows tid / CPR (+ 256 / CPR), 2 float4 per chunk
#pragma unroll
        for (int j = 0; j < NJ_FK; ++j) {
          const int64_t row = min(r0 + (tid / kXCPR) + (256 / kXCPR) * (j >> 1), R - 1);
          const int64_t k = kb + (tid % kXCPR) * 8 + 4 * (j & 1);
          ok[j] = KF || k < k_hi;
          v[j] = *reinterpret_cast<const uint4*>(X + row * ld + (ok[j] ? k : k_lo));
        }
      } else {              // thread: 4 consecutive rows 4 (tid % CT), k rows tid / CT + KR j
        const int64_t col = min(r0 + 4 * (tid % CT_F), R - 4);
#pragma unroll
        for (int j = 0; j < NJ_FM; ++j) {
          const int64_t k = kb + (tid / CT_F) + KR_F * j;
          ok[j] = KF || k < k_hi;
          v[j] = *reinterpret_cast<const uint4*>(X + (ok[j] ? k : k_lo) * ld + col);
        }
      }
    } else {
      const uint16_t* __restrict__ Xh = static_cast<const uint16_t*>(Xv);
      const uint16_t* __restrict__ Xl = static_cast<const uint16_t*>(Xlv);
      if constexpr (KC) {   // thread: chunk tid % CPR of rows tid / CPR (+ 256 / CPR)
#pragma unroll
        for (int j = 0; j < NJ_SK; ++j) {
          const int64_t row = min(r0 + (tid / kXCPR) + (256 / kXCPR) * j, R - 1);
          const int64_t k = kb + (tid % kXCPR) * 8;
          ok[j] = KF || k < k_hi;
          const int64_t o = row * ld + (ok[j] ? k : k_lo);
          v[j] = *reinterpret_cast<const uint4*>(Xh + o);
          v[2 + j] = *reinterpret_cast<const uint4*>(Xl + o);
        }
      } else {              // thread: 8 consecutive rows 8 (tid % CT), k rows tid / CT + KR j
        const int64_t col = min(r0 + 8 * (tid % CT_S), R - 8);
#pragma unroll
        for (int j = 0; j < NJ_SM; ++j) {
          const int64_t k = kb + (tid / CT_S) + KR_S * j;
          ok[j] = KF || k < k_hi;
          const int64_t o = (ok[j] ? k : k_lo) * ld + col;
          v[j] = *reinterpret_cast<const uint4*>(Xh + o);
          v[2 + j] = *reinterpret_cast<const uint4*>(Xl + o);
        }
      }
    }
  }

  __device__ __forceinline__ void store(char* hi_plane, char* lo_plane, int tid) const {
    if constexpr (!SP) {
      constexpr int NJ = KC ? NJ_FK : NJ_FM;
      float4 w[4];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 f = __builtin_bit_cast(float4, v[j]);
        const bool k = ok[j];
        w[j] = make_float4(k ? f.x : 0.f, k ? f.y : 0.f, k ? f.z : 0.f, k ? f.w : 0.f);
      }
      if constexpr (KC) {
#pragma unroll
        for (int c2 = 0; c2 < NJ_FK / 2; ++c2) {
          const int rr = (tid / kXCPR) + (256 / kXCPR) * c2, c = tid % kXCPR;
          const int off = row_off(rr, c);
          uint4 h, l;
          split_bf16x2(w[2 * c2].x, w[2 * c2].y, h.x, l.x);
          split_bf16x2(w[2 * c2].z, w[2 * c2].w, h.y, l.y);
          split_bf16x2(w[2 * c2 + 1].x, w[2 * c2 + 1].y, h.z, l.z);
          split_bf16x2(w[2 * c2 + 1].z, w[2 * c2 + 1].w, h.w, l.w);
          *reinterpret_cast<uint4*>(hi_plane + off) = h;
          *reinterpret_cast<uint4*>(lo_plane + off) = l;
        }
      } else {
        const int m = 4 * (tid % CT_F);
#pragma unroll
        for (int j = 0; j < NJ_FM; ++j) {
          const int kr = (tid / CT_F) + KR_F * j;
          const int off = col_off<TR>(kr, m >> 3) + (((m >> 2) & 1) << 3);
          uint2 h, l;
          split_bf16x2(w[j].x, w[j].y, h.x, l.x);
          split_bf16x2(w[j].z, w[j].w, h.y, l.y);
          *reinterpret_cast<uint2*>(hi_plane + off) = h;
          *reinterpret_cast<uint2*>(lo_plane + off) = l;
        }
      }
    } else {
      constexpr int NJ = KC ? NJ_SK : NJ_SM;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bool k = ok[j];
        const uint4 h0 = v[j], l0 = v[2 + j];
        const uint4 h = make_uint4(k ? h0.x : 0u, k ? h0.y : 0u, k ? h0.z : 0u, k ? h0.w : 0u);
        const uint4 l = make_uint4(k ? l0.x : 0u, k ? l0.y : 0u, k ? l0.z : 0u, k ? l0.w : 0u);
        int off;
        if constexpr (KC) {
          const int rr = (tid / kXCPR) + (256 / kXCPR) * j, c = tid % kXCPR;
          off = row_off(rr, c);
        } else {
          const int kr = (tid / CT_S) + KR_S * j;
          off = col_off<TR>(kr, tid % CT_S);
        }
        *reinterpret_cast<uint4*>(hi_plane + off) = h;
        *reinterpret_cast<uint4*>(lo_plane + off) = l;
      }
    }
  }
};

// 16x16x32 operand fragment (8 bf16: row rb + lane % 16, k = 8 (lane / 16) + 0..7 of the stage).
template <bool KC, int TR = 128>
__device__ __forceinline__ bf16x8_t xfrag16(const char* plane, int rb, int lane) {
  if constexpr (KC) {
    const int rr = rb + (lane & 15), c = lane >> 4;
    return *reinterpret_cast<const bf16x8_t*>(plane + row_off(rr, c));
  } else {
    // ds_read_b64_tr_b16 per 16-lane group G (k-rows 8G .. 8G + 7 in two 4-row blocks): lane
    // 4q + p supplies the address of k-row q, rows 4p..4p+3, and receives row (lane % 16).
    const int G = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int m = rb + 4 * p;
    s16x4_t t[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kr = 8 * G + 4 * u + q;
      const int off = col_off<TR>(kr, m >> 3) + (((m >> 2) & 1) << 3);
      t[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4_t*)(plane + off));
    }
    typedef short s16x8_t __attribute__((ext_vector_type(8)));
    const s16x8_t r = {t[0].x, t[0].y, t[0].z, t[0].w, t[1].x, t[1].y, t[1].z, t[1].w};
    return __builtin_bit_cast(bf16x8_t, r);
  }
}

// The epilogue codes (X3Epi: kEpiStore, kEpiSiluFwd, kEpiSiluBwd, kEpiAdd) are gemm_plan.h's.
struct X3Epilogue {
  const float* Z;    // kEpiSiluBwd: pre-activations (ld = ldc)
  uint16_t* Hh;      // split output planes (ld = ldh)
  uint16_t* Hl;
  int64_t ldh;
  uint32_t thr;      // dropout threshold (0 = none) and scale
  float scale;
  uint64_t seed;
  int acc;           // kEpiStore, unsplit: C += A B^T (an accumulating call without the slab reduction)
};

// Epilogue SiLU on the hardware exp / reciprocal (v_exp_f32, v_rcp_f32: ~1 ulp each) instead of
// the IEEE expf + division of the standalone kernels (dropout.hip): the result is split to bf16
// planes at ~2^-17 right after, so the last bits do not survive anyway, and the epilogue VALU drops
// ~3x. s = sigmoid(z) = 1 / (1 + 2^(-z log2 e)).
__device__ __forceinline__ float sigmoid_fast(float z) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * z));
}

// Epilogue stores; NT: non-temporal (the wide kernel's all-CU write bursts)
typedef unsigned ux4_t __attribute__((ext_vector_type(4)));
typedef unsigned ux2_t __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ void epi_st16(void* p, float4 v) {
  if constexpr (NT) __builtin_nontemporal_store(__builtin_bit_cast(ux4_t, v), reinterpret_cast<ux4_t*>(p));
  else *reinterpret_cast<float4*>(p) = v;
}
template <bool NT>
__device__ __forceinline__ void epi_st8(void* p, uint2 v) {
  if constexpr (NT) __builtin_nontemporal_store(__builtin_bit_cast(ux2_t, v), reinterpret_cast<ux2_t*>(p));
  else *reinterpret_cast<uint2*>(p) = v;
}

// What the epilogue of lane quad (m, n .. n + 3) reads besides the accumulators: Z (SiLU', residual add) or,
// for an accumulating plain store, the current C quad; zeros otherwise. Loaded for a whole group of quads
// before any of their stores (x3_epi4z): the output pointers may alias Z for the compiler, so a load written
// after a store waits for that store and its own round trip, one quad at a time.
template <int EPI>
__device__ __forceinline__ float4 x3_epi_in(int m, int n, float* __restrict__ Cs, int64_t ldc, const X3Epilogue& ep) {
  if constexpr (EPI == kEpiSiluBwd || EPI == kEpiAdd) {
    return *reinterpret_cast<const float4*>(ep.Z + (int64_t)m * ldc + n);
  } else if constexpr (EPI == kEpiStore) {
    if (ep.acc) return *reinterpret_cast<const float4*>(Cs + (int64_t)m * ldc + n);
  }
  return make_float4(0.f, 0.f, 0.f, 0.f);
}

// Epilogue of one lane quad C[m][n .. n + 3] = v (fp32 accumulator values) with its input quad z
// (x3_epi_in); Cs = the split-K slab (kEpiStore) or C itself.
template <int EPI, bool DROP, bool NT = false>
__device__ __forceinline__ void x3_epi4z(const float4 v, const float4 z, int m, int n, int N, float* __restrict__ C,
                                         float* __restrict__ Cs, int64_t ldc, const X3Epilogue& ep) {
  if constexpr (EPI == kEpiStore) {
    float4* c = reinterpret_cast<float4*>(Cs + (int64_t)m * ldc + n);
    if (ep.acc) {   // fixed order c + v: bitwise the slab reduction's C[j] + P[0][j]
      const float4 o = z;
      epi_st16<NT>(c, make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w));
    } else {
      epi_st16<NT>(c, v);
    }
  } else if constexpr (EPI == kEpiAdd) {
    const float4 r = z;
    if constexpr (DROP) {   // C = Z + Dropout(A B^T): dropout_add_fwd's mask (element m N + n) and arithmetic
      const uint64_t e = (uint64_t)m * N + n;
      float d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = keep1(ep.seed, e + j, ep.thr) ? ep.scale : 0.f;
      epi_st16<NT>(C + (int64_t)m * ldc + n, make_float4(r.x + v.x * d[0], r.y + v.y * d[1], r.z + v.z * d[2], r.w + v.w * d[3]));
    } else {
      epi_st16<NT>(C + (int64_t)m * ldc + n, make_float4(v.x + r.x, v.y + r.y, v.z + r.z, v.w + r.w));
    }
  } else {
    const uint64_t e = (uint64_t)m * N + n;
    float d[4] = {1.f, 1.f, 1.f, 1.f};   // dropout multipliers (0 or 1 / (1 - p))
    if constexpr (DROP) {
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = keep1(ep.seed, e + j, ep.thr) ? ep.scale : 0.f;
    }
    float4 o;
    if constexpr (EPI == kEpiSiluFwd) {
      epi_st16<NT>(C + (int64_t)m * ldc + n, v);
      o = make_float4(v.x * sigmoid_fast(v.x) * d[0], v.y * sigmoid_fast(v.y) * d[1], v.z * sigmoid_fast(v.z) * d[2],
                      v.w * sigmoid_fast(v.w) * d[3]);
    } else {   // silu'(z) g = g s (1 + z (1 - s)), g = Dropout(A B^T)
      const float sx = sigmoid_fast(z.x), sy = sigmoid_fast(z.y), sz = sigmoid_fast(z.z), sw = sigmoid_fast(z.w);
      o = make_float4(v.x * d[0] * sx * (1.f + z.x * (1.f - sx)), v.y * d[1] * sy * (1.f + z.y * (1.f - sy)),
                      v.z * d[2] * sz * (1.f + z.z * (1.f - sz)), v.w * d[3] * sw * (1.f + z.w * (1.f - sw)));
    }
    uint2 hi, lo;
    split_bf16x2(o.x, o.y, hi.x, lo.x);
    split_bf16x2(o.z, o.w, hi.y, lo.y);
    epi_st8<NT>(ep.Hh + (int64_t)m * ep.ldh + n, hi);
    epi_st8<NT>(ep.Hl + (int64_t)m * ep.ldh + n, lo);
  }
}

template <int EPI, bool DROP, bool NT = false>
__device__ __forceinline__ void x3_epi4(const float4 v, int m, int n, int N, float* __restrict__ C,
                                        float* __restrict__ Cs, int64_t ldc, const X3Epilogue& ep) {
  x3_epi4z<EPI, DROP, NT>(v, x3_epi_in<EPI>(m, n, Cs, ldc, ep), m, n, N, C, Cs, ldc, ep);
}

__device__ __forceinline__ void split_store1(float v, uint16_t* hi, uint16_t* lo) {
  const __bf16 h = (__bf16)v;
  *hi = __builtin_bit_cast(uint16_t, h);
  *lo = __builtin_bit_cast(uint16_t, (__bf16)(v - (float)h));
}

// One LDS stage of MFMA work per wave. Transposed product D = B A^T (tile rows = n, columns = m):
// each lane then holds consecutive n of one row m, so the epilogue stores vectors.
#define RQ_X3_MMA                                                                                             \
  {                                                                                                           \
    bf16x8_t fa_h[kP], fa_l[kP], fb_h[kP], fb_l[kP];                                                          \
    _Pragma("unroll") for (int p = 0; p < kP; ++p) {                                                          \
      fa_h[p] = xfrag16<AKC, TS>(ah, wm * kWTile + 16 * p, lane);                                             \
      fa_l[p] = xfrag16<AKC, TS>(al, wm * kWTile + 16 * p, lane);                                             \
      fb_h[p] = xfrag16<BKC, TS>(bh, wn * kWTile + 16 * p, lane);                                             \
      fb_l[p] = xfrag16<BKC, TS>(bl, wn * kWTile + 16 * p, lane);                                             \
    }                                                                                                         \
    _Pragma("unroll") for (int p = 0; p < kP; ++p) _Pragma("unroll") for (int q = 0; q < kP; ++q) {          \
      acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_h[q], fa_l[p], acc[p][q], 0, 0, 0);              \
      acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_l[q], fa_h[p], acc[p][q], 0, 0, 0);              \
      acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_h[q], fa_h[p], acc[p][q], 0, 0, 0);              \
    }                                                                                                         \
  }

// One launch's problem (operands, shape, plan, output, epilogue): the kernel argument of the 128-/64-tile
// kernel and of the paired launch (gemm_x3_pair_kernel) that runs two problems' workgroups in one grid.
struct X3Args {
  const void* A;
  const void* Al;
  int64_t lda;
  const void* B;
  const void* Bl;
  int64_t ldb;
  int M, N;
  int64_t K;
  int tiles_n, tiles, S;
  int64_t chunk;
  int per;
  float* C;
  int64_t ldc;
  X3Epilogue ep;
  int kf;   // 1: K and chunk are multiples of kXK (the unmasked staging path)
};

// LDS bytes of one plane of the TS-tile form (the 64-tile form's compact images: half of every plane)
template <int TS>
constexpr int x3_plane_bytes() { return TS == 64 ? kXPlane / 2 : kXPlane; }

// TS = output tile (128, or 64 for launches whose 128-tiles cannot fill the chip: the decoder's 1,280
// future-token rows): 4 waves of (TS / 2)^2 outputs, the same k order (so the same result) either way.
// The body of one workgroup `bid` of problem `a` over the LDS block `lds` (8 planes).
template <bool AKC, bool ASP, bool BKC, bool BSP, int EPI, bool DROP, int TS, bool KF>
__device__ __forceinline__ void x3_body_k(const X3Args& a, int bid, char* __restrict__ lds) {
  const void* __restrict__ A = a.A;
  const void* __restrict__ Al = a.Al;
  const void* __restrict__ B = a.B;
  const void* __restrict__ Bl = a.Bl;
  const int64_t lda = a.lda, ldb = a.ldb, K = a.K, chunk = a.chunk, ldc = a.ldc;
  const int M = a.M, N = a.N, tiles_n = a.tiles_n, tiles = a.tiles, S = a.S, per = a.per;
  float* __restrict__ C = a.C;
  X3Epilogue ep = a.ep;
  ep.seed = epoch_seed(ep.seed);
  constexpr int kPl = x3_plane_bytes<TS>();
  const int lw = (bid & 7) * per + (bid >> 3);   // XCD-major: neighbours (same A rows / same k chunk) share an L2
  if (lw >= tiles * S) return;
  const int s = lw / tiles, t = lw % tiles;
  const int m0 = (t / tiles_n) * TS, n0 = (t % tiles_n) * TS;
  static_assert(TS == 128 || TS == 64, "output tile");
  constexpr int kWTile = TS / 2, kP = TS / 32;   // per-wave tile, 16-row MFMA tiles per wave side
  const int64_t k_lo = (int64_t)s * chunk;
  const int64_t k_hi = k_lo + chunk < K ? k_lo + chunk : K;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;

  floatx4v acc[kP][kP];
#pragma unroll
  for (int p = 0; p < kP; ++p)
#pragma unroll
    for (int q = 0; q < kP; ++q) acc[p][q] = floatx4v{0.f, 0.f, 0.f, 0.f};

  auto plane = [&](int buf, int op, int hl) { return lds + buf * 4 * kPl + op * 2 * kPl + hl * kPl; };
  const int nst = (int)((k_hi - k_lo + kXK - 1) / kXK);
  // Two register stage sets: stage st + 2 is loaded while stage st is multiplied and stage st + 1
  // (loaded earlier) is written to the other LDS buffer, so each load has two stages of MFMA work to
  // land in (HBM latency under load is ~2-4k cycles, one 128-tile stage ~1.5k; a 64-tile stage is 4x
  // less MFMA work, and measured within 3 % at 2, 3 and 4 sets, so both forms keep 2).
  constexpr int kDepth = 2;
  XStage<AKC, ASP, TS, KF> sa0, sa1;
  XStage<BKC, BSP, TS, KF> sb0, sb1;
  sa0.load(A, Al, lda, m0, M, k_lo, k_lo, k_hi, tid);
  sb0.load(B, Bl, ldb, n0, N, k_lo, k_lo, k_hi, tid);
  sa1.load(A, Al, lda, m0, M, k_lo + (int64_t)min(1, nst - 1) * kXK, k_lo, k_hi, tid);
  sb1.load(B, Bl, ldb, n0, N, k_lo + (int64_t)min(1, nst - 1) * kXK, k_lo, k_hi, tid);
  sa0.store(plane(0, 0, 0), plane(0, 0, 1), tid);
  sb0.store(plane(0, 1, 0), plane(0, 1, 1), tid);
  __syncthreads();

#define RQ_X3_STAGE(ST, LA, LB, SA, SB)                                                                       \
  {                                                                                                           \
    const int st_ = (ST), buf = st_ & 1;                                                                      \
    {  /* unconditional (past the end: the last stage again, an L2 hit) so vmcnt counts stay static */       \
      const int64_t kb = k_lo + (int64_t)min(st_ + kDepth, nst - 1) * kXK;                                    \
      LA.load(A, Al, lda, m0, M, kb, k_lo, k_hi, tid);                                                        \
      LB.load(B, Bl, ldb, n0, N, kb, k_lo, k_hi, tid);                                                        \
    }                                                                                                         \
    const char* ah = plane(buf, 0, 0);                                                                        \
    const char* al = plane(buf, 0, 1);                                                                        \
    const char* bh = plane(buf, 1, 0);                                                                        \
    const char* bl = plane(buf, 1, 1);                                                                        \
    RQ_X3_MMA                                                                                                 \
    SA.store(plane(buf ^ 1, 0, 0), plane(buf ^ 1, 0, 1), tid);                                                \
    SB.store(plane(buf ^ 1, 1, 0), plane(buf ^ 1, 1, 1), tid);                                                \
    __syncthreads();                                                                                          \
  }
  // Stage body: the MFMAs on buffer buf, then the write of the next stage's registers into buf ^ 1
  // (free since the previous barrier; unconditional: past the last stage it writes a buffer nobody
  // reads, and a conditional store would leave the set's loads possibly pending, so the compiler
  // would wait vmcnt(0) before reloading it).
  // Set j % 2 holds stage j: after multiplying stage st its set is reloaded with st + 2. The loop is
  // peeled so that every stage slot multiplies (no runtime test around the MFMAs).
  int st = 0;
  for (; st + 1 < nst; st += 2) {
    RQ_X3_STAGE(st, sa0, sb0, sa1, sb1)
    RQ_X3_STAGE(st + 1, sa1, sb1, sa0, sb0)
  }
  if (st < nst) RQ_X3_STAGE(st, sa0, sb0, sa1, sb1)
#undef RQ_X3_STAGE
#undef RQ_X3_MMA

  // Each lane stores C[m][n .. n + 3] quads: 16-B fp32 / 8-B bf16 stores (N % 4 == 0).
  float* Cs = C + (int64_t)s * M * N;   // split-K partial slab (S > 1: ldc == N)
  // 16x16 C/D map of D = B A^T: column (lane & 15) = m, row 4 (lane >> 4) + j = n (j = register).
  auto quad_m = [&](int p) { return m0 + wm * kWTile + 16 * p + (lane & 15); };
  auto quad_n = [&](int q) { return n0 + wn * kWTile + 16 * q + 4 * (lane >> 4); };
  // the SiLU' epilogue's Z quads for every quad first: one round trip, not one per quad (the residual add
  // keeps its per-quad reads: preloaded it measured 2 us slower per decoder launch, profiles/r06/epi_z)
  constexpr bool kZ = EPI == kEpiSiluBwd;
  float4 zin[kP][kP];
#pragma unroll
  for (int p = 0; p < kP; ++p)
#pragma unroll
    for (int q = 0; q < kP; ++q) {
      const int m = quad_m(p), n = quad_n(q);
      zin[p][q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kZ && m < M && n < N) zin[p][q] = x3_epi_in<EPI>(m, n, Cs, ldc, ep);
    }
#pragma unroll
  for (int p = 0; p < kP; ++p) {
    const int m = quad_m(p);
    if (m < M) {
#pragma unroll
      for (int q = 0; q < kP; ++q)
        // A one-trip loop (a leftover of the 32x32 accumulator map's four register quads per tile): without
        // it hipcc schedules these kernels differently, and the generated code is pinned by measurement.
#pragma unroll
        for (int g = 0; g < 1; ++g) {
          const int n = quad_n(q);
          const float4 v = make_float4(acc[p][q][0], acc[p][q][1], acc[p][q][2], acc[p][q][3]);
          if (n >= N) continue;
          if constexpr (kZ) x3_epi4z<EPI, DROP>(v, zin[p][q], m, n, N, C, Cs, ldc, ep);
          else x3_epi4<EPI, DROP>(v, m, n, N, C, Cs, ldc, ep);
        }
    }
  }
}

// The body with the staging path picked once per workgroup (uniform): unmasked when every stage is full.
template <bool AKC, bool ASP, bool BKC, bool BSP, int EPI, bool DROP, int TS>
__device__ __forceinline__ void x3_body(const X3Args& a, int bid, char* __restrict__ lds) {
  if (a.kf)
    x3_body_k<AKC, ASP, BKC, BSP, EPI, DROP, TS, true>(a, bid, lds);
  else
    x3_body_k<AKC, ASP, BKC, BSP, EPI, DROP, TS, false>(a, bid, lds);
}

template <bool AKC, bool ASP, bool BKC, bool BSP, int EPI, bool DROP = false, int TS = 128>
__global__ void __launch_bounds__(256, TS == 64 ? kXWG64 : kXWG) gemm_bf16x3_kernel(X3Args a) {
  __shared__ __attribute__((aligned(16))) char lds[8 * x3_plane_bytes<TS>()];
  x3_body<AKC, ASP, BKC, BSP, EPI, DROP, TS>(a, blockIdx.x, lds);
}

// Two problems in ONE launch: workgroups [0, n1) run problem 1, the rest problem 2 (each with its own
// XCD-major tile order and plan). The backward's data-gradient and weight-gradient GEMMs of a Linear are
// independent; one launch instead of two saves a launch and lets the pair fill the chip together (the
// decoder's 1,280-row launches fill 160..480 of 1,024 slots each; the 11,332-row data gradients 356 of 512).
// P1 / P2: x3_body instantiations (X3Body<form..., TS>); both the same tile size.
template <bool AKC, bool ASP, bool BKC, bool BSP, int EPI, bool DROP, int TS>
struct X3Body {
  static constexpr int kTS = TS;
  __device__ __forceinline__ static void run(const X3Args& a, int bid, char* lds) {
    x3_body<AKC, ASP, BKC, BSP, EPI, DROP, TS>(a, bid, lds);
  }
};

template <class P1, class P2>
__global__ void __launch_bounds__(256, P1::kTS == 64 ? kXWG64 : kXWG) gemm_x3_pair_kernel(X3Args a1, X3Args a2, int n1) {
  static_assert(P1::kTS == P2::kTS, "paired problems share the tile size");
  __shared__ __attribute__((aligned(16))) char lds[8 * x3_plane_bytes<P1::kTS>()];
  const int bid = blockIdx.x;
  if (bid < n1)
    P1::run(a1, bid, lds);
  else
    P2::run(a2, bid - n1, lds);
}

// ---------------------------------------------------------------------------------------------
// Wide split-bf16 GEMM ("x3w"): 256 x 256 output tile per workgroup, 8 waves (2 along m x 4
// along n, 128 x 64 outputs each), both operands already split into bf16 planes. The operand tile
// of one 32-deep k step is four "halves" (A rows 0-127 / 128-255, B rows 0-127 / 128-255), each a
// hi and a lo plane of 8 KiB: a row image for a k-contiguous operand (64-B rows, 16-B chunk c of
// row r at c ^ ((r >> 2) & 2): conflict-free for the 16x16x32 fragment's ds_read_b128 lane
// groups), else the column image of gemm_bf16x3_kernel read by ds_read_b64_tr_b16. A (the
// streamed activation: HBM / Infinity-Cache misses) has THREE k-step slots, B (the weights, L2
// hits) two: 3 x 32 + 2 x 32 KiB = 160 KiB, the whole LDS, one workgroup per CU.
//
// Staging is LDS-DMA (buffer_load_dwordx4 ... lds: no VGPR round trip; the images' XOR swizzles go on
// the per-lane SOURCE address, the LDS side stays lane-linear: wave w fills bytes [1 KiB w,
// 1 KiB (w + 1)) of every half-plane). A k step is four phases, one per C quadrant of the wave
// (A half h x B half g), in the order (0,0) (0,1) (1,1) (1,0); reads: A0 + B0 (phase 0), B1 (1),
// A1 (2), none (3: B0 kept in registers). Phase p of step t issues, 2 DMA instructions per wave
// each, B0 (t + 1), B1 (t + 1), A0 (t + 2), A1 (t + 2): A lands 5-7 phases after issue, B in 4,
// and since vmcnt retires in issue order, B issued after A never waits on A's misses early. The
// only waits are a counted vmcnt(6) (three halves left in flight) at the end of phases 3 and 0;
// phase 2's A1 was retired by phase 0's. Never vmcnt(0) inside the loop. The two wave groups
// (waves 0-3 / 4-7: one of each per SIMD) run staggered by one barrier with two barriers per
// phase, so on every SIMD one wave issues its LDS reads and DMAs while the other runs its 24
// MFMAs. Ordering rules:
//  * RAW: data read in phase f is retired (each wave's own vmcnt) before the barrier that ends
//    the interval BEFORE either group's read interval of phase f: group 0 waits at the end of its
//    MFMA interval of phase f - 1, group 1 (one interval behind) at the end of its read interval;
//  * WAR: a DMA overwrites a slot last read >= 3 phases earlier (A: step t - 1's copy; B: step
//    t - 1's), those reads retired by lgkmcnt(0) before their phase's MFMAs.
// Per k step and wave: 24 ds_read_b128 / tr reads, 8 DMA instructions, 96 MFMAs (16x16x32 bf16).
// The accumulation order over k equals gemm_bf16x3_kernel's (same 32-deep steps, same product
// order), so for the same split the two kernels agree bitwise.
// ---------------------------------------------------------------------------------------------
constexpr int kWH = 8192;          // one half-plane: 128 rows x 32 k bf16
static_assert(kWH == (kWT2 / 2) * kWK * 2, "gemm_plan.h: the wide kernel's tile (kWT2) and k step (kWK)");
constexpr int kWStep = 4 * kWH;    // one operand's k step: 2 halves x 2 planes
constexpr int kWB0 = 3 * kWStep;   // B's slots follow A's three
constexpr int kWLds = 5 * kWStep;  // 160 KiB

__device__ __forceinline__ int wrow_swz(int r) { return (r >> 2) & 2; }

// Element offset (from the k step's base) of the 16 bytes lane `lane` of wave `wave` DMAs into its
// slot of a half-plane image whose first row (m or n) is r0.
template <bool KC>
__device__ __forceinline__ int64_t x3w_src(int64_t ld, int r0, int R, int wave, int lane) {
  if constexpr (KC) {   // row image: 16 rows x 4 chunks per 1 KiB; position c holds k-chunk c ^ swz
    const int row = 16 * wave + (lane >> 2);
    const int kc = (lane & 3) ^ wrow_swz(row);
    return (int64_t)min(r0 + row, R - 1) * ld + 8 * kc;
  } else {              // column image: 4 k-rows x 16 chunks per 1 KiB; position c holds m-chunk c ^ col_swz
    const int kr = 4 * wave + (lane >> 4);
    const int mc = (lane & 15) ^ col_swz(kr);
    return (int64_t)kr * ld + min(r0 + 8 * mc, R - 8);
  }
}

// 16x16x32 operand fragment of a wide-kernel half-plane (row rb + lane % 16, k = 8 (lane / 16) + 0..7).
template <bool KC>
__device__ __forceinline__ bf16x8_t wfrag16(const char* plane, int rb, int lane) {
  if constexpr (KC) {
    const int rr = rb + (lane & 15), c = lane >> 4;
    return *reinterpret_cast<const bf16x8_t*>(plane + rr * 64 + ((c ^ wrow_swz(rr)) << 4));
  } else {
    return xfrag16<false>(plane, rb, lane);
  }
}

#define RQ_W_BAR() __builtin_amdgcn_s_barrier()
#define RQ_W_VM6() asm volatile("s_waitcnt vmcnt(6)" ::: "memory")
#define RQ_W_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// bijective XCD-major remap of the grid: consecutive work items (same A rows, same k chunk) share an L2
__device__ __forceinline__ int x3w_work_item() {
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = bid & 7;
  return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
}

// One workgroup's share of one problem: work item lw (k chunk lw / tiles, output tile lw % tiles). The body
// of gemm_x3w_kernel (lw over its own grid) and of gemm_x3w_group_kernel (lw within the workgroup's problem).
// The __restrict__ parameters matter: inlined, they give the LDS-DMA writes and the fragment reads alias scopes,
// without which hipcc (ROCm 7.2) puts a vmcnt(0) before each batch of column-image (m/n-contiguous operand)
// fragment reads — 2 per k step with one such operand, 3 with two, none for k-contiguous x k-contiguous —
// draining the DMAs that the counted vmcnt(6) waits leave in flight; so it did while the body stood in the
// kernel, and does again with the qualifiers removed. Nothing pins this to a compiler version: after a change
// check every instantiation's loop with tools/asm_sync.py (profiles/r07/group_wgrad/README.md).
template <bool AKC, bool BKC, int EPI, bool DROP>
__device__ __forceinline__ void
x3w_body(const uint16_t* __restrict__ Ah, const uint16_t* __restrict__ Al, int64_t lda,
         const uint16_t* __restrict__ Bh, const uint16_t* __restrict__ Bl, int64_t ldb, int M, int N, int64_t K,
         int tiles_n, int tiles, int64_t chunk, float* __restrict__ C, int64_t ldc, X3Epilogue ep, int lw) {
  __shared__ __attribute__((aligned(16))) char lds[kWLds];   // the kernel's only LDS object (DMA waits)
  const int s = lw / tiles, t = lw - s * tiles;
  const int m0 = (t / tiles_n) * kWT2, n0 = (t % tiles_n) * kWT2;
  const int64_t k_lo = (int64_t)s * chunk;
  const int64_t k_hi = k_lo + chunk < K ? k_lo + chunk : K;
  const int nk = (int)((k_hi - k_lo) >> 5);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const bool g1 = wr != 0;   // the second wave group, staggered one barrier behind the first

  const int64_t da = AKC ? 32 : 32 * lda, db = BKC ? 32 : 32 * ldb;
  const int64_t ka = AKC ? k_lo : k_lo * lda, kb = BKC ? k_lo : k_lo * ldb;
  const int64_t oa0 = ka + x3w_src<AKC>(lda, m0, M, wave, lane), oa1 = ka + x3w_src<AKC>(lda, m0 + 128, M, wave, lane);
  const int64_t ob0 = kb + x3w_src<BKC>(ldb, n0, N, wave, lane), ob1 = kb + x3w_src<BKC>(ldb, n0 + 128, N, wave, lane);
  char* const wl = lds + 1024 * wave;
  // A half h of k step `step` into A slot `slot`; B half g of step `step` into B parity step & 1.
  // Steps past the end are clamped (the last step again, into a slot nobody reads), so every wave
  // issues the same DMA count in every phase and the vmcnt counts stay static.
  // The DMA is buffer_load ... lds (an SGPR descriptor + a 32-bit byte offset: 1-2.5 % faster than
  // global_load_lds with 64-bit per-lane addresses, profiles/r06/gemm_diag). The descriptors are based at
  // the workgroup's first A / B row (k-contiguous) or first k row (m/n-contiguous): every offset below is
  // then < x3w_span() elements, which x3_prepare keeps under 2^30 (32-bit byte offsets)
  const int64_t abase = AKC ? (int64_t)m0 * lda : k_lo * lda, bbase = BKC ? (int64_t)n0 * ldb : k_lo * ldb;
  const __amdgpu_buffer_rsrc_t rah = __builtin_amdgcn_make_buffer_rsrc((void*)(Ah + abase), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t ral = __builtin_amdgcn_make_buffer_rsrc((void*)(Al + abase), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rbh = __builtin_amdgcn_make_buffer_rsrc((void*)(Bh + bbase), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rbl = __builtin_amdgcn_make_buffer_rsrc((void*)(Bl + bbase), (short)0, 0x7fffffff, 0x00020000);
  auto bdma = [](__amdgpu_buffer_rsrc_t r, int64_t rel, char* dst) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, (int)(rel * 2), 0, 0, 0);
  };
  auto issue_a = [&](int h, int step, int slot) {
    const int sa = step < nk ? step : nk - 1;
    const int64_t o = (h == 0 ? oa0 : oa1) + (int64_t)sa * da;
    char* dst = wl + slot * kWStep + h * 2 * kWH;
    bdma(rah, o - abase, dst);
    bdma(ral, o - abase, dst + kWH);
  };
  auto issue_b = [&](int g, int step) {
    const int sb = step < nk ? step : nk - 1;
    const int64_t o = (g == 0 ? ob0 : ob1) + (int64_t)sb * db;
    char* dst = wl + kWB0 + (step & 1) * kWStep + g * 2 * kWH;
    bdma(rbh, o - bbase, dst);
    bdma(rbl, o - bbase, dst + kWH);
  };
  auto aplane = [&](int slot, int h, int pl) -> const char* { return lds + slot * kWStep + (h * 2 + pl) * kWH; };
  auto bplane = [&](int par, int g, int pl) -> const char* {
    return lds + kWB0 + par * kWStep + (g * 2 + pl) * kWH;
  };

  floatx4v acc[2][2][4][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[h][g][i][j] = floatx4v{0.f, 0.f, 0.f, 0.f};
  bf16x8_t fah[4], fal[4], fb0h[2], fb0l[2], fb1h[2], fb1l[2];

#define RQ_W_READ_A(SLOT, H)                                                                   \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                              \
    fah[i] = wfrag16<AKC>(aplane(SLOT, H, 0), wr * 64 + 16 * i, lane);                         \
    fal[i] = wfrag16<AKC>(aplane(SLOT, H, 1), wr * 64 + 16 * i, lane);                         \
  }
#define RQ_W_READ_B(PAR, G, BH, BL)                                                            \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                              \
    BH[j] = wfrag16<BKC>(bplane(PAR, G, 0), wc * 32 + 16 * j, lane);                           \
    BL[j] = wfrag16<BKC>(bplane(PAR, G, 1), wc * 32 + 16 * j, lane);                           \
  }
#define RQ_W_MMA(H, G, BH, BL) /* s_setprio(1) around the cluster keeps hipcc from moving it */ \
  __builtin_amdgcn_s_setprio(1);                                                               \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) { \
    floatx4v& c_ = acc[H][G][i][j];                                                            \
    c_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(BH[j], fal[i], c_, 0, 0, 0);                  \
    c_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(BL[j], fah[i], c_, 0, 0, 0);                  \
    c_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(BH[j], fah[i], c_, 0, 0, 0);                  \
  }                                                                                            \
  __builtin_amdgcn_s_setprio(0);

  // prologue, in the steady state's issue order (A of steps 0 and 1, B of step 0); phase 0 of
  // step 0 needs A0 (0) and B0 (0): B1 (0), A0 (1), A1 (1) may stay in flight
  issue_a(0, 0, 0);
  issue_a(1, 0, 0);
  issue_b(0, 0);
  issue_b(1, 0);
  issue_a(0, 1, 1);
  issue_a(1, 1, 1);
  RQ_W_VM6();
  RQ_W_BAR();
  if (g1) RQ_W_BAR();   // group 1 runs one barrier behind
  int slot = 0;         // A slot of step st (st % 3); step st + 2 goes to (st + 2) % 3
  for (int st = 0; st < nk; ++st) {
    const int par = st & 1, slot2 = slot == 0 ? 2 : slot - 1;
    // phase 0: quadrant (A0, B0)
    RQ_W_READ_A(slot, 0)
    RQ_W_READ_B(par, 0, fb0h, fb0l)
    issue_b(0, st + 1);
    if (g1) RQ_W_VM6();   // B1 (and A1) of this step, for phases 1 and 2
    RQ_W_BAR();
    RQ_W_LGKM0();
    RQ_W_MMA(0, 0, fb0h, fb0l)
    if (!g1) RQ_W_VM6();
    RQ_W_BAR();
    // phase 1: (A0, B1)
    RQ_W_READ_B(par, 1, fb1h, fb1l)
    issue_b(1, st + 1);
    RQ_W_BAR();
    RQ_W_LGKM0();
    RQ_W_MMA(0, 1, fb1h, fb1l)
    RQ_W_BAR();
    // phase 2: (A1, B1)
    RQ_W_READ_A(slot, 1)
    issue_a(0, st + 2, slot2);
    RQ_W_BAR();
    RQ_W_LGKM0();
    RQ_W_MMA(1, 1, fb1h, fb1l)
    RQ_W_BAR();
    // phase 3: (A1, B0) from registers
    issue_a(1, st + 2, slot2);
    if (g1) RQ_W_VM6();   // A0 and B0 of the next step, for its phase 0
    RQ_W_BAR();
    RQ_W_MMA(1, 0, fb0h, fb0l)
    if (!g1) RQ_W_VM6();
    RQ_W_BAR();
    slot = slot == 2 ? 0 : slot + 1;
  }
#undef RQ_W_READ_A
#undef RQ_W_READ_B
#undef RQ_W_MMA
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (!g1) RQ_W_BAR();   // balance group 1's extra barrier

  float* Cs = C + (int64_t)s * M * N;   // split-K partial slab (S > 1: ldc == N)
  // Epilogue through LDS, one 128-row half of the tile at a time (128 KiB): the waves scatter their
  // accumulator quads into a [128][256] fp32 image (16-B chunk c of row r at c ^ (r & 15): the
  // 16 rows of a quad store and the 16 chunks of a row read hit distinct bank groups), then each
  // wave runs the epilogue on 16 whole rows, one 1 KiB row segment per instruction (coalesced
  // stores / Z reads instead of 64-B pieces of 16 rows).
  __syncthreads();   // every wave's DMAs retired (vmcnt(0) above) and its reads done: LDS is free
  float* const img = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int r = wr * 64 + 16 * i + (lane & 15);
          const int c = 32 * g + 8 * wc + 4 * j + (lane >> 4);
          *reinterpret_cast<floatx4v*>(img + r * 256 + 4 * (c ^ (r & 15))) = acc[h][g][i][j];
        }
    const int n = n0 + 4 * lane;
    if constexpr (EPI == kEpiSiluBwd) {
      // the 16 rows' Z quads in flight together, in the registers this half's accumulators just left
      // (x3_epi_in: one round trip instead of one per row)
      float4 zin[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = m0 + 128 * h + wave * 16 + q;
        zin[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < M && n < N) zin[q] = x3_epi_in<EPI>(m, n, Cs, ldc, ep);
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = wave * 16 + q, m = m0 + 128 * h + r;
        const floatx4v a = *reinterpret_cast<const floatx4v*>(img + r * 256 + 4 * (lane ^ (r & 15)));
        if (m < M && n < N)
          x3_epi4z<EPI, DROP, true>(make_float4(a[0], a[1], a[2], a[3]), zin[q], m, n, N, C, Cs, ldc, ep);
      }
    } else {   // store-only epilogues (the accumulating store's C read stays per row: unsplit wide calls only)
      __syncthreads();
#pragma unroll 4
      for (int q = 0; q < 16; ++q) {
        const int r = wave * 16 + q, m = m0 + 128 * h + r;
        const floatx4v a = *reinterpret_cast<const floatx4v*>(img + r * 256 + 4 * (lane ^ (r & 15)));
        if (m < M && n < N) x3_epi4<EPI, DROP, true>(make_float4(a[0], a[1], a[2], a[3]), m, n, N, C, Cs, ldc, ep);
      }
    }
    __syncthreads();
  }
}

template <bool AKC, bool BKC, int EPI, bool DROP>
__global__ void __launch_bounds__(512, 1)
gemm_x3w_kernel(const uint16_t* __restrict__ Ah, const uint16_t* __restrict__ Al, int64_t lda,
                const uint16_t* __restrict__ Bh, const uint16_t* __restrict__ Bl, int64_t ldb, int M, int N, int64_t K,
                int tiles_n, int tiles, int64_t chunk, float* __restrict__ C, int64_t ldc, X3Epilogue ep) {
  ep.seed = epoch_seed(ep.seed);
  x3w_body<AKC, BKC, EPI, DROP>(Ah, Al, lda, Bh, Bl, ldb, M, N, K, tiles_n, tiles, chunk, C, ldc, ep, x3w_work_item());
}

// Several weight-gradient problems (m/n-contiguous split operands, plain store to split-K slabs) in one
// grid: problem p owns work items first[p] .. first[p + 1) of the XCD-remapped grid, tiles[p] x S[p] of
// them, each the single-problem kernel's work item (k chunk, tile) of that problem with that problem's own
// chunk, so every member runs the wide tile over a long k loop on its proportional share of the chip.
struct X3WProb {
  const uint16_t* Ah;
  const uint16_t* Al;
  int64_t lda;
  const uint16_t* Bh;
  const uint16_t* Bl;
  int64_t ldb;
  int64_t K, chunk;
  float* slabs;   // S slabs of M x N fp32 (ld = N)
  int M, N, tiles_n, tiles, S, pad;
};
struct X3WGroup {
  X3WProb p[kX3GroupMax];
  int first[kX3GroupMax + 1];
  int count;
};

__global__ void __launch_bounds__(512, 1) gemm_x3w_group_kernel(X3WGroup g) {
  const int lw = x3w_work_item();
  int e = 0;
  while (e + 1 < g.count && lw >= g.first[e + 1]) ++e;
  const X3WProb& q = g.p[e];
  X3Epilogue ep{};
  x3w_body<false, false, kEpiStore, false>(q.Ah, q.Al, q.lda, q.Bh, q.Bl, q.ldb, q.M, q.N, q.K, q.tiles_n, q.tiles,
                                           q.chunk, q.slabs, q.N, ep, lw - g.first[e]);
}
#undef RQ_W_BAR
#undef RQ_W_VM6
#undef RQ_W_LGKM0

// Split-K slab reduction with the GEMM's epilogue: element j of the (M, N) output (ldc == N) is the
// fixed-order sum over s of P[s][j] (slab_sum_w4: the partial sums of s = w, w + 4, ... for w = 0..3,
// added in that order by one thread per float4 column: deterministic, no atomics), then (ACC) plus the
// current C[j], then the epilogue of x3_epi4 at (m, n) = (j / N, j % N). Lets every epilogue — SiLU fwd / bwd with dropout, residual
// add, accumulation into an existing gradient — use split-K when the output tiles cannot fill the
// chip (the decoder's 1,280 future-token rows: 40 tiles of 128 x 128).
constexpr int kRedColsPerWg = 256;   // float4 columns per workgroup (layout 0)

template <int EPI, bool DROP, bool ACC>
__global__ void __launch_bounds__(256) x3_reduce_kernel(const float* __restrict__ P, int S, int64_t n, int N,
                                                        float* __restrict__ C, X3Epilogue ep) {
  ep.seed = epoch_seed(ep.seed);
  const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= n) return;
  float4 r = slab_sum_w4(P, S, n, j);
  if constexpr (ACC) {
    const float4 c = *reinterpret_cast<const float4*>(C + j);
    r = make_float4(c.x + r.x, c.y + r.y, c.z + r.z, c.w + r.w);
  }
  x3_epi4<EPI, DROP>(r, (int)(j / N), (int)(j % N), N, C, C, N, ep);
}

// Elementwise split (weights once per step, a large chain input once per step). HBM-bound: 4 B
// read + 2 x 2 B written per element. VEC: float4 loads and 8-B plane stores, 2 float4 in flight
// per thread per iteration (n % 4 == 0, 16-B aligned x, 8-B aligned planes); else scalar.
template <bool VEC>
__global__ void __launch_bounds__(256) split_bf16x3_kernel(const float* __restrict__ x, int64_t n,
                                                           uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
  if constexpr (VEC) {
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + stride < n4; i += 2 * stride) {
      const float4 a = reinterpret_cast<const float4*>(x)[i];
      const float4 b = reinterpret_cast<const float4*>(x)[i + stride];
      split_store4(a, hi + 4 * i, lo + 4 * i);
      split_store4(b, hi + 4 * (i + stride), lo + 4 * (i + stride));
    }
    if (i < n4) split_store4(reinterpret_cast<const float4*>(x)[i], hi + 4 * i, lo + 4 * i);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
      split_store1(x[i], hi + i, lo + i);
  }
}

// Several tensors at once (all weights of an MLP chain: one launch instead of one per weight).
constexpr int kSplitMax = 48;   // a decoder's every GEMM weight in one launch (kernel arguments ~1.6 KB)
constexpr int kSplitPer = 4;    // units (float4 / scalars) per thread: one workgroup = 1,024 units of ONE tensor
struct SplitMulti {
  const float* x[kSplitMax];
  uint16_t* hi[kSplitMax];
  uint16_t* lo[kSplitMax];
  int64_t n[kSplitMax];           // units per tensor
  int blk0[kSplitMax + 1];        // prefix sums of the workgroups per tensor
  int count;
};

// VEC: every tensor's element count % 4 == 0 and its pointers aligned (16 B x, 8 B planes): float4 units
// with two 8-B plane stores each; else scalar units. Each workgroup owns 1,024 consecutive units of one
// tensor, found by a uniform scan of blk0 (scalar kernel-argument loads: the per-thread binary search it
// replaces indexed the argument block per lane, one dependent search per float4 — 2.6 TB/s on the
// decoder's weights), and keeps its thread's 4 loads in flight.
template <bool VEC>
__global__ void __launch_bounds__(256) split_bf16x3_multi_kernel(SplitMulti sm) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < sm.count && b >= sm.blk0[t + 1]) ++t;
  const int64_t n = sm.n[t];
  const int64_t j0 = (int64_t)(b - sm.blk0[t]) * (256 * kSplitPer) + threadIdx.x;
  const float* __restrict__ x = sm.x[t];
  uint16_t* __restrict__ hi = sm.hi[t];
  uint16_t* __restrict__ lo = sm.lo[t];
  if constexpr (VEC) {
    float4 v[kSplitPer];
#pragma unroll
    for (int u = 0; u < kSplitPer; ++u) {
      const int64_t j = j0 + 256 * u;
      if (j < n) v[u] = reinterpret_cast<const float4*>(x)[j];
    }
#pragma unroll
    for (int u = 0; u < kSplitPer; ++u) {
      const int64_t j = j0 + 256 * u;
      if (j < n) split_store4(v[u], hi + 4 * j, lo + 4 * j);
    }
  } else {
#pragma unroll
    for (int u = 0; u < kSplitPer; ++u) {
      const int64_t j = j0 + 256 * u;
      if (j < n) split_store1(x[j], hi + j, lo + j);
    }
  }
}

}  // namespace rqhip

using namespace rqhip;

extern "C" {

size_t rq_linear_wgrad_workspace(int64_t Bn, int64_t O, int64_t I) {
  if (Bn <= 0 || O <= 0 || I <= 0) return 0;
  return wgrad_plan(Bn, O, I, x3_cus()).ws_bytes;
}

int rq_linear_wgrad(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t Bn, int64_t O, int64_t I,
                    float* dW, float* db, void* workspace, size_t ws_bytes, void* stream) {
  RQ_CHECK_ARG(((g && x) || Bn == 0) && dW && Bn >= 0 && O > 0 && I > 0 && O < (1 << 30) && I < (1 << 30),
               "rq_linear_wgrad: bad arguments");
  RQ_CHECK_ARG(O % 4 == 0 && I % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && ldg >= O && ldx >= I,
               "rq_linear_wgrad: O, I and leading dims must be multiples of 4 (float4 rows)");
  RQ_CHECK_ARG(((uintptr_t)g | (uintptr_t)x | (uintptr_t)dW | (uintptr_t)db) % 16 == 0,
               "rq_linear_wgrad: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (Bn == 0) {
    RQ_HIP(zero_async(dW, (size_t)(O * I) * sizeof(float), s));
    if (db) RQ_HIP(zero_async(db, (size_t)O * sizeof(float), s));
    return 0;
  }
  const WgradPlan p = wgrad_plan(Bn, O, I, x3_cus());
  RQ_CHECK_ARG(workspace != nullptr && ws_bytes >= p.ws_bytes, "rq_linear_wgrad: workspace %zu < %zu bytes", ws_bytes,
               p.ws_bytes);
  float* P = static_cast<float*>(workspace);
  float* Pb = db ? P + (int64_t)p.S * O * I : nullptr;
  hipLaunchKernelGGL(wgrad_partial_kernel, dim3(p.grid), dim3(256), 0, s, g, ldg, x, ldx, Bn, (int)O,
                     (int)I, p.tiles_i, p.tiles, p.S, p.chunk, p.per, P, Pb);
  RQ_LAUNCH_CHECK("wgrad_partial_kernel");
  const int64_t n = O * I;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n / 4 + 63) / 64)), dim3(256), 0, s, P, p.S, n, dW);
  RQ_LAUNCH_CHECK("wgrad_reduce_kernel");
  if (db) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((O / 4 + 63) / 64)), dim3(256), 0, s, Pb, p.S, O, db);
    RQ_LAUNCH_CHECK("wgrad_reduce_kernel(bias)");
  }
  return 0;
}


size_t rq_gemm_bf16x3_workspace(int64_t M, int64_t N, int64_t K) { return x3_workspace_bytes(M, N, K, x3_cus()); }

}  // extern "C"

namespace rqhip {

// One validated and planned rq_gemm_bf16x3 call (x3_prepare), its kernel launch (x3_launch) and its slab
// reduction or deferral (x3_post): rq_gemm_bf16x3_run runs the three in a row, rq_gemm_bf16x3_pair prepares
// two calls and, where gemm_plan.h pairs them (x3_pair_plan), launches both problems in one gemm_x3_pair_kernel.
struct X3Call {
  X3Plan pl;      // gemm_plan.h: the kernel, its grid, split-K and slabs
  X3Args xa;      // the kernel's argument block; xa.C = where the kernel stores (C, or the slabs)
  bool trivial;   // K == 0: nothing to launch
  int epilogue, accumulate, defer;   // what x3_post applies to the slabs, and to ...
  float* C;                          // ... the call's real output
};

// Validate and plan one call. dry = planning only (rq_gemm_bf16x3_plan): no stream work, no workspace check.
static int x3_prepare(const rq_gemm_desc& d, hipStream_t s, X3Call* c, bool dry = false) {
  const void *A = d.A, *A_lo = d.A_lo, *B = d.B, *B_lo = d.B_lo;
  const int64_t lda = d.lda, ldb = d.ldb, M = d.M, N = d.N, K = d.K, ldc = d.ldc, ldh = d.ldh;
  const int a_kcontig = d.a_kcontig, b_kcontig = d.b_kcontig, epilogue = d.epilogue, accumulate = d.accumulate;
  float* C = d.C;
  const bool asp = A_lo != nullptr, bsp = B_lo != nullptr;
  *c = X3Call{};
  RQ_CHECK_ARG(dry || (((A && B) || K == 0) && M > 0 && N > 0), "rq_gemm_bf16x3: bad arguments");
  RQ_CHECK_ARG(K >= 0 && M > 0 && N > 0 && M < (1 << 30) && N < (1 << 30) && epilogue >= 0 && epilogue <= 3,
               "rq_gemm_bf16x3: bad arguments");
  const bool needs_h = epilogue == kEpiSiluFwd || epilogue == kEpiSiluBwd;
  RQ_CHECK_ARG(dry || ((epilogue == kEpiSiluBwd || C) && (!needs_h || (d.H_hi && d.H_lo && ldh >= N)) &&
                       ((epilogue != kEpiSiluBwd && epilogue != kEpiAdd) || d.Z)),
               "rq_gemm_bf16x3: epilogue %d needs %s", epilogue,
               epilogue == kEpiSiluBwd ? "Z and H planes"
                                       : (epilogue == kEpiSiluFwd ? "C and H planes" : (epilogue ? "C and Z" : "C")));
  // float4 (fp32) / 8 x bf16 (split) vectors along each operand's contiguous axis
  const int64_t va = asp ? 8 : 4, vb = bsp ? 8 : 4;
  RQ_CHECK_ARG((a_kcontig ? K % va == 0 : M % va == 0) && (b_kcontig ? K % vb == 0 : N % vb == 0) && lda % va == 0 &&
                   ldb % vb == 0,
               "rq_gemm_bf16x3: the contiguous axis of each operand and its leading dim must be multiples of %d "
               "(fp32) / 8 (split)", 4);
  RQ_CHECK_ARG(lda >= (a_kcontig ? K : M) && ldb >= (b_kcontig ? K : N) && (epilogue == kEpiSiluBwd || ldc >= N),
               "rq_gemm_bf16x3: leading dimension too small");
  RQ_CHECK_ARG(N % 4 == 0 && ldc % 4 == 0 && ldh % 4 == 0 && ((uintptr_t)C | (uintptr_t)d.Z) % 16 == 0 &&
                   ((uintptr_t)d.H_hi | (uintptr_t)d.H_lo) % 8 == 0,
               "rq_gemm_bf16x3: N and the output leading dims must be multiples of 4 (vector stores), outputs aligned");
  RQ_CHECK_ARG(((uintptr_t)A | (uintptr_t)A_lo | (uintptr_t)B | (uintptr_t)B_lo) % 16 == 0,
               "rq_gemm_bf16x3: operand pointers must be 16-byte aligned");
  X3Epilogue ep{d.Z, d.H_hi, d.H_lo, ldh, 0u, 1.f, d.seed, 0};
  dropout_params(d.p, &ep.thr, &ep.scale);
  RQ_CHECK_ARG(!accumulate || epilogue == kEpiStore, "rq_gemm_bf16x3: accumulate needs the plain epilogue");
  c->trivial = K == 0;
  if (K == 0) {
    RQ_CHECK_ARG(epilogue == kEpiStore, "rq_gemm_bf16x3: K == 0 needs the plain epilogue");
    if (!accumulate && !dry)
      RQ_HIP(hipMemset2DAsync(C, (size_t)ldc * sizeof(float), 0, (size_t)N * sizeof(float), (size_t)M, s));
    return 0;
  }
  const X3Plan pl = x3_call_plan(x3_shape(d, ep.thr != 0), x3_cus());
  // slab path: x3_reduce_kernel applies the real epilogue (and the accumulation); an unsplit accumulating call
  // adds in the GEMM's epilogue
  ep.acc = accumulate && !pl.slab;
  float* out = C;
  if (pl.slab && !dry) {
    RQ_CHECK_ARG(d.workspace != nullptr && d.ws_bytes >= pl.slab_bytes && ldc == N,
                 "rq_gemm_bf16x3: split-K / accumulate needs ldc == N and workspace %zu >= %zu bytes", d.ws_bytes,
                 pl.slab_bytes);
    out = static_cast<float*>(d.workspace);
  }
  const X3Args xa{A, A_lo, lda, B, B_lo, ldb, (int)M, (int)N, K, pl.tiles_n, pl.tiles, pl.S, pl.chunk, pl.per, out,
                  pl.slab ? N : ldc, ep, pl.kfull};
  *c = X3Call{pl, xa, false, epilogue, accumulate, d.defer, C};
  return 0;
}

// The launchers' switch arms are the only place that names template arguments, one arm per entry of gemm_plan.h's
// built-form table (kX3Built): the operand flags come from the layout code, the key is (kernel epilogue, code).
#define RQ_X3_OPS(CODE) ((CODE) & kCodeAK) != 0, ((CODE) & kCodeAS) != 0, ((CODE) & kCodeBK) != 0, ((CODE) & kCodeBS) != 0
#define RQ_X3_KEY(EP, CODE) ((EP) << 5 | (CODE))

static int x3_launch(const X3Call& c, hipStream_t s) {
  const X3Plan& pl = c.pl;
  const X3Args& xa = c.xa;
  RQ_CHECK_ARG(x3_form_built(pl.kind, pl.code, pl.epi_k),
               "rq_gemm_bf16x3: operand combination (a_kcontig %d, a_split %d, b_kcontig %d, b_split %d) "
               "not built for epilogue %d", (pl.code & kCodeAK) != 0, (pl.code & kCodeAS) != 0, (pl.code & kCodeBK) != 0,
               (pl.code & kCodeBS) != 0, c.epilogue);
  const dim3 grid(pl.grid), block(pl.block);
  if (pl.kind == kX3Wide) {
    const uint16_t *ah = static_cast<const uint16_t*>(xa.A), *al = static_cast<const uint16_t*>(xa.Al);
    const uint16_t *bh = static_cast<const uint16_t*>(xa.B), *bl = static_cast<const uint16_t*>(xa.Bl);
#define RQ_X3WD(CODE, EP, DR)                                                                                       \
  hipLaunchKernelGGL((gemm_x3w_kernel<((CODE) & kCodeAK) != 0, ((CODE) & kCodeBK) != 0, EP, DR>), grid, block, 0, s, \
                     ah, al, xa.lda, bh, bl, xa.ldb, xa.M, xa.N, xa.K, xa.tiles_n, xa.tiles, xa.chunk, xa.C, xa.ldc, xa.ep)
#define RQ_X3W(EP, CODE)                                                                                            \
  case RQ_X3_KEY(EP, CODE):                                                                                         \
    if (pl.drop) RQ_X3WD(CODE, EP, (EP != kEpiStore)); else RQ_X3WD(CODE, EP, false);                               \
    break
    switch (RQ_X3_KEY(pl.epi_k, pl.code)) {
      RQ_X3W(kEpiStore, 30); RQ_X3W(kEpiStore, 26); RQ_X3W(kEpiStore, 14); RQ_X3W(kEpiStore, 10);
      RQ_X3W(kEpiSiluFwd, 30);
      RQ_X3W(kEpiSiluBwd, 26);
      RQ_X3W(kEpiAdd, 30);
      default: break;   // unreachable: x3_form_built
    }
#undef RQ_X3W
#undef RQ_X3WD
  } else {
#define RQ_X3D(CODE, EP, DR)                                                                                        \
  do {                                                                                                              \
    if (pl.kind == kX3Tile64)                                                                                       \
      hipLaunchKernelGGL((gemm_bf16x3_kernel<RQ_X3_OPS(CODE), EP, DR, 64>), grid, block, pl.lds_pad, s, xa);        \
    else                                                                                                            \
      hipLaunchKernelGGL((gemm_bf16x3_kernel<RQ_X3_OPS(CODE), EP, DR>), grid, block, 0, s, xa);                     \
  } while (0)
#define RQ_X3(EP, CODE)                                                                                             \
  case RQ_X3_KEY(EP, CODE):                                                                                         \
    if (pl.drop) RQ_X3D(CODE, EP, (EP != kEpiStore)); else RQ_X3D(CODE, EP, false);                                 \
    break
    switch (RQ_X3_KEY(pl.epi_k, pl.code)) {
      // every layout with fp32 operands (the generic entry point)
      RQ_X3(kEpiStore, 20); RQ_X3(kEpiStore, 16); RQ_X3(kEpiStore, 4); RQ_X3(kEpiStore, 0);
      // fused MLP chain: forward of the last layer, data grads with split weights, weight grads
      RQ_X3(kEpiStore, 30); RQ_X3(kEpiStore, 22); RQ_X3(kEpiStore, 26); RQ_X3(kEpiStore, 18);
      RQ_X3(kEpiStore, 10); RQ_X3(kEpiStore, 8); RQ_X3(kEpiStore, 2);
      RQ_X3(kEpiSiluFwd, 22); RQ_X3(kEpiSiluFwd, 30);
      RQ_X3(kEpiSiluBwd, 18); RQ_X3(kEpiSiluBwd, 26);
      RQ_X3(kEpiAdd, 22);   // Linear (split weight) + residual
      RQ_X3(kEpiAdd, 30);   // MLP chain's last layer + residual
      default: break;       // unreachable: x3_form_built
    }
#undef RQ_X3
#undef RQ_X3D
  }
  RQ_LAUNCH_CHECK("gemm_bf16x3_kernel");
  return 0;
}

static int x3_post(const X3Call& c, int* splits, hipStream_t s) {
  if (!c.pl.slab) return 0;
  const int S = c.pl.S;
  if (c.defer && c.accumulate && c.epilogue == kEpiStore && splits) {   // the caller reduces later
    *splits = S;                                                        // (rq_reduce_partials, layout 0)
    return 0;
  }
  const int N = c.xa.N;
  const int64_t n = (int64_t)c.xa.M * N;
  const dim3 rg((unsigned)((n / 4 + kRedColsPerWg - 1) / kRedColsPerWg)), rb(256);
  const X3Epilogue& ep = c.xa.ep;
  const bool drop = ep.thr != 0 && c.epilogue != kEpiStore;
#define RQ_X3R(EP, DR, AC) hipLaunchKernelGGL((x3_reduce_kernel<EP, DR, AC>), rg, rb, 0, s, c.xa.C, S, n, N, c.C, ep)
  switch (c.epilogue) {
    case kEpiStore: if (c.accumulate) RQ_X3R(kEpiStore, false, true); else RQ_X3R(kEpiStore, false, false); break;
    case kEpiSiluFwd: if (drop) RQ_X3R(kEpiSiluFwd, true, false); else RQ_X3R(kEpiSiluFwd, false, false); break;
    case kEpiSiluBwd: if (drop) RQ_X3R(kEpiSiluBwd, true, false); else RQ_X3R(kEpiSiluBwd, false, false); break;
    default: if (drop) RQ_X3R(kEpiAdd, true, false); else RQ_X3R(kEpiAdd, false, false); break;
  }
#undef RQ_X3R
  RQ_LAUNCH_CHECK("x3_reduce_kernel");
  return 0;
}

// The paired launch of two problems on the 128- or 64-tile kernel (TS), as x3_pair_plan paired them.
template <class P1, class P2>
static void x3_pair_go(const X3Call& c1, const X3Call& c2, const X3PairPlan& pp, hipStream_t s) {
  hipLaunchKernelGGL((gemm_x3_pair_kernel<P1, P2>), dim3(pp.grid), dim3(256), pp.lds_pad, s, c1.xa, c2.xa, (int)pp.n1);
}
// c2 of a (data gradient, weight gradient) pair: m-contiguous A (fp32 / split) x n-contiguous B (fp32 / split), plain store
template <class P1, int TS>
static void x3_pair_p2(const X3Call& c1, const X3Call& c2, const X3PairPlan& pp, hipStream_t s) {
#define RQ_X3P2(CODE) \
  case CODE: x3_pair_go<P1, X3Body<RQ_X3_OPS(CODE), kEpiStore, false, TS>>(c1, c2, pp, s); break
  switch (c2.pl.code) {
    RQ_X3P2(0); RQ_X3P2(2); RQ_X3P2(8); RQ_X3P2(10);
    default: break;   // unreachable: x3_form_built(kX3PairWgrad)
  }
#undef RQ_X3P2
}
// c1 of that pair: k-contiguous A (fp32 / split) x n-contiguous split B; plain or SiLU' (+ dropout)
template <int TS>
static void x3_pair_grad(const X3Call& c1, const X3Call& c2, const X3PairPlan& pp, hipStream_t s) {
#define RQ_X3P1(EP, CODE, DR) x3_pair_p2<X3Body<RQ_X3_OPS(CODE), EP, DR, TS>, TS>(c1, c2, pp, s)
  switch (RQ_X3_KEY(c1.pl.epi_k, c1.pl.code)) {
    case RQ_X3_KEY(kEpiStore, 18): RQ_X3P1(kEpiStore, 18, false); break;
    case RQ_X3_KEY(kEpiStore, 26): RQ_X3P1(kEpiStore, 26, false); break;
    case RQ_X3_KEY(kEpiSiluBwd, 18):
      if (c1.pl.drop) RQ_X3P1(kEpiSiluBwd, 18, true); else RQ_X3P1(kEpiSiluBwd, 18, false);
      break;
    default: break;   // unreachable: x3_form_built(kX3PairDgrad)
  }
#undef RQ_X3P1
}
// two forward projections: k-contiguous A (fp32 / split) x k-contiguous split B, plain store
template <int TS>
static void x3_pair_fwd(const X3Call& c1, const X3Call& c2, const X3PairPlan& pp, hipStream_t s) {
  using F32 = X3Body<RQ_X3_OPS(22), kEpiStore, false, TS>;   // fp32 A
  using SPL = X3Body<RQ_X3_OPS(30), kEpiStore, false, TS>;   // split A
  const bool a1 = c1.pl.code == 30, a2 = c2.pl.code == 30;
  if (!a1 && !a2) x3_pair_go<F32, F32>(c1, c2, pp, s);
  else if (!a1) x3_pair_go<F32, SPL>(c1, c2, pp, s);
  else if (!a2) x3_pair_go<SPL, F32>(c1, c2, pp, s);
  else x3_pair_go<SPL, SPL>(c1, c2, pp, s);
}

static void x3_pair_launch(const X3Call& c1, const X3Call& c2, const X3PairPlan& pp, hipStream_t s) {
  const bool t64 = c1.pl.kind == kX3Tile64;
  if (pp.kind == kX3PairFwd)
    t64 ? x3_pair_fwd<64>(c1, c2, pp, s) : x3_pair_fwd<128>(c1, c2, pp, s);
  else
    t64 ? x3_pair_grad<64>(c1, c2, pp, s) : x3_pair_grad<128>(c1, c2, pp, s);
}
#undef RQ_X3_OPS
#undef RQ_X3_KEY

// The grouped launch of the members of g (gemm_plan.h: x3_group_plan), each to split-K slabs in its own workspace.
static int x3_group_launch(const rq_gemm_desc* d, const X3Call* c, int count, const X3GroupPlan& g, hipStream_t s) {
  X3WGroup w{};
  int n = 0;
  for (int i = 0; i < count; ++i) {
    if (!g.in[i]) continue;
    const X3Plan& pl = g.pl[i];
    const X3Args& xa = c[i].xa;
    RQ_CHECK_ARG(d[i].workspace != nullptr && d[i].ws_bytes >= pl.slab_bytes && ((uintptr_t)d[i].workspace) % 16 == 0,
                 "rq_gemm_bf16x3_group: member %d needs workspace %zu >= %zu bytes", i, d[i].ws_bytes, pl.slab_bytes);
    w.p[n] = X3WProb{static_cast<const uint16_t*>(xa.A), static_cast<const uint16_t*>(xa.Al), xa.lda,
                     static_cast<const uint16_t*>(xa.B), static_cast<const uint16_t*>(xa.Bl), xa.ldb, xa.K, pl.chunk,
                     static_cast<float*>(d[i].workspace), xa.M, xa.N, pl.tiles_n, pl.tiles, pl.S, 0};
    w.first[n + 1] = w.first[n] + (int)pl.grid;   // the members' work items, in order: one round when the model grouped
    ++n;
  }
  w.count = n;
  hipLaunchKernelGGL(gemm_x3w_group_kernel, dim3((unsigned)w.first[n]), dim3(512), 0, s, w);
  RQ_LAUNCH_CHECK("gemm_x3w_group_kernel");
  return 0;
}

// Plan `count` descriptors without a stream (the host-only *_plan entry points). false: one is empty or invalid.
static bool x3_plan_only(const rq_gemm_desc* d, int count, X3Call* c) {
  for (int i = 0; i < count; ++i)
    if (d[i].M <= 0 || d[i].N <= 0 || d[i].K <= 0 || x3_prepare(d[i], nullptr, &c[i], true) != 0) return false;
  return true;
}

static X3GroupPlan x3_group_of(const rq_gemm_desc* d, const X3Call* c, int count, bool model) {
  X3Shape sh[kX3GroupMax];
  X3Plan own[kX3GroupMax];
  for (int i = 0; i < count; ++i) {
    sh[i] = x3_shape(d[i]);
    own[i] = c[i].pl;
  }
  return x3_group_plan(sh, own, count, model, x3_cus());
}

}  // namespace rqhip

extern "C" {

static_assert(sizeof(rq_gemm_desc) == 192, "rq_gemm_desc layout (the ctypes mirror in rqvae_hip/ops.py)");

int rq_gemm_bf16x3_run(const rq_gemm_desc* d, int* splits, void* stream) {
  RQ_CHECK_ARG(d != nullptr, "rq_gemm_bf16x3_run: null descriptor");
  if (splits) *splits = 0;
  hipStream_t s = (hipStream_t)stream;
  X3Call c;
  const int rc = x3_prepare(*d, s, &c);
  if (rc || c.trivial) return rc;
  const int rl = x3_launch(c, s);
  if (rl) return rl;
  return x3_post(c, splits, s);
}

int rq_gemm_bf16x3_pair(const rq_gemm_desc* d, int* splits, void* stream) {
  RQ_CHECK_ARG(d != nullptr, "rq_gemm_bf16x3_pair: null descriptors");
  if (splits) splits[0] = splits[1] = 0;
  hipStream_t s = (hipStream_t)stream;
  X3Call c[2];
  for (int i = 0; i < 2; ++i) {
    const int rc = x3_prepare(d[i], s, &c[i]);
    if (rc) return rc;
  }
  X3PairPlan pp{};
  if (!c[0].trivial && !c[1].trivial && !((d[0].flags | d[1].flags) & RQ_GEMM_NO_PAIR))
    pp = x3_pair_plan(c[0].pl, c[1].pl, x3_cus());
  if (pp.kind) {
    x3_pair_launch(c[0], c[1], pp, s);
    RQ_LAUNCH_CHECK("gemm_x3_pair_kernel");
  } else {
    for (int i = 0; i < 2; ++i) {
      if (c[i].trivial) continue;
      const int rl = x3_launch(c[i], s);
      if (rl) return rl;
    }
  }
  // two plain-store slab outputs: one batched reduction (rq_reduce_partials layout 0 = x3_reduce_kernel's
  // order, bitwise) instead of two launches
  auto plain_slab = [](const X3Call& x) { return x.pl.slab && x.epilogue == kEpiStore && !x.accumulate; };
  if (plain_slab(c[0]) && plain_slab(c[1])) {
    const float* P[2] = {c[0].xa.C, c[1].xa.C};
    float* out[2] = {c[0].C, c[1].C};
    const int64_t n[2] = {(int64_t)c[0].xa.M * c[0].xa.N, (int64_t)c[1].xa.M * c[1].xa.N};
    const int S[2] = {c[0].pl.S, c[1].pl.S}, layout[2] = {0, 0}, acc[2] = {0, 0};
    return rq_reduce_partials(2, P, out, n, S, layout, acc, stream);
  }
  for (int i = 0; i < 2; ++i) {
    if (c[i].trivial) continue;
    const int rp = x3_post(c[i], splits ? splits + i : nullptr, s);
    if (rp) return rp;
  }
  return 0;
}

int rq_gemm_bf16x3_plan(const rq_gemm_desc* d, int* splits) {
  if (splits) *splits = 0;
  X3Call c;
  if (!d || !x3_plan_only(d, 1, &c)) return -1;
  if (splits) *splits = c.pl.S;
  return c.pl.kind;
}

int rq_gemm_bf16x3_pair_plan(const rq_gemm_desc* d) {
  X3Call c[2];
  if (!d || ((d[0].flags | d[1].flags) & RQ_GEMM_NO_PAIR) || !x3_plan_only(d, 2, c)) return 0;
  return x3_pair_plan(c[0].pl, c[1].pl, x3_cus()).kind ? 1 : 0;
}

int rq_gemm_bf16x3_pair_resplit(const rq_gemm_desc* d) {
  X3Call c[2];
  if (!d || !x3_plan_only(d, 2, c)) return 0;
  return x3_pair_resplit(c[0].pl, c[1].pl, d[0].K, d[1].K, x3_cus());
}

// Up to kX3GroupMax independent calls, the weight gradients of one MLP chain: the members that carry explicit
// split counts (x3_group_plan; the model's counts come from rq_gemm_bf16x3_group_plan)
// run in ONE gemm_x3w_group_kernel launch, each to split-K slabs in its own workspace; the others run as
// rq_gemm_bf16x3_run would run them. A grouped member's slabs are reduced here in one rq_reduce_partials
// launch (layout 0, accumulating where the call accumulates) or, for a deferring accumulating call, left to
// the caller (splits[i] = its slab count, as rq_gemm_bf16x3_run reports).
int rq_gemm_bf16x3_group(const rq_gemm_desc* d, int count, int* splits, void* stream) {
  RQ_CHECK_ARG(d != nullptr && count >= 1 && count <= kX3GroupMax, "rq_gemm_bf16x3_group: 1..%d descriptors",
               kX3GroupMax);
  hipStream_t s = (hipStream_t)stream;
  X3Call c[kX3GroupMax];
  for (int i = 0; i < count; ++i) {
    if (splits) splits[i] = 0;
    const int rc = x3_prepare(d[i], s, &c[i]);
    if (rc) return rc;
  }
  const X3GroupPlan g = x3_group_of(d, c, count, false);
  if (g.n) {
    const int rl = x3_group_launch(d, c, count, g, s);
    if (rl) return rl;
  }
  const float* P[kX3GroupMax];
  float* out[kX3GroupMax];
  int64_t n[kX3GroupMax];
  int S[kX3GroupMax], layout[kX3GroupMax], acc[kX3GroupMax], nr = 0;
  for (int i = 0; i < count; ++i) {
    if (c[i].trivial) continue;
    if (!g.in[i]) {
      const int rl = x3_launch(c[i], s);
      if (rl) return rl;
      const int rp = x3_post(c[i], splits ? splits + i : nullptr, s);
      if (rp) return rp;
    } else if (c[i].defer && c[i].accumulate && splits) {
      splits[i] = g.pl[i].S;
    } else {
      P[nr] = static_cast<const float*>(d[i].workspace);
      out[nr] = c[i].C;
      n[nr] = (int64_t)c[i].xa.M * c[i].xa.N;
      S[nr] = g.pl[i].S;
      layout[nr] = 0;
      acc[nr++] = c[i].accumulate != 0;
    }
  }
  return nr ? rq_reduce_partials(nr, P, out, n, S, layout, acc, stream) : 0;
}

int rq_gemm_bf16x3_group_plan(const rq_gemm_desc* d, int count, int* splits) {
  if (splits)
    for (int i = 0; i < count && i < kX3GroupMax; ++i) splits[i] = 0;
  X3Call c[kX3GroupMax];
  if (!d || count < 2 || count > kX3GroupMax || !x3_plan_only(d, count, c)) return 0;
  const X3GroupPlan g = x3_group_of(d, c, count, true);
  if (splits)
    for (int i = 0; i < count; ++i) splits[i] = g.in[i] ? g.pl[i].S : 0;
  return g.n;
}

// Deferred partial reductions, many in one launch: out_i[j] (+)= sum_s P_i[s n_i + j] for every entry i,
// each in the SAME order as the reduction it replaces — layout 0 = x3_reduce_kernel's (slab_sum_w4, one
// thread per float4 column; a workgroup owns 256 of them), layout 1 = rms_reduce_kernel's (64 lanes
// over s, fixed LDS tree; 4 float4 columns) — so a deferred result is bitwise the immediate one.
constexpr int kRedSegMax = 48;
struct RedSegTable {
  const float* P[kRedSegMax];
  float* out[kRedSegMax];
  int64_t n[kRedSegMax];
  int S[kRedSegMax];
  int layout[kRedSegMax];
  int acc[kRedSegMax];
  int blk0[kRedSegMax + 1];
  int count;
};

__global__ void __launch_bounds__(256) reduce_partials_kernel(RedSegTable t) {
  __shared__ float4 red[256];
  const int b = blockIdx.x;
  int e = 0;
  while (e + 1 < t.count && b >= t.blk0[e + 1]) ++e;
  const int lb = b - t.blk0[e];
  const float* __restrict__ P = t.P[e];
  float* __restrict__ out = t.out[e];
  const int64_t n = t.n[e];
  const int S = t.S[e];
  const int tid = threadIdx.x;
  if (t.layout[e] == 0) {   // one thread per float4 column (slab_sum_w4: the same order)
    const int64_t j = ((int64_t)lb * 256 + tid) * 4;
    if (j >= n) return;
    float4 r = slab_sum_w4(P, S, n, j);
    if (t.acc[e]) {
      const float4 c = *reinterpret_cast<const float4*>(out + j);
      r = make_float4(c.x + r.x, c.y + r.y, c.z + r.z, c.w + r.w);
    }
    *reinterpret_cast<float4*>(out + j) = r;
  } else {
    constexpr int kC = 4, kQ = 256 / kC;
    const int c = tid % kC, q = tid / kC;
    const int64_t j = ((int64_t)lb * kC + c) * 4;
    const bool ok = j < n;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) a = strided_slab_sum(P, S, n, j, q, kQ);
    red[q * kC + c] = a;
    __syncthreads();
#pragma unroll
    for (int h = kQ / 2; h >= 1; h >>= 1) {
      if (q < h) {
        const float4 u = red[q * kC + c], v = red[(q + h) * kC + c];
        red[q * kC + c] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
      }
      __syncthreads();
    }
    if (q == 0 && ok) {
      float4 r = red[c];
      if (t.acc[e]) {
        const float4 o = *reinterpret_cast<const float4*>(out + j);
        r = make_float4(o.x + r.x, o.y + r.y, o.z + r.z, o.w + r.w);
      }
      *reinterpret_cast<float4*>(out + j) = r;
    }
  }
}

int rq_reduce_partials(int count, const float* const* P, float* const* out, const int64_t* n, const int* S,
                       const int* layout, const int* accumulate, void* stream) {
  RQ_CHECK_ARG(count >= 0 && (count == 0 || (P && out && n && S && layout && accumulate)),
               "rq_reduce_partials: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < count; base += kRedSegMax) {
    RedSegTable t;
    t.count = std::min(kRedSegMax, count - base);
    int blk = 0;
    for (int i = 0; i < t.count; ++i) {
      const int k = base + i;
      RQ_CHECK_ARG(P[k] && out[k] && n[k] > 0 && n[k] % 4 == 0 && S[k] >= 1 && (layout[k] == 0 || layout[k] == 1) &&
                       ((uintptr_t)P[k] | (uintptr_t)out[k]) % 16 == 0,
                   "rq_reduce_partials: entry %d: need n %% 4 == 0, S >= 1, layout 0/1, 16-B aligned pointers", k);
      t.P[i] = P[k];
      t.out[i] = out[k];
      t.n[i] = n[k];
      t.S[i] = S[k];
      t.layout[i] = layout[k];
      t.acc[i] = accumulate[k] != 0;
      t.blk0[i] = blk;
      blk += (int)((n[k] / 4 + (layout[k] == 0 ? kRedColsPerWg - 1 : 3)) / (layout[k] == 0 ? kRedColsPerWg : 4));
    }
    t.blk0[t.count] = blk;
    if (blk == 0) continue;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)blk), dim3(256), 0, st, t);
    RQ_LAUNCH_CHECK("reduce_partials_kernel");
  }
  return 0;
}

int rq_gemm_bf16x3(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb, int b_kcontig, int64_t M,
                   int64_t N, int64_t K, float* C, int64_t ldc, void* workspace, size_t ws_bytes, void* stream) {
  rq_gemm_desc d{};
  d.A = A;
  d.lda = lda;
  d.a_kcontig = a_kcontig;
  d.B = B;
  d.ldb = ldb;
  d.b_kcontig = b_kcontig;
  d.M = M;
  d.N = N;
  d.K = K;
  d.C = C;
  d.ldc = ldc;
  d.epilogue = kEpiStore;
  d.workspace = workspace;
  d.ws_bytes = ws_bytes;
  return rq_gemm_bf16x3_run(&d, nullptr, stream);
}

int rq_split_bf16x3_multi(int count, const float* const* x, const int64_t* n, uint16_t* const* hi,
                          uint16_t* const* lo, void* stream) {
  RQ_CHECK_ARG(count >= 0 && count <= kSplitMax && (count == 0 || (x && n && hi && lo)),
               "rq_split_bf16x3_multi: 0 <= count <= %d tensors", kSplitMax);
  SplitMulti sm;
  sm.count = count;
  sm.blk0[0] = 0;
  bool vec = true;
  for (int t = 0; t < count; ++t) {
    RQ_CHECK_ARG(n[t] >= 0 && (n[t] == 0 || (x[t] && hi[t] && lo[t])), "rq_split_bf16x3_multi: bad tensor %d", t);
    vec = vec && n[t] % 4 == 0 && (uintptr_t)x[t] % 16 == 0 && ((uintptr_t)hi[t] | (uintptr_t)lo[t]) % 8 == 0;
  }
  int64_t blocks = 0;
  for (int t = 0; t < count; ++t) {
    sm.x[t] = x[t];
    sm.hi[t] = hi[t];
    sm.lo[t] = lo[t];
    sm.n[t] = vec ? n[t] / 4 : n[t];
    blocks += (sm.n[t] + 256 * kSplitPer - 1) / (256 * kSplitPer);
    RQ_CHECK_ARG(blocks < (1ll << 31), "rq_split_bf16x3_multi: too many elements");
    sm.blk0[t + 1] = (int)blocks;
  }
  if (count == 0 || blocks == 0) return 0;
  const dim3 grid((unsigned)blocks);
  if (vec)
    hipLaunchKernelGGL((split_bf16x3_multi_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, sm);
  else
    hipLaunchKernelGGL((split_bf16x3_multi_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, sm);
  RQ_LAUNCH_CHECK("split_bf16x3_multi_kernel");
  return 0;
}

// x (n fp32) -> hi = RN_bf16(x), lo = RN_bf16(x - hi): the split form the GEMM consumes.
int rq_split_bf16x3(const float* x, int64_t n, uint16_t* hi, uint16_t* lo, void* stream) {
  RQ_CHECK_ARG(n >= 0 && (n == 0 || (x && hi && lo)), "rq_split_bf16x3: bad arguments");
  if (n == 0) return 0;
  const bool vec = n % 4 == 0 && (uintptr_t)x % 16 == 0 && ((uintptr_t)hi | (uintptr_t)lo) % 8 == 0;
  // vector path: 8 elements per thread per iteration; a grid of 8 x 256 workgroups keeps every CU busy
  const int64_t blocks = vec ? (n / 4 + 511) / 512 : (n + 255) / 256;
  const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
  if (vec)
    hipLaunchKernelGGL((split_bf16x3_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, x, n, hi, lo);
  else
    hipLaunchKernelGGL((split_bf16x3_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, x, n, hi, lo);
  RQ_LAUNCH_CHECK("split_bf16x3_kernel");
  return 0;
}


}  // extern "C"

int rqhip::seed_epoch_addr_linear(void** out) { return (int)hipGetSymbolAddress(out, HIP_SYMBOL(rqhip::rq_seed_epoch)); }
