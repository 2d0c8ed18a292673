// Patch merging between two backbone stages (the step between the stages of the layer loop:
// `f_v = my_blk.downsample(f_v)` / `f_a = htsat_blk.downsample(f_a)`, DG-SCT/AVE/nets/net_trans.py:914-916).
//
// Input x: bf16 [B][H*W][C], token-major.  Output row r = (b, i, j), i < H/2, j < W/2, is the product of the VIRTUAL row
//   cat(x[b][2i][2j], x[b][2i+1][2j], x[b][2i][2j+1], x[b][2i+1][2j+1])          (4C wide, the reference's x0 | x1 | x2 | x3)
// with W^T (W: bf16 [2C][4C], no bias).  The [rows][4C] concatenation is never written by a forward: the gather is the address
// arithmetic of 16-byte loads (a chunk of 8 channels never straddles a segment because C % 8 == 0).
//
//   DGSCT_PMERGE_NORM_FIRST (HTS-AT, htsat.py:259-295)   out = LN_4C(gather(x)) . W^T
//     pm_fwd_k<FIRST>     one launch: a workgroup owns BM output rows (64 up to 4C = 384, 32 above), loads their four segments,
//                         takes the fp32 row statistics over 4C (two passes over registers), writes mu / rstd, normalises and rounds
//                         to bf16 ONCE into an LDS A image [BM][4C] (the rounding point of LayerNorm-then-Linear in bf16), then walks
//                         the 2C output columns in tiles of 128 with v_mfma_f32_32x32x16_bf16, W streamed through LDS in [128][64]
//                         tiles; rows leave as 16-byte stores through an LDS tile.
//     backward            pm_dgemm_k<false>: g = dout . W -> ws [rows][4C] bf16;  pm_lnbwd_k<true>: one wavefront per row re-gathers x,
//                         recomputes x^ from mu / rstd, applies the LayerNorm backward over 4C and scatters the four segments.
//   DGSCT_PMERGE_NORM_LAST (Swin-V2, timm 0.6.12 PatchMerging as the AVE loop calls it)   out = LN_2C(gather(x) . W^T)
//     pm_fwd_k<LAST>      the same product with the gathered A operand streamed in [64][64] k-tiles (K = 4C up to 3072) -> pre
//                         [rows][2C] bf16 (kept for backward); then the library's row kernel (dgsct_layer_norm_forward): two launches.
//     backward            pm_lnbwd_k<false>: dpre = LN backward of dout over 2C from pre / mu / rstd -> ws [rows][2C] bf16;
//                         pm_dgemm_k<true>: dx = dpre . W with the scatter as the store addressing of the epilogue.
//   Every element of dx is written exactly once (the 2 x 2 cells do not overlap): no atomics, no pre-zeroing.
//   A TRAINABLE merge (dgsct_patch_merge_backward_params): the same launches with pm_lnbwd_sums_k in the place of pm_lnbwd_k -- the same
//   row arithmetic, so dx is bit for bit the same, plus the column sums d ln_w / d ln_b -- and pm_wgrad_k for dW [2C][4C] = D^T . A with
//   the A operand staged from the token map (fp32 atomics over at most 40 row slabs).  All three gradients fp32, zeroed by the call.
//
// Limits (enforced below): H, W even and >= 2; C % 32 == 0, C >= 32; 4C <= 1536 (NORM_FIRST) / 2C <= 1536 (NORM_LAST); bf16 only.
// Global loads that can run past the last row are UNCONDITIONAL from clamped addresses and masked in the register.
//
// The extern "C" entry points live here (as csrc/frontend.hip's do): the host emulation of the CPU tests has no patch merging.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dgsct.h"
#include "prims.h"
#include "device_util.h"
#include "mma_tile.h"
#include "err.h"

namespace dgsct {

constexpr int PM_BN = 128, PM_BK = 64;
constexpr int PM_P_KM = MT<DT_BF16>::km_pitch(PM_BK);      // 144 B: [..][64] image, contraction along the row
constexpr int PM_P_MN = mt_mn_pitch_bf16(PM_BN);           // 320 B: [64][128] image, contraction across rows
constexpr int PM_P_O = PM_BN * 2 + 16;                     // 272 B: output tile [BM][128]

struct PmGeom {
  int B, H, W, C, H2, W2;
  long rows;
};

// element offset of the (2i, 2j) token of output row r
// (rows < 2^29, checked on the host: the two divisions are 32-bit)
__device__ __forceinline__ long pm_base(const PmGeom& g, long r) {
  const unsigned ur = (unsigned)r, t = ur / (unsigned)g.W2, j = ur - t * (unsigned)g.W2, b = t / (unsigned)g.H2, i = t - b * (unsigned)g.H2;
  return (((long)b * g.H + 2 * i) * g.W + 2 * j) * g.C;
}
__device__ __forceinline__ long pm_shfl(long v, int src) {
  const int lo = __shfl((int)(v & 0xffffffffL), src, 64), hi = __shfl((int)(v >> 32), src, 64);
  return ((long)hi << 32) | (unsigned)lo;
}
// ... plus this for element k (a multiple of 8) of the virtual row: segment k / C = 0..3 -> (dh, dw) = (0,0) (1,0) (0,1) (1,1)
__device__ __forceinline__ int pm_seg(const PmGeom& g, int k) {
  const int seg = k / g.C, off = k - seg * g.C;
  return ((seg & 1) * g.W + (seg >> 1)) * g.C + off;
}
__device__ __forceinline__ uint4 pm_ld16(const void* p, long el) { return *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(p) + el); }
__device__ __forceinline__ void pm_st16(void* p, long el, const uint4& v) { *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(p) + el) = v; }
__device__ __forceinline__ uint4 pm_pack(const float (&v)[8]) {
  return make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7]));
}

// accumulator tiles -> bf16 LDS tile [BM][128] -> 16-byte global stores.  SCATTER: the output row is a virtual 4C row of the map.
// The tile aliases the W tile of the main loop: a barrier before it is written, one before it is read.
template <int BM, bool SCATTER>
__device__ __forceinline__ void pm_store_tile(const PmGeom& g, const mt_f32x16 (&acc)[BM / 32], bool wave_on, char* O, void* out, long ldo,
                                              int r0, int n0, int ncols, int tid) {
  const int lane = tid & 63, wv = tid >> 6;
  __syncthreads();
  if (wave_on) {
#pragma unroll
    for (int i = 0; i < BM / 32; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        *reinterpret_cast<unsigned short*>(O + (32 * i + mt_row(r, lane)) * PM_P_O + (32 * wv + (lane & 31)) * 2) = f2bf(acc[i][r]);
  }
  __syncthreads();
  for (int i = tid; i < BM * (PM_BN / 8); i += 256) {
    const int r = i / (PM_BN / 8), c = (i % (PM_BN / 8)) * 8;
    const long row = (long)r0 + r;
    const int col = n0 + c;
    if (row < g.rows && col < ncols) {
      const uint4 v = *reinterpret_cast<const uint4*>(O + r * PM_P_O + c * 2);
      pm_st16(out, SCATTER ? pm_base(g, row) + pm_seg(g, col) : row * ldo + col, v);
    }
  }
}

// ---- forward product: out / pre [rows][2C] = A . W^T, A = the gathered rows (NORM_LAST) or their LayerNorm (NORM_FIRST) ------------
// LDS: W tile [128][64], re-used as the output tile [BM][128] | A image ([BM][4C] NORM_FIRST, [BM][64] NORM_LAST)
constexpr int pm_max(int a, int b) { return a > b ? a : b; }
template <int BM> constexpr int pm_fwd_lds(int mode, int C) {
  return pm_max(PM_BN * PM_P_KM, BM * PM_P_O) + BM * (mode == DGSCT_PMERGE_NORM_FIRST ? 4 * C * 2 + 16 : PM_P_KM);
}
// NIT = 16-byte chunks per lane of a 4C row (NORM_FIRST): ceil(4C / 512)
template <int MODE, int BM, int NIT>
__global__ __launch_bounds__(256) void pm_fwd_k(PmGeom g, const void* __restrict__ x, const void* __restrict__ w, const float* __restrict__ ln_w,
                                                const float* __restrict__ ln_b, float eps, void* __restrict__ out, float* __restrict__ mu,
                                                float* __restrict__ rstd) {
  extern __shared__ __attribute__((aligned(16))) char pm_smem[];
  constexpr bool FIRST = MODE == DGSCT_PMERGE_NORM_FIRST;
  char* Bimg = pm_smem;
  char* Oimg = pm_smem;
  char* Aimg = pm_smem + pm_max(PM_BN * PM_P_KM, BM * PM_P_O);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K = 4 * g.C, N = 2 * g.C;
  const int r0 = blockIdx.x * BM;
  const int pa = FIRST ? K * 2 + 16 : PM_P_KM;
  const long last = g.rows - 1;

  if (FIRST) {
    // a wavefront owns RPW consecutive rows and takes them R at a time: the R * NIT loads of a batch are in flight together
    constexpr int RPW = BM / 4, R = 8 / NIT;
    static_assert(RPW % R == 0, "row batches must tile a wavefront's rows");
    const int nch = K / 8;
    const float invK = 1.f / (float)K;
    int so[NIT];
    bool cok[NIT];
    float lw[NIT][8], lb[NIT][8];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int c = lane + 64 * it;
      cok[it] = c < nch;
      const int cc = (cok[it] ? c : nch - 1) * 8;
      so[it] = pm_seg(g, cc);
      ldf<8>(ln_w, cc, lw[it]);
      ldf<8>(ln_b, cc, lb[it]);
    }
    const long rw = (long)r0 + wv * RPW;                   // lane l works out the address of the wavefront's row l % RPW, once
    const long mine = rw + (lane % RPW);
    const long mybase = pm_base(g, mine < g.rows ? mine : last);
    for (int t0 = 0; t0 < RPW; t0 += R) {
      uint4 raw[R][NIT];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const long base = pm_shfl(mybase, t0 + u);
#pragma unroll
        for (int it = 0; it < NIT; ++it) raw[u][it] = pm_ld16(x, base + so[it]);
      }
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int rr = wv * RPW + t0 + u;
        const long r = (long)r0 + rr;
        const bool rv = r < g.rows;
        float v[NIT][8];
        float s = 0.f;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          unpack<DT_BF16, 8>(raw[u][it], v[it]);
          if (cok[it]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[it][e];
          }
        }
        const float mean = group_sum(s, 64) * invK;
        float q = 0.f;
#pragma unroll
        for (int it = 0; it < NIT; ++it)
          if (cok[it]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[it][e] - mean; q += d * d; }
          }
        const float rs = rsqrtf(group_sum(q, 64) * invK + eps);
        if (lane == 0 && rv) { mu[r] = mean; rstd[r] = rs; }
#pragma unroll
        for (int it = 0; it < NIT; ++it)
          if (cok[it]) {
            float y[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) y[e] = rv ? (v[it][e] - mean) * rs * lw[it][e] + lb[it][e] : 0.f;
            *reinterpret_cast<uint4*>(Aimg + rr * pa + (lane + 64 * it) * 16) = pm_pack(y);
          }
      }
    }
  }
  // NORM_LAST: the rows this thread stages in every k-step (chunk i = it * 256 + tid of the [BM][64] tile: row i / 8, channels (i % 8) * 8)
  constexpr int AIT = BM * (PM_BK / 8) / 256;
  long abase[AIT];
  bool aok[AIT];
  if (!FIRST) {
#pragma unroll
    for (int it = 0; it < AIT; ++it) {
      const long r = (long)r0 + (it * 256 + tid) / 8;
      aok[it] = r < g.rows;
      abase[it] = pm_base(g, aok[it] ? r : last);
    }
  }
  const int nt0 = FIRST ? 0 : (int)blockIdx.y, nt1 = FIRST ? (N + PM_BN - 1) / PM_BN : (int)blockIdx.y + 1;
  for (int nt = nt0; nt < nt1; ++nt) {
    const int n0 = nt * PM_BN;
    const bool wave_on = n0 + 32 * wv < N;          // N % 64 == 0: a wavefront's 32 columns are all inside or all outside
    mt_f32x16 acc[BM / 32];
#pragma unroll
    for (int i = 0; i < BM / 32; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += PM_BK) {
      __syncthreads();                               // the previous tiles (and, first time round, the A image) are complete / consumed
      stage_tile<DT_BF16, PM_BN, PM_BK>(Bimg, PM_P_KM, w, K, n0, N, k0, K, tid);
      if (!FIRST) {
#pragma unroll
        for (int it = 0; it < AIT; ++it) {
          const int i = it * 256 + tid, c = (i % 8) * 8;
          uint4 raw = pm_ld16(x, abase[it] + pm_seg(g, k0 + c));
          if (!aok[it]) raw = make_uint4(0, 0, 0, 0);
          *reinterpret_cast<uint4*>(Aimg + (i / 8) * PM_P_KM + c * 2) = raw;
        }
      }
      __syncthreads();
      if (wave_on) {
#pragma unroll
        for (int i = 0; i < BM / 32; ++i)
          mma_tile<DT_BF16, true, true>(acc[i], FIRST ? Aimg + k0 * 2 : Aimg, pa, 32 * i, Bimg, PM_P_KM, 32 * wv, PM_BK, lane);
      }
    }
    pm_store_tile<BM, false>(g, acc, wave_on, Oimg, out, N, r0, n0, N, tid);   // (the next column tile starts with a barrier)
  }
}

// ---- backward product: D [rows][4C] = A [rows][2C] . W [2C][4C]; SCATTER: D's rows are virtual rows of dx ---------------------------
constexpr int PM_DG_BM = 64;
constexpr int PM_DG_LDS = PM_DG_BM * PM_P_KM + PM_BK * PM_P_MN + PM_DG_BM * PM_P_O;
template <bool SCATTER>
__global__ __launch_bounds__(256) void pm_dgemm_k(PmGeom g, const void* __restrict__ a, const void* __restrict__ w, void* __restrict__ d) {
  extern __shared__ __attribute__((aligned(16))) char pm_smem[];
  constexpr int BM = PM_DG_BM;
  char* Aimg = pm_smem;
  char* Bimg = Aimg + BM * PM_P_KM;
  char* Oimg = Bimg + PM_BK * PM_P_MN;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K = 2 * g.C, N = 4 * g.C;               // N % 128 == 0
  const int r0 = blockIdx.x * BM, n0 = blockIdx.y * PM_BN;
  const int rows = (int)g.rows;
  mt_f32x16 acc[BM / 32];
#pragma unroll
  for (int i = 0; i < BM / 32; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += PM_BK) {
    __syncthreads();
    stage_tile<DT_BF16, BM, PM_BK>(Aimg, PM_P_KM, a, K, r0, rows, k0, K, tid);
    stage_tile<DT_BF16, PM_BK, PM_BN>(Bimg, PM_P_MN, w, N, k0, K, n0, N, tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < BM / 32; ++i)
      mma_tile<DT_BF16, true, false>(acc[i], Aimg, PM_P_KM, 32 * i, Bimg, PM_P_MN, 32 * wv, PM_BK, lane);
  }
  pm_store_tile<BM, SCATTER>(g, acc, true, Oimg, d, N, r0, n0, N, tid);
}

// ---- LayerNorm backward over rows of Cn channels, one wavefront per row --------------------------------------------------------------
// dx = rstd (dy w - mean(dy w) - x^ mean(dy w x^)), x^ = (x - mu) rstd.  GATHER: x is the token map, the row is its virtual 4C row and dx
// is scattered to the four tokens; otherwise x (= pre) and dx are plain [rows][Cn].
// One row.  SUMS: the lane also adds dy x^ and dy (dy BEFORE the multiplication with ln_w) into its per-channel sums sw / sb, the
// row's terms of d ln_w / d ln_b; what reaches dx is the same arithmetic with and without.
template <bool GATHER, int NIT, bool SUMS>
__device__ __forceinline__ void pm_lnbwd_row(const PmGeom& g, int Cn, long row, int lane, const void* __restrict__ dy, const void* __restrict__ xs,
                                             const float* __restrict__ ln_w, const float* __restrict__ mu, const float* __restrict__ rstd,
                                             void* __restrict__ dx, float (&sw)[NIT][8], float (&sb)[NIT][8]) {
  const int nch = Cn / 8;
  const long base = GATHER ? pm_base(g, row) : row * Cn;
  const float m = mu[row], rs = rstd[row];
  float xh[NIT][8], dh[NIT][8];
  long off[NIT];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = lane + 64 * it, cc = (c < nch ? c : nch - 1) * 8;
    off[it] = base + (GATHER ? pm_seg(g, cc) : cc);
    const uint4 rx = pm_ld16(xs, off[it]);
    const uint4 rd = pm_ld16(dy, row * Cn + cc);
    float lw[8];
    ldf<8>(ln_w, cc, lw);
    unpack<DT_BF16, 8>(rx, xh[it]);
    unpack<DT_BF16, 8>(rd, dh[it]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xh[it][e] = (xh[it][e] - m) * rs;
      if (SUMS) { sw[it][e] += dh[it][e] * xh[it][e]; sb[it][e] += dh[it][e]; }      // (a clamped chunk's sums are never flushed)
      dh[it][e] *= lw[e];
      if (c < nch) { s1 += dh[it][e]; s2 += dh[it][e] * xh[it][e]; }
    }
  }
  group_sum2(s1, s2, 64);
  const float m1 = s1 / (float)Cn, m2 = s2 / (float)Cn;
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    if (lane + 64 * it < nch) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = rs * (dh[it][e] - m1 - xh[it][e] * m2);
      pm_st16(dx, off[it], pm_pack(o));
    }
}

template <bool GATHER, int NIT>
__global__ __launch_bounds__(256) void pm_lnbwd_k(PmGeom g, int Cn, const void* __restrict__ dy, const void* __restrict__ xs,
                                                  const float* __restrict__ ln_w, const float* __restrict__ mu, const float* __restrict__ rstd,
                                                  void* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= g.rows) return;                         // (no barrier in this kernel)
  float none[NIT][8];
  pm_lnbwd_row<GATHER, NIT, false>(g, Cn, row, lane, dy, xs, ln_w, mu, rstd, dx, none, none);
}

// ---- the same with the column sums of a trainable norm: d ln_w[c] = sum_r dy[r][c] x^[r][c], d ln_b[c] = sum_r dy[r][c] -----------------
// A wavefront walks the rows wave, wave + 4 gridDim.x, ... and keeps both sums of its 8 NIT channels in registers; the grid is at most one
// round of resident workgroups.  The four wavefronts combine by store / barrier / column-sum through LDS ([4][Cn] floats, one
// quantity after the other), and the workgroup leaves with plain stores into its own partials part[wg][2][Cn], finished by part_reduce.
constexpr int PM_SUMS_MAX_WG = 2048, PM_SUMS_ROWS_PER_WG = 32;
static long pm_sums_max_wgs(long rows) {
  const long n = (rows + PM_SUMS_ROWS_PER_WG - 1) / PM_SUMS_ROWS_PER_WG;
  return n < PM_SUMS_MAX_WG ? n : PM_SUMS_MAX_WG;
}
template <bool GATHER, int NIT>
__global__ __launch_bounds__(256) void pm_lnbwd_sums_k(PmGeom g, int Cn, const void* __restrict__ dy, const void* __restrict__ xs,
                                                       const float* __restrict__ ln_w, const float* __restrict__ mu,
                                                       const float* __restrict__ rstd, void* __restrict__ dx, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char pm_smem[];
  float* red = reinterpret_cast<float*>(pm_smem);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nch = Cn / 8;
  float sw[NIT][8], sb[NIT][8];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int e = 0; e < 8; ++e) sw[it][e] = sb[it][e] = 0.f;
  for (long row = (long)blockIdx.x * 4 + wv; row < g.rows; row += 4L * gridDim.x)
    pm_lnbwd_row<GATHER, NIT, true>(g, Cn, row, lane, dy, xs, ln_w, mu, rstd, dx, sw, sb);
  float* p = part + (long)blockIdx.x * 2 * Cn;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (lane + 64 * it < nch) {
        const float(&a)[8] = q == 0 ? sw[it] : sb[it];
        float* d = red + wv * Cn + (lane + 64 * it) * 8;
        *reinterpret_cast<float4*>(d) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4*>(d + 4) = make_float4(a[4], a[5], a[6], a[7]);
      }
    __syncthreads();
    for (int c = tid; c < Cn; c += 256) p[q * Cn + c] = (red[c] + red[Cn + c]) + (red[2 * Cn + c] + red[3 * Cn + c]);
  }
}

// ---- weight gradient: dW [2C][4C] += D^T . A over a slab of rows ---------------------------------------------------------------------------
// D [rows][2C] bf16 (dout for NORM_FIRST, dpre for NORM_LAST), A [rows][4C] = the operand the forward multiplied with W: the gathered row
// (NORM_LAST) or bf16(x^ ln_w + ln_b) of it (NORM_FIRST: pm_fwd_k's expression re-evaluated from the saved mu / rstd -- nothing pins
// the two kernels to the same fma contraction, so an element may differ from the forward's by one bf16 ulp).  A is staged from the token map
// and exists in LDS only.  The rows are the contraction, so both LDS images are [64 rows][128] MN-major (transpose reads).  A workgroup
// owns a 128 x 128 tile of dW (blockIdx.x: column tile fastest) and the slab blockIdx.y of `sps` 64-row steps; a wavefront owns 32 columns
// of the tile and all four 32-row blocks (2C % 64 == 0: a block of the ragged last tile is wholly inside or outside).  fp32 atomicAdd
// into dW: one contributor per slab, at most PM_WG_MAX_SLABS.
constexpr int PM_WG_BR = 64, PM_WG_MAX_SLABS = 40;
constexpr int PM_WG_LDS = 2 * PM_WG_BR * PM_P_MN;
template <bool FIRST>
__global__ __launch_bounds__(256) void pm_wgrad_k(PmGeom g, int sps, const void* __restrict__ d, const void* __restrict__ x,
                                                  const float* __restrict__ ln_w, const float* __restrict__ ln_b, const float* __restrict__ mu,
                                                  const float* __restrict__ rstd, float* __restrict__ dw) {
  extern __shared__ __attribute__((aligned(16))) char pm_smem[];
  char* Dimg = pm_smem;
  char* Aimg = pm_smem + PM_WG_BR * PM_P_MN;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K = 4 * g.C, N = 2 * g.C;
  const int kt = K / PM_BN;
  const int n0 = ((int)blockIdx.x / kt) * PM_BN, k0 = ((int)blockIdx.x % kt) * PM_BN;
  const int rows = (int)g.rows;
  const int rbeg = (int)blockIdx.y * sps * PM_WG_BR;
  const int rend = imin_d(rows, rbeg + sps * PM_WG_BR);
  // this thread's chunk of every 16-row group of the A tile: channels k0 + ac .. + 7 of row tid / 16
  const int ac = (tid & 15) * 8, ar = tid >> 4;
  const int so = pm_seg(g, k0 + ac);
  float lw[8], lb[8];
  if (FIRST) { ldf<8>(ln_w, k0 + ac, lw); ldf<8>(ln_b, k0 + ac, lb); }
  mt_f32x16 acc[PM_BN / 32];
#pragma unroll
  for (int i = 0; i < PM_BN / 32; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  for (int r0 = rbeg; r0 < rend; r0 += PM_WG_BR) {
    uint4 raw[PM_WG_BR / 16];
    float mean[PM_WG_BR / 16], rs[PM_WG_BR / 16];
#pragma unroll
    for (int it = 0; it < PM_WG_BR / 16; ++it) {
      const int r = r0 + it * 16 + ar, rc = r < rows ? r : rows - 1;
      raw[it] = pm_ld16(x, pm_base(g, rc) + so);
      if (FIRST) { mean[it] = mu[rc]; rs[it] = rstd[rc]; }
    }
    __syncthreads();                                 // the previous step's images are consumed
    stage_tile<DT_BF16, PM_WG_BR, PM_BN>(Dimg, PM_P_MN, d, N, r0, rows, n0, N, tid);
#pragma unroll
    for (int it = 0; it < PM_WG_BR / 16; ++it) {
      const bool rv = r0 + it * 16 + ar < rows;
      uint4 a = raw[it];
      if (FIRST) {
        float v[8], y[8];
        unpack<DT_BF16, 8>(raw[it], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = rv ? (v[e] - mean[it]) * rs[it] * lw[e] + lb[e] : 0.f;
        a = pm_pack(y);
      } else if (!rv) {
        a = make_uint4(0, 0, 0, 0);
      }
      *reinterpret_cast<uint4*>(Aimg + (it * 16 + ar) * PM_P_MN + ac * 2) = a;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PM_BN / 32; ++i)
      if (n0 + 32 * i < N)
        mma_tile<DT_BF16, false, false>(acc[i], Dimg, PM_P_MN, 32 * i, Aimg, PM_P_MN, 32 * wv, PM_WG_BR, lane);
  }
  if (rbeg >= rend) return;
#pragma unroll
  for (int i = 0; i < PM_BN / 32; ++i)
    if (n0 + 32 * i < N) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        unsafeAtomicAdd(dw + (long)(n0 + 32 * i + mt_row(r, lane)) * K + k0 + 32 * wv + (lane & 31), acc[i][r]);
    }
}

static bool pm_check(const char* who, int mode, int B, int H, int W, int C, PmGeom& g) {
  if (mode != DGSCT_PMERGE_NORM_FIRST && mode != DGSCT_PMERGE_NORM_LAST) { set_error("%s: unknown mode %d", who, mode); return false; }
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2) { set_error("%s: need B >= 1 and H, W even and >= 2 (got %d, %d x %d)", who, B, H, W); return false; }
  const int cmax = mode == DGSCT_PMERGE_NORM_FIRST ? 1536 / 4 : 1536 / 2;
  if (C < 32 || C % 32 || C > cmax) {
    set_error("%s: need C a multiple of 32, 32 .. %d (%s; got %d)", who, cmax, mode == DGSCT_PMERGE_NORM_FIRST ? "NORM_FIRST: 4C <= 1536" : "NORM_LAST: 2C <= 1536", C);
    return false;
  }
  if ((int64_t)B * H * W > 0x7fffffffLL / 4) { set_error("%s: tensor too large", who); return false; }
  g.B = B; g.H = H; g.W = W; g.C = C; g.H2 = H / 2; g.W2 = W / 2;
  g.rows = (long)B * g.H2 * g.W2;
  return true;
}

template <typename K, typename... A>
static void pm_launch(K kern, dim3 grid, size_t shmem, hipStream_t s, A... args) {
  if (shmem > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess) {
    (void)hipGetLastError();
    set_error("dgsct_patch_merge: the device refuses %zu bytes of dynamic LDS per workgroup", shmem);
    return;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), shmem, s, args...);
}

template <bool GATHER>
static void pm_lnbwd(dim3 grid, hipStream_t s, const PmGeom& g, int Cn, const void* dy, const void* xs, const float* ln_w, const float* mu,
                     const float* rstd, void* dx) {
  if (Cn <= 512) hipLaunchKernelGGL((pm_lnbwd_k<GATHER, 1>), grid, dim3(256), 0, s, g, Cn, dy, xs, ln_w, mu, rstd, dx);
  else if (Cn <= 1024) hipLaunchKernelGGL((pm_lnbwd_k<GATHER, 2>), grid, dim3(256), 0, s, g, Cn, dy, xs, ln_w, mu, rstd, dx);
  else hipLaunchKernelGGL((pm_lnbwd_k<GATHER, 3>), grid, dim3(256), 0, s, g, Cn, dy, xs, ln_w, mu, rstd, dx);
}

// the column-sum variant: at most one round of resident workgroups, each with at least PM_SUMS_ROWS_PER_WG rows where there are that many
template <bool GATHER>
static void pm_lnbwd_sums(hipStream_t s, const PmGeom& g, int Cn, const void* dy, const void* xs, const float* ln_w, const float* mu,
                          const float* rstd, void* dx, float* part, float* dln_w, float* dln_b) {
  const size_t shmem = (size_t)4 * Cn * sizeof(float);
  auto go = [&](auto kern) {
    long nwg = wg_capacity(reinterpret_cast<const void*>(kern), shmem);
    const long most = pm_sums_max_wgs(g.rows);
    if (nwg > most) nwg = most;
    if (nwg < 1) nwg = 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(256), shmem, s, g, Cn, dy, xs, ln_w, mu, rstd, dx, part);
    PartTable t;
    t.NQ = 2; t.C = Cn;
    t.d[0] = PartDesc{0, 1, (int)nwg, 1, dln_w, 0, 1.f};
    t.d[1] = PartDesc{1, 1, (int)nwg, 1, dln_b, 0, 1.f};
    part_reduce((void*)s, part, t, 2);
  };
  if (Cn <= 512) go(pm_lnbwd_sums_k<GATHER, 1>);
  else if (Cn <= 1024) go(pm_lnbwd_sums_k<GATHER, 2>);
  else go(pm_lnbwd_sums_k<GATHER, 3>);
}

template <bool FIRST>
static void pm_wgrad(hipStream_t s, const PmGeom& g, const void* d, const void* x, const float* ln_w, const float* ln_b, const float* mu,
                     const float* rstd, float* dw) {
  const long steps = (g.rows + PM_WG_BR - 1) / PM_WG_BR;
  const long sps = (steps + PM_WG_MAX_SLABS - 1) / PM_WG_MAX_SLABS;          // whole 64-row steps per slab
  const long slabs = (steps + sps - 1) / sps;                                // <= PM_WG_MAX_SLABS, none empty
  const int tiles = ((2 * g.C + PM_BN - 1) / PM_BN) * (4 * g.C / PM_BN);
  hipLaunchKernelGGL((pm_wgrad_k<FIRST>), dim3((unsigned)tiles, (unsigned)slabs), dim3(256), (size_t)PM_WG_LDS, s, g, (int)sps, d, x, ln_w, ln_b,
                     mu, rstd, dw);
}

static long pm_ws_rows_bytes(int mode, const PmGeom& g) { return g.rows * (mode == DGSCT_PMERGE_NORM_FIRST ? 4 : 2) * g.C * 2; }
static long pm_part_offset(int mode, const PmGeom& g) { return (pm_ws_rows_bytes(mode, g) + 255) / 256 * 256; }

}  // namespace dgsct

using namespace dgsct;

extern "C" {

int64_t dgsct_patch_merge_ws_bytes(int mode, int B, int H, int W, int C) {
  clear_error();
  PmGeom g;
  if (!pm_check("dgsct_patch_merge_ws_bytes", mode, B, H, W, C, g)) return -1;
  return pm_ws_rows_bytes(mode, g);
}

int64_t dgsct_patch_merge_params_ws_bytes(int mode, int B, int H, int W, int C) {
  clear_error();
  PmGeom g;
  if (!pm_check("dgsct_patch_merge_params_ws_bytes", mode, B, H, W, C, g)) return -1;
  const long cn = (mode == DGSCT_PMERGE_NORM_FIRST ? 4 : 2) * C;
  return pm_part_offset(mode, g) + pm_sums_max_wgs(g.rows) * 2 * cn * (long)sizeof(float);
}

int dgsct_patch_merge_forward(int mode, int B, int H, int W, int C, const void* x, const void* w_bf16, const float* ln_w, const float* ln_b,
                              float eps, void* out, void* pre, float* mu, float* rstd, void* stream) {
  clear_error();
  const char* who = "dgsct_patch_merge_forward";
  PmGeom g;
  if (!pm_check(who, mode, B, H, W, C, g)) return 2;
  if (!x || !w_bf16 || !ln_w || !ln_b || !out || !mu || !rstd) { set_error("%s: NULL argument", who); return 2; }
  if (mode == DGSCT_PMERGE_NORM_LAST && !pre) { set_error("%s: NORM_LAST needs `pre` (the product before the norm, kept for backward)", who); return 2; }
  hipStream_t s = (hipStream_t)stream;
  clear_async();
  if (mode == DGSCT_PMERGE_NORM_FIRST) {
    // up to 4C = 384 a workgroup takes 64 rows (W is re-read half as often and two workgroups still share a CU's LDS), above 32
    auto go = [&](auto kern, int bm, size_t shmem) {
      pm_launch(kern, dim3((unsigned)((g.rows + bm - 1) / bm)), shmem, s, g, x, w_bf16, ln_w, ln_b, eps, out, mu, rstd);
    };
    if (4 * C <= 384) go(pm_fwd_k<DGSCT_PMERGE_NORM_FIRST, 64, 1>, 64, (size_t)pm_fwd_lds<64>(mode, C));
    else if (4 * C <= 512) go(pm_fwd_k<DGSCT_PMERGE_NORM_FIRST, 32, 1>, 32, (size_t)pm_fwd_lds<32>(mode, C));
    else if (4 * C <= 1024) go(pm_fwd_k<DGSCT_PMERGE_NORM_FIRST, 32, 2>, 32, (size_t)pm_fwd_lds<32>(mode, C));
    else go(pm_fwd_k<DGSCT_PMERGE_NORM_FIRST, 32, 3>, 32, (size_t)pm_fwd_lds<32>(mode, C));
    check_async(who);
    return has_error() ? 1 : 0;
  }
  pm_launch(pm_fwd_k<DGSCT_PMERGE_NORM_LAST, 64, 1>, dim3((unsigned)((g.rows + 63) / 64), (unsigned)((2 * C + PM_BN - 1) / PM_BN)),
            (size_t)pm_fwd_lds<64>(mode, C), s, g, x, w_bf16, ln_w, ln_b, eps, pre, mu, rstd);
  check_async(who);
  if (has_error()) return 1;
  return dgsct_layer_norm_forward(DGSCT_BF16, g.rows, 2 * C, pre, ln_w, ln_b, eps, nullptr, out, mu, rstd, stream);
}

int dgsct_patch_merge_backward(int mode, int B, int H, int W, int C, const void* dout, const void* x, const void* w_bf16, const float* ln_w,
                               const void* pre, const float* mu, const float* rstd, float eps, void* dx, void* ws, void* stream) {
  clear_error();
  const char* who = "dgsct_patch_merge_backward";
  PmGeom g;
  if (!pm_check(who, mode, B, H, W, C, g)) return 2;
  if (!dout || !w_bf16 || !ln_w || !mu || !rstd || !dx || !ws) { set_error("%s: NULL argument", who); return 2; }
  if (mode == DGSCT_PMERGE_NORM_FIRST ? !x : !pre) { set_error("%s: NORM_FIRST needs `x`, NORM_LAST needs `pre`", who); return 2; }
  (void)eps;                                          // rstd already carries it
  hipStream_t s = (hipStream_t)stream;
  const dim3 ggrid((unsigned)((g.rows + PM_DG_BM - 1) / PM_DG_BM), (unsigned)(4 * C / PM_BN)), rgrid((unsigned)((g.rows + 3) / 4));
  clear_async();
  if (mode == DGSCT_PMERGE_NORM_FIRST) {
    pm_launch(pm_dgemm_k<false>, ggrid, (size_t)PM_DG_LDS, s, g, dout, w_bf16, ws);
    pm_lnbwd<true>(rgrid, s, g, 4 * C, (const void*)ws, x, ln_w, mu, rstd, dx);
  } else {
    pm_lnbwd<false>(rgrid, s, g, 2 * C, dout, pre, ln_w, mu, rstd, ws);
    pm_launch(pm_dgemm_k<true>, ggrid, (size_t)PM_DG_LDS, s, g, (const void*)ws, w_bf16, dx);
  }
  check_async(who);
  return has_error() ? 1 : 0;
}

int dgsct_patch_merge_backward_params(int mode, int B, int H, int W, int C, const void* dout, const void* x, const void* w_bf16,
                                      const float* ln_w, const float* ln_b, const void* pre, const float* mu, const float* rstd, float eps,
                                      void* dx, float* dw, float* dln_w, float* dln_b, void* ws, void* stream) {
  clear_error();
  const char* who = "dgsct_patch_merge_backward_params";
  PmGeom g;
  if (!pm_check(who, mode, B, H, W, C, g)) return 2;
  if (!dout || !x || !w_bf16 || !ln_w || !ln_b || !mu || !rstd || !dx || !dw || !dln_w || !dln_b || !ws) { set_error("%s: NULL argument", who); return 2; }
  if (mode == DGSCT_PMERGE_NORM_LAST && !pre) { set_error("%s: NORM_LAST needs `pre` as well as `x`", who); return 2; }
  (void)eps;                                          // rstd already carries it
  hipStream_t s = (hipStream_t)stream;
  const dim3 ggrid((unsigned)((g.rows + PM_DG_BM - 1) / PM_DG_BM), (unsigned)(4 * C / PM_BN));
  const int cn = (mode == DGSCT_PMERGE_NORM_FIRST ? 4 : 2) * C;
  float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + pm_part_offset(mode, g));
  clear_async();
  if (hipMemsetAsync(dw, 0, (size_t)8 * C * C * sizeof(float), s) != hipSuccess || hipMemsetAsync(dln_w, 0, (size_t)cn * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(dln_b, 0, (size_t)cn * sizeof(float), s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: hipMemsetAsync of the gradient buffers failed", who);
    return 1;
  }
  if (mode == DGSCT_PMERGE_NORM_FIRST) {
    pm_launch(pm_dgemm_k<false>, ggrid, (size_t)PM_DG_LDS, s, g, dout, w_bf16, ws);
    pm_lnbwd_sums<true>(s, g, cn, (const void*)ws, x, ln_w, mu, rstd, dx, part, dln_w, dln_b);
    pm_wgrad<true>(s, g, dout, x, ln_w, ln_b, mu, rstd, dw);
  } else {
    pm_lnbwd_sums<false>(s, g, cn, dout, pre, ln_w, mu, rstd, ws, part, dln_w, dln_b);
    pm_launch(pm_dgemm_k<true>, ggrid, (size_t)PM_DG_LDS, s, g, (const void*)ws, w_bf16, dx);
    pm_wgrad<false>(s, g, (const void*)ws, x, ln_w, ln_b, mu, rstd, dw);
  }
  check_async(who);
  return has_error() ? 1 : 0;
}

}  // extern "C"
