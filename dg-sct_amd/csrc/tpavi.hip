// The audio-visual TPAVI block of the AVS models in LINEAR form (reference DG-SCT/AVS/avs_scripts/avs_s4/model/TPAVI.py, mode 'dot',
// audio branch).  'dot' has no softmax and phi(audio) is constant over h, w, so the block up to its BatchNorm
// is a per-clip C x C linear map of x; the per-clip setup (A_b [C][C], c_b [C]; ~13 MFLOP) stays in torch, these kernels do the passes
// over x, fp32 throughout:
//   u = A_b x_p + c_b     v = BatchNorm3d(u) (batch statistics; eval: folded into A, c by the caller)     z = LayerNorm_C(v + x)
//
// One engine for every pass: a workgroup (256 threads, 4 wavefronts) owns a TILE of 64 positions of one (b, t) plane (tiles never
// straddle planes: H W = 49 is one tile with 49 live positions) and ALL C channels of it, so the LayerNorm over C stays inside the
// workgroup.  x[:, tile] sits in LDS as [C][64]; A_b streams through LDS in 64-column chunks; u is C/32 x 2 MFMA tiles of
// v_mfma_f32_32x32x2_f32 (mma_tile.h, the fp32 parity engine of gemm.hip), C/64 per wavefront.  Wavefront w owns the position half w & 1
// and the channel blocks (w >> 1) + 2 j.  Planes are not aligned, so x, z, dz, dx move as scalar loads / stores, 32 consecutive floats
// per half wavefront; addresses of dead positions are clamped and the register masked.
//
// forward, train: tp_stats_k (sum of u - mu0 and of (u - mu0)^2 per channel; mu0 is the caller's mean of u from the frame sums, so the
//   variance is accumulated centred) -> tp_bn_fin_k (rows summed in row order in double; mean, 1/std, running statistics) -> tp_apply_k
//   (u recomputed, BatchNorm, residual, LayerNorm, z).  eval: tp_apply_k alone.
// backward: tp_bwd1_k (recomputes u, v, the LayerNorm statistics; dr = LayerNorm backward, written into the dx buffer; per-channel sums
//   for d ln_w, d ln_b, d bn_w, d bn_b) -> tp_rows_k -> tp_bwd2_k (recomputes u; du from dr through the BatchNorm; dx = dr + A_b^T du + ds;
//   du stored once in the workspace) -> tp_wgrad_k (dA_b = sum_p du_p x_p^T, dc_b = sum_p du_p; G workgroups per clip and 64-column block)
//   -> tp_wsum_k.
// Every reduction is per-workgroup partial rows summed in a fixed order: no atomics, results are bit-identical from call to call.
// Grids are capped (TP_MAX_WGS persistent workgroups over the tiles; TP_MAX_SPLIT per clip in tp_wgrad_k).
//
// The extern "C" entry points live here (like csrc/head.hip's): the host emulation of the CPU tests has no TPAVI.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dgsct.h"
#include "prims.h"
#include "device_util.h"
#include "mma_tile.h"
#include "err.h"

namespace dgsct {

constexpr int TP_P = 64, TP_KC = 64, TP_MAX_WGS = 256, TP_MAX_SPLIT = 16, TP_MAX_T = 16, TP_MIN_C = 64, TP_MAX_C = 256;
constexpr int TP_APITCH = TP_KC * 4 + 16;     // bytes: the [C][KC] k-major chunk of A (mma_tile.h km_pitch)
constexpr int TP_WPITCH = TP_P * 4 + 16;      // bytes: the [rows][64] k-major images of tp_wgrad_k

struct TpArgs {
  int B, C, T, HW, ntp, ntiles;
  const float* x; long xb, xc, xt;            // element strides of (b, c, t); a plane's H W positions are contiguous
  float* z; long zb, zc, zt;                  // forward: z; backward: dx (holds dr between tp_bwd1_k and tp_bwd2_k)
  const float* dz; long gb, gc, gt;
  const float *A, *cvec, *mu0, *stat, *bn_w, *bn_b, *ln_w, *ln_b, *ds, *k1, *k2;
  float ln_eps, invM;
  float *part, *du;
};

#define TP_FOR(j, r) _Pragma("unroll") for (int j = 0; j < TPW; ++j) _Pragma("unroll") for (int r = 0; r < 16; ++r)

__device__ __forceinline__ void tp_tile(const TpArgs& p, int tau, int& b, int& t, int& p0, int& nv) {
  const int per = p.T * p.ntp;
  b = tau / per;
  const int q = tau - b * per;
  t = q / p.ntp;
  p0 = (q - t * p.ntp) * TP_P;
  nv = imin_d(TP_P, p.HW - p0);
}
// rows x 64 positions of one plane -> img[r][q] (pitch in floats); positions >= nv arrive as zeros (clamped address, masked register)
// rows is a multiple of 64.  16 loads in flight per thread before the first LDS store: with one wavefront per SIMD a load-store-load chain
// would pay the memory latency 64 times per tile.
__device__ __forceinline__ void tp_load_rows(float* img, int pitchf, const float* src, long rs, int rows, int nv, int tid) {
  const int q = tid & 63, r0 = tid >> 6, qc = q < nv ? q : nv - 1;
  for (int rb = 0; rb < rows; rb += 64) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = src[(long)(rb + 4 * u + r0) * rs + qc];
#pragma unroll
    for (int u = 0; u < 16; ++u) img[(rb + 4 * u + r0) * pitchf + q] = q < nv ? v[u] : 0.f;
  }
}
// acc = A_b . Xs   (A_b [C][C] row-major in global, Xs [C][64] in LDS).  Starts with a barrier: Xs written before the call is visible.
template <int TPW>
__device__ __forceinline__ void tp_gemm_u(mt_f32x16 (&acc)[TPW], const float* Ab, char* Aimg, const float* Xs, int tid) {
  constexpr int C = 64 * TPW;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  for (int k0 = 0; k0 < C; k0 += TP_KC) {
    __syncthreads();
    stage_tile_f32<DT_F32, C, TP_KC, false>(Aimg, nullptr, TP_APITCH, Ab, C, 0, C, k0, C, tid);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      mma_tile<DT_F32, true, false>(acc[j], Aimg, TP_APITCH, 32 * ((wave >> 1) + 2 * j), reinterpret_cast<const char*>(Xs + k0 * TP_P),
                                    TP_P * 4, 32 * (wave & 1), TP_KC, lane);
  }
}
// acc = A_b^T . Ds   (contraction over A's ROW index)
template <int TPW>
__device__ __forceinline__ void tp_gemm_t(mt_f32x16 (&acc)[TPW], const float* Ab, char* Aimg, const float* Ds, int tid) {
  constexpr int C = 64 * TPW;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  for (int k0 = 0; k0 < C; k0 += TP_KC) {
    __syncthreads();
    stage_tile_f32<DT_F32, TP_KC, C, false>(Aimg, nullptr, C * 4, Ab, C, k0, C, 0, C, tid);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      mma_tile<DT_F32, false, false>(acc[j], Aimg, C * 4, 32 * ((wave >> 1) + 2 * j), reinterpret_cast<const char*>(Ds + k0 * TP_P),
                                     TP_P * 4, 32 * (wave & 1), TP_KC, lane);
  }
}
// sum over the C channels of one position: the two lane halves and the two wavefronts that share the position half.  red: [2][64]
__device__ __forceinline__ float tp_pos_sum(float part, float* red, int wave, int lane, int pos) {
  part += __shfl_xor(part, 32, 64);
  if (lane < 32) red[(wave >> 1) * TP_P + pos] = part;
  __syncthreads();
  return red[pos] + red[TP_P + pos];
}
// sum over the tile's 64 positions of f(j, r), per channel: through buf [C][64]; thread c < C returns channel c's sum (rotated start:
// conflict-free), the others 0
template <int TPW, typename F>
__device__ __forceinline__ float tp_chan_sum(float* buf, int wave, int lane, int tid, F f) {
  constexpr int C = 64 * TPW;
  const int pos = 32 * (wave & 1) + (lane & 31);
  __syncthreads();
  TP_FOR(j, r) buf[(32 * ((wave >> 1) + 2 * j) + mt_row(r, lane)) * TP_P + pos] = f(j, r);
  __syncthreads();
  float s = 0.f;
  if (tid < C)
    for (int q = 0; q < TP_P; ++q) s += buf[tid * TP_P + ((q + tid) & (TP_P - 1))];
  return s;
}

#define TP_PROLOGUE                                                                                          \
  constexpr int C = 64 * TPW;                                                                                \
  extern __shared__ float4 tp_smem4[];                                                                       \
  float* Xs = reinterpret_cast<float*>(tp_smem4);                                                            \
  char* Aimg = reinterpret_cast<char*>(Xs + C * TP_P);                                                       \
  float* red = reinterpret_cast<float*>(Aimg + C * TP_APITCH);                                               \
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, mt0 = wave >> 1;                            \
  const int pos = 32 * (wave & 1) + (lane & 31);                                                             \
  (void)red; (void)mt0
#define TP_CH(j, r) (32 * (mt0 + 2 * (j)) + mt_row((r), lane))

static size_t tp_lds(int C) { return (size_t)C * TP_P * 4 + (size_t)C * TP_APITCH + 8 * TP_P * 4; }

// s[b][t][c] = sum over the plane; one wavefront per plane
__global__ __launch_bounds__(256) void tp_frame_sum_k(const TpArgs p, float* s) {
  const long plane = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (plane >= (long)p.B * p.T * p.C) return;
  const int c = (int)(plane % p.C), t = (int)((plane / p.C) % p.T), b = (int)(plane / ((long)p.C * p.T));
  const float* src = p.x + b * p.xb + c * p.xc + t * p.xt;
  float a = 0.f;
  for (int q = lane; q < p.HW; q += 64) a += src[q];
  a = group_sum(a, 64);
  if (lane == 0) s[plane] = a;
}

template <int TPW>
__global__ __launch_bounds__(256) void tp_stats_k(const TpArgs p) {
  TP_PROLOGUE;
  float a1 = 0.f, a2 = 0.f;
  for (int tau = blockIdx.x; tau < p.ntiles; tau += gridDim.x) {
    int b, t, p0, nv;
    tp_tile(p, tau, b, t, p0, nv);
    __syncthreads();
    tp_load_rows(Xs, TP_P, p.x + b * p.xb + t * p.xt + p0, p.xc, C, nv, tid);
    mt_f32x16 acc[TPW];
    tp_gemm_u<TPW>(acc, p.A + (long)b * C * C, Aimg, Xs, tid);
    TP_FOR(j, r) {
      const int ch = TP_CH(j, r);
      acc[j][r] = pos < nv ? acc[j][r] + p.cvec[b * C + ch] - p.mu0[ch] : 0.f;
    }
    a1 += tp_chan_sum<TPW>(Xs, wave, lane, tid, [&](int j, int r) { return acc[j][r]; });
    a2 += tp_chan_sum<TPW>(Xs, wave, lane, tid, [&](int j, int r) { return acc[j][r] * acc[j][r]; });
  }
  if (tid < C) {
    p.part[(long)blockIdx.x * 2 * C + tid] = a1;
    p.part[(long)blockIdx.x * 2 * C + C + tid] = a2;
  }
}

// one workgroup: the G rows in row order, in double.  stat = mean [C] | 1/std [C]; running statistics as nn.BatchNorm3d updates them
__global__ __launch_bounds__(256) void tp_bn_fin_k(const float* part, int G, int C, double M, const float* mu0, float* stat, float* run_mean,
                                                   float* run_var, float momentum, float eps) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s1 = 0., s2 = 0.;
  for (int g = 0; g < G; ++g) { s1 += part[(long)g * 2 * C + c]; s2 += part[(long)g * 2 * C + C + c]; }
  const double d = s1 / M, mean = mu0[c] + d;
  double var = s2 / M - d * d;
  if (var < 0.) var = 0.;
  stat[c] = (float)mean;
  stat[C + c] = (float)(1. / sqrt(var + (double)eps));
  if (run_mean) run_mean[c] = (float)((1. - momentum) * run_mean[c] + momentum * mean);
  if (run_var) run_var[c] = (float)((1. - momentum) * run_var[c] + momentum * (M > 1. ? var * M / (M - 1.) : var));
}

template <int TPW>
__global__ __launch_bounds__(256) void tp_apply_k(const TpArgs p) {
  TP_PROLOGUE;
  for (int tau = blockIdx.x; tau < p.ntiles; tau += gridDim.x) {
    int b, t, p0, nv;
    tp_tile(p, tau, b, t, p0, nv);
    __syncthreads();
    tp_load_rows(Xs, TP_P, p.x + b * p.xb + t * p.xt + p0, p.xc, C, nv, tid);
    mt_f32x16 acc[TPW];
    tp_gemm_u<TPW>(acc, p.A + (long)b * C * C, Aimg, Xs, tid);
    float s = 0.f;
    TP_FOR(j, r) {
      const int ch = TP_CH(j, r);
      float u = acc[j][r] + p.cvec[b * C + ch];
      if (p.stat) u = (u - p.stat[ch]) * p.stat[C + ch] * p.bn_w[ch] + p.bn_b[ch];
      u += Xs[ch * TP_P + pos];
      acc[j][r] = u;
      s += u;
    }
    const float mean = tp_pos_sum(s, red, wave, lane, pos) * (1.f / C);
    s = 0.f;
    TP_FOR(j, r) { const float d = acc[j][r] - mean; s += d * d; }
    const float rs = 1.f / sqrtf(tp_pos_sum(s, red + 2 * TP_P, wave, lane, pos) * (1.f / C) + p.ln_eps);
    if (pos < nv) {
      float* dst = p.z + b * p.zb + t * p.zt + p0 + pos;
      TP_FOR(j, r) {
        const int ch = TP_CH(j, r);
        dst[ch * p.zc] = (acc[j][r] - mean) * rs * p.ln_w[ch] + p.ln_b[ch];
      }
    }
  }
}

// LayerNorm backward per position; dr -> the dx buffer; partial row of the workgroup: d ln_w | d ln_b | sum dr | sum dr u^ (each [C])
template <int TPW>
__global__ __launch_bounds__(256) void tp_bwd1_k(const TpArgs p) {
  TP_PROLOGUE;
  float a_lw = 0.f, a_lb = 0.f, a_bb = 0.f, a_bw = 0.f;
  for (int tau = blockIdx.x; tau < p.ntiles; tau += gridDim.x) {
    int b, t, p0, nv;
    tp_tile(p, tau, b, t, p0, nv);
    __syncthreads();
    tp_load_rows(Xs, TP_P, p.x + b * p.xb + t * p.xt + p0, p.xc, C, nv, tid);
    mt_f32x16 acc[TPW];
    float uh[TPW][16], g[TPW][16];
    tp_gemm_u<TPW>(acc, p.A + (long)b * C * C, Aimg, Xs, tid);
    float s = 0.f;
    TP_FOR(j, r) {
      const int ch = TP_CH(j, r);
      float u = acc[j][r] + p.cvec[b * C + ch];
      uh[j][r] = 0.f;
      if (p.stat) {
        uh[j][r] = (u - p.stat[ch]) * p.stat[C + ch];
        u = uh[j][r] * p.bn_w[ch] + p.bn_b[ch];
      }
      u += Xs[ch * TP_P + pos];
      acc[j][r] = u;
      s += u;
    }
    const float mean = tp_pos_sum(s, red, wave, lane, pos) * (1.f / C);
    s = 0.f;
    TP_FOR(j, r) { const float d = acc[j][r] - mean; s += d * d; }
    const float rs = 1.f / sqrtf(tp_pos_sum(s, red + 2 * TP_P, wave, lane, pos) * (1.f / C) + p.ln_eps);
    float sg = 0.f, sgy = 0.f;
    const float* gsrc = p.dz + b * p.gb + t * p.gt + p0 + (pos < nv ? pos : nv - 1);
    TP_FOR(j, r) {
      const int ch = TP_CH(j, r);
      const float y = (acc[j][r] - mean) * rs;
      float dzv = gsrc[ch * p.gc];
      if (pos >= nv) dzv = 0.f;
      acc[j][r] = y;
      g[j][r] = dzv;
      const float gg = dzv * p.ln_w[ch];
      sg += gg;
      sgy += gg * y;
    }
    sg = tp_pos_sum(sg, red + 4 * TP_P, wave, lane, pos) * (1.f / C);
    sgy = tp_pos_sum(sgy, red + 6 * TP_P, wave, lane, pos) * (1.f / C);
    a_lw += tp_chan_sum<TPW>(Xs, wave, lane, tid, [&](int j, int r) { return g[j][r] * acc[j][r]; });
    a_lb += tp_chan_sum<TPW>(Xs, wave, lane, tid, [&](int j, int r) { return g[j][r]; });
    float* dst = p.z + b * p.zb + t * p.zt + p0 + pos;
    TP_FOR(j, r) {
      const int ch = TP_CH(j, r);
      const float dr = rs * (g[j][r] * p.ln_w[ch] - sg - acc[j][r] * sgy);      // 0 at dead positions: g = sg = sgy = 0 there
      g[j][r] = dr;
      if (pos < nv) dst[ch * p.zc] = dr;
    }
    if (p.stat) {
      a_bb += tp_chan_sum<TPW>(Xs, wave, lane, tid, [&](int j, int r) { return g[j][r]; });
      a_bw += tp_chan_sum<TPW>(Xs, wave, lane, tid, [&](int j, int r) { return g[j][r] * uh[j][r]; });
    }
  }
  if (tid < C) {
    float* row = p.part + (long)blockIdx.x * 4 * C;
    row[tid] = a_lw; row[C + tid] = a_lb; row[2 * C + tid] = a_bb; row[3 * C + tid] = a_bw;
  }
}

// the G rows of tp_bwd1_k in row order -> d ln_w, d ln_b, d bn_b, d bn_w (the last two may be NULL)
__global__ __launch_bounds__(256) void tp_rows_k(const float* part, int G, int C, float* o0, float* o1, float* o2, float* o3) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * C) return;
  float* const o = i < C ? o0 : i < 2 * C ? o1 : i < 3 * C ? o2 : o3;
  if (!o) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[(long)g * 4 * C + i];
  o[i % C] = s;
}

// du from dr through the train-mode BatchNorm (k1 = sum dr, k2 = sum dr u^; without BatchNorm du = dr); dx = dr + A_b^T du + ds;
// du -> workspace [B][C][T][HW]
template <int TPW>
__global__ __launch_bounds__(256) void tp_bwd2_k(const TpArgs p) {
  TP_PROLOGUE;
  for (int tau = blockIdx.x; tau < p.ntiles; tau += gridDim.x) {
    int b, t, p0, nv;
    tp_tile(p, tau, b, t, p0, nv);
    __syncthreads();
    tp_load_rows(Xs, TP_P, p.x + b * p.xb + t * p.xt + p0, p.xc, C, nv, tid);
    mt_f32x16 acc[TPW];
    float drv[TPW][16];
    tp_gemm_u<TPW>(acc, p.A + (long)b * C * C, Aimg, Xs, tid);
    float* dst = p.z + b * p.zb + t * p.zt + p0;
    const int cp = pos < nv ? pos : nv - 1;
    TP_FOR(j, r) {
      const int ch = TP_CH(j, r);
      float dr = dst[ch * p.zc + cp];
      if (pos >= nv) dr = 0.f;
      drv[j][r] = dr;
      float du = dr;
      if (p.stat) {
        const float rstd = p.stat[C + ch];
        const float uhat = (acc[j][r] + p.cvec[b * C + ch] - p.stat[ch]) * rstd;
        du = pos < nv ? p.bn_w[ch] * rstd * (dr - p.k1[ch] * p.invM - uhat * p.k2[ch] * p.invM) : 0.f;
      }
      acc[j][r] = du;
    }
    __syncthreads();                                     // every wavefront is done reading x out of Xs
    float* dud = p.du + ((long)b * C * p.T + t) * p.HW + p0 + pos;
    TP_FOR(j, r) {
      const int ch = TP_CH(j, r);
      Xs[ch * TP_P + pos] = acc[j][r];
      if (pos < nv) dud[(long)ch * p.T * p.HW] = acc[j][r];
    }
    tp_gemm_t<TPW>(acc, p.A + (long)b * C * C, Aimg, Xs, tid);
    if (pos < nv) {
      TP_FOR(j, r) {
        const int ch = TP_CH(j, r);
        dst[ch * p.zc + pos] = drv[j][r] + acc[j][r] + (p.ds ? p.ds[((long)b * p.T + t) * C + ch] : 0.f);
      }
    }
  }
}

static size_t tp_wgrad_lds(int C) { return (size_t)(C + 64) * TP_WPITCH; }
__host__ __device__ inline long tp_wrow(int C) { return (long)C * C + C; }

// dA_b[:, j0 : j0 + 64] and (j0 = 0) dc_b over the tiles g, g + G, ... of clip b; grid (G, C / 64, B); row (b, g) of part: dA [C][C] | dc [C]
template <int TPW>
__global__ __launch_bounds__(256) void tp_wgrad_k(const TpArgs p) {
  constexpr int C = 64 * TPW, PF = TP_WPITCH / 4;
  extern __shared__ float4 tp_smem4[];
  float* Ds = reinterpret_cast<float*>(tp_smem4);        // [C][64] du, k-major
  float* Xs = Ds + C * PF;                               // [64][64] x rows j0 .., k-major
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, mt0 = wave >> 1;
  const int g = blockIdx.x, G = gridDim.x, j0 = blockIdx.y * 64, b = blockIdx.z;
  mt_f32x16 acc[TPW];
  TP_FOR(j, r) acc[j][r] = 0.f;
  float adc = 0.f;
  for (int q = g; q < p.T * p.ntp; q += G) {
    const int t = q / p.ntp, p0 = (q - t * p.ntp) * TP_P, nv = imin_d(TP_P, p.HW - p0);
    __syncthreads();
    tp_load_rows(Ds, PF, p.du + ((long)b * C * p.T + t) * p.HW + p0, (long)p.T * p.HW, C, nv, tid);
    tp_load_rows(Xs, PF, p.x + b * p.xb + j0 * p.xc + t * p.xt + p0, p.xc, 64, nv, tid);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      mma_tile<DT_F32, true, true>(acc[j], reinterpret_cast<const char*>(Ds), TP_WPITCH, 32 * (mt0 + 2 * j), reinterpret_cast<const char*>(Xs),
                                   TP_WPITCH, 32 * (wave & 1), TP_P, lane);
    if (blockIdx.y == 0 && tid < C)
      for (int k = 0; k < TP_P; ++k) adc += Ds[tid * PF + ((k + tid) & (TP_P - 1))];
  }
  float* row = p.part + ((long)b * G + g) * tp_wrow(C);
  TP_FOR(j, r) row[(long)TP_CH(j, r) * C + j0 + 32 * (wave & 1) + (lane & 31)] = acc[j][r];
  if (blockIdx.y == 0 && tid < C) row[(long)C * C + tid] = adc;
}

// the G rows of every clip in row order -> dA [B][C][C], dc [B][C]
__global__ __launch_bounds__(256) void tp_wsum_k(const float* part, int B, int G, int C, float* dA, float* dc) {
  const long R = tp_wrow(C), i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * R) return;
  const int b = (int)(i / R);
  const long e = i - b * R;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[((long)b * G + g) * R + e];
  if (e < (long)C * C) dA[(long)b * C * C + e] = s;
  else dc[(long)b * C + (e - (long)C * C)] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static bool tp_ok(const char* who, int B, int C, int T, int H, int W) {
  if (B < 1 || C < TP_MIN_C || C > TP_MAX_C || C % 64 || T < 1 || T > TP_MAX_T || H < 1 || W < 1) {
    set_error("%s: need B >= 1, C a multiple of 64 with %d <= C <= %d, 1 <= T <= %d, H, W >= 1 (got B=%d, C=%d, T=%d, H=%d, W=%d)", who,
              TP_MIN_C, TP_MAX_C, TP_MAX_T, B, C, T, H, W);
    return false;
  }
  const int64_t hw = (int64_t)H * W, ntp = (hw + TP_P - 1) / TP_P;
  if (hw > 0x3fffffffLL || (int64_t)B * T * ntp > 0x7fffffffLL || (int64_t)B * C * T * hw > (1LL << 40)) {
    set_error("%s: tensor too large", who);
    return false;
  }
  return true;
}
static void tp_dims(TpArgs& p, int B, int C, int T, int H, int W) {
  p.B = B; p.C = C; p.T = T; p.HW = H * W;
  p.ntp = (p.HW + TP_P - 1) / TP_P;
  p.ntiles = B * T * p.ntp;
}
static int tp_wgs(const TpArgs& p) { return p.ntiles < TP_MAX_WGS ? p.ntiles : TP_MAX_WGS; }
static int tp_split(const TpArgs& p) { const int n = p.T * p.ntp; return n < TP_MAX_SPLIT ? n : TP_MAX_SPLIT; }
static inline bool tp_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// workspace of the backward (the forward's fits inside): rows of tp_bwd1_k | du [B][C][T][HW] | rows of tp_wgrad_k
static long tp_ws_rows(int C) { return (long)TP_MAX_WGS * 4 * C; }
static long tp_ws_floats(const TpArgs& p) {
  return tp_ws_rows(p.C) + (long)p.B * p.C * p.T * p.HW + (long)p.B * tp_split(p) * tp_wrow(p.C);
}

template <typename Kern>
static bool tp_launch(const char* who, Kern kern, dim3 grid, size_t shmem, hipStream_t s, const TpArgs& p) {
  if (shmem > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: the device refuses %zu bytes of dynamic LDS per workgroup", who, shmem);
    return false;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), shmem, s, p);
  return true;
}
#define TP_DISPATCH(KERN, grid, shmem)                                                     \
  (p.C == 64    ? tp_launch(who, KERN<1>, grid, shmem, s, p)                               \
   : p.C == 128 ? tp_launch(who, KERN<2>, grid, shmem, s, p)                               \
   : p.C == 192 ? tp_launch(who, KERN<3>, grid, shmem, s, p)                               \
                : tp_launch(who, KERN<4>, grid, shmem, s, p))

}  // namespace dgsct

using namespace dgsct;

extern "C" {

int64_t dgsct_tpavi_ws_bytes(int B, int C, int T, int H, int W) {
  clear_error();
  if (!tp_ok("dgsct_tpavi_ws_bytes", B, C, T, H, W)) return -1;
  TpArgs p{};
  tp_dims(p, B, C, T, H, W);
  return (int64_t)tp_ws_floats(p) * (int64_t)sizeof(float);
}

int dgsct_tpavi_frame_sum(int B, int C, int T, int H, int W, const float* x, int64_t xb, int64_t xc, int64_t xt, float* s, void* stream) {
  clear_error();
  const char* who = "dgsct_tpavi_frame_sum";
  if (!tp_ok(who, B, C, T, H, W)) return 2;
  if (!x || !s) { set_error("%s: NULL argument", who); return 2; }
  TpArgs p{};
  tp_dims(p, B, C, T, H, W);
  p.x = x; p.xb = xb; p.xc = xc; p.xt = xt;
  const long planes = (long)B * T * C;
  clear_async();
  hipLaunchKernelGGL(tp_frame_sum_k, dim3((unsigned)((planes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, s);
  check_async(who);
  return has_error() ? 1 : 0;
}

int dgsct_tpavi_forward(int B, int C, int T, int H, int W, const float* x, int64_t xb, int64_t xc, int64_t xt, const float* A, const float* c,
                        const float* mu0, const float* bn_w, const float* bn_b, float* run_mean, float* run_var, float momentum, float bn_eps,
                        const float* ln_w, const float* ln_b, float ln_eps, float* z, int64_t zb, int64_t zc, int64_t zt, float* stat, void* ws,
                        void* stream) {
  clear_error();
  const char* who = "dgsct_tpavi_forward";
  if (!tp_ok(who, B, C, T, H, W)) return 2;
  if (!x || !A || !c || !ln_w || !ln_b || !z) { set_error("%s: NULL argument", who); return 2; }
  if (mu0 && (!bn_w || !bn_b || !stat || !ws)) { set_error("%s: batch statistics (mu0) need bn_w, bn_b, stat and the workspace", who); return 2; }
  if (!tp_al16(A)) { set_error("%s: A must be 16-byte aligned", who); return 2; }
  TpArgs p{};
  tp_dims(p, B, C, T, H, W);
  p.x = x; p.xb = xb; p.xc = xc; p.xt = xt; p.z = z; p.zb = zb; p.zc = zc; p.zt = zt;
  p.A = A; p.cvec = c; p.mu0 = mu0; p.bn_w = bn_w; p.bn_b = bn_b; p.ln_w = ln_w; p.ln_b = ln_b; p.ln_eps = ln_eps;
  p.part = static_cast<float*>(ws);
  hipStream_t s = (hipStream_t)stream;
  const int G = tp_wgs(p);
  const size_t shmem = tp_lds(C);
  clear_async();
  if (mu0) {
    if (!TP_DISPATCH(tp_stats_k, dim3((unsigned)G), shmem)) return 1;
    hipLaunchKernelGGL(tp_bn_fin_k, dim3(1), dim3(256), 0, s, static_cast<const float*>(ws), G, C, (double)B * T * H * W, mu0, stat, run_mean,
                       run_var, momentum, bn_eps);
    p.stat = stat;
  }
  if (!TP_DISPATCH(tp_apply_k, dim3((unsigned)G), shmem)) return 1;
  check_async(who);
  return has_error() ? 1 : 0;
}

int dgsct_tpavi_backward(int B, int C, int T, int H, int W, const float* x, int64_t xb, int64_t xc, int64_t xt, const float* A, const float* c,
                         const float* stat, const float* bn_w, const float* bn_b, const float* ln_w, float ln_eps, const float* dz, int64_t gb,
                         int64_t gc, int64_t gt, const float* ds, float* dx, int64_t db, int64_t dcs, int64_t dt, float* dA, float* dc,
                         float* dbn_w, float* dbn_b, float* dln_w, float* dln_b, void* ws, void* stream) {
  clear_error();
  const char* who = "dgsct_tpavi_backward";
  if (!tp_ok(who, B, C, T, H, W)) return 2;
  if (!x || !A || !c || !ln_w || !dz || !dx || !dA || !dc || !dln_w || !dln_b || !ws) { set_error("%s: NULL argument", who); return 2; }
  if (stat && (!bn_w || !bn_b || !dbn_w || !dbn_b)) { set_error("%s: the BatchNorm backward (stat) needs bn_w, bn_b, dbn_w and dbn_b", who); return 2; }
  if (!tp_al16(A)) { set_error("%s: A must be 16-byte aligned", who); return 2; }
  TpArgs p{};
  tp_dims(p, B, C, T, H, W);
  p.x = x; p.xb = xb; p.xc = xc; p.xt = xt; p.z = dx; p.zb = db; p.zc = dcs; p.zt = dt; p.dz = dz; p.gb = gb; p.gc = gc; p.gt = gt;
  p.A = A; p.cvec = c; p.stat = stat; p.bn_w = bn_w; p.bn_b = bn_b; p.ln_w = ln_w; p.ln_eps = ln_eps; p.ds = ds;
  p.k1 = dbn_b; p.k2 = dbn_w; p.invM = (float)(1.0 / ((double)B * T * H * W));
  float* rows = static_cast<float*>(ws);
  p.part = rows;
  p.du = rows + tp_ws_rows(C);
  hipStream_t s = (hipStream_t)stream;
  const int G = tp_wgs(p), S = tp_split(p);
  const size_t shmem = tp_lds(C);
  clear_async();
  if (!TP_DISPATCH(tp_bwd1_k, dim3((unsigned)G), shmem)) return 1;
  hipLaunchKernelGGL(tp_rows_k, dim3((unsigned)((4 * C + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(rows), G, C, dln_w, dln_b,
                     stat ? dbn_b : nullptr, stat ? dbn_w : nullptr);
  if (!TP_DISPATCH(tp_bwd2_k, dim3((unsigned)G), shmem)) return 1;
  p.part = p.du + (long)B * C * T * H * W;
  if (!TP_DISPATCH(tp_wgrad_k, dim3((unsigned)S, (unsigned)(C / 64), (unsigned)B), tp_wgrad_lds(C))) return 1;
  const long tot = (long)B * tp_wrow(C);
  hipLaunchKernelGGL(tp_wsum_k, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(p.part), B, S, C, dA, dc);
  check_async(who);
  return has_error() ? 1 : 0;
}

}  // extern "C"
