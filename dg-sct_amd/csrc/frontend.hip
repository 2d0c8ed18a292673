// Audio and image front ends (the part in front of the first block): what turns a waveform / an image into the
// patch tokens the backbone blocks consume.  Both inputs are data: no kernel here returns an input gradient.  The sub-modules are frozen
// in every AVE / AVVP configuration; AVS-S4 trains `bn0` and `patch_embed`, and patch_embed_bwd_k returns their gradients.
//
//   logmel_k       waveform [B][L] -> log-mel [B][T][64], T = L / 320 + 1.  Replaces `spectrogram_extractor` + `logmel_extractor`
//                  (DG-SCT/AVE/nets/net_trans.py:857-858; htsat.py:443-449): reflect padding, periodic Hann window, 1024-point DFT,
//                  power, mel matrix, 10 log10(max(., 1e-10)).  One workgroup of 256 threads transforms TWO frames of one clip at a
//                  time as the real and imaginary part of one complex 1024-point FFT (radix 4, five passes, in place in LDS, fp32,
//                  twiddles from sincospif), separates the two spectra by their symmetry, and contracts the 513 powers with melW
//                  over the non-zero row range of each mel column.  The power spectrogram never leaves LDS.  Optionally each
//                  thread that writes log-mel values leaves their count, mean and sum of squared deviations (shifted sums;
//                  logmel_stats_k combines them into mean and biased variance for `bn0` in batch-statistics mode).
//   patch_embed_k  4 x 4 / stride 4 patch convolution + bias + LayerNorm over the embedding (layers.py:56-86).  Image mode reads
//                  [B][in_chans][H][W]; audio mode reads the log-mel and folds `bn0` (one scale / shift per mel bin) and
//                  `reshape_wav2img` (htsat.py:719-734: bicubic T -> 1024 along time, align_corners, A = -0.75, then the fold
//                  image[q*64 + f][t'] = logmel[q*256 + t'][f]) into the address arithmetic of its loads.  One wavefront computes four
//                  tokens at a time: its 64 lanes fetch the 4 x 16 pixels of the four patches (per channel), every lane owns the
//                  embedding channels lane, lane + 64, lane + 128, pixels reach all lanes through v_readlane, the [K][C] weights sit
//                  in LDS (read conflict-free: consecutive lanes, consecutive channels).
//   patch_embed_bwd_k      gradients of proj.weight / proj.bias / norm.weight / norm.bias and, in audio mode, the two sums per mel bin that
//                  give d bn0.weight / d bn0.bias, from dOut (fp32 | bf16), all in fp32.  The forward's ownership and address arithmetic;
//                  the convolution and the LayerNorm statistics are recomputed from x (the forward stores nothing for it), the sums stay in
//                  registers across the grid-stride loop, the four waves meet in LDS, each workgroup stores one partial row and
//                  patch_embed_bwd_sum_k adds the rows in a fixed order: no atomics, bit-identical from call to call.
//   AUG = true     (audio mode) the train-time augmentation of htsat.py:451 / nets/utils.py:143-153 between `bn0` and the stretch, inside
//                  the same loads: `spec_augmenter` (two time and two mel stripes per sample set to 0) is a zero at a tap, `do_mixup`
//                  (lam[b] x[b] + (1 - lam[b]) x[B-1-b]) a second tap from the mirrored sample.  fe_pixels then returns the pair (R, K)
//                  with pixel = scale R + shift K; without augmentation K is 1.  Ownership, grid, workspace and summation order are
//                  those of the plain kernels, which the AUG = false instantiations remain.
//
// The extern "C" entry points live here (not in capi.cpp): the host emulation of the CPU tests links capi.cpp against host
// primitives and has no front end.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dgsct.h"
#include "prims.h"
#include "device_util.h"
#include "err.h"

namespace dgsct {

constexpr int FE_NFFT = 1024, FE_HOP = 320, FE_NMEL = 64, FE_NBIN = FE_NFFT / 2 + 1;
constexpr int FE_MAX_T = 1024;            // reshape_wav2img takes at most spec_size * freq_ratio = 1024 frames
constexpr int FE_LOGMEL_MAX_WG = 2048;    // 8 workgroups (19 744 B of LDS each) per CU

// LDS index of FFT element i: one pad word per 32 keeps the stride-4 / stride-16 passes off a single bank
__device__ __forceinline__ int fe_pad(int i) { return i + (i >> 5); }
// position of X[k] after five in-place radix-4 DIF passes: the base-4 digits of k reversed
__device__ __forceinline__ int fe_rev4(int k) {
  const unsigned r = __brev((unsigned)k) >> 22;                 // 10 bits reversed
  return (int)(((r & 0x155u) << 1) | ((r >> 1) & 0x155u));      // ... and the two bits of every digit swapped back
}
__device__ __forceinline__ int fe_reflect(int s, int L) { return s < 0 ? -s : (s >= L ? 2 * (L - 1) - s : s); }

// b_m = W^(m j) * sum_p a_p (-i)^(p m): one radix-4 decimation-in-frequency butterfly; tw[n] = exp(-2 pi i n / 1024), tj = j * 1024 / span
__device__ __forceinline__ void fe_bfly(float (&r)[4], float (&i)[4], int tj, const float2* tw) {
  const float t0r = r[0] + r[2], t0i = i[0] + i[2], t1r = r[0] - r[2], t1i = i[0] - i[2];
  const float t2r = r[1] + r[3], t2i = i[1] + i[3], t3r = r[1] - r[3], t3i = i[1] - i[3];
  r[0] = t0r + t2r; i[0] = t0i + t2i;
  const float b1r = t1r + t3i, b1i = t1i - t3r, b2r = t0r - t2r, b2i = t0i - t2i, b3r = t1r - t3i, b3i = t1i + t3r;
  const float2 w1 = tw[tj], w2 = tw[2 * tj], w3 = tw[3 * tj];
  r[1] = b1r * w1.x - b1i * w1.y; i[1] = b1r * w1.y + b1i * w1.x;
  r[2] = b2r * w2.x - b2i * w2.y; i[2] = b2r * w2.y + b2i * w2.x;
  r[3] = b3r * w3.x - b3i * w3.y; i[3] = b3r * w3.y + b3i * w3.x;
}

// part: [gridDim.x][3][128] per thread f * 64 + m (frame parity f, mel bin m): count, mean and sum of squared deviations from that mean
// of the values it wrote (NULL: not wanted).  Accumulated as sums of v - pivot, pivot = the thread's first value: a mel bin that holds a
// steady tone has a variance of ~0.05 dB^2 around a mean of ~20 dB, and fp32 sums of v^2 would lose it to cancellation.
__global__ __launch_bounds__(256) void logmel_k(const float* __restrict__ wave, const float* __restrict__ melW, const int* __restrict__ ranges,
                                                float* __restrict__ out, float* __restrict__ part, int L, int T, int npc, int npairs) {
  __shared__ float sre[FE_NFFT + FE_NFFT / 32], sim[FE_NFFT + FE_NFFT / 32];
  __shared__ float2 tw[768];                       // the largest twiddle index is 3 * 255
  __shared__ float P[2][FE_NBIN + 3];
  __shared__ float pm[2][2][FE_NMEL];
  const int tid = threadIdx.x;
  for (int n = tid; n < 768; n += 256) {
    float s, c;
    sincospif((float)n * (1.f / 512.f), &s, &c);
    tw[n] = make_float2(c, -s);
  }
  float win[4];                                    // periodic Hann at this thread's four samples n = tid + 256 r
#pragma unroll
  for (int r = 0; r < 4; ++r) win[r] = 0.5f - 0.5f * cospif((float)(tid + 256 * r) * (1.f / 512.f));
  // role in the mel product: frame mf, half mh of the rows, mel bin mm
  const int mf = tid >> 7, mh = (tid >> 6) & 1, mm = tid & 63;
  int lo = ranges ? ranges[2 * mm] : 0, hi = ranges ? ranges[2 * mm + 1] : FE_NBIN;
  lo = lo < 0 ? 0 : lo; hi = hi > FE_NBIN ? FE_NBIN : hi;        // whatever the caller's table says, stay inside P and melW
  float piv = 0.f, sd = 0.f, sd2 = 0.f;
  int cnt = 0;
  __syncthreads();
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int b = pair / npc, t0 = (pair - b * npc) * 2;
    const bool two = t0 + 1 < T;
    const float* x = wave + (long)b * L;
    float ar[4], ai[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s0 = FE_HOP * t0 - FE_NFFT / 2 + tid + 256 * r;
      ar[r] = x[fe_reflect(s0, L)] * win[r];
      ai[r] = two ? x[fe_reflect(s0 + FE_HOP, L)] * win[r] : 0.f;
    }
    fe_bfly(ar, ai, tid, tw);                      // pass 0 (span 1024) on the loaded registers
#pragma unroll
    for (int m = 0; m < 4; ++m) { sre[fe_pad(tid + 256 * m)] = ar[m]; sim[fe_pad(tid + 256 * m)] = ai[m]; }
    __syncthreads();
#pragma unroll
    for (int s = 1; s < 5; ++s) {                  // spans 256, 64, 16, 4
      const int q = 256 >> (2 * s), j = tid & (q - 1), base = (tid - j) * 4 + j;
#pragma unroll
      for (int m = 0; m < 4; ++m) { ar[m] = sre[fe_pad(base + m * q)]; ai[m] = sim[fe_pad(base + m * q)]; }
      fe_bfly(ar, ai, j << (2 * s), tw);
#pragma unroll
      for (int m = 0; m < 4; ++m) { sre[fe_pad(base + m * q)] = ar[m]; sim[fe_pad(base + m * q)] = ai[m]; }
      __syncthreads();
    }
    // Z = FFT(a + i b), a and b real: A[k] = (Z[k] + conj Z[N-k]) / 2, B[k] = (Z[k] - conj Z[N-k]) / 2i
    for (int k = tid; k < FE_NBIN; k += 256) {
      const int pk = fe_pad(fe_rev4(k)), pn = fe_pad(fe_rev4((FE_NFFT - k) & (FE_NFFT - 1)));
      const float zr = sre[pk], zi = sim[pk], nr = sre[pn], ni = sim[pn];
      const float a_r = zr + nr, a_i = zi - ni, b_r = zi + ni, b_i = zr - nr;
      P[0][k] = 0.25f * (a_r * a_r + a_i * a_i);
      P[1][k] = 0.25f * (b_r * b_r + b_i * b_i);
    }
    __syncthreads();
    float acc = 0.f;
    for (int k = lo + mh; k < hi; k += 2) acc += P[mf][k] * melW[k * FE_NMEL + mm];
    pm[mf][mh][mm] = acc;
    __syncthreads();
    if (tid < 128) {
      const int f = tid >> 6, t = t0 + f;
      if (t < T) {
        const float v = 10.f * log10f(fmaxf(pm[f][0][mm] + pm[f][1][mm], 1e-10f));
        out[((long)b * T + t) * FE_NMEL + mm] = v;
        if (cnt++ == 0) piv = v;
        const float d = v - piv;
        sd += d; sd2 += d * d;
      }
    }
  }
  if (part && tid < 128) {
    const float md = cnt ? sd / (float)cnt : 0.f;
    float* p = part + (long)blockIdx.x * 384 + tid;
    p[0] = (float)cnt; p[128] = piv + md; p[256] = fmaxf(sd2 - sd * md, 0.f);
  }
}

// stats[0][m] = mean, stats[1][m] = biased variance of mel bin m over all B T frames: the 2 nwg groups (count, mean, M2) of logmel_k
// combined in double, M2 = sum_g M2_g + n_g (mean_g - mean)^2
__global__ __launch_bounds__(1024) void logmel_stats_k(const float* __restrict__ part, int nwg, float* __restrict__ stats) {
  __shared__ double red[2][16][64];
  const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  double sn = 0.0, sm = 0.0;
  for (int g = sl; g < 2 * nwg; g += 16) {
    const float* p = part + (long)(g >> 1) * 384 + (g & 1) * 64 + c;
    const double n = (double)p[0];
    sn += n; sm += n * (double)p[128];
  }
  red[0][sl][c] = sn; red[1][sl][c] = sm;
  __syncthreads();
  sn = 0.0; sm = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) { sn += red[0][i][c]; sm += red[1][i][c]; }
  const double mean = sm / sn;                      // sn = B T >= 1
  __syncthreads();
  double m2 = 0.0;
  for (int g = sl; g < 2 * nwg; g += 16) {
    const float* p = part + (long)(g >> 1) * 384 + (g & 1) * 64 + c;
    const double d = (double)p[128] - mean;
    m2 += (double)p[256] + (double)p[0] * d * d;
  }
  red[0][sl][c] = m2;
  __syncthreads();
  if (threadIdx.x < 64) {
    m2 = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) m2 += red[0][i][c];
    stats[c] = (float)mean;
    stats[64 + c] = (float)(m2 / sn);
  }
}

// ---- patch embedding -----------------------------------------------------------------------------------------------------------------
struct PatchArgs {
  const void* x; int xdt;                  // image: [B][IC][H][W] fp32 | bf16;   audio: log-mel [B][T][64] fp32
  const float *bn_scale, *bn_shift;        // audio: [64] each
  const float *w, *bias, *ln_w, *ln_b;     // [C][IC][4][4], [C], [C], [C]
  void* out; int odt;                      // [B][Hp * Wp][C]
  int H, W, Hp, Wp, C, T;
  long tokens;                             // B * Hp * Wp
  float eps, tscale;                       // tscale = (T - 1) / 1023 (bicubic, align_corners)
  const int* stripes;                      // AUG: [B][4][2] (begin, end) half-open; rows 0, 1 over the T frames, rows 2, 3 over the mel bins (NULL: none)
  const float* lam;                        // AUG: [B], sample b becomes lam[b] x[b] + (1 - lam[b]) x[B-1-b] (NULL: no mix-up)
  int B;
};

// PyTorch's cubic convolution coefficients (A = -0.75) for the taps at -1, 0, +1, +2 around floor(src), fraction t
__device__ __forceinline__ void fe_cubic(float t, float (&c)[4]) {
  constexpr float A = -0.75f;
  const float u = 1.f - t, a = t + 1.f, d = u + 1.f;
  c[0] = ((A * a - 5.f * A) * a + 8.f * A) * a - 4.f * A;
  c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  c[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  c[3] = ((A * d - 5.f * A) * d + 8.f * A) * d - 4.f * A;
}

// One sample's stripes (AUG): whether mel bin f / frame t survives them.  The values are only ever compared with indices, so a table
// with entries outside its axis is harmless here (the callers refuse it all the same).
struct FeStripes {
  int s[8];
  __device__ __forceinline__ void load(const int* tab, long b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = tab ? tab[b * 8 + i] : 0;
  }
  __device__ __forceinline__ bool mel(int f) const { return !((f >= s[4] && f < s[5]) || (f >= s[6] && f < s[7])); }
  __device__ __forceinline__ bool frame(int t) const { return !((t >= s[0] && t < s[1]) || (t >= s[2] && t < s[3])); }
};

// The pixels (row r, column dx) of token `tok`, one per input channel, as the convolution sees them (0 past the last token).  Audio mode:
// the bicubic stretch and the fold are the address arithmetic, `bn0` the scale / shift; `raw` is the stretched log-mel before `bn0` and
// f its mel bin (what the `bn0` gradients are collected over).  AUG: with keep_b(t, f) = 0 inside a stripe of sample b, b' = B - 1 - b,
//   raw = R = sum_e cf_e (lam_b keep_b lm[b] + (1 - lam_b) keep_b' lm[b']),   kk = K = sum_e cf_e (lam_b keep_b + (1 - lam_b) keep_b')
// over the clamped taps e, and the pixel is scale R + shift K (not AUG: kk = 1 and the pixel is scale raw + shift).
template <int IC, bool AUDIO, bool AUG = false>
__device__ __forceinline__ void fe_pixels(const PatchArgs& p, long tok, int r, int dx, float (&v)[IC], float& raw, float& kk, int& f) {
  const long P = (long)p.Hp * p.Wp;
#pragma unroll
  for (int ch = 0; ch < IC; ++ch) v[ch] = 0.f;
  raw = 0.f; f = 0; kk = AUG ? 0.f : 1.f;
  if (tok < p.tokens) {
    const long b = tok / P;
    const int pi = (int)(tok - b * P), pr = pi / p.Wp, pc = pi - pr * p.Wp;
    if (AUDIO) {
      f = 4 * (pr & 15) + r;
      const int tp = (pr >> 4) * 256 + 4 * pc + dx;                              // image[q*64 + f][t'] = logmel'[q*256 + t'][f]
      const float* lm = reinterpret_cast<const float*>(p.x) + b * (long)p.T * FE_NMEL + f;
      float val;
      if (AUG) {
        const bool mix = p.lam != nullptr;
        // the four tokens of a group lie in one sample (4096 tokens each): b is wave-uniform, and saying so keeps lam and the two stripe
        // tables in scalar registers, fetched by scalar loads
        const long bu = (long)__builtin_amdgcn_readfirstlane((int)b), b2 = (long)p.B - 1 - bu;
        const float la = mix ? p.lam[bu] : 1.f, lb = 1.f - la;
        const float* lm2 = reinterpret_cast<const float*>(p.x) + b2 * (long)p.T * FE_NMEL + f;
        FeStripes sa, sb;
        sa.load(p.stripes, bu);
        sb.load(mix ? p.stripes : nullptr, b2);
        const bool ma = sa.mel(f), mb = sb.mel(f);
        float cf[4] = {1.f, 0.f, 0.f, 0.f};
        int i0 = tp + 1, ne = 1;                                                 // T == 1024: the one tap tp with weight 1
        if (p.T != FE_MAX_T) {
          const float src = p.tscale * (float)tp, fl = floorf(src);
          i0 = (int)fl; ne = 4;
          fe_cubic(src - fl, cf);
        }
        val = 0.f;
        float ks = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (e < ne) {
            int ii = i0 - 1 + e;
            ii = ii < 0 ? 0 : (ii > p.T - 1 ? p.T - 1 : ii);
            const bool ka = ma && sa.frame(ii);
            float x = la * (ka ? lm[(long)ii * FE_NMEL] : 0.f), k = ka ? la : 0.f;
            if (mix) {
              const bool kb = mb && sb.frame(ii);
              x += lb * (kb ? lm2[(long)ii * FE_NMEL] : 0.f);
              k += kb ? lb : 0.f;
            }
            val += cf[e] * x; ks += cf[e] * k;
          }
        }
        raw = val; kk = ks;
        v[0] = val * p.bn_scale[f] + ks * p.bn_shift[f];
      } else {
        if (p.T == FE_MAX_T) val = lm[(long)tp * FE_NMEL];
        else {
          const float src = p.tscale * (float)tp, fl = floorf(src);
          const int i0 = (int)fl;
          float cf[4];
          fe_cubic(src - fl, cf);
          val = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            int ii = i0 - 1 + e;
            ii = ii < 0 ? 0 : (ii > p.T - 1 ? p.T - 1 : ii);
            val += cf[e] * lm[(long)ii * FE_NMEL];
          }
        }
        raw = val;
        v[0] = val * p.bn_scale[f] + p.bn_shift[f];
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < IC; ++ch)
        v[ch] = lde_rt(p.x, p.xdt, ((b * IC + ch) * p.H + 4 * pr + r) * (long)p.W + 4 * pc + dx);
    }
  }
}

template <int IC, bool AUDIO, int NJ, bool AUG = false>
__global__ __launch_bounds__(256) void patch_embed_k(const PatchArgs p) {
  constexpr int K = IC * 16;
  __shared__ float Wt[K * NJ * 64];                // [k][c], c < C (rows packed at pitch C)
  const int C = p.C, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < K * C; i += 256) {
    const int c = i / K, k = i - c * K;
    Wt[k * C + c] = p.w[i];
  }
  float bias[NJ], lw[NJ], lb[NJ];
  int cw[NJ];                                      // this lane's channels, clamped for the reads (lanes past C compute and drop)
  bool cv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    cv[j] = c < C;
    cw[j] = cv[j] ? c : C - 1;
    bias[j] = p.bias[cw[j]]; lw[j] = p.ln_w[cw[j]]; lb[j] = p.ln_b[cw[j]];
  }
  __syncthreads();
  const int r = lane >> 4, tt = (lane >> 2) & 3, dx = lane & 3;      // this lane's pixel: row r, column dx of token tt of the group
  const long ngroups = (p.tokens + 3) >> 2;
  const float invC = 1.f / (float)C;
  for (long grp = (long)blockIdx.x * 4 + (threadIdx.x >> 6); grp < ngroups; grp += (long)gridDim.x * 4) {
    const long tok0 = grp * 4, tok = tok0 + tt;
    float v[IC], raw, kk;
    int f;
    fe_pixels<IC, AUDIO, AUG>(p, tok, r, dx, v, raw, kk, f);
    float acc[4][NJ];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[t][j] = bias[j];
#pragma unroll
    for (int ch = 0; ch < IC; ++ch)
#pragma unroll
      for (int rd = 0; rd < 16; ++rd) {            // rd = row * 4 + column inside the patch
        float w[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) w[j] = Wt[(ch * 16 + rd) * C + cw[j]];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float xv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[ch]), (rd >> 2) * 16 + t * 4 + (rd & 3)));
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[t][j] += xv * w[j];
        }
      }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (tok0 + t >= p.tokens) break;             // wave-uniform
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) s += cv[j] ? acc[t][j] : 0.f;
      const float mean = group_sum(s, 64) * invC;
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) { acc[t][j] -= mean; q += cv[j] ? acc[t][j] * acc[t][j] : 0.f; }
      const float rstd = 1.f / sqrtf(group_sum(q, 64) * invC + p.eps);
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (cv[j]) ste_rt(p.out, p.odt, (tok0 + t) * C + lane + 64 * j, acc[t][j] * rstd * lw[j] + lb[j]);
    }
  }
}

template <int IC, bool AUDIO, int NJ, bool AUG = false>
static void patch_embed_launch(const PatchArgs& a, hipStream_t s) {
  const void* fn = reinterpret_cast<const void*>(&patch_embed_k<IC, AUDIO, NJ, AUG>);
  const long want = ((a.tokens + 3) / 4 + 3) / 4;
  const long cap = wg_capacity(fn, 0);
  hipLaunchKernelGGL((patch_embed_k<IC, AUDIO, NJ, AUG>), dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, s, a);
}
template <int IC, bool AUDIO, bool AUG = false>
static void patch_embed_nj(const PatchArgs& a, hipStream_t s) {
  const int nj = (a.C + 63) / 64;
  if (nj == 1) patch_embed_launch<IC, AUDIO, 1, AUG>(a, s);
  else if (nj == 2) patch_embed_launch<IC, AUDIO, 2, AUG>(a, s);
  else patch_embed_launch<IC, AUDIO, 3, AUG>(a, s);
}

// ---- patch embedding: parameter gradients ------------------------------------------------------------------------------------------
constexpr int PE_BWD_MAX_WG = 1024;       // rows of the workspace: one partial row per workgroup, summed by patch_embed_bwd_sum_k

struct PatchBwdArgs {
  PatchArgs f;                             // the forward's operands (out / odt / ln_b unused)
  const void* dout; int ddt;               // [B][Hp * Wp][C] fp32 | bf16
  const float* pivot;                      // audio: [64], what the `bn0` sums are centred on (the mean `bn0` used)
  float* ws; int rs;                       // [gridDim.x][rs], rs = (K + 3) C (+ 128 in audio mode)
};

// Gradients of proj.weight / proj.bias / norm.weight / norm.bias (and the two `bn0` sums in audio mode) from dOut, with the forward's
// ownership: one wavefront per four tokens, a lane owns the channels lane, lane + 64, lane + 128 and fetches one pixel of the group.  Per
// group: the convolution and the LayerNorm statistics are recomputed from x (nothing token-sized is read but x and dOut), then per token
//   yh = (conv - mean) rstd,  d norm.weight += dOut yh,  d norm.bias += dOut,  dy = dOut norm.weight,
//   dconv = rstd (dy - mean_c(dy) - yh mean_c(dy yh)),   d proj.bias += dconv,   d proj.weight[c][k] += dconv[c] pix[k].
// Audio mode: with dpix = W^T dconv, g1[f] = sum dpix (S(lm) - pivot[f]) and g0[f] = sum dpix per mel bin f.  The four tokens of a group
// share their patch row, so f = 4 (pr & 15) + r depends on the pixel row r alone: a lane forms, per row and over its own channels,
// sum_c dconv[c] sum_dx W[4r + dx][c] s[r][dx] and sum_c dconv[c] sum_dx W[4r + dx][c], the wave sums those eight numbers once per group and
// adds them to its 2 x 64 bins in LDS.  Everything else stays in registers across the grid-stride loop; at the end the four waves add
// their registers into one [K + 3][C] LDS buffer one after the other (a fixed order) and the workgroup stores ONE row of the workspace.
// No atomics: the result depends on the grid alone.
// AUG: the pixel is scale R + shift K, so g1 is collected over R - pivot K and g0 over K; the per-row shortcut of g0 above (sum_dx W, K = 1)
// becomes the sum weighted by K[r][dx], formed like g1's.  The recomputed convolution sees the augmented pixels.
template <int IC, bool AUDIO, int NJ, bool AUG = false>
__global__ __launch_bounds__(256) void patch_embed_bwd_k(const PatchBwdArgs a) {
  constexpr int K = IC * 16, KR = K + 3;
  __shared__ float sm[KR * NJ * 64];               // the weights [k][c] at pitch C during the loop, the combined sums [K + 3][C] after it
  __shared__ float bins[AUDIO ? 4 * 128 : 1];      // [wave][g1 | g0][mel bin]
  const PatchArgs& p = a.f;
  const int C = p.C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < K * C; i += 256) {
    const int c = i / K, k = i - c * K;
    sm[k * C + c] = p.w[i];
  }
  if (AUDIO)
    for (int i = threadIdx.x; i < 4 * 128; i += 256) bins[i] = 0.f;
  float bias[NJ], lw[NJ];
  int cw[NJ];                                      // this lane's channels, clamped for the reads (lanes past C carry zeros)
  bool cv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    cv[j] = c < C;
    cw[j] = cv[j] ? c : C - 1;
    bias[j] = p.bias[cw[j]]; lw[j] = p.ln_w[cw[j]];
  }
  __syncthreads();
  float wrow[4][NJ];                               // audio: sum_dx W[4r + dx][c]
  if (AUDIO && !AUG) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        wrow[rr][j] = (sm[(4 * rr) * C + cw[j]] + sm[(4 * rr + 1) * C + cw[j]]) + (sm[(4 * rr + 2) * C + cw[j]] + sm[(4 * rr + 3) * C + cw[j]]);
  }
  float dW[K][NJ], db[NJ], dlw[NJ], dlb[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    db[j] = 0.f; dlw[j] = 0.f; dlb[j] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) dW[k][j] = 0.f;
  }
  const int r = lane >> 4, tt = (lane >> 2) & 3, dx = lane & 3;      // this lane's pixel: row r, column dx of token tt of the group
  const long ngroups = (p.tokens + 3) >> 2;
  const float invC = 1.f / (float)C;
  for (long grp = (long)blockIdx.x * 4 + wave; grp < ngroups; grp += (long)gridDim.x * 4) {
    const long tok0 = grp * 4;
    float v[IC], raw, kk;
    int f;
    fe_pixels<IC, AUDIO, AUG>(p, tok0 + tt, r, dx, v, raw, kk, f);
    const float sv = AUDIO ? (AUG ? raw - a.pivot[f] * kk : raw - a.pivot[f]) : 0.f;
    float g[4][NJ];                                // dOut of the four tokens, in flight while the convolution is recomputed
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        g[t][j] = (cv[j] && tok0 + t < p.tokens) ? lde_rt(a.dout, a.ddt, (tok0 + t) * C + lane + 64 * j) : 0.f;
    float acc[4][NJ];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[t][j] = bias[j];
#pragma unroll
    for (int ch = 0; ch < IC; ++ch)
#pragma unroll
      for (int rd = 0; rd < 16; ++rd) {            // rd = row * 4 + column inside the patch
        float w[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) w[j] = sm[(ch * 16 + rd) * C + cw[j]];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float xv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[ch]), (rd >> 2) * 16 + t * 4 + (rd & 3)));
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[t][j] += xv * w[j];
        }
      }
    // LayerNorm backward per token: acc becomes dconv (0 in the lanes past C and for the tokens past the last one)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (tok0 + t < p.tokens) {                   // wave-uniform
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) s += cv[j] ? acc[t][j] : 0.f;
        const float mean = group_sum(s, 64) * invC;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) { acc[t][j] -= mean; q += cv[j] ? acc[t][j] * acc[t][j] : 0.f; }
        const float rstd = 1.f / sqrtf(group_sum(q, 64) * invC + p.eps);
        float dy[NJ], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          acc[t][j] *= rstd;                       // yh
          dlw[j] += g[t][j] * acc[t][j]; dlb[j] += g[t][j];
          dy[j] = g[t][j] * lw[j];                 // (g is 0 in the lanes past C)
          s1 += dy[j]; s2 += dy[j] * acc[t][j];
        }
        group_sum2(s1, s2, 64);
        const float m1 = s1 * invC, m2 = s2 * invC;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          acc[t][j] = cv[j] ? rstd * (dy[j] - m1 - acc[t][j] * m2) : 0.f;
          db[j] += acc[t][j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[t][j] = 0.f;
      }
    }
    float p1[4] = {0.f, 0.f, 0.f, 0.f}, p0[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < IC; ++ch)
#pragma unroll
      for (int rd = 0; rd < 16; ++rd) {
        const int k = ch * 16 + rd;
        float u[NJ], uk[NJ];                       // audio: sum_t dconv[t][c] s[t][rd]  (AUG: and sum_t dconv[t][c] K[t][rd])
#pragma unroll
        for (int j = 0; j < NJ; ++j) { u[j] = 0.f; uk[j] = 0.f; }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int src = (rd >> 2) * 16 + t * 4 + (rd & 3);
          const float xv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[ch]), src));
#pragma unroll
          for (int j = 0; j < NJ; ++j) dW[k][j] += xv * acc[t][j];
          if (AUDIO) {
            const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sv), src));
#pragma unroll
            for (int j = 0; j < NJ; ++j) u[j] += sx * acc[t][j];
            if (AUG) {
              const float kx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, kk), src));
#pragma unroll
              for (int j = 0; j < NJ; ++j) uk[j] += kx * acc[t][j];
            }
          }
        }
        if (AUDIO) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) p1[rd >> 2] += u[j] * sm[k * C + cw[j]];
          if (AUG) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) p0[rd >> 2] += uk[j] * sm[k * C + cw[j]];
          }
        }
      }
    if (AUDIO) {
      if (!AUG) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const float ds = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) p0[rr] += ds * wrow[rr][j];
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) group_sum2(p1[rr], p0[rr], 64);
      if (lane < 8) {                              // lane = which * 4 + row: one bin each
        const int rr = lane & 3;
        const float a1 = rr == 0 ? p1[0] : rr == 1 ? p1[1] : rr == 2 ? p1[2] : p1[3];
        const float a0 = rr == 0 ? p0[0] : rr == 1 ? p0[1] : rr == 2 ? p0[2] : p0[3];
        const int pr = (int)(tok0 % ((long)p.Hp * p.Wp)) / p.Wp;     // the group's patch row (Wp = 64: four tokens never straddle two)
        bins[wave * 128 + (lane >> 2) * 64 + 4 * (pr & 15) + rr] += lane < 4 ? a1 : a0;
      }
    }
  }
  // the four waves' registers into sm, one wave after the other
  __syncthreads();                                 // every wave is done with the weights
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (cv[j]) {
          const int c = lane + 64 * j;
#pragma unroll
          for (int k = 0; k < K; ++k) sm[k * C + c] = (w ? sm[k * C + c] : 0.f) + dW[k][j];
          sm[K * C + c] = (w ? sm[K * C + c] : 0.f) + db[j];
          sm[(K + 1) * C + c] = (w ? sm[(K + 1) * C + c] : 0.f) + dlw[j];
          sm[(K + 2) * C + c] = (w ? sm[(K + 2) * C + c] : 0.f) + dlb[j];
        }
    }
    __syncthreads();
  }
  float* row = a.ws + (long)blockIdx.x * a.rs;
  for (int i = threadIdx.x; i < KR * C; i += 256) row[i] = sm[i];
  if (AUDIO && threadIdx.x < 128)
    row[KR * C + threadIdx.x] = (bins[threadIdx.x] + bins[128 + threadIdx.x]) + (bins[256 + threadIdx.x] + bins[384 + threadIdx.x]);
}

// column sums of the workspace in a fixed order: 16 columns x 16 row slices per workgroup, every slice summed in row order, the slices
// in slice order.  Column k C + c goes to dweight[c][k] (the [C][IC][4][4] layout), the rest to dbias / dln_weight / dln_bias / dbn.
__global__ __launch_bounds__(256) void patch_embed_bwd_sum_k(const float* __restrict__ ws, int rows, int rs, int K, int C, float* __restrict__ dw,
                                                             float* __restrict__ db, float* __restrict__ dlw, float* __restrict__ dlb,
                                                             float* __restrict__ dbn) {
  __shared__ float red[16][17];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4, col = blockIdx.x * 16 + cl;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < rs) {
    const float* q = ws + col;
    int i = sl;
    for (; i + 48 < rows; i += 64) {
      const float v0 = q[(long)i * rs], v1 = q[(long)(i + 16) * rs], v2 = q[(long)(i + 32) * rs], v3 = q[(long)(i + 48) * rs];
      s0 += v0; s1 += v1; s2 += v2; s3 += v3;
    }
    for (; i < rows; i += 16) s0 += q[(long)i * rs];
  }
  red[sl][cl] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (threadIdx.x < 16 && col < rs) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += red[i][cl];
    const int KC = K * C;
    if (col < KC) { const int k = col / C, c = col - k * C; dw[c * K + k] = s; }
    else if (col < KC + C) db[col - KC] = s;
    else if (col < KC + 2 * C) dlw[col - KC - C] = s;
    else if (col < KC + 3 * C) dlb[col - KC - 2 * C] = s;
    else dbn[col - KC - 3 * C] = s;
  }
}

static long pe_bwd_rows(long tokens) {
  const long want = ((tokens + 3) / 4 + 3) / 4;
  return want < PE_BWD_MAX_WG ? want : PE_BWD_MAX_WG;
}
template <int IC, bool AUDIO, int NJ, bool AUG = false>
static void patch_embed_bwd_launch(PatchBwdArgs& a, float* dw, float* db, float* dlw, float* dlb, float* dbn, hipStream_t s) {
  const void* fn = reinterpret_cast<const void*>(&patch_embed_bwd_k<IC, AUDIO, NJ, AUG>);
  const long rows = pe_bwd_rows(a.f.tokens), cap = wg_capacity(fn, 0);
  const int grid = (int)(rows < cap ? rows : cap);                   // <= the rows the workspace holds
  hipLaunchKernelGGL((patch_embed_bwd_k<IC, AUDIO, NJ, AUG>), dim3(grid), dim3(256), 0, s, a);
  hipLaunchKernelGGL(patch_embed_bwd_sum_k, dim3((a.rs + 15) / 16), dim3(256), 0, s, (const float*)a.ws, grid, a.rs, IC * 16, a.f.C, dw, db, dlw, dlb, dbn);
}
template <int IC, bool AUDIO, bool AUG = false>
static void patch_embed_bwd_nj(PatchBwdArgs& a, float* dw, float* db, float* dlw, float* dlb, float* dbn, hipStream_t s) {
  const int nj = (a.f.C + 63) / 64;
  if (nj == 1) patch_embed_bwd_launch<IC, AUDIO, 1, AUG>(a, dw, db, dlw, dlb, dbn, s);
  else if (nj == 2) patch_embed_bwd_launch<IC, AUDIO, 2, AUG>(a, dw, db, dlw, dlb, dbn, s);
  else patch_embed_bwd_launch<IC, AUDIO, 3, AUG>(a, dw, db, dlw, dlb, dbn, s);
}

static int fe_logmel_wgs(int B, int64_t L) {
  const int64_t T = L / FE_HOP + 1, npairs = (int64_t)B * ((T + 1) / 2);
  return (int)(npairs < FE_LOGMEL_MAX_WG ? npairs : FE_LOGMEL_MAX_WG);
}
static bool fe_logmel_check(const char* who, int B, int64_t L, int n_fft, int hop, int n_mels) {
  if (n_fft != FE_NFFT || hop != FE_HOP || n_mels != FE_NMEL) {
    set_error("%s: only n_fft = 1024, hop = 320, n_mels = 64 are built (got %d, %d, %d)", who, n_fft, hop, n_mels);
    return false;
  }
  if (B < 1 || L <= FE_NFFT / 2 || L / FE_HOP + 1 > FE_MAX_T || (int64_t)B * (L / FE_HOP + 1) > 0x7fffffffLL / FE_NMEL) {
    set_error("%s: need B >= 1 and %d < L with at most %d frames (got B = %d, L = %lld)", who, FE_NFFT / 2, FE_MAX_T, B, (long long)L);
    return false;
  }
  return true;
}

// mode / shape limits shared by the forward, the parameter-gradient backward and its workspace size
static bool fe_patch_geometry(const char* who, int mode, int B, int in_chans, int H, int W, int T, int C) {
  if (B < 1 || C < 32 || C > 192 || C % 32) { set_error("%s: need B >= 1 and C a multiple of 32 up to 192 (got %d, %d)", who, B, C); return false; }
  if (mode == DGSCT_PATCH_AUDIO) {
    if (in_chans != 1 || H != 256 || W != 256 || T < 2 || T > FE_MAX_T) {
      set_error("%s: audio mode takes an fp32 log-mel of 2 .. %d frames, bn scale / shift, in_chans = 1 and a 256 x 256 image", who, FE_MAX_T);
      return false;
    }
  } else if (mode == DGSCT_PATCH_IMAGE) {
    if ((in_chans != 1 && in_chans != 3) || H < 4 || W < 4 || H % 4 || W % 4) {
      set_error("%s: image mode takes in_chans 1 or 3 and H, W multiples of 4 (got %d, %d x %d)", who, in_chans, H, W); return false;
    }
  } else { set_error("%s: unknown mode %d", who, mode); return false; }
  const long tokens = (long)B * (H / 4) * (W / 4);
  if (tokens * C > 0x7fffffffffLL || (long)B * in_chans * H * W > 0x7fffffffffLL) { set_error("%s: tensor too large", who); return false; }
  return true;
}
// ... and the operands: fills `a` (everything but out / odt); tok_dtype = the dtype of the tokens (out) or of their gradient (dout)
static bool fe_patch_check(const char* who, int mode, int in_dtype, int tok_dtype, int B, int in_chans, int H, int W, int T, int C, const void* x,
                           const float* bn_scale, const float* bn_shift, const float* weight, const float* bias, const float* ln_weight,
                           const float* ln_bias, float eps, PatchArgs& a) {
  if (!x || !weight || !bias || !ln_weight || !ln_bias) { set_error("%s: NULL argument", who); return false; }
  if ((tok_dtype != DGSCT_F32 && tok_dtype != DGSCT_BF16) || (in_dtype != DGSCT_F32 && in_dtype != DGSCT_BF16)) {
    set_error("%s: dtypes must be DGSCT_F32 or DGSCT_BF16", who); return false;
  }
  if (mode == DGSCT_PATCH_AUDIO && (in_dtype != DGSCT_F32 || !bn_scale || !bn_shift)) {
    set_error("%s: audio mode takes an fp32 log-mel of 2 .. %d frames, bn scale / shift, in_chans = 1 and a 256 x 256 image", who, FE_MAX_T);
    return false;
  }
  if (!fe_patch_geometry(who, mode, B, in_chans, H, W, T, C)) return false;
  a.x = x; a.xdt = in_dtype; a.bn_scale = bn_scale; a.bn_shift = bn_shift; a.w = weight; a.bias = bias; a.ln_w = ln_weight; a.ln_b = ln_bias;
  a.C = C; a.eps = eps;
  if (mode == DGSCT_PATCH_AUDIO) { a.T = T; a.tscale = (float)(T - 1) / (float)(FE_MAX_T - 1); }
  a.H = H; a.W = W; a.Hp = H / 4; a.Wp = W / 4;
  a.tokens = (long)B * a.Hp * a.Wp;
  a.B = B;
  return true;
}
static long pe_bwd_row_floats(int mode, int in_chans, int C) { return (long)(in_chans * 16 + 3) * C + (mode == DGSCT_PATCH_AUDIO ? 2 * FE_NMEL : 0); }

}  // namespace dgsct

using namespace dgsct;

extern "C" {

int64_t dgsct_logmel_scratch_floats(int B, int64_t L, int n_fft, int hop, int n_mels) {
  clear_error();
  if (!fe_logmel_check("dgsct_logmel_scratch_floats", B, L, n_fft, hop, n_mels)) return -1;
  return (int64_t)fe_logmel_wgs(B, L) * 384;
}

int dgsct_logmel_forward(int B, int64_t L, int n_fft, int hop, int n_mels, const float* waveform, const float* melW, const int32_t* ranges,
                         float* out, float* stats, float* scratch, void* stream) {
  clear_error();
  if (!fe_logmel_check("dgsct_logmel_forward", B, L, n_fft, hop, n_mels)) return 2;
  if (!waveform || !melW || !out) { set_error("dgsct_logmel_forward: NULL argument"); return 2; }
  if (stats && !scratch) { set_error("dgsct_logmel_forward: statistics need `scratch` (dgsct_logmel_scratch_floats)"); return 2; }
  const int T = (int)(L / FE_HOP) + 1, npc = (T + 1) / 2, npairs = B * npc, wgs = fe_logmel_wgs(B, L);
  hipStream_t s = (hipStream_t)stream;
  clear_async();                                   // (after the argument checks: those are pure host code)
  hipLaunchKernelGGL(logmel_k, dim3(wgs), dim3(256), 0, s, waveform, melW, (const int*)ranges, out, stats ? scratch : nullptr, (int)L, T, npc, npairs);
  if (stats) hipLaunchKernelGGL(logmel_stats_k, dim3(1), dim3(1024), 0, s, (const float*)scratch, wgs, stats);
  check_async("dgsct_logmel_forward");
  return has_error() ? 1 : 0;
}

int dgsct_patch_embed_forward(int mode, int in_dtype, int out_dtype, int B, int in_chans, int H, int W, int T, int C, const void* x,
                              const float* bn_scale, const float* bn_shift, const float* weight, const float* bias, const float* ln_weight,
                              const float* ln_bias, float eps, void* out, void* stream) {
  clear_error();
  const char* who = "dgsct_patch_embed_forward";
  if (!out) { set_error("%s: NULL argument", who); return 2; }
  PatchArgs a{};
  if (!fe_patch_check(who, mode, in_dtype, out_dtype, B, in_chans, H, W, T, C, x, bn_scale, bn_shift, weight, bias, ln_weight, ln_bias, eps, a)) return 2;
  a.out = out; a.odt = out_dtype;
  hipStream_t s = (hipStream_t)stream;
  clear_async();
  if (mode == DGSCT_PATCH_AUDIO) patch_embed_nj<1, true>(a, s);
  else if (in_chans == 1) patch_embed_nj<1, false>(a, s);
  else patch_embed_nj<3, false>(a, s);
  check_async(who);
  return has_error() ? 1 : 0;
}

int dgsct_patch_embed_forward_aug(int out_dtype, int B, int T, int C, const float* logmel, const float* bn_scale, const float* bn_shift,
                                  const int32_t* stripes, const float* lam, const float* weight, const float* bias, const float* ln_weight,
                                  const float* ln_bias, float eps, void* out, void* stream) {
  clear_error();
  const char* who = "dgsct_patch_embed_forward_aug";
  if (!out) { set_error("%s: NULL argument", who); return 2; }
  PatchArgs a{};
  if (!fe_patch_check(who, DGSCT_PATCH_AUDIO, DGSCT_F32, out_dtype, B, 1, 256, 256, T, C, logmel, bn_scale, bn_shift, weight, bias, ln_weight, ln_bias,
                      eps, a)) return 2;
  a.out = out; a.odt = out_dtype; a.stripes = (const int*)stripes; a.lam = lam;
  hipStream_t s = (hipStream_t)stream;
  clear_async();
  if (stripes || lam) patch_embed_nj<1, true, true>(a, s);
  else patch_embed_nj<1, true>(a, s);
  check_async(who);
  return has_error() ? 1 : 0;
}

int64_t dgsct_patch_embed_params_ws_floats(int mode, int B, int in_chans, int H, int W, int C) {
  clear_error();
  const char* who = "dgsct_patch_embed_params_ws_floats";
  if (!fe_patch_geometry(who, mode, B, in_chans, H, W, mode == DGSCT_PATCH_AUDIO ? 2 : 0, C)) return -1;
  const long tokens = (long)B * (H / 4) * (W / 4);
  return pe_bwd_rows(tokens) * pe_bwd_row_floats(mode, in_chans, C);
}

int dgsct_patch_embed_backward_params(int mode, int in_dtype, int dout_dtype, int B, int in_chans, int H, int W, int T, int C, const void* x,
                                      const float* bn_scale, const float* bn_shift, const float* bn_pivot, const float* weight, const float* bias,
                                      const float* ln_weight, const float* ln_bias, float eps, const void* dout, float* dweight, float* dbias,
                                      float* dln_weight, float* dln_bias, float* dbn, float* ws, void* stream) {
  clear_error();
  const char* who = "dgsct_patch_embed_backward_params";
  if (!dout || !dweight || !dbias || !dln_weight || !dln_bias || !ws) { set_error("%s: NULL argument", who); return 2; }
  if (mode == DGSCT_PATCH_AUDIO && (!bn_pivot || !dbn)) { set_error("%s: audio mode needs bn_pivot and dbn", who); return 2; }
  PatchBwdArgs a{};
  if (!fe_patch_check(who, mode, in_dtype, dout_dtype, B, in_chans, H, W, T, C, x, bn_scale, bn_shift, weight, bias, ln_weight, ln_bias, eps, a.f)) return 2;
  a.dout = dout; a.ddt = dout_dtype; a.pivot = bn_pivot; a.ws = ws; a.rs = (int)pe_bwd_row_floats(mode, in_chans, C);
  hipStream_t s = (hipStream_t)stream;
  clear_async();
  if (mode == DGSCT_PATCH_AUDIO) patch_embed_bwd_nj<1, true>(a, dweight, dbias, dln_weight, dln_bias, dbn, s);
  else if (in_chans == 1) patch_embed_bwd_nj<1, false>(a, dweight, dbias, dln_weight, dln_bias, nullptr, s);
  else patch_embed_bwd_nj<3, false>(a, dweight, dbias, dln_weight, dln_bias, nullptr, s);
  check_async(who);
  return has_error() ? 1 : 0;
}

int dgsct_patch_embed_backward_params_aug(int dout_dtype, int B, int T, int C, const float* logmel, const float* bn_scale, const float* bn_shift,
                                          const float* bn_pivot, const int32_t* stripes, const float* lam, const float* weight, const float* bias,
                                          const float* ln_weight, const float* ln_bias, float eps, const void* dout, float* dweight, float* dbias,
                                          float* dln_weight, float* dln_bias, float* dbn, float* ws, void* stream) {
  clear_error();
  const char* who = "dgsct_patch_embed_backward_params_aug";
  if (!dout || !dweight || !dbias || !dln_weight || !dln_bias || !ws) { set_error("%s: NULL argument", who); return 2; }
  if (!bn_pivot || !dbn) { set_error("%s: audio mode needs bn_pivot and dbn", who); return 2; }
  PatchBwdArgs a{};
  if (!fe_patch_check(who, DGSCT_PATCH_AUDIO, DGSCT_F32, dout_dtype, B, 1, 256, 256, T, C, logmel, bn_scale, bn_shift, weight, bias, ln_weight, ln_bias,
                      eps, a.f)) return 2;
  a.f.stripes = (const int*)stripes; a.f.lam = lam;
  a.dout = dout; a.ddt = dout_dtype; a.pivot = bn_pivot; a.ws = ws; a.rs = (int)pe_bwd_row_floats(DGSCT_PATCH_AUDIO, 1, C);
  hipStream_t s = (hipStream_t)stream;
  clear_async();
  if (stripes || lam) patch_embed_bwd_nj<1, true, true>(a, dweight, dbias, dln_weight, dln_bias, dbn, s);
  else patch_embed_bwd_nj<1, true>(a, dweight, dbias, dln_weight, dln_bias, dbn, s);
  check_async(who);
  return has_error() ? 1 : 0;
}

}  // extern "C"
