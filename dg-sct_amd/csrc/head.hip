// The live part of the CMBS event head of the AVE model (reference DG-SCT/AVE/nets/net_trans.py:254-292 with the
// SupvLocalizeModule of :116-138), fp32 throughout as the reference runs it:
//   cas_m[t,b,k] = W_m[k] . x_m[t,b] + b_m[k]                     m = video (x = v) | audio (x = a)
//   s_m[b,k]     = mean of the 4 largest of cas_m[:,b,k] over t   (sort descending, [:4], mean)
//   av[b,k]      = (s_v + s_a) / 2
//   f[t,b]       = (v[t,b] + a[t,b]) / 2
//   is_event[t,b]= wc . f[t,b] + bc
//   mx[b,d]      = max_t f[t,b,d]
//   event[b,k]   = We[k] . mx[b] + be[k] + gamma * av[b,k]
// v, a are time-major [T][B][D].  About 0.3 MFLOP per clip: no MFMA (fp32 parity is the contract and the products are tiny), plain VALU
// dot products out of LDS.
//
// Forward, ONE launch: one workgroup per clip.  The clip's 2 T D inputs are staged in LDS once (20 KB at T = 10, D = 256; 128 KB at the
// limits, which needs the dynamic-LDS attribute and leaves one workgroup per CU; with only B short workgroups that is not expected to matter).
// 16-lane groups own one (modality, class) weight row in registers and walk the T staged rows: float4 LDS reads laid out to be
// conflict-free (16 lanes x 16 contiguous bytes; not profiled), a 4-step DPP sum inside the row of lanes.  Instead of the sort permutation the backward gets `topmask` (bit t: timestep t is one of the
// four selected) and `argmax` (the first t attaining mx).
//
// Backward, TWO launches: the input gradients need only the masks and the arg-max (no staging); with parameter gradients every
// workgroup owns the clips b = wg, wg + G, ... (G = min(B, 64)) and accumulates their contributions into ITS row of a workspace (the same
// thread always owns the same element: plain read-modify-write, no atomics); a second kernel sums the G rows in a fixed order, so the
// parameter gradients are bit-identical from call to call (the convention of patch_embed_bwd_k / dgsct_patch_merge_backward_params,
// not the atomics of tgate_bwd_k).
//
// The extern "C" entry points live here (as csrc/frontend.hip's and csrc/pmerge.hip's do): the host emulation of the CPU tests
// compiles capi.cpp against host loops and has no event head.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/dgsct.h"
#include "prims.h"
#include "device_util.h"
#include "err.h"

namespace dgsct {

constexpr int HEAD_TOPK = 4, HEAD_MAX_T = 32, HEAD_MAX_D = 512, HEAD_MAX_K = 32, HEAD_MAX_WGS = 64;

struct HeadArgs {
  int T, B, D, K; float gamma;
  const float *v, *a, *Wvc, *bvc, *Wac, *bac, *wc, *bc, *We, *be;
  float *is_event, *event, *av; int *topmask, *argmax;                 // forward outputs (backward: topmask / argmax are read)
  const float *d_is, *d_ev, *d_av;                                     // cotangents, each may be null (= 0)
  float *dv, *da, *part;                                               // part: [gridDim.x][head_row_floats] or null (frozen head)
};
struct HeadGrads { float *dWvc, *dbvc, *dWac, *dbac, *dwc, *dbc, *dWe, *dbe; };

// one partial row: dWvc [K D] | dWac [K D] | dWe [K D] | dwc [D] | dbvc [K] | dbac [K] | dbe [K] | dbc [1]
__host__ __device__ inline long head_row_floats(int D, int K) { return 3L * K * D + D + 3L * K + 1; }

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// the clip's rows of v and a -> sv, sa [T][D]
__device__ __forceinline__ void head_stage(const HeadArgs& p, int b, float* sv, float* sa) {
  const int D4 = p.D >> 2;
  for (int i = threadIdx.x; i < p.T * D4; i += 256) {
    const int t = i / D4, c = (i - t * D4) * 4;
    const long o = ((long)t * p.B + b) * p.D + c;
    *reinterpret_cast<float4*>(sv + t * p.D + c) = *reinterpret_cast<const float4*>(p.v + o);
    *reinterpret_cast<float4*>(sa + t * p.D + c) = *reinterpret_cast<const float4*>(p.a + o);
  }
}

static size_t head_fwd_lds(int T, int D, int K) { return ((size_t)2 * T * D + (size_t)2 * T * K + D + 2 * K) * sizeof(float); }

__global__ __launch_bounds__(256) void head_fwd_k(const HeadArgs p) {
  extern __shared__ float4 head_smem4[];
  const int T = p.T, B = p.B, D = p.D, K = p.K, b = blockIdx.x, tid = threadIdx.x;
  float* sv = reinterpret_cast<float*>(head_smem4);
  float* sa = sv + T * D;
  float* mx = sa + T * D;                // [D]       (before cas: float4 reads need the 16-byte alignment)
  float* cas = mx + D;                   // [2][T][K]
  float* ssum = cas + 2 * T * K;         // [2][K]
  head_stage(p, b, sv, sa);
  __syncthreads();

  // class activation scores: a 16-lane group keeps W_m[k] in registers (lane gl: columns gl*4 + 64 i) and walks the T rows
  const int grp = tid >> 4, gl = tid & 15;
  for (int pr = grp; pr < 2 * K; pr += 16) {
    const int m = pr >= K, k = pr - m * K;
    const float* W = (m ? p.Wac : p.Wvc) + (long)k * D + gl * 4;
    const float bias = (m ? p.bac : p.bvc)[k];
    const float* x = (m ? sa : sv) + gl * 4;
    float4 w[HEAD_MAX_D / 64];
#pragma unroll
    for (int i = 0; i < HEAD_MAX_D / 64; ++i)
      if (i * 64 < D) w[i] = *reinterpret_cast<const float4*>(W + i * 64);
    for (int t = 0; t < T; ++t) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < HEAD_MAX_D / 64; ++i)
        if (i * 64 < D) s += dot4(*reinterpret_cast<const float4*>(x + t * D + i * 64), w[i]);
      s = group_sum(s, 16);
      if (gl == 0) cas[(m * T + t) * K + k] = s + bias;
    }
  }

  // is_event: one wavefront per timestep
  const int wave = tid >> 6, lane = tid & 63;
  for (int t = wave; t < T; t += 4) {
    float s = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
      const float4 x = *reinterpret_cast<const float4*>(sv + t * D + c), y = *reinterpret_cast<const float4*>(sa + t * D + c);
      const float4 w = *reinterpret_cast<const float4*>(p.wc + c);
      s += (x.x + y.x) * 0.5f * w.x + (x.y + y.y) * 0.5f * w.y + (x.z + y.z) * 0.5f * w.z + (x.w + y.w) * 0.5f * w.w;
    }
    s = group_sum(s, 64);
    if (lane == 0) p.is_event[(long)t * B + b] = s + *p.bc;
  }

  // max over time of the fused feature, first arg-max
  for (int d = tid; d < D; d += 256) {
    float best = (sv[d] + sa[d]) * 0.5f;
    int bt = 0;
    for (int t = 1; t < T; ++t) {
      const float f = (sv[t * D + d] + sa[t * D + d]) * 0.5f;
      if (f > best) { best = f; bt = t; }
    }
    mx[d] = best;
    p.argmax[(long)b * D + d] = bt;
  }
  __syncthreads();

  // mean of the four largest scores over time, per (modality, class): four selection passes, ties to the earlier timestep
  if (tid < 2 * K) {
    const int m = tid >= K, k = tid - m * K;
    unsigned mask = 0u;
    float sum = 0.f;
    for (int j = 0; j < HEAD_TOPK; ++j) {
      float best = 0.f;
      int bt = -1;
      for (int t = 0; t < T; ++t) {
        if ((mask >> t) & 1u) continue;
        const float c = cas[(m * T + t) * K + k];
        if (bt < 0 || c > best) { best = c; bt = t; }
      }
      mask |= 1u << bt;
      sum += best;
    }
    ssum[tid] = sum * 0.25f;
    p.topmask[(long)b * 2 * K + tid] = (int)mask;
  }
  __syncthreads();

  // event scores
  for (int k = grp; k < K; k += 16) {
    const float* W = p.We + (long)k * D + gl * 4;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < HEAD_MAX_D / 64; ++i)
      if (i * 64 < D) s += dot4(*reinterpret_cast<const float4*>(mx + gl * 4 + i * 64), *reinterpret_cast<const float4*>(W + i * 64));
    s = group_sum(s, 16);
    if (gl == 0) {
      const float avs = (ssum[k] + ssum[K + k]) * 0.5f;
      p.av[(long)b * K + k] = avs;
      p.event[(long)b * K + k] = s + p.be[k] + p.gamma * avs;
    }
  }
}

static size_t head_bwd_lds(int T, int D, int K, bool params) {
  // g8 [K] | dev [K] | dis [T] | mask [2K] (int) | am [D] (int)   and with parameter gradients   mvec [D] | sv [T D] | sa [T D]
  return ((size_t)4 * K + T + D + (params ? (size_t)D + (size_t)2 * T * D : 0)) * sizeof(float);
}

__global__ __launch_bounds__(256) void head_bwd_k(const HeadArgs p) {
  extern __shared__ float4 head_smem4[];
  const int T = p.T, B = p.B, D = p.D, K = p.K, tid = threadIdx.x;
  float* base = reinterpret_cast<float*>(head_smem4);
  float* sv = base;                                        // [T][D]   (parameter gradients only; first, for their 16-byte alignment)
  float* sa = sv + (p.part ? T * D : 0);
  float* mvec = sa + (p.part ? T * D : 0);                 // [D]      (parameter gradients only)
  float* g8 = mvec + (p.part ? D : 0);                     // [K]  (d_av + gamma d_ev) / 8: the gradient of a selected score
  float* dev = g8 + K;                                     // [K]
  float* dis = dev + K;                                    // [T]
  unsigned* mask = reinterpret_cast<unsigned*>(dis + T);   // [2][K]
  int* am = reinterpret_cast<int*>(mask + 2 * K);          // [D]
  const long KD = (long)K * D;
  float* row = p.part ? p.part + (long)blockIdx.x * head_row_floats(D, K) : nullptr;
  bool first = true;
  for (int b = blockIdx.x; b < B; b += gridDim.x, first = false) {
    __syncthreads();                                       // the previous clip's readers are done
    if (tid < K) {
      const float de = p.d_ev ? p.d_ev[(long)b * K + tid] : 0.f, da = p.d_av ? p.d_av[(long)b * K + tid] : 0.f;
      dev[tid] = de;
      g8[tid] = (da + p.gamma * de) * 0.125f;
    }
    if (tid < 2 * K) mask[tid] = (unsigned)p.topmask[(long)b * 2 * K + tid];
    if (tid < T) dis[tid] = p.d_is ? p.d_is[(long)tid * B + b] : 0.f;
    for (int d = tid; d < D; d += 256) am[d] = p.argmax[(long)b * D + d];
    if (row) head_stage(p, b, sv, sa);
    __syncthreads();

    if (p.dv) {
      for (int d = tid; d < D; d += 256) {
        float u = 0.f;                                     // sum_k d_ev[k] We[k][d]: goes to the arg-max timestep
        float accv[HEAD_MAX_T], acca[HEAD_MAX_T];
#pragma unroll
        for (int t = 0; t < HEAD_MAX_T; ++t) { accv[t] = 0.f; acca[t] = 0.f; }
        for (int k = 0; k < K; ++k) {
          u += dev[k] * p.We[(long)k * D + d];
          const float g = g8[k], wv = g * p.Wvc[(long)k * D + d], wa = g * p.Wac[(long)k * D + d];
          const unsigned mv = mask[k], ma = mask[K + k];
#pragma unroll
          for (int t = 0; t < HEAD_MAX_T; ++t)
            if (t < T) { accv[t] += ((mv >> t) & 1u) ? wv : 0.f; acca[t] += ((ma >> t) & 1u) ? wa : 0.f; }
        }
        const float w = p.wc[d];
        const int at = am[d];
#pragma unroll
        for (int t = 0; t < HEAD_MAX_T; ++t)
          if (t < T) {
            const float common = 0.5f * (dis[t] * w + (at == t ? u : 0.f));
            const long o = ((long)t * B + b) * D + d;
            p.dv[o] = accv[t] + common;
            p.da[o] = acca[t] + common;
          }
      }
    }

    if (row) {
      for (int d = tid; d < D; d += 256) {
        const int at = am[d];
        mvec[d] = (sv[at * D + d] + sa[at * D + d]) * 0.5f;
        float s = 0.f;                                     // d wc
        for (int t = 0; t < T; ++t) s += dis[t] * ((sv[t * D + d] + sa[t * D + d]) * 0.5f);
        row[3 * KD + d] = first ? s : row[3 * KD + d] + s;
      }
      __syncthreads();
      for (long e = tid; e < KD; e += 256) {
        const int k = (int)(e / D), d = (int)(e - (long)k * D);
        const unsigned mv = mask[k], ma = mask[K + k];
        float s1 = 0.f, s2 = 0.f;
        for (int t = 0; t < T; ++t) {
          if ((mv >> t) & 1u) s1 += sv[t * D + d];
          if ((ma >> t) & 1u) s2 += sa[t * D + d];
        }
        const float c1 = g8[k] * s1, c2 = g8[k] * s2, c3 = dev[k] * mvec[d];
        row[e] = first ? c1 : row[e] + c1;
        row[KD + e] = first ? c2 : row[KD + e] + c2;
        row[2 * KD + e] = first ? c3 : row[2 * KD + e] + c3;
      }
      float* rb = row + 3 * KD + D;
      if (tid < K) {
        const float c1 = g8[tid] * (float)__popc(mask[tid]), c2 = g8[tid] * (float)__popc(mask[K + tid]), c3 = dev[tid];
        rb[tid] = first ? c1 : rb[tid] + c1;
        rb[K + tid] = first ? c2 : rb[K + tid] + c2;
        rb[2 * K + tid] = first ? c3 : rb[2 * K + tid] + c3;
      }
      if (tid == 0) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += dis[t];
        rb[3 * K] = first ? s : rb[3 * K] + s;
      }
    }
  }
}

// second stage: the G partial rows summed in row order, one thread per parameter element
__global__ __launch_bounds__(256) void head_reduce_k(const float* part, int G, int D, int K, const HeadGrads o) {
  const long P = head_row_floats(D, K), KD = (long)K * D;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float s = 0.f;
  for (int r = 0; r < G; ++r) s += part[(long)r * P + i];
  if (i < KD) o.dWvc[i] = s;
  else if (i < 2 * KD) o.dWac[i - KD] = s;
  else if (i < 3 * KD) o.dWe[i - 2 * KD] = s;
  else if (i < 3 * KD + D) o.dwc[i - 3 * KD] = s;
  else if (i < 3 * KD + D + K) o.dbvc[i - 3 * KD - D] = s;
  else if (i < 3 * KD + D + 2 * K) o.dbac[i - 3 * KD - D - K] = s;
  else if (i < 3 * KD + D + 3 * K) o.dbe[i - 3 * KD - D - 2 * K] = s;
  else o.dbc[0] = s;
}

static bool head_ok(const char* who, int T, int B, int D, int K) {
  if (T < HEAD_TOPK || T > HEAD_MAX_T || B < 1 || D < 64 || D % 64 || D > HEAD_MAX_D || K < 1 || K > HEAD_MAX_K) {
    set_error("%s: need %d <= T <= %d (top-k is fixed at %d), D a multiple of 64 and <= %d, 1 <= K <= %d, B >= 1 (got T=%d, B=%d, D=%d, K=%d)",
              who, HEAD_TOPK, HEAD_MAX_T, HEAD_TOPK, HEAD_MAX_D, HEAD_MAX_K, T, B, D, K);
    return false;
  }
  if ((int64_t)T * B * D > 0x7fffffffLL) { set_error("%s: tensor too large", who); return false; }
  return true;
}
static inline bool head_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static int head_wgs(int B) { return B < HEAD_MAX_WGS ? B : HEAD_MAX_WGS; }

template <typename Kern>
static bool head_lds_ok(const char* who, Kern kern, size_t shmem) {
  if (shmem > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: the device refuses %zu bytes of dynamic LDS per workgroup", who, shmem);
    return false;
  }
  return true;
}

}  // namespace dgsct

using namespace dgsct;

extern "C" {

int64_t dgsct_cmbs_head_ws_bytes(int T, int B, int D, int K) {
  clear_error();
  if (!head_ok("dgsct_cmbs_head_ws_bytes", T, B, D, K)) return -1;
  return (int64_t)head_wgs(B) * head_row_floats(D, K) * (int64_t)sizeof(float);
}

int dgsct_cmbs_head_forward(int T, int B, int D, int K, float gamma, const float* v, const float* a, const float* Wvc, const float* bvc,
                            const float* Wac, const float* bac, const float* wc, const float* bc, const float* We, const float* be,
                            float* is_event, float* event, float* av, int32_t* topmask, int32_t* argmax, void* stream) {
  clear_error();
  const char* who = "dgsct_cmbs_head_forward";
  if (!head_ok(who, T, B, D, K)) return 2;
  if (!v || !a || !Wvc || !bvc || !Wac || !bac || !wc || !bc || !We || !be || !is_event || !event || !av || !topmask || !argmax) {
    set_error("%s: NULL argument", who);
    return 2;
  }
  if (!head_al16(v) || !head_al16(a) || !head_al16(Wvc) || !head_al16(Wac) || !head_al16(wc) || !head_al16(We)) {
    set_error("%s: v, a and the weight matrices must be 16-byte aligned", who);
    return 2;
  }
  HeadArgs p{};
  p.T = T; p.B = B; p.D = D; p.K = K; p.gamma = gamma;
  p.v = v; p.a = a; p.Wvc = Wvc; p.bvc = bvc; p.Wac = Wac; p.bac = bac; p.wc = wc; p.bc = bc; p.We = We; p.be = be;
  p.is_event = is_event; p.event = event; p.av = av; p.topmask = topmask; p.argmax = argmax;
  const size_t shmem = head_fwd_lds(T, D, K);
  clear_async();
  if (!head_lds_ok(who, head_fwd_k, shmem)) return 1;
  hipLaunchKernelGGL(head_fwd_k, dim3((unsigned)B), dim3(256), shmem, (hipStream_t)stream, p);
  check_async(who);
  return has_error() ? 1 : 0;
}

int dgsct_cmbs_head_backward(int T, int B, int D, int K, float gamma, const float* v, const float* a, const float* Wvc, const float* Wac,
                             const float* wc, const float* We, const int32_t* topmask, const int32_t* argmax, const float* d_is,
                             const float* d_ev, const float* d_av, float* dv, float* da, float* dWvc, float* dbvc, float* dWac, float* dbac,
                             float* dwc, float* dbc, float* dWe, float* dbe, void* ws, void* stream) {
  clear_error();
  const char* who = "dgsct_cmbs_head_backward";
  if (!head_ok(who, T, B, D, K)) return 2;
  if (!Wvc || !Wac || !wc || !We || !topmask || !argmax) { set_error("%s: NULL argument", who); return 2; }
  if ((dv == nullptr) != (da == nullptr)) { set_error("%s: dv and da are returned together (both or neither)", who); return 2; }
  float* const grads[8] = {dWvc, dbvc, dWac, dbac, dwc, dbc, dWe, dbe};
  int have = 0;
  for (float* g : grads) have += g != nullptr;
  if (have != 0 && have != 8) { set_error("%s: the eight parameter gradients are returned together (all or none)", who); return 2; }
  if (have && (!v || !a || !ws)) { set_error("%s: parameter gradients need v, a and the workspace", who); return 2; }
  if (!have && !dv) return 0;
  if ((have && (!head_al16(v) || !head_al16(a) || !head_al16(ws)))) { set_error("%s: v, a and ws must be 16-byte aligned", who); return 2; }
  HeadArgs p{};
  p.T = T; p.B = B; p.D = D; p.K = K; p.gamma = gamma;
  p.v = v; p.a = a; p.Wvc = Wvc; p.Wac = Wac; p.wc = wc; p.We = We;
  p.topmask = const_cast<int32_t*>(topmask); p.argmax = const_cast<int32_t*>(argmax);
  p.d_is = d_is; p.d_ev = d_ev; p.d_av = d_av; p.dv = dv; p.da = da; p.part = have ? static_cast<float*>(ws) : nullptr;
  const int G = head_wgs(B);
  const size_t shmem = head_bwd_lds(T, D, K, have != 0);
  hipStream_t s = (hipStream_t)stream;
  clear_async();
  if (!head_lds_ok(who, head_bwd_k, shmem)) return 1;
  hipLaunchKernelGGL(head_bwd_k, dim3((unsigned)G), dim3(256), shmem, s, p);
  if (have) {
    const HeadGrads o{dWvc, dbvc, dWac, dbac, dwc, dbc, dWe, dbe};
    const long P = head_row_floats(D, K);
    hipLaunchKernelGGL(head_reduce_k, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(ws), G, D, K, o);
  }
  check_async(who);
  return has_error() ? 1 : 0;
}

}  // extern "C"
