// extern "C" surface of libdgsct.so (include/dgsct.h).  No exceptions, no torch types, no device
// allocations: descriptors in, raw device pointers in, status code out.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/dgsct.h"
#include "err.h"
#include "plan.h"
#include "prims.h"
#include "gemm_int.h"
#include "tune.h"

using namespace dgsct;

// Entry of every call: forget this thread's previous dgsct error AND any stale sticky HIP error another library (PyTorch)
// left on the thread, so that check_async() at the end reports only what THIS call raised.
static inline void begin_call() { clear_error(); clear_async(); }
// pure host entry points (queries, layout introspection): no HIP runtime call at all
static inline void begin_host_call() { clear_error(); }

extern "C" {

int dgsct_version(void) { return DGSCT_VERSION; }
const char* dgsct_arch(void) { return "gfx950"; }
const char* dgsct_last_error(void) { return last_error(); }

int dgsct_query(const dgsct_adapter_desc* desc, dgsct_sizes* out) {
  begin_host_call();
  if (!desc || !out) { set_error("dgsct_query: NULL argument"); return 2; }
  Plan p(*desc);
  if (!p.ok) return 2;
  out->prep_bytes = p.prep_bytes;
  out->saved_bytes = p.saved_bytes;
  out->ws_fwd_bytes = p.ws_fwd_bytes;
  out->ws_bwd_bytes = p.ws_bwd_bytes;
  out->grad_floats = p.grad_floats;
  for (int i = 0; i < DGSCT_P_COUNT; ++i) { out->grad_offset[i] = p.grad_off[i]; out->grad_numel[i] = p.grad_numel[i]; }
  return 0;
}

int dgsct_prepare(const dgsct_adapter_desc* desc, float* const* params, void* prep, void* stream) {
  begin_call();
  if (!desc || !params || !prep) { set_error("dgsct_prepare: NULL argument"); return 2; }
  Plan p(*desc);
  if (!p.ok) return 2;
  return p.prepare(params, prep, stream);
}

int dgsct_adapter_forward(const dgsct_adapter_desc* desc, float* const* params, const void* prep, const void* X,
                          const void* Y, void* out, float* map, float* tmap, void* saved, void* ws, void* stream) {
  begin_call();
  if (!desc || !params || !prep || !X || !Y || !out || !map || !saved || !ws) {
    set_error("dgsct_adapter_forward: NULL argument");
    return 2;
  }
  Plan p(*desc);
  if (!p.ok) return 2;
  return p.forward(params, prep, X, Y, out, map, tmap, saved, ws, stream);
}

int dgsct_adapter_forward_ex(const dgsct_adapter_desc* desc, float* const* params, const void* prep, const void* X,
                             const void* Y, const void* residual, void* out, float* map, float* tmap, void* saved, void* ws,
                             void* stream, void* aux_stream) {
  begin_call();
  if (!desc || !params || !prep || !X || !Y || !out || !map || !saved || !ws) {
    set_error("dgsct_adapter_forward_ex: NULL argument");
    return 2;
  }
  if (residual && out == residual) {        // rows are read and written by the same lanes, but keep the contract simple
    set_error("dgsct_adapter_forward_ex: out must not alias residual");
    return 2;
  }
  Plan p(*desc);
  if (!p.ok) return 2;
  void* rec = call_prof_begin(stream, 0, desc->N, desc->C);
  const int rc = p.forward(params, prep, X, Y, out, map, tmap, saved, ws, stream, residual, aux_stream);
  call_prof_end(rec);
  return rc;
}

int dgsct_adapter_backward(const dgsct_adapter_desc* desc, float* const* params, const void* prep, const void* X,
                           const void* Y, const void* saved, const void* dOut, const float* dMap, const float* dTmap,
                           void* dX, void* dY, float* grads, void* ws, void* stream) {
  return dgsct_adapter_backward_ex(desc, params, prep, X, Y, saved, dOut, dMap, dTmap, dX, dY, grads, ws, stream, nullptr, 0);
}

int dgsct_adapter_backward_ex(const dgsct_adapter_desc* desc, float* const* params, const void* prep, const void* X,
                              const void* Y, const void* saved, const void* dOut, const float* dMap, const float* dTmap,
                              void* dX, void* dY, float* grads, void* ws, void* stream, void* aux_stream,
                              int skip_into_dx) {
  begin_call();
  if (!desc || !params || !prep || !X || !Y || !saved || !dOut || !dX || !dY || !grads || !ws) {
    set_error("dgsct_adapter_backward: NULL argument");
    return 2;
  }
  Plan p(*desc);
  if (!p.ok) return 2;
  void* rec = call_prof_begin(stream, 1, desc->N, desc->C);
  const int rc = p.backward(params, prep, X, Y, saved, dOut, dMap, dTmap, dX, dY, grads, ws, stream, aux_stream, (skip_into_dx & DGSCT_BWD_SKIP_INTO_DX) != 0,
                            (skip_into_dx & DGSCT_BWD_NO_JOIN) != 0);
  call_prof_end(rec);
  return rc;
}

int dgsct_adapter_backward_ex2(const dgsct_adapter_desc* desc, float* const* params, const void* prep, const void* X,
                               const void* Y, const void* saved, const void* dOut, const float* dMap, const float* dTmap,
                               void* dX, void* dY, float* grads, void* ws, void* stream, void* aux_stream,
                               const dgsct_bwd_opts* opts) {
  begin_call();
  if (!opts) { set_error("dgsct_adapter_backward_ex2: NULL options"); return 2; }
  const int fl = opts->flags;
  if ((fl & DGSCT_BWD_HOLD_DY) && (fl & DGSCT_BWD_ONLY_DY)) { set_error("dgsct_adapter_backward_ex2: HOLD_DY and ONLY_DY are the two parts of one call"); return 2; }
  BwdPair pr;
  pr.phase = (fl & DGSCT_BWD_HOLD_DY) ? 1 : (fl & DGSCT_BWD_ONLY_DY) ? 2 : 0;
  pr.dy_residual = opts->dy_residual; pr.dx_event = opts->dx_ready_event; pr.dy_wait = opts->dy_wait_event;
  if (pr.phase == 1 && pr.dy_residual) { set_error("dgsct_adapter_backward_ex2: dy_residual belongs to the part that writes dY"); return 2; }
  if (pr.phase == 2) {
    if (!desc || !params || !prep || !dY || !ws) { set_error("dgsct_adapter_backward_ex2 (ONLY_DY): NULL argument"); return 2; }
  } else if (!desc || !params || !prep || !X || !Y || !saved || !dOut || !dX || !grads || !ws || (pr.phase == 0 && !dY)) {
    set_error("dgsct_adapter_backward_ex2: NULL argument");
    return 2;
  }
  Plan p(*desc);
  if (!p.ok) return 2;
  void* rec = pr.phase == 2 ? nullptr : call_prof_begin(stream, 1, desc->N, desc->C);
  const int rc = p.backward(params, prep, X, Y, saved, dOut, dMap, dTmap, dX, dY, grads, ws, stream, aux_stream, (fl & DGSCT_BWD_SKIP_INTO_DX) != 0,
                            (fl & DGSCT_BWD_NO_JOIN) != 0, &pr);
  if (rec) call_prof_end(rec);
  return rc;
}

int dgsct_saved_region(const dgsct_adapter_desc* desc, int i, char* name, int name_cap, int64_t* offset, int64_t* bytes) {
  begin_host_call();
  if (!desc) return 2;
  Plan p(*desc, true);
  if (!p.ok) return 2;
  if (i < 0 || i >= (int)p.saved_regions.size()) return 1;
  const Region& r = p.saved_regions[i];
  if (name && name_cap > 0) { std::strncpy(name, r.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (offset) *offset = r.offset;
  if (bytes) *bytes = r.bytes;
  return 0;
}

int dgsct_stream_create(int priority_class, void** stream) {
  begin_call();
  if (!stream) return 2;
  *stream = stream_create(priority_class);
  return has_error() ? 1 : 0;
}

int dgsct_stream_destroy(void* stream) {
  begin_call();
  stream_destroy(stream);
  return has_error() ? 1 : 0;
}

static int pool_args_ok(int dtype, int BT, int N, int C, const void* F, const float* map) {
  if ((dtype != DGSCT_F32 && dtype != DGSCT_BF16) || BT <= 0 || N <= 0 || C <= 0 || C % 4 != 0 || !F || !map) {
    set_error("map_pool: dtype must be DGSCT_F32 / DGSCT_BF16, BT, N, C positive, C a multiple of 4, F and map non-null");
    return 0;
  }
  return 1;
}

int dgsct_map_pool_forward(int dtype, int BT, int N, int C, const void* F, const float* map, float* pooled, void* stream) {
  begin_call();
  if (!pool_args_ok(dtype, BT, N, C, F, map) || !pooled) { if (!has_error()) set_error("map_pool: pooled is null"); return 2; }
  Ctx ctx{stream, dtype};
  zero(ctx, pooled, (size_t)BT * C * sizeof(float));
  colsum_batched(ctx, F, C, (long)N * C, BT, N, C, map, N, 1.f, pooled, C);
  return has_error() ? 1 : 0;
}

int dgsct_map_pool_backward(int dtype, int BT, int N, int C, const void* F, const float* map, const float* dPooled,
                            void* dF, float* dMap, void* stream) {
  begin_call();
  if (!pool_args_ok(dtype, BT, N, C, F, map) || !dPooled) { if (!has_error()) set_error("map_pool: dPooled is null"); return 2; }
  Ctx ctx{stream, dtype};
  if (dF) outer_rows(ctx, map, dPooled, BT, N, C, dF);
  if (dMap) rowdot_batched(ctx, F, C, (long)N * C, BT, N, C, dPooled, DT_F32, C, nullptr, nullptr, dMap);
  return has_error() ? 1 : 0;
}

int dgsct_temporal_gate_forward(int R, int D, float gamma, const float* akv, const float* vkv, const float* vq, const float* aq,
                                const float* wa, const float* ba, const float* wv, const float* bv, float* out_v, float* out_a,
                                float* gate, float* ga, float* gv, void* stream) {
  begin_call();
  if (!akv || !vkv || !vq || !aq || !wa || !ba || !wv || !bv || !out_v || !out_a || !gate || !ga || !gv) {
    set_error("dgsct_temporal_gate_forward: NULL argument");
    return 2;
  }
  Ctx ctx{stream, DT_F32};
  temporal_gate_fwd(ctx, R, D, gamma, akv, vkv, vq, aq, wa, ba, wv, bv, out_v, out_a, gate, ga, gv);
  check_async("dgsct_temporal_gate_forward");
  return has_error() ? 1 : 0;
}
int dgsct_temporal_gate_backward(int R, int D, float gamma, const float* akv, const float* vkv, const float* vq, const float* aq,
                                 const float* wa, const float* wv, const float* ga, const float* gv, const float* dOv,
                                 const float* dOa, const float* dg, float* dakv, float* dvkv, float* dvq, float* daq, float* dwa,
                                 float* dba, float* dwv, float* dbv, void* stream) {
  begin_call();
  if (!akv || !vkv || !vq || !aq || !wa || !wv || !ga || !gv || !dOv || !dOa || !dakv || !dvkv || !dvq || !daq || !dwa || !dba ||
      !dwv || !dbv) {
    set_error("dgsct_temporal_gate_backward: NULL argument");
    return 2;
  }
  Ctx ctx{stream, DT_F32};
  temporal_gate_bwd(ctx, R, D, gamma, akv, vkv, vq, aq, wa, wv, ga, gv, dOv, dOa, dg, dakv, dvkv, dvq, daq, dwa, dba, dwv, dbv);
  check_async("dgsct_temporal_gate_backward");
  return has_error() ? 1 : 0;
}

int dgsct_frame_scale_forward(int dtype, int rows, int64_t inner, float gamma, const void* x, const float* g, void* y, void* stream) {
  begin_call();
  if (!x || !g || !y) { set_error("dgsct_frame_scale_forward: NULL argument"); return 2; }
  if (dtype != DGSCT_F32 && dtype != DGSCT_BF16) { set_error("dgsct_frame_scale_forward: dtype"); return 2; }
  Ctx ctx{stream, dtype};
  frame_scale_fwd(ctx, rows, (long)inner, gamma, x, g, y);
  check_async("dgsct_frame_scale_forward");
  return has_error() ? 1 : 0;
}
int dgsct_frame_scale_backward(int dtype, int rows, int64_t inner, float gamma, const void* x, const float* g, const void* dy, void* dx,
                               float* dg, void* stream) {
  begin_call();
  if (!x || !g || !dy) { set_error("dgsct_frame_scale_backward: NULL argument"); return 2; }
  if (dtype != DGSCT_F32 && dtype != DGSCT_BF16) { set_error("dgsct_frame_scale_backward: dtype"); return 2; }
  Ctx ctx{stream, dtype};
  frame_scale_bwd(ctx, rows, (long)inner, gamma, x, g, dy, dx, dg);
  check_async("dgsct_frame_scale_backward");
  return has_error() ? 1 : 0;
}

int dgsct_test_gemm(const dgsct_gemm_args* a, void* stream) {
  begin_call();
  if (!a) return 2;
  Ctx ctx{stream, a->mode};
  Gemm g;
  g.M = a->M; g.N = a->N; g.K = a->K; g.KB = a->KB; g.batch = a->batch; g.splitk = a->splitk; g.atomic = a->atomic != 0;
  g.sole_writer = a->atomic == 2;                      // atomic = 2: D is pre-zeroed and this product is its only writer
  g.A.p = a->A; g.A.ld = a->lda; g.A.kmajor = a->a_kmajor; g.A.bs = a->a_bs; g.A.kbs = a->a_kbs;
  g.B.p = a->B; g.B.ld = a->ldb; g.B.kmajor = a->b_kmajor; g.B.bs = a->b_bs; g.B.kbs = a->b_kbs;
  g.D = a->D; g.ddt = a->ddt; g.ldd = a->ldd; g.dbs = a->dbs;
  g.alpha = a->alpha; g.alpha_ptr = a->alpha_ptr;
  g.bias_m = a->bias_m; g.bias_n = a->bias_n; g.bias_n_bs = a->bias_n_bs; g.m_mod = a->m_mod;
  g.r1_m = a->r1_m; g.r1_n = a->r1_n; g.act = a->act;
  g.R = a->R; g.rdt = a->rdt; g.ldr = a->ldr; g.rbs = a->rbs; g.beta = a->beta;
  g.mask = a->mask; g.ldmask = a->ldmask; g.maskbs = a->maskbs;
  g.R2 = a->R2; g.sm_scale = a->sm_scale; g.sm_dot = a->sm_dot;
  gemm(ctx, g);
  return has_error() ? 1 : 0;
}

int64_t dgsct_test_attn_scratch_floats(int B, int N, int C, int tk) {
  return tokattn_scratch_floats(B, N, C) + (int64_t)B * tk + 64;
}
int dgsct_test_attn(int op, const dgsct_attn_args* a, void* stream) {
  begin_call();
  if (!a) return 2;
  Ctx ctx{stream, a->mode};
  switch (op) {
    case 0: tokattn_fwd(ctx, a->Yp, a->T0, a->B, a->N, a->C, a->tk, a->tok, a->lse, a->a, a->aE, a->scratch, a->tokpk, a->T0pk); break;
    case 1: xattn_fwd(ctx, a->X, a->tok, a->gate_av, a->B, a->N, a->C, a->tk, a->out, a->tokpk); break;
    case 2: xattn_bwd(ctx, a->X, a->dX1, a->tok, a->gate_av, a->B, a->N, a->C, a->tk, a->out, a->R2, a->dtok, a->dgate, a->tokpk); break;
    case 3: tokattn_bwd(ctx, a->Yp, a->T0, a->tok, a->lse, a->dtok, a->da, a->invN, a->B, a->N, a->C, a->tk, a->out, a->dT0b,
                        a->scratch, a->T0pk, a->dtokpk); break;
    case 4: if (a->T0pk) tok_pack(ctx, a->T0, 1, a->tk, a->C, a->T0pk); break;
    default: set_error("dgsct_test_attn: unknown op %d", op); return 2;
  }
  check_async("dgsct_test_attn");
  return has_error() ? 1 : 0;
}

int dgsct_window_attn_forward_ex(int B, int H, int W, int ws, int shift, int heads, int hd, int nwm, int flags, const void* qkv, const float* bm,
                                 const float* scale, void* out, float* lse, void* stream) {
  begin_call();
  if (!qkv || !bm || !scale || !out || !lse) { set_error("dgsct_window_attn_forward: NULL argument"); return 2; }
  if (flags & ~DGSCT_WATTN_COSINE) { set_error("dgsct_window_attn_forward: unknown flag bits 0x%x", flags); return 2; }
  const int rc = window_attn_forward(stream, B, H, W, ws, shift, heads, hd, nwm, qkv, bm, scale, out, lse, flags & DGSCT_WATTN_COSINE);
  if (rc) return rc;
  check_async("dgsct_window_attn_forward");
  return has_error() ? 1 : 0;
}
int dgsct_window_attn_backward_ex(int B, int H, int W, int ws, int shift, int heads, int hd, int nwm, int flags, const void* qkv, const float* bm,
                                  const float* scale, const void* out, const float* lse, const void* dout, void* dqkv, void* stream) {
  begin_call();
  if (!qkv || !bm || !scale || !out || !lse || !dout || !dqkv) { set_error("dgsct_window_attn_backward: NULL argument"); return 2; }
  if (flags & ~DGSCT_WATTN_COSINE) { set_error("dgsct_window_attn_backward: unknown flag bits 0x%x", flags); return 2; }
  const int rc = window_attn_backward(stream, B, H, W, ws, shift, heads, hd, nwm, qkv, bm, scale, out, lse, dout, dqkv, flags & DGSCT_WATTN_COSINE);
  if (rc) return rc;
  check_async("dgsct_window_attn_backward");
  return has_error() ? 1 : 0;
}
int dgsct_window_attn_forward(int B, int H, int W, int ws, int shift, int heads, int hd, int nwm, const void* qkv, const float* bm,
                              const float* scale, void* out, float* lse, void* stream) {
  return dgsct_window_attn_forward_ex(B, H, W, ws, shift, heads, hd, nwm, 0, qkv, bm, scale, out, lse, stream);
}
int dgsct_window_attn_backward(int B, int H, int W, int ws, int shift, int heads, int hd, int nwm, const void* qkv, const float* bm,
                               const float* scale, const void* out, const float* lse, const void* dout, void* dqkv, void* stream) {
  return dgsct_window_attn_backward_ex(B, H, W, ws, shift, heads, hd, nwm, 0, qkv, bm, scale, out, lse, dout, dqkv, stream);
}

static bool ln_check(const char* who, int dtype, int64_t rows, int C) {
  if (dtype != DGSCT_F32 && dtype != DGSCT_BF16) { set_error("%s: dtype must be DGSCT_F32 or DGSCT_BF16", who); return false; }
  if (rows < 1 || rows > 0x7fffffffLL || C < 4 || C > 1536 || C % 4 || (dtype == DGSCT_BF16 && C % 8)) {
    set_error("%s: rows must be 1 .. 2^31-1, C a multiple of 4 (bf16: 8) and <= 1536 (got %lld x %d)", who, (long long)rows, C);
    return false;
  }
  return true;
}
int64_t dgsct_layer_norm_scratch_floats(int C) { return row_part_floats(0, C); }
int dgsct_layer_norm_forward(int dtype, int64_t rows, int C, const void* x, const float* w, const float* b, float eps, const void* residual,
                             void* out, float* mu, float* rstd, void* stream) {
  begin_call();
  if (!x || !w || !b || !out || !mu || !rstd) { set_error("dgsct_layer_norm_forward: NULL argument"); return 2; }
  if (!ln_check("dgsct_layer_norm_forward", dtype, rows, C)) return 2;
  Ctx ctx{stream, dtype};
  tail_fwd(ctx, x, nullptr, nullptr, w, b, nullptr, 0, eps, (long)rows, C, out, mu, rstd, residual, nullptr);
  check_async("dgsct_layer_norm_forward");
  return has_error() ? 1 : 0;
}
int dgsct_layer_norm_backward(int dtype, int64_t rows, int C, const void* dout, const void* x, const float* w, const float* b, const float* mu,
                              const float* rstd, float eps, void* dx, float* dw, float* db, float* scratch, void* stream) {
  begin_call();
  if (!dout || !x || !w || !b || !mu || !rstd || !dx || !dw || !db) { set_error("dgsct_layer_norm_backward: NULL argument"); return 2; }
  if (!ln_check("dgsct_layer_norm_backward", dtype, rows, C)) return 2;
  Ctx ctx{stream, dtype};
  tail_bwd(ctx, dout, x, nullptr, nullptr, nullptr, nullptr, w, b, nullptr, 0, mu, rstd, (long)rows, C, dx, dw, db, nullptr, nullptr, eps,
           scratch, scratch ? row_part_floats(0, C) : 0);
  check_async("dgsct_layer_norm_backward");
  return has_error() ? 1 : 0;
}

int dgsct_test_gemm_fp8(int M, int N, int K, const void* A, const float* W, const float* bias, int relu, void* D, void* w8,
                        float* scale, void* stream) {
  begin_call();
  if (!A || !W || !D || !w8 || !scale) { set_error("dgsct_test_gemm_fp8: NULL argument"); return 2; }
  Ctx ctx{stream, DT_BF16};
  fp8_quantize(ctx, W, (long)N * K, w8, scale, scale + 1);
  gemm_fp8(ctx, M, N, K, A, K, w8, scale, bias, relu, D, N);
  check_async("dgsct_test_gemm_fp8");
  return has_error() ? 1 : 0;
}

// The what-if switches ("skip", "skipminc", "skipmaxc", "noatomic") drop launches / atomics: RESULTS ARE GARBAGE, timing is real.  They are
// process-global, so they can be SET only in a process that opted in with DGSCT_WHATIF=1 (tools/call_overlap.py does; nothing in the
// package, the tests or bench.py does); querying (value < 0) is always allowed and bench.py refuses to print a line while one is set.
static bool whatif_allowed(int value) {
  if (value < 0) return true;
  static const bool on = getenv("DGSCT_WHATIF") && !strcmp(getenv("DGSCT_WHATIF"), "1");
  if (!on && value != 0) set_error("dgsct_test_tune: what-if switches need DGSCT_WHATIF=1 in the environment (results are garbage with them)");
  return on || value == 0;
}

int dgsct_test_tune(const char* key, int value) {
  const int id = tune_find(key);
  if (id < 0) return -1;
  if (tune_is_whatif((TuneId)id) && !whatif_allowed(value)) return -2;
  if (id == T_CALLPROF && value == 2) { call_prof_dump(getenv("DGSCT_CALL_PROF") ? getenv("DGSCT_CALL_PROF") : "/tmp/dgsct_callprof.txt"); return 0; }
  return tune_set((TuneId)id, value);
}

int dgsct_prof_enable(int on) { gemm_prof_enable(on); return 0; }
int dgsct_prof_collect(int64_t* launches, double* total_ms, double* total_flops) {
  long n = 0;
  gemm_prof_collect(&n, total_ms, total_flops);
  if (launches) *launches = n;
  return 0;
}

}  // extern "C"
