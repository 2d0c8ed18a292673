// The run-time switches behind dgsct_test_tune (tests, tools, A/B runs): ONE table (tune_entries below) holds every key with its default,
// its clamp rule and its what-if flag, for libdgsct.so and for the host emulation (tests/emu) alike.  Header-only (inline variables, one
// instance per library): every file that includes prims.h has it, and no build recipe has to name a file for it.
// Process-wide and atomic: DataParallel replicas run on threads.
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>

namespace dgsct {

enum TuneId {
  T_GEMM8,      // 8-wave LDS-DMA GEMM (gemm8.hip): 0 off, 1 on, 2 also below the size gates
  T_G8STAG,     // ... its two wave halves issue their LDS-DMA shares a quarter k-tile apart (1) or in lock-step (0)
  T_GEMMFX,     // fused-engine call sites (plan.cpp), bit mask: 1 dZ (BN2 backward), 2 dX3 (ReLU + BN1 backward), 4 dXc (ReLU backward +
                // channel-gate backward), 8 dX1 += dvq1 Wv1 (ReLU backward); 16: the A-operand prologues of sites 4 / 8 at every width
                // (default: C <= 256); 32: site 4 never with its prologue (tests); FORWARD sites: 64 vq1 product + per-frame column
                // sums / positive counts, 128 the two bottleneck products + their BatchNorm sums; 0 = the separate launches
  T_WGBT,       // batched small weight gradients (gemm_wgbt.hip)
  T_SKINNY,     // [BT, C] gate-MLP products with K split over the waves (gemm_skinny.hip)
  T_GEMMTALL,   // weight gradients over the token rows (gemm_tall.hip): 2 takes everything from 16 384 rows (tests)
  T_VQ1FUSE,    // fused vq1 pass (fused_gate.hip): 2 = fused, and the forward also stores vq1 (tests)
  T_GATEFUSE,   // fused gate chain (fused_gate.hip): 2 = fused, and the forward also stores vq2 (tests)
  T_ROWFUSE,    // fused row passes (prims_proj.hip)
  T_BNFOLD,     // BatchNorm finalize folded into the consumers (prims_strip.hip)
  T_SKFUSE,     // fused skinny products (gemm_skinny.hip)
  T_CALLPROF,   // per-call time line (gemm.hip)
  T_SKIP,       // what-if (timing only, results are garbage): mask of launch classes left out of the schedule (plan.cpp)
  T_SKIPMINC,   // ... only for adapters at least / at most that wide
  T_SKIPMAXC,
  T_NOATOMIC,   // what-if: split-K partial tiles leave as plain stores instead of fp32 atomics
  T_COUNT
};

inline std::atomic<int> g_tune[T_COUNT];      // zero-initialised before any initialiser runs; tune_init() fills it

// the only thing a launch path does: one relaxed load, no string lookup
inline int tune(TuneId id) { return g_tune[id].load(std::memory_order_relaxed); }

enum TuneClamp {
  TC_ANY,          // stored as given
  TC_BOOL,         // set ? 1 : 0
  TC_BYTE,         // set & 255
  TC_UPTO2,        // 0 / 1 / 2; anything above is 1
  TC_ONLY01,       // 0 / 1; anything else is not stored
  TC_ZERO_IS_MAX   // 0 is stored as 1 << 30 ("no upper bound")
};
struct TuneEntry { const char* key; int dflt; const char* env; TuneClamp clamp; bool whatif; };

// THE table, in TuneId order.  `env`: read once at load, its value is the key's initial value.
inline const TuneEntry tune_entries[T_COUNT] = {
  /* T_GEMM8    */ {"gemm8",    1,             "DGSCT_GEMM8",       TC_ANY,         false},
  /* T_G8STAG   */ {"g8stag",   1,             nullptr,             TC_BOOL,        false},
  /* T_GEMMFX   */ {"gemmfx",   15 + 64 + 128, nullptr,             TC_BYTE,        false},
  /* T_WGBT     */ {"wgbt",     1,             nullptr,             TC_BOOL,        false},
  /* T_SKINNY   */ {"skinny",   1,             "DGSCT_GEMM_SKINNY", TC_ANY,         false},
  /* T_GEMMTALL */ {"gemmtall", 1,             nullptr,             TC_UPTO2,       false},
  /* T_VQ1FUSE  */ {"vq1fuse",  1,             nullptr,             TC_UPTO2,       false},
  /* T_GATEFUSE */ {"gatefuse", 1,             nullptr,             TC_UPTO2,       false},
  /* T_ROWFUSE  */ {"rowfuse",  1,             nullptr,             TC_BOOL,        false},
  /* T_BNFOLD   */ {"bnfold",   1,             nullptr,             TC_BOOL,        false},
  /* T_SKFUSE   */ {"skfuse",   1,             nullptr,             TC_BOOL,        false},
  /* T_CALLPROF */ {"callprof", 0,             nullptr,             TC_ONLY01,      false},
  /* T_SKIP     */ {"skip",     0,             nullptr,             TC_ANY,         true},
  /* T_SKIPMINC */ {"skipminc", 0,             nullptr,             TC_ANY,         true},
  /* T_SKIPMAXC */ {"skipmaxc", 1 << 30,       nullptr,             TC_ZERO_IS_MAX, true},
  /* T_NOATOMIC */ {"noatomic", 0,             nullptr,             TC_ANY,         true},
};

inline bool tune_init() {
  for (int i = 0; i < T_COUNT; ++i) {
    const TuneEntry& e = tune_entries[i];
    const char* v = e.env ? getenv(e.env) : nullptr;
    g_tune[i].store(v ? atoi(v) : e.dflt, std::memory_order_relaxed);
  }
  return true;
}
// Runs at load (tune_at_load), or earlier when another file's initialiser sets a key first: a set made at load is not overwritten.
inline bool tune_ensure_init() { static const bool done = tune_init(); return done; }
inline const bool tune_at_load = tune_ensure_init();

// stores `value` through the key's clamp rule (value < 0: query only); returns the old value
inline int tune_set(TuneId id, int value) {
  tune_ensure_init();
  const int old = tune(id);
  if (value < 0) return old;
  switch (tune_entries[id].clamp) {
    case TC_ANY: break;
    case TC_BOOL: value = value ? 1 : 0; break;
    case TC_BYTE: value &= 255; break;
    case TC_UPTO2: value = value > 2 ? 1 : value; break;
    case TC_ONLY01: if (value > 1) return old; break;
    case TC_ZERO_IS_MAX: value = value ? value : (1 << 30); break;
  }
  g_tune[id].store(value, std::memory_order_relaxed);
  return old;
}

// TuneId of a dgsct_test_tune key, -1: unknown
inline int tune_find(const char* key) {
  for (int i = 0; key && i < T_COUNT; ++i)
    if (!strcmp(key, tune_entries[i].key)) return i;
  return -1;
}

inline bool tune_is_whatif(TuneId id) { return tune_entries[id].whatif; }

}  // namespace dgsct
