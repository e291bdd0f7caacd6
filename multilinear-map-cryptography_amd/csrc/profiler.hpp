// profiler.hpp -- per-stage device time from HIP events around the launches of one named stage.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace tns {

// Per-stage device time from HIP events recorded around the launches of one named stage
// (enabled by tns_profile_enable; used by bench.py for the roofline's live kernel duration).
// Besides the summed launch durations, each stage keeps the union of its launch intervals
// (stages of two MSM lanes overlap) and an optional operation count (MSM mixed additions).
struct KernelProfiler {
  bool enabled = false;
  hipEvent_t ref = nullptr;  // recorded at enable: common time origin of every stream
  struct Rec {
    std::string name;
    hipEvent_t a, b;
    double bytes;
  };
  struct Tot {
    double ms = 0, bytes = 0, ops = 0, busy_ms = 0;
    uint64_t launches = 0;
    std::vector<std::pair<double, double>> iv;
  };
  std::vector<Rec> pending;
  std::map<std::string, Tot> totals;
  std::string only;  // non-empty: time this stage alone
  void start(hipStream_t s) {
    reset();
    if (!ref) (void)hipEventCreate(&ref);
    (void)hipEventRecord(ref, s);
  }
  void reset() {
    collect();
    totals.clear();
  }
  void add_ops(const char *name, double ops) {
    if (enabled) totals[name].ops += ops;
  }
  void collect() {
    for (auto &r : pending) {
      float ms = 0.f, t0 = 0.f, t1 = 0.f;
      if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
        static const bool dbg = getenv("TNS_PROF_DEBUG") != nullptr;  // (diagnostics: read once)
        if (dbg) fprintf(stderr, "prof %s %.3f ms\n", r.name.c_str(), ms);
        auto &t = totals[r.name];
        t.ms += ms;
        t.launches += 1;
        t.bytes += r.bytes;
        if (ref && hipEventElapsedTime(&t0, ref, r.a) == hipSuccess && hipEventElapsedTime(&t1, ref, r.b) == hipSuccess)
          t.iv.emplace_back(t0, t1);
      }
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
    pending.clear();
    for (auto &kv : totals) {  // union of the launch intervals
      auto &iv = kv.second.iv;
      std::sort(iv.begin(), iv.end());
      double busy = 0, lo = -1, hi = -1;
      for (auto &x : iv) {
        if (x.first > hi) {
          busy += hi - lo;
          lo = x.first;
          hi = x.second;
        } else if (x.second > hi) {
          hi = x.second;
        }
      }
      busy += hi - lo;
      kv.second.busy_ms = busy;
    }
  }
};

struct ProfScope {
  KernelProfiler *p = nullptr;
  hipStream_t s;
  KernelProfiler::Rec r;
  ProfScope(KernelProfiler &prof, hipStream_t st, const char *name, double alg_bytes) : s(st) {
    if (!prof.enabled || (!prof.only.empty() && prof.only != name)) return;
    p = &prof;
    r.name = name;
    r.bytes = alg_bytes;
    (void)hipEventCreate(&r.a);
    (void)hipEventCreate(&r.b);
    (void)hipEventRecord(r.a, s);
  }
  ~ProfScope() {
    if (!p) return;
    (void)hipEventRecord(r.b, s);
    p->pending.push_back(r);
  }
};

#define TNS_CAT2(a, b) a##b
#define TNS_CAT(a, b) TNS_CAT2(a, b)
// TNS_PROF(ctx, "stage", algorithmic_bytes_of_this_launch): ctx is a Ctx * (ctx.hpp)
#define TNS_PROF(ctx, name, bytes) \
  ::tns::ProfScope TNS_CAT(_tns_prof_, __LINE__)((ctx)->prof, (ctx)->stream, name, (double)(bytes))
#define TNS_PROF_ON(ctx, stream, name, bytes) \
  ::tns::ProfScope TNS_CAT(_tns_prof_, __LINE__)((ctx)->prof, stream, name, (double)(bytes))

}  // namespace tns
