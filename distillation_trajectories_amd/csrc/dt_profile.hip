// The in-library profiler: optional per-launch timing with HIP events on the launch stream (bench.py's roofline numbers).
// A process global: every instrumented launch of the library opens a ProfileScope (dt_internal.h), whatever handle it
// belongs to.  Also the marker kernel that lets an external profiler bracket a region of a stream.
#include <atomic>
#include <mutex>
#include <vector>

#include "dt_internal.h"

using namespace dt;

namespace {
struct ProfRecord { hipEvent_t a, b; int cls; double flops, bytes; };
struct Profiler {
  std::mutex mu;          // launches may come from several host threads (one per stream)
  std::atomic<bool> on{false};   // read by every launch without the lock
  std::vector<ProfRecord> rec;
  std::vector<hipEvent_t> pool;     // events are recycled between sessions
  size_t used = 0;
  hipEvent_t get() {
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      pool.push_back(e);
    }
    return pool[used++];
  }
} g_prof;
const char *kClassName[KC_COUNT - KC_CONV_COUNT] = {
    "splitk_epilogue_kernel", "first_conv_kernel", "maxpool_kernel", "upcat_kernel", "head_kernel", "head_upsample_kernel",
    "time_bias_kernel", "cfg_update_kernel", "traj_metrics_kernel", "wasserstein_kernel", "resampled_distance_kernel",
    "unet_fused_kernel", "pair_metrics_kernel", "conv_strip_pair_bf16x6_kernel<256,128>", "spectral_kernel",
    "swd_scan_kernel", "swd_project_kernel", "swd_sort_kernel", "swd_pair_kernel<sort>", "swd_pair_kernel", "swd_reduce_kernel",
    "sinkhorn_scan_kernel", "sinkhorn_init_kernel", "sinkhorn_cost_kernel", "sinkhorn_row_kernel", "sinkhorn_col_kernel",
    "sinkhorn_finish_kernel", "sinkhorn_rowsum_kernel", "sinkhorn_mean_kernel"};
// the printed name of a class: a convolution class is named after the form(s) that carry it (dt_conv_forms.h)
const char *class_name(int cls) {
  switch (cls) {
#define DT_GEMM(c, kind, bm, bn, kc, wk) case c: return "conv_gemm_kernel<" #bm "," #bn ">";
#define DT_BF16(c, kind, bm, bn, kc, wk) case c: return "conv_gemm_bf16x6_kernel<" #bm "," #bn ">";
#define DT_STRIP(c, kind, bm, bn, kc, wk) case c: return "conv_strip_bf16x6_kernel<" #bm "," #bn ">";
#define DT_STRIPK(c, kind, bm, bn, kc, wk) case c: return "conv_strip_bf16x6_kernel<" #bm "," #bn ",K" #kc ">";
    DT_CONV_FORMS_FP32(DT_GEMM) DT_CONV_FORMS_BF16(DT_BF16) DT_CONV_FORMS_STRIP(DT_STRIP) DT_CONV_FORMS_STRIPK(DT_STRIPK)
    default: return kClassName[cls - KC_CONV_COUNT];
  }
}
}  // namespace

namespace dt {
ProfileScope::ProfileScope(int cls, double flops, double bytes, hipStream_t s) : slot(-1), stream(s), end_event(nullptr) {
  if (!g_prof.on.load(std::memory_order_relaxed)) return;
  hipEvent_t a;
  {
    std::lock_guard<std::mutex> lock(g_prof.mu);
    if (!g_prof.on.load(std::memory_order_relaxed)) return;   // a concurrent dt_profile_end
    a = g_prof.get();
    hipEvent_t b = g_prof.get();
    if (!a || !b) return;
    g_prof.rec.push_back(ProfRecord{a, b, cls, flops, bytes});
    slot = (int)g_prof.rec.size() - 1;
    end_event = b;             // kept here: a concurrent dt_profile_begin may clear `rec` before the destructor runs
  }
  (void)hipEventRecord(a, s);
}
ProfileScope::~ProfileScope() {
  if (slot < 0) return;
  (void)hipEventRecord((hipEvent_t)end_event, stream);
}
bool profiling_on() { return g_prof.on.load(); }
}  // namespace dt

extern "C" {

// an empty kernel with a recognisable name: lets an external profiler (rocprofv3 traces) bracket a region of the stream
__global__ void profile_marker_kernel(int) {}

int dt_profile_marker(int id, void *stream) {
  profile_marker_kernel<<<1, 64, 0, (hipStream_t)stream>>>(id);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

int dt_profile_begin(void) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  g_prof.rec.clear();
  g_prof.used = 0;
  g_prof.on = true;
  return DT_OK;
}

int dt_profile_end(void) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  g_prof.on = false;
  return DT_OK;
}

int dt_profile_class_count(void) { return KC_COUNT; }

int dt_profile_read(int cls, const char **name, long long *launches, double *ms, double *flops, double *bytes) {
  if (cls < 0 || cls >= KC_COUNT || !launches || !ms || !flops || !bytes) return DT_E_ARG;
  if (name) *name = class_name(cls);
  *launches = 0; *ms = 0; *flops = 0; *bytes = 0;
  std::lock_guard<std::mutex> lock(g_prof.mu);
  for (const ProfRecord &r : g_prof.rec) {
    if (r.cls != cls) continue;
    DT_HIP_TRY(hipEventSynchronize(r.b));
    float t = 0.f;
    DT_HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
    *launches += 1; *ms += t; *flops += r.flops; *bytes += r.bytes;
  }
  return DT_OK;
}

}  // extern "C"
