// The device-resident reverse-diffusion loop of a U-Net handle: the record of one sampler call, the loop over its steps
// (fused: up to kFusedMaxSteps per launch; layered: a forward and an update per step), the opt-in graph replay and the three
// sampler entries of include/dt_hip.h and include/dt_hip_edit.h.
#include <cstdio>
#include <cstdlib>

#include "../../include/dt_hip_edit.h"
#include "dt_unet.h"

using namespace dt;

namespace {

// One sampler call: the record every entry below fills by name, the loop runs and the graph replay keys.
struct SampleArgs {
  int rule = 0;
  BatchSplit b{};
  int H = 0, W = 0, n_steps = 0;
  const float *tb = nullptr;
  const float *coef = nullptr;            // host, [n_steps][4]
  const int32_t *has_noise = nullptr;     // host, [n_steps]
  const float *z = nullptr;
  const int32_t *z_row = nullptr;
  const int64_t *z_shift = nullptr;       // host, [n_steps] or null
  const float *w = nullptr;
  float w_scalar = 1.f;
  float *traj = nullptr;
  void *ws = nullptr;
  size_t ws_bytes = 0;
  hipStream_t s = nullptr;
  MaskArgs mk{};      // the masked entry only (dt_sample_trajectory_masked): known-region blend after every update

  // every field by value, the three host arrays by content: two calls with equal keys issue the same launches
  std::vector<unsigned char> key() const {
    static_assert(sizeof(SampleArgs) == 160, "a field was added or removed: serialise it below, then correct this size");
    std::vector<unsigned char> k;
    auto put = [&k](const void *p, size_t n) { const unsigned char *c = (const unsigned char *)p; k.insert(k.end(), c, c + n); };
    const int ints[9] = {rule, b.B, b.n_pass, b.B_single, b.tb_div, H, W, n_steps, z_shift ? 1 : 0};
    const void *ptrs[11] = {tb, z, z_row, w, traj, ws, (const void *)s, mk.mask, mk.mask_row, mk.known, mk.known_row};
    put(ints, sizeof(ints)); put(ptrs, sizeof(ptrs)); put(&w_scalar, sizeof(w_scalar)); put(&ws_bytes, sizeof(ws_bytes));
    put(coef, sizeof(float) * 4 * n_steps); put(has_noise, sizeof(int32_t) * n_steps);
    if (z_shift) put(z_shift, sizeof(int64_t) * n_steps);
    return k;
  }
};

// the loop over a batch the entry has checked (loop_status, dt_batch.h)
int sample_loop(const dt_unet *h, const SampleArgs &a) {
  const UnetGeom &g = h->geo;
  const int B = a.b.B, H = a.H, W = a.W;
  const int E = g.desc.channels * H * W;
  const size_t slot = (size_t)B * E;
  const int tb_rows = a.b.tb_rows();            // time-bias rows per step
  const Plan pl = make_plan(g, a.b.shape(H, W));
  if (pl.total * sizeof(float) > a.ws_bytes) return DT_E_WORKSPACE;
  if (use_fused(h, H, W)) {
    // small model: forward + CFG mix + update of up to kFusedMaxSteps timesteps per launch, images resident in LDS
    for (int i0 = 0; i0 < a.n_steps; i0 += kFusedMaxSteps) {
      const int n = a.n_steps - i0 < kFusedMaxSteps ? a.n_steps - i0 : kFusedMaxSteps;
      FusedArgs fa{};
      fused_common(h, fa, a.b, a.tb + (size_t)i0 * tb_rows * g.tb_stride);
      fa.mode = FUSED_LOOP; fa.rule = a.rule; fa.n_steps = n;
      fa.traj = a.traj + (size_t)i0 * slot; fa.z = a.z; fa.z_row = a.z_row; fa.wg = a.w; fa.w_scalar = a.w_scalar;
      fa.mk = a.mk;                                  // (travels with every launch of a loop longer than kFusedMaxSteps)
      for (int i = 0; i < n; ++i) {
        fa.coef[i][0] = a.coef[4 * (i0 + i)]; fa.coef[i][1] = a.coef[4 * (i0 + i) + 1]; fa.coef[i][2] = a.coef[4 * (i0 + i) + 2];
        fa.z_shift[i] = a.z_shift ? (long long)a.z_shift[i0 + i] : 0;
        if (a.has_noise[i0 + i]) fa.noise_mask |= 1ull << i;
        if (a.has_noise[i0 + i] && !a.z) return DT_E_NULL;
      }
      const int st = launch_unet_fused(fa, a.s);
      if (st) return st;
    }
    return DT_OK;
  }
  const float *lowres = (const float *)a.ws + pl.lowres;   // the low-resolution head output [Bt][H/2][W/2][4]
  for (int i = 0; i < a.n_steps; ++i) {
    const float *x = a.traj + (size_t)i * slot;
    float *xn = a.traj + (size_t)(i + 1) * slot;
    const bool dead = a.rule == DT_RULE_ENGINE && !a.has_noise[i];   // t == 0: the prediction is never used
    if (!dead) {      // the forward stops at the low-resolution head output; the update interpolates it (no eps tensor)
      int st = forward_impl(h, x, a.b, H, W, a.tb + (size_t)i * tb_rows * g.tb_stride, nullptr, (float *)a.ws, a.ws_bytes, a.s);
      if (st) return st;
    }
    // second-pass rows start at row B and belong to images B_single .. B-1: indexed by image through a pointer shifted back
    int st = launch_cfg_update_lowres(a.rule, x, lowres, a.b.n_pass == 2 ? lowres + (size_t)(B - a.b.B_single) * (H / 2) * (W / 2) * 4 : nullptr, a.z,
                                      a.z_row, a.z_shift ? (long long)a.z_shift[i] : 0, a.coef + 4 * i, a.has_noise[i], a.w, a.w_scalar, xn,
                                      B, g.desc.channels, H, W, a.b.B_single, a.s, a.mk);
    if (st) return st;
  }
  return DT_OK;
}

/* The loop is a fixed chain of (n_steps x ~45) launches whose arguments depend only on this call's arguments, so a
 * repeated call (same buffers, same schedule) can replay an instantiated hipGraph instead of re-issuing each launch.
 * Opt-in with DT_GRAPH=1: measured on MI355X / ROCm 7.2 the replay is time-neutral (batch 8: 31.5 vs 31.5 ms per
 * 100 forwards, batch 256: 94.9 vs 94.9 ms/step) -- the loop is bound by the GPU-side latency of its dependent
 * kernels (~6 us each at batch 8), not by host launch cost, which the host threads already hide.
 * Reached from dt_sample_trajectory only; the key (SampleArgs::key) nevertheless covers the whole record. */
int run_or_replay(const dt_unet *h, const SampleArgs &a) {
  const char *genv = getenv("DT_GRAPH");
  const bool use_graph = genv && atoi(genv) != 0;
  if (!use_graph || profiling_on() || a.n_steps < 4) return sample_loop(h, a);
  GraphCache &cache = h->graphs;
  std::vector<unsigned char> key = a.key();
  std::lock_guard<std::mutex> lock(cache.mu);
  if (const LoopGraph *g = cache.find(key)) return (int)hipGraphLaunch(g->exec, a.s);
  // ---- first call with these arguments: capture the loop, instantiate, keep
  hipError_t e = hipStreamBeginCapture(a.s, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {   // stream cannot be captured (e.g. the legacy default stream): plain launches
    (void)hipGetLastError();
    return sample_loop(h, a);
  }
  const int st = sample_loop(h, a);
  LoopGraph g;
  e = hipStreamEndCapture(a.s, &g.graph);
  if (e != hipSuccess) g.graph = nullptr;   // a failed capture leaves nothing to own
  if (st != DT_OK) return st;
  if (e != hipSuccess) return (int)e;
  e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
  if (e != hipSuccess) return (int)e;
  g.key = std::move(key);
  const LoopGraph &kept = cache.insert(std::move(g));
  if (getenv("DT_GRAPH_DEBUG")) fprintf(stderr, "[dt_hip] captured sampler loop: %d steps, batch %d -> graph #%zu\n", a.n_steps, a.b.B, cache.size());
  return (int)hipGraphLaunch(kept.exec, a.s);
}

}  // namespace

extern "C" {

// what every sampler entry is given, by name (the batch, w_scalar and the mask are the entry's own)
#define DT_LOOP_ARGS(a)                                                                                                  \
  SampleArgs a;                                                                                                          \
  a.rule = rule; a.H = H; a.W = W; a.n_steps = n_steps; a.tb = tb; a.coef = coef; a.has_noise = has_noise; a.z = z;     \
  a.z_row = z_row; a.z_shift = z_shift; a.w = w; a.traj = traj; a.ws = ws; a.ws_bytes = ws_bytes; a.s = (hipStream_t)stream

int dt_sample_trajectory(const dt_unet *h, int rule, int B, int n_pass, int H, int W, int n_steps, const float *tb,
                         const float *coef, const int32_t *has_noise, const float *z, const int32_t *z_row,
                         const int64_t *z_shift, const float *w, float w_scalar, float *traj, void *ws, size_t ws_bytes,
                         void *stream) {
  DT_LOOP_ARGS(a);
  a.b = BatchSplit{B, n_pass, 0, B};           // one time-bias row per pass
  a.w_scalar = w_scalar;
  if (const int bad = sample_status(h, rule, a.b, H, W, n_steps, tb, coef, has_noise, traj, ws)) return bad;
  return run_or_replay(h, a);
}

int dt_sample_trajectory_mixed(const dt_unet *h, int rule, int B, int B_single, int H, int W, int n_steps, const float *tb,
                               int tb_div, const float *coef, const int32_t *has_noise, const float *z, const int32_t *z_row,
                               const int64_t *z_shift, const float *w, float *traj, void *ws, size_t ws_bytes, void *stream) {
  DT_LOOP_ARGS(a);
  a.b = BatchSplit{B, 2, B_single, tb_div};     // (w_scalar stays 1: the guidance weights are per image)
  if (const int bad = sample_mixed_status(h, rule, a.b, H, W, n_steps, tb, coef, has_noise, w, traj, ws, h && h->geo.share_enc1)) return bad;
  return sample_loop(h, a);
}

// The masked loop of the editing stage (include/dt_hip_edit.h).  Always plain launches: it takes no part in the opt-in graph replay.
int dt_sample_trajectory_masked(const dt_unet *h, int rule, int B, int n_pass, int B_single, int H, int W, int n_steps,
                                const float *tb, int tb_div, const float *coef, const int32_t *has_noise, const float *z,
                                const int32_t *z_row, const int64_t *z_shift, const float *w, float w_scalar, const float *mask,
                                const int32_t *mask_row, const float *known, const int32_t *known_row, float *traj, void *ws,
                                size_t ws_bytes, void *stream) {
  DT_LOOP_ARGS(a);
  a.b = BatchSplit{B, n_pass, B_single, tb_div};
  a.w_scalar = w_scalar;
  a.mk = MaskArgs{mask, mask_row, known, known_row};
  if (const int bad = sample_masked_status(h, rule, a.b, H, W, n_steps, tb, coef, has_noise, w, mask, known, traj, ws, h && h->geo.share_enc1)) return bad;
  a.b = a.b.normalised();                      // every image takes one pass: a one-pass batch
  return sample_loop(h, a);
}
#undef DT_LOOP_ARGS

}  // extern "C"
