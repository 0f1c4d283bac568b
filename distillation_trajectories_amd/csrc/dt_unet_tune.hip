// The tuner of a U-Net handle and the plan hooks: timing of single convolution launches, the search over the admissible
// (tile, split, kind) of every slot of a forward shape, and reading / pinning a slot's choice.
#include <algorithm>
#include <cstring>

#include "dt_unet.h"

using namespace dt;

namespace {

// HIP-event timing of one convolution launch for the autotuner and dt_unet_time_conv (synchronises the stream)
struct ConvTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~ConvTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  int create() {
    DT_HIP_TRY(hipEventCreate(&e0));
    DT_HIP_TRY(hipEventCreate(&e1));
    return DT_OK;
  }
  // *ms: average milliseconds of `reps` back-to-back launches of q after one warm launch: in the sampler launches queue
  // behind each other, so a launch is not charged the idle-queue launch latency per kernel (which would bias against
  // split launches = two kernels).  Returns the status of the launches.
  int time(const ConvParams &q, bool strip_pair, int reps, hipStream_t s, float *ms) {
    *ms = 0.f;
    int st = launch_conv(q, s, strip_pair);
    if (st != DT_OK) return st;
    (void)hipEventRecord(e0, s);
    for (int rep = 0; rep < reps && st == DT_OK; ++rep) st = launch_conv(q, s, strip_pair);
    (void)hipEventRecord(e1, s);
    if (hipEventSynchronize(e1) != hipSuccess) st = (int)hipGetLastError();
    if (st != DT_OK) return st;
    (void)hipEventElapsedTime(ms, e0, e1);
    *ms /= reps;
    return DT_OK;
  }
};

// the caller's checks of a (block, slot) pair of the plan hooks
bool slot_exists(int block, int slot) { return block >= 0 && block < kBlocks && slot >= 0 && slot <= 2; }

// launches are timed on an otherwise idle GPU, where extra workgroups are free, whereas in the sampler other streams fill idle
// CUs: a split launch (slab traffic + one more launch) must be this much faster to be taken
constexpr float kSplitMargin = 1.05f;

// The choices the tuner times for one convolution, in the order it times them (the order decides ties).  Search policy (the
// search is paid once per model and shape, so it is pruned to what the per-layer tables show can win): exact-fp32 mode -> the
// fp32-MFMA kind only; otherwise the strip kinds for full 3x3 walks that some strip tile reaches and the plain split-bf16 kind
// for everything else.  Which candidates can run at all is conv_admissible's, asked of the bound launch.
// feeds_head: the layer is dec1.conv2 of a handle whose head fusion is on.
std::vector<ConvChoice> tune_candidates(const ConvLayer &L, int precision, bool feeds_head) {
  std::vector<ConvChoice> out;
  const bool strip_ok = L.taps == 9 && strip_reaches(L.W);
  for (const int kind : {KIND_FP32, KIND_BF16, KIND_STRIP, KIND_STRIP2, KIND_STRIPK}) {
    if (precision == DT_PREC_FP32 ? kind != KIND_FP32 : kind == KIND_FP32) continue;
    if (is_strip(kind) ? !strip_ok : (kind == KIND_BF16 && strip_ok)) continue;
    for (int bm = 64; bm <= 256; bm *= 2)
      for (int bn = 64; bn <= 128; bn += 64) {
        // dec1.conv2 with one N tile also evaluates the head (saves the head launch and dec1's output round trip)
        if (feeds_head && L.n_p <= 128 && bn != L.n_p) continue;
        // 3x3 walks split by taps 1/3/9; the strip kernel and single-tap layers by channel chunks 1/2/4/8
        const long long tiles = (long long)((L.M + bm - 1) / bm) * (L.n_p / bn);
        for (int sp = 1; sp <= (L.splittable ? 9 : 1); sp *= ((is_strip(kind) || L.taps != 9) ? 2 : 3))
          for (int fuse = 0; fuse <= ((L.foldable && sp == 1) ? 1 : 0); ++fuse) {
            if (sp > 1 && tiles * (sp / 2) >= 1024) continue;          // already >= 4 workgroups per CU without this split
            out.push_back(ConvChoice{bm, bn, sp, kind, fuse});
          }
      }
  }
  return out;
}

}  // namespace

extern "C" {

// Times every admissible (tile, tap split) of every conv launch of one forward shape with HIP events on
// `stream` (synchronises; call it outside hot loops and graph captures) and records the fastest.
// Activations in the workspace are whatever the last forward left there (run one first: all-zero or
// garbage operands would let the chip clock differently from real data).
int dt_unet_autotune(dt_unet *h, int batch_total, int H, int W, int images, int single, void *workspace, size_t ws_bytes,
                     void *stream) {
  if (!h || !workspace) return DT_E_NULL;
  TunedShape t{{batch_total, H, W, images, single}, {}};
  if (const int bad = t.shape.validate()) return bad;
  hipStream_t s = (hipStream_t)stream;
  const Plan pl = make_plan(h->geo, t.shape);
  if (pl.total * sizeof(float) > ws_bytes) return DT_E_WORKSPACE;
  float *ws = (float *)workspace;
  ConvTimer timer;
  if (const int bad = timer.create()) return bad;
  const ResolvedForward f = resolve_forward(h, t.shape, nullptr);   // candidates start from the defaults
  const float *tb = h->slab;   // any readable floats: only timing matters here
  int st = DT_OK;
  {   // The clocks of an idle GPU take tens of milliseconds of load to settle (the same launch measures 15 % slower
      // cold): run one mid-sized layer for a while first so that the first candidates are not timed against a ramp.
    const ConvParams wp = bind_conv(h, f, 1, 1, f.c[1][1], ws + pl.input(1), ws, pl, tb, batch_total);
    for (int rep = 0; rep < 200 && st == DT_OK; ++rep) st = launch_conv(wp, s, h->strip_pair);
    if (hipStreamSynchronize(s) != hipSuccess) st = (int)hipGetLastError();
  }
  // the timed average of one candidate; < 0: the launch cannot run here
  auto measure = [&](const ConvParams &q, int reps) -> float {
    float ms;
    const int lst = timer.time(q, h->strip_pair, reps, s, &ms);
    if (lst != DT_OK && lst != DT_E_SHAPE && lst != DT_E_ARG) st = lst;
    return lst == DT_OK ? ms : -1.f;
  };
  for (int j = 0; j < kBlocks && st == DT_OK; ++j) {
    const float *in = ws + pl.input(j);   // (enc1: conv1's output stands in for the image)
    float skip_ms = 0.f;
    for (int slot = 0; slot < 3 && st == DT_OK; ++slot) {
      if (!h->geo.has_launch(j, slot)) continue;
      ConvChoice best = f.c[j][slot];
      best.fuse = 0;               // candidates start from the UNFUSED launch (the default may have folded the skip in)
      const ConvLayer L = conv_layer(h, f, j, slot);
      float best_ms = 1e30f;
      struct Cand { ConvChoice c; ConvParams q; float cost; };
      std::vector<Cand> cands;
      // a fused conv2 also saves the separate skip launch measured for slot 0; a split must win by kSplitMargin
      auto cost_of = [&](float ms, const ConvChoice &c) {
        return (ms + (c.fuse ? 0.f : (L.foldable ? skip_ms : 0.f))) * (c.splits > 1 ? kSplitMargin : 1.0f);
      };
      const bool feeds_head = j == kBlocks - 1 && slot == 2 && h->head_fusion && h->geo.desc.channels <= 3;
      for (const ConvChoice &c : tune_candidates(L, h->precision, feeds_head)) {
        const ConvParams q = bind_conv(h, f, j, slot, c, in, ws, pl, tb, batch_total);
        if (conv_admissible(q) != DT_OK) continue;
        const float ms = measure(q, 3);
        if (ms < 0.f) continue;
        cands.push_back(Cand{c, q, cost_of(ms, c)});
      }
      // second look at the three cheapest: longer, interleaved runs (clock drift and timing noise otherwise flip
      // choices between near-equal candidates from run to run); ties within 1 % go to the later (larger-tile) candidate
      if (!cands.empty() && st == DT_OK) {
        std::vector<size_t> top;
        for (size_t i = 0; i < cands.size(); ++i) top.push_back(i);
        std::stable_sort(top.begin(), top.end(), [&](size_t a, size_t b) { return cands[a].cost < cands[b].cost; });
        if (top.size() > 3) top.resize(3);
        std::sort(top.begin(), top.end());
        std::vector<float> fin(top.size(), 1e30f);
        for (int round = 0; round < 2 && st == DT_OK; ++round)
          for (size_t k = 0; k < top.size() && st == DT_OK; ++k) {
            const float ms = measure(cands[top[k]].q, 10);
            if (ms >= 0.f && ms < fin[k]) fin[k] = ms;
          }
        for (size_t k = 0; k < top.size(); ++k) {
          const float cost = cost_of(fin[k], cands[top[k]].c);
          if (cost < best_ms * 1.01f) { best_ms = cost < best_ms ? cost : best_ms; best = cands[top[k]].c; }
        }
      }
      t.c[j][slot] = best;
      if (slot == 0) skip_ms = best_ms;
    }
  }
  if (st != DT_OK) return st;
  if (TunedShape *old = tuned_for(h, t.shape)) *old = t;
  else h->tuned.push_back(t);
  h->graphs.clear();
  return DT_OK;
}

/* tuning / profiling aid: average milliseconds (HIP events, synchronises) of ONE convolution launch of a
 * forward shape under an explicit (tile, split, arithmetic, fuse) choice, plus its algorithmic FLOPs */
int dt_unet_time_conv(const dt_unet *h, int batch_total, int H, int W, int images, int single, int block, int slot, int bm,
                      int bn, int splits, int prec, int fuse, int reps, void *workspace, size_t ws_bytes, void *stream,
                      float *ms, double *flops) {
  if (!h || !workspace || !ms || !flops) return DT_E_NULL;
  if (!slot_exists(block, slot) || reps < 1) return DT_E_ARG;
  TunedShape req{{batch_total, H, W, images, single}, {}};
  if (const int bad = req.shape.validate()) return bad;
  const Plan pl = make_plan(h->geo, req.shape);
  if (pl.total * sizeof(float) > ws_bytes) return DT_E_WORKSPACE;
  float *ws = (float *)workspace;
  if (!h->geo.has_launch(block, slot)) { *ms = 0.f; *flops = 0.0; return DT_OK; }
  // every slot asks for the choice: (block, slot) is bound with what follows from its own resolution only
  std::fill_n(&req.c[0][0], kBlocks * 3, ConvChoice{bm, bn, splits, prec, fuse});
  const ResolvedForward f = resolve_forward(h, req.shape, &req);
  const ConvParams p = bind_conv(h, f, block, slot, f.c[block][slot], ws + pl.input(block), ws, pl, h->slab, batch_total);
  *flops = 2.0 * p.M * (double)p.cout_real * ((double)p.cin_real * p.ksize * p.ksize + (p.in2 ? p.cin2_real : 0));
  ConvTimer timer;
  if (const int bad = timer.create()) return bad;
  return timer.time(p, h->strip_pair, reps, (hipStream_t)stream, ms);
}

/* test / report hook: the (bm, bn, splits) in use for block j, slot (0 skip, 1 conv1, 2 conv2) at a shape */
int dt_unet_conv_choice(const dt_unet *h, int batch_total, int H, int W, int images, int single, int block, int slot, int *bm,
                        int *bn, int *splits, int *prec, int *tuned) {
  if (!h || !bm || !bn || !splits || !prec || !tuned) return DT_E_NULL;
  if (!slot_exists(block, slot)) return DT_E_ARG;
  const FwdShape sh{batch_total, H, W, images, single};
  if (const int bad = sh.validate()) return bad;
  const TunedShape *t = find_tuned(h, sh);
  const ResolvedForward f = resolve_forward(h, sh, t);
  const ConvChoice &c = f.c[block][slot];   // (all zero where the slot has no launch of its own)
  *bm = c.bm; *bn = c.bn; *splits = c.splits; *prec = c.kind + (c.fuse ? 8 : 0); *tuned = t && h->geo.has_launch(block, slot);
  if (slot == 0 && f.c[block][2].fuse) *bm = *bn = *splits = 0;   // folded into conv2
  return DT_OK;
}

int dt_unet_set_conv_choice(dt_unet *h, int batch_total, int H, int W, int images, int single, int block, int slot, int bm,
                            int bn, int splits, int prec, int fuse) {
  if (!h) return DT_E_NULL;
  if (!slot_exists(block, slot)) return DT_E_ARG;
  const FwdShape sh{batch_total, H, W, images, single};
  if (const int bad = sh.validate()) return bad;
  const ConvChoice c{bm, bn, splits, prec, fuse};
  if (!conv_choice_valid(c, slot, h->geo.blk[block].n_p)) return DT_E_ARG;
  TunedShape *t = tuned_for(h, sh);
  if (!t) {   // start from what an untuned forward would launch
    TunedShape fresh{sh, {}};
    memcpy(fresh.c, resolve_forward(h, sh, nullptr).c, sizeof(fresh.c));
    h->tuned.push_back(fresh);
    t = &h->tuned.back();
  }
  t->c[block][slot] = c;
  h->graphs.clear();
  return DT_OK;
}

}  // extern "C"
