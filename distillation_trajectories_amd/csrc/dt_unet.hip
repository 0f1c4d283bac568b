// Host side of libdt_hip.so: the U-Net handle (packed weights), the forward launch plan, the
// device-resident reverse-diffusion loop and the extern "C" surface declared in include/dt_hip.h.
//
// Plan of one forward (reference models.py:159-224), NHWC activations with channels padded to 16:
//   x(NCHW) -> enc1.conv1 (direct fp32 conv, shared by the passes)
//   enc1 @H      -> pool -> enc2 @H/2 -> pool -> enc3 @H/4 -> pool -> enc4 @H/8 -> pool -> bottleneck @H/16
//   up+cat(enc4) -> dec3 @H/8 -> up+cat(enc3) -> dec2 @H/4 -> up+cat(enc2) -> dec1 @H/2 -> up + 1x1 head @H
// Each residual block is up to three implicit-GEMM launches (1x1 skip, conv1, conv2) whose epilogues
// carry BN/ReLU/time-bias/residual, so a forward is 8 blocks * (2..3) + 4 pools + 3 upcats + 2 = ~32 launches.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "dt_batch.h"
#include "dt_fused.h"
#include "../../include/dt_hip_edit.h"
#include "dt_internal.h"

using namespace dt;

// ------------------------------------------------------------------------------ profiler
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
    "unet_fused_kernel", "pair_metrics_kernel"};
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
}  // namespace dt

// One convolution of a block, under its slot: 0 = the 1x1 skip, 1 = conv1 (both over the block input), 2 = conv2 (over
// conv1's output) -- the key of ResolvedForward::c, has_launch, conv_layer and every plan hook.
struct ConvW {
  int cin, cin_p;         // real / padded input channels
  int split_c, split_cp;  // concat split of the input channels (== cin, cin_p when no concat)
  int cin_w;              // input channels per tap of the split-bf16 pack: cin_p padded to kChunkPad chunks
  int ksize;              // 1 or 3
  float *w, *wb;          // packed weights: fp32 tiles (dt_conv.hip), three bf16 planes (dt_conv_bf16.hip); nullptr: no such launch
  float *scale, *shift;   // folded BN (a plain conv: 1 and its bias); nullptr: no such conv
};
constexpr int kSlotWeight[3] = {DT_BT_RES_W, DT_BT_CONV1_W, DT_BT_CONV2_W};   // a slot's OIHW weights among a block's tensors

struct BlockW {
  int cin, cout;          // real channels
  int cin_p, cout_p, n_p; // padded
  int split_c, split_cp;  // concat split of the block input
  bool has_res;
  ConvW c[3];             // enc1: c[1].w is the direct first-layer kernel's pack, c[0] is empty (w3 instead)
  float *w3;              // enc1 only: skip weights for the in-epilogue 1x1 (n_p x 4)
  int tb_off;             // channel offset of this block in a time-bias row
};

// (tile, split) choice of the three conv slots (0 = 1x1 skip, 1 = conv1, 2 = conv2) of every block for
// one forward shape, filled in by dt_unet_autotune; absent shapes use heuristic_choice
struct TunedShape {
  FwdShape shape;
  ConvChoice c[kBlocks][3];
};

// an instantiated hipGraph of one dt_sample_trajectory call (every launch of the loop), keyed by all its arguments
struct LoopGraph {
  std::vector<unsigned char> key;
  hipGraphExec_t exec;
  hipGraph_t graph;
};

struct dt_unet {
  std::vector<TunedShape> tuned;
  // replay cache of the sampler loop (not part of the handle's logical state, hence mutable + its own lock: the
  // sampler may be entered from several host threads); dropped whenever the launch plan changes
  mutable std::vector<LoopGraph> graphs;
  mutable std::mutex graph_mu;
  int precision;          // DT_PREC_*: which convolution arithmetic the heuristic / autotuner may use
  bool head_fusion = true;   // dec1.conv2's epilogue evaluates the final 1x1 head (dt_unet_set_head_fusion)
  // enc1 runs ONCE per step for all CFG passes (they share x): conv1 without the time bias over the B images, conv2 over the
  // B images with the passes' time biases entering as class-bias rows in its epilogue (tap_bias_kernel); DT_NO_SHARED_ENC1=1
  // at create time keeps the per-pass formulation (A/B runs, and the form the reference's operation order follows literally)
  bool share_enc1 = true;
  int tb_cols = 0;           // projected channels of a time-bias row; the class-bias columns follow
  dt_unet_desc desc;
  BlockW blk[kBlocks];
  int cp[4];              // padded dims
  int tb_stride;
  float *slab;            // one device allocation holding everything below
  size_t slab_floats;
  TembWeights tw;
  const float *final_w, *final_b;   // borrowed? no: copied into the slab
  // Small models (padded dims <= 32 / 64) at 16 x 16: the whole forward -- and the whole sampler loop -- is ONE launch of
  // unet_fused_kernel (dt_fused.hip) with every activation in LDS.  fused_ok: the packs below exist; fused_on: the switch
  // (dt_unet_set_fused; DT_NO_FUSED=1 at create time starts with it off).
  bool fused_ok = false, fused_on = false;
  int fused_G = 2;
  float *fused_slab = nullptr;      // packed fp32 weights of the fused kernel + its layer table
  FusedOp *fused_ops_dev = nullptr;
  int fused_n_ops = 0;
  FusedLds fused_lds{};
  int fused_par = 0, fused_n_par = 0;   // the parameter block inside the fused slab
};

namespace {

struct Bump {
  size_t off = 0;
  size_t take(size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; }   // 256-B aligned
};

bool use_fused(const dt_unet *u, int H, int W);
void fused_common(const dt_unet *u, FusedArgs &a, const BatchSplit &b, const float *tb);

// activation buffers of one forward, as float offsets into the workspace
struct Plan {
  size_t h[kBlocks], r[kBlocks], o[kBlocks];   // conv1 out, skip out, block out
  size_t pool[4], cat[3];
  size_t slab, lowres;                         // split-K partial sums; low-resolution head output
  size_t total;
  int H[kBlocks], W[kBlocks];                  // spatial size of each block
};

// level (power-of-two divisor of the image size) of the 8 blocks
const int kDiv[kBlocks] = {1, 2, 4, 8, 16, 8, 4, 2};

Plan make_plan(const dt_unet *u, const FwdShape &sh) {
  const int Bt = sh.Bt, H = sh.H, W = sh.W;
  Plan p{};
  Bump b;
  size_t slab = 0;
  for (int j = 0; j < kBlocks; ++j) {
    const int h = H / kDiv[j], w = W / kDiv[j];
    p.H[j] = h; p.W[j] = w;
    const size_t px = (size_t)Bt * h * w;
    if (j >= 1 && j <= 4) p.pool[j - 1] = b.take(px * u->blk[j].cin_p);
    if (j >= 5) p.cat[j - 5] = b.take(px * u->blk[j].cin_p);
    p.h[j] = b.take(px * u->blk[j].cout_p);
    p.r[j] = (u->blk[j].has_res && j > 0) ? b.take(px * u->blk[j].cout_p) : 0;
    p.o[j] = b.take(px * u->blk[j].cout_p);
    if (j > 0 && px <= (size_t)kSplitMaxRows) {
      const size_t need = (size_t)9 * px * u->blk[j].cout_p;    // room for the deepest split
      if (need > slab) slab = need;
    }
  }
  p.slab = b.take(slab);
  p.lowres = b.take((size_t)Bt * (H / 2) * (W / 2) * 4);
  p.total = b.off;
  return p;
}

void drop_graphs(dt_unet *u) {
  std::lock_guard<std::mutex> lock(u->graph_mu);
  for (LoopGraph &g : u->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
  u->graphs.clear();
}

const TunedShape *find_tuned(const dt_unet *u, const FwdShape &sh) {
  for (const TunedShape &t : u->tuned)
    if (t.shape == sh) return &t;
  return nullptr;
}

// The launches of one forward shape, resolved once and free of pointers: the choice of every convolution slot (0 = 1x1 skip,
// 1 = conv1, 2 = conv2) of every block and the per-block facts that follow from them.  bind_conv() binds one slot to buffers.
struct ResolvedForward {
  FwdShape shape;
  bool shared_enc1;                 // enc1 runs once over the images for all passes (its conv2 writes every pass)
  ConvChoice c[kBlocks][3];         // c[j][2].fuse: conv2 folds the block's 1x1 skip in (slot 0 does not launch)
  bool pool_fused[kBlocks];         // enc1..enc4: conv2's epilogue writes the 2x2 max pool
  bool concat_in_place[kBlocks];    // dec3..dec1: conv1 and the folded skip read the concat's skip half from the encoder
  bool head_fused;                  // dec1.conv2's epilogue evaluates the final 1x1 head
};

// whether slot `slot` of block j is a convolution of its own: enc1.conv1 is the direct first-layer kernel and enc1's skip is
// recomputed in conv2's epilogue; identity skips have none
bool has_launch(const dt_unet *u, int j, int slot) { return slot == 2 || (j > 0 && (slot == 1 || u->blk[j].has_res)); }

ConvLayer conv_layer(const dt_unet *u, const ResolvedForward &f, int j, int slot) {
  const BlockW &k = u->blk[j];
  const int h = f.shape.H / kDiv[j], w = f.shape.W / kDiv[j];
  const int M = (j == 0 && f.shared_enc1 ? f.shape.imgs : f.shape.Bt) * h * w;
  const int taps = slot == 0 || (h == 1 && w == 1) ? 1 : 9;   // a 1x1 image only ever sees the centre tap of a padded 3x3 kernel
  return ConvLayer{M, w, k.n_p, k.c[slot].cin_p, taps, j > 0 && M <= kSplitMaxRows, slot == 2 && j > 0 && k.has_res};
}

ResolvedForward resolve_forward(const dt_unet *u, const FwdShape &sh, const TunedShape *tuned) {
  ResolvedForward f{};
  f.shape = sh;
  f.shared_enc1 = u->share_enc1 && (sh.Bt + sh.single) % sh.imgs == 0;
  for (int j = 0; j < kBlocks; ++j)
    for (int slot = 0; slot < 3; ++slot)
      if (has_launch(u, j, slot)) f.c[j][slot] = resolve_conv_choice(conv_layer(u, f, j, slot), tuned ? &tuned->c[j][slot] : nullptr, u->precision);
  for (int j = 0; j < kBlocks; ++j) {
    const ConvChoice &c2 = f.c[j][2];
    const int h = sh.H / kDiv[j], w = sh.W / kDiv[j];
    // encoder blocks enc1..enc4 feed a 2x2 max pool: folded into conv2's staged epilogue where a 32-row tile holds whole row
    // pairs (W a power of two <= 16); split launches pool in their slab-summing epilogue kernel instead
    f.pool_fused[j] = j <= 3 && h % 2 == 0 && w % 2 == 0 && (c2.splits > 1 || (w <= 16 && (w & (w - 1)) == 0));
    // a decoder block reads the concat [upsampled | skip]: when both of its readers are strip launches (conv1, and the 1x1 skip
    // folded into conv2) they fetch the skip half straight from the encoder's output and the concat holds the upsampled half only
    f.concat_in_place[j] = j >= 5 && u->blk[j].has_res && is_strip(f.c[j][1].kind) && is_strip(c2.kind) && c2.fuse;
  }
  // dec1.conv2 also evaluates the final 1x1 head when its workgroups hold whole rows (one N tile, no split): the head is dec1's
  // only consumer, so dec1's own output is then never written
  const ConvChoice &last = f.c[kBlocks - 1][2];
  f.head_fused = u->head_fusion && last.splits == 1 && u->blk[kBlocks - 1].n_p == last.bn && u->desc.channels <= 3;
  return f;
}

// Parameters of slot `slot` of block j under choice c (the resolved one, or an autotuning candidate), bound to the workspace;
// `in` is the block input (enc1: the NCHW image).  The pool / head epilogues follow f's choice of the slot.
ConvParams bind_conv(const dt_unet *u, const ResolvedForward &f, int j, int slot, const ConvChoice &c, const float *in, float *ws,
                     const Plan &pl, const float *tb, int tb_div) {
  const BlockW &k = u->blk[j];
  const ConvW &cw = k.c[slot];
  const ConvLayer L = conv_layer(u, f, j, slot);
  const int h = pl.H[j], w = pl.W[j];
  ConvParams p{};
  p.M = L.M; p.H = h; p.W = w;
  p.cin_p = L.cin_p; p.cout_p = k.cout_p; p.n_p = k.n_p;
  p.cin_real = cw.cin; p.cout_real = k.cout;
  p.tb_stride = u->tb_stride; p.m_per_tb = h * w * tb_div;
  p.slab = ws + pl.slab;
  p.in = slot == 2 ? ws + pl.h[j] : in;
  p.ksize = cw.ksize;
  p.scale = cw.scale; p.shift = cw.shift;
  p.tap_lo = slot > 0 && L.taps == 1 ? 4 : 0; p.tap_hi = p.tap_lo + L.taps;
  p.relu = slot > 0;
  if (slot == 0) {
    p.out = ws + pl.r[j];
  } else if (slot == 1) {
    p.tb = tb + k.tb_off; p.out = ws + pl.h[j];
  } else {
    p.out = ws + pl.o[j];
    if (f.pool_fused[j]) p.pool_out = ws + pl.pool[j];
    if (j == 0) {
      // the C-channel skip of enc1 is recomputed in the epilogue from the patches' centre taps (k = 9c+4)
      p.x3 = in; p.w3 = k.w3; p.x3_hw = h * w; p.x3_imgs = f.shape.imgs; p.x3_c = u->desc.channels;
      if (f.shared_enc1) {   // one launch over the images for all their passes
        p.n_dup = (f.shape.Bt + f.shape.single) / f.shape.imgs; p.dup_rows = p.M; p.dup_skip = f.shape.single * h * w; p.tbc = tb + u->tb_cols;
        p.skip_out = u->head_fusion && p.pool_out ? 1 : 0;   // only the pool reads enc1's output (else a pooling launch does)
      }
    } else {
      p.add = k.has_res ? ws + pl.r[j] : in;   // identity skip: cin_p == cout_p
    }
    if (j == kBlocks - 1 && f.head_fused) {
      p.head_w = u->final_w; p.head_b = u->final_b; p.head_out = ws + pl.lowres;
      p.head_c = u->desc.channels; p.head_cin = u->desc.dims[0];
    }
  }
  // the choice: tile, kind, the weight pack of the kind (and its chunk width), the folded skip walk where c folds it
  const bool fp32 = c.kind == KIND_FP32;
  p.bm = c.bm; p.bn = c.bn; p.splits = c.splits; p.kind = c.kind;
  p.w = fp32 ? cw.w : cw.wb;
  p.ccw = (fp32 ? cw.cin_p : cw.cin_w) >> 4;
  if (c.fuse) {   // conv2 with the block's 1x1 skip (slot 0) folded into its K walk (the slot-0 launch is then skipped)
    const ConvW &sk = k.c[0];
    p.add = nullptr;
    p.in2 = in; p.w2 = fp32 ? sk.w : sk.wb; p.bias2 = sk.shift; p.cin2_p = sk.cin_p; p.cin2_real = sk.cin;
    p.ccw2 = (fp32 ? sk.cin_p : sk.cin_w) >> 4;
  }
  return p;
}

int run_block(const dt_unet *u, const ResolvedForward &f, int j, const float *in, float *ws, const Plan &pl, const float *tb,
              int tb_div, hipStream_t s) {
  if (j == 0) {
    const BlockW &k = u->blk[0];
    if (!f.shared_enc1 && f.shape.single) return DT_E_ARG;   // mixed batches exist in the shared-enc1 formulation only
    // (shared: the passes' time biases enter in conv2's epilogue)
    const int st = launch_first_conv(in, k.c[1].w, k.c[1].scale, k.c[1].shift, f.shared_enc1 ? nullptr : tb + k.tb_off, u->tb_stride, tb_div, ws + pl.h[0],
                                     f.shape.imgs, f.shared_enc1 ? 1 : f.shape.Bt / f.shape.imgs, u->desc.channels, pl.H[0], pl.W[0], k.cout, k.cout_p, s);
    if (st) return st;
  }
  for (int slot = 0; slot < 3; ++slot) {
    if (!has_launch(u, j, slot) || (slot == 0 && f.c[j][2].fuse)) continue;
    ConvParams p = bind_conv(u, f, j, slot, f.c[j][slot], in, ws, pl, tb, tb_div);
    if (f.concat_in_place[j]) {
      const int skip = 8 - j;            // dec3<-enc4(3), dec2<-enc3(2), dec1<-enc2(1)
      p.cc_a = u->blk[j].split_cp >> 4;
      p.b_stride = u->blk[skip].cout_p;
      if (slot == 1) p.in_b = ws + pl.o[skip];
      if (slot == 2) p.in2_b = ws + pl.o[skip];
    }
    const int st = launch_conv(p, s);
    if (st) return st;
  }
  return DT_OK;
}

// One forward of the batch b (dt_batch.h), which the caller has checked: forward_status, forward_mixed_status or loop_status.
// eps == nullptr: the forward stops at the low-resolution head output.
int forward_impl(const dt_unet *u, const float *x, const BatchSplit &b, int H, int W, const float *tb, float *eps, float *ws,
                 size_t ws_bytes, hipStream_t s) {
  const FwdShape sh = b.shape(H, W);
  const int Bt = sh.Bt, tb_div = b.tb_div;
  const Plan pl = make_plan(u, sh);
  if (pl.total * sizeof(float) > ws_bytes) return DT_E_WORKSPACE;
  if (use_fused(u, H, W) && eps) {           // small model: the whole forward is one launch (dt_fused.hip)
    if (Bt % tb_div) return DT_E_ARG;
    FusedArgs a{};
    fused_common(u, a, b, tb);
    a.mode = FUSED_FORWARD; a.x = x; a.eps = eps;
    return launch_unet_fused(a, s);
  }
  const ResolvedForward f = resolve_forward(u, sh, find_tuned(u, sh));
  int st = DT_OK;
  const float *cur = x;                     // enc1 reads the NCHW image itself (first-layer kernel, skip in conv2's epilogue)
  for (int j = 0; j < kBlocks; ++j) {
    if (j >= 1 && j <= 4) {        // encoder: pool the previous block's output (unless its conv2 already did)
      if (!f.pool_fused[j - 1])
      st = launch_maxpool(ws + pl.o[j - 1], ws + pl.pool[j - 1], Bt,
                          pl.H[j - 1], pl.W[j - 1], u->blk[j - 1].cout_p, s);
      if (st) return st;
      cur = ws + pl.pool[j - 1];
    } else if (j >= 5) {           // decoder: upsample previous output, concat the matching encoder output
      const int skip = 8 - j;      // dec3<-enc4(3), dec2<-enc3(2), dec1<-enc2(1)
      st = launch_upcat(ws + pl.o[j - 1], f.concat_in_place[j] ? nullptr : ws + pl.o[skip], ws + pl.cat[j - 5],
                        Bt, pl.H[j - 1], pl.W[j - 1], u->blk[j - 1].cout_p, u->blk[skip].cout_p, s);
      if (st) return st;
      cur = ws + pl.cat[j - 5];
    }
    st = run_block(u, f, j, cur, ws, pl, tb, tb_div, s);
    if (st) return st;
  }
  if (!f.head_fused) {   // head at the low resolution (unless dec1.conv2's epilogue already produced it), then the 3-channel upsample
    st = launch_head(ws + pl.o[7], u->final_w, u->final_b, ws + pl.lowres, Bt, pl.H[7], pl.W[7], u->blk[7].cout_p,
                     u->desc.channels, u->desc.dims[0], s);
    if (st) return st;
  }
  if (!eps) return DT_OK;                  // the sampler's fused update interpolates the low-resolution output itself
  return launch_head_upsample(ws + pl.lowres, eps, Bt, pl.H[7], pl.W[7], u->desc.channels, s);
}


// ---- the fused small-model path (dt_fused.hip): packs + layer table at create time, one launch per forward / sampler call
int build_fused(dt_unet *u, const float *const *bt, hipStream_t s) {
  const int C = u->desc.channels, c0p = u->cp[0], c1p = u->cp[1];
  if (u->cp[2] != c1p || u->cp[3] != c1p || u->desc.dims[2] != u->desc.dims[1] || u->desc.dims[3] != u->desc.dims[1]) return DT_OK;
  if (!fused_eligible(C, c0p, c1p)) return DT_OK;
  const int G = u->fused_G;
  if (fused_lds_bytes(G, c0p, c1p) > 160 * 1024) return DT_OK;
  // one slab: the parameter block (per block the folded BN vectors of conv1 / conv2 and the skip conv's bias, cout_p floats each,
  // then enc1's image-skip rows: the kernel copies this block into LDS), the packed weights of conv1 (blocks 1..7), conv2
  // (all) and the 1x1 skip convs (enc1's image skip aside), enc1.conv1 as two K chunks, and the layer table
  Bump bump;
  const int tb_cols = 2 * c0p + 6 * c1p;
  const size_t o_par = bump.take((size_t)5 * tb_cols + 4 * c0p);
  size_t o_w[kBlocks][3] = {};
  for (int j = 0; j < kBlocks; ++j)
    for (int slot = 0; slot < 3; ++slot) {
      const ConvW &c = u->blk[j].c[slot];
      if (has_launch(u, j, slot)) o_w[j][slot] = bump.take((size_t)c.ksize * c.ksize * c.cin_p * u->blk[j].cout_p);
    }
  const size_t o_wf = bump.take((size_t)2 * (c0p / 16) * 256);
  const size_t o_ops = bump.take((sizeof(FusedOp) * kFusedMaxOps + 3) / 4);
  if (bump.off >= (1u << 30)) return DT_OK;                     // offsets are ints
  hipError_t e = hipMalloc((void **)&u->fused_slab, bump.off * sizeof(float));
  if (e != hipSuccess) return (int)e;
  float *F = u->fused_slab;
  FusedModel m{};
  m.c0p = c0p; m.c1p = c1p; m.wf = (int)o_wf; m.w3 = 5 * tb_cols;
  int st = DT_OK;
  auto d2d = [&](size_t off, const float *src, size_t n) {
    if (st == DT_OK) {
      const hipError_t ee = hipMemcpyAsync(F + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, s);
      if (ee != hipSuccess) st = (int)ee;
    }
  };
  st = launch_pack_fused_first(bt[DT_BT_CONV1_W], F + o_wf, u->blk[0].cout, C, c0p / 16, s);
  d2d(o_par + 5 * tb_cols, u->blk[0].w3, (size_t)4 * c0p);
  int pj = 0;                                                   // the block's offset inside the parameter block
  for (int j = 0; j < kBlocks && st == DT_OK; ++j) {
    const BlockW &k = u->blk[j];
    const float *const *t = bt + j * DT_BT_COUNT;
    FusedBlockW &f = m.blk[j];
    const int cp = k.cout_p;
    f.tb_off = k.tb_off;
    // the block's five vectors in the parameter block: conv1's scale and shift, conv2's, the skip conv's bias
    FusedConvW *const fc[3] = {&f.cr, &f.c1, &f.c2};
    const int at_scale[3] = {-1, 0, 2}, at_shift[3] = {4, 1, 3};
    for (int slot = 0; slot < 3 && st == DT_OK; ++slot) {
      const ConvW &c = k.c[slot];
      const int scale = slot ? pj + at_scale[slot] * cp : 0, shift = pj + at_shift[slot] * cp;
      if (slot && c.scale) d2d(o_par + scale, c.scale, cp);
      if (c.shift) d2d(o_par + shift, c.shift, cp);
      *fc[slot] = FusedConvW{(int)o_w[j][slot], scale, shift};
      if (st == DT_OK && has_launch(u, j, slot))
        st = launch_pack_fused_conv(t[kSlotWeight[slot]], F + o_w[j][slot], k.cout, c.cin, c.ksize * c.ksize, c.cin_p / 16, k.cout_p / 16,
                                    c.split_c, c.split_cp, s);
    }
    pj += 5 * cp;
  }
  if (st == DT_OK && hipMemsetAsync(F + o_par + 4 * c0p, 0, sizeof(float) * c0p, s) != hipSuccess) st = (int)hipGetLastError();   // (enc1 has no skip-conv bias)
  u->fused_par = (int)o_par; u->fused_n_par = 5 * tb_cols + 4 * c0p;
  if (st != DT_OK) return st;
  FusedOp ops[kFusedMaxOps];
  u->fused_n_ops = fused_ops(m, G, ops);
  u->fused_ops_dev = reinterpret_cast<FusedOp *>(F + o_ops);
  // (a synchronous copy: `ops` lives on this stack frame)
  e = hipMemcpy(u->fused_ops_dev, ops, sizeof(FusedOp) * u->fused_n_ops, hipMemcpyHostToDevice);
  if (e != hipSuccess) return (int)e;
  u->fused_lds = fused_lds(G, c0p, c1p);
  u->fused_ok = true;
  u->fused_on = getenv("DT_NO_FUSED") == nullptr;
  return DT_OK;
}

// (head fusion off = the test hook that materialises every block output in the workspace: only the layered path has those)
bool use_fused(const dt_unet *u, int H, int W) { return u->fused_ok && u->fused_on && u->head_fusion && H == 16 && W == 16; }

void fused_common(const dt_unet *u, FusedArgs &a, const BatchSplit &b, const float *tb) {
  a.ops = u->fused_ops_dev; a.n_ops = u->fused_n_ops; a.fbase = u->fused_slab; a.par = u->fused_par; a.n_par = u->fused_n_par;
  a.head_w = u->final_w; a.head_b = u->final_b;
  a.tb = tb; a.tb_stride = u->tb_stride; a.tb_div = b.tb_div;
  a.lds = u->fused_lds; a.G = u->fused_G;
  a.C = u->desc.channels; a.c0 = u->desc.dims[0]; a.c0p = u->cp[0];
  a.B = b.B; a.n_pass = b.n_pass; a.B_single = b.B_single;
  a.tb_rows = b.tb_rows();
  a.flops_per_row = fused_flops_per_row(a.C, u->desc.dims[0], u->desc.dims[1]);
}

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
  int time(const ConvParams &q, int reps, hipStream_t s, float *ms) {
    *ms = 0.f;
    int st = launch_conv(q, s);
    if (st != DT_OK) return st;
    (void)hipEventRecord(e0, s);
    for (int rep = 0; rep < reps && st == DT_OK; ++rep) st = launch_conv(q, s);
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
}  // namespace

extern "C" {

int dt_abi_version(void) { return DT_ABI_VERSION; }

const char *dt_status_string(int st) {
  switch (st) {
    case DT_OK: return "ok";
    case DT_E_NULL: return "required pointer is NULL";
    case DT_E_SHAPE: return "unsupported or inconsistent shape";
    case DT_E_ARG: return "bad enum or count";
    case DT_E_WORKSPACE: return "workspace too small";
    default: return st > 0 ? hipGetErrorString((hipError_t)st) : "unknown dt status";
  }
}

int dt_unet_create(const dt_unet_desc *desc, const float *const *bt, const float *const *gt, void *stream,
                   dt_unet **out) {
  if (!desc || !bt || !gt || !out) return DT_E_NULL;
  if (desc->channels < 1 || desc->channels > 3 || desc->temb_dim < 2) return DT_E_SHAPE;
  for (int i = 0; i < 4; ++i)
    if (desc->dims[i] < 1) return DT_E_SHAPE;
  for (int i = 0; i < DT_GT_COUNT; ++i)
    if (!gt[i]) return DT_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  dt_unet *u = new (std::nothrow) dt_unet();
  if (!u) return (int)hipErrorOutOfMemory;
  u->desc = *desc;
  u->precision = DT_PREC_AUTO;
  const int C = desc->channels, D = desc->temb_dim;
  const int *d = desc->dims;
  for (int i = 0; i < 4; ++i) u->cp[i] = round_up(d[i], kChanPad);
  // (cin, cout) and the concat split of the eight blocks -- models.py:138-154
  const int cin[kBlocks] = {C, d[0], d[1], d[2], d[3], d[3] + d[3], d[2] + d[2], d[1] + d[1]};
  const int cout[kBlocks] = {d[0], d[1], d[2], d[3], d[3], d[2], d[1], d[0]};
  const int up_c[kBlocks] = {0, 0, 0, 0, 0, d[3], d[2], d[1]};   // channels coming from the upsampled branch
  Bump bump;
  struct { size_t w, wb, ss; } o_c[kBlocks][3] = {};   // a slot's fp32 pack, bf16x3 pack, scale + shift
  size_t o_w3 = 0;
  int tb = 0;
  for (int j = 0; j < kBlocks; ++j) {
    BlockW &k = u->blk[j];
    k.cin = cin[j]; k.cout = cout[j];
    k.cout_p = round_up(cout[j], kChanPad);
    k.n_p = round_up(cout[j], kNPad);
    if (j >= 5) {
      k.split_c = up_c[j]; k.split_cp = round_up(up_c[j], kChanPad);
      k.cin_p = k.split_cp + round_up(cin[j] - up_c[j], kChanPad);
    } else {
      k.cin_p = round_up(cin[j], kChanPad);                    // (enc1.conv1 is the direct first-layer kernel)
      k.split_c = cin[j]; k.split_cp = k.cin_p;
    }
    k.has_res = cin[j] != cout[j];
    for (int t = 0; t < DT_BT_COUNT; ++t) {
      const bool optional = t == DT_BT_RES_W || t == DT_BT_RES_B;
      if (!bt[j * DT_BT_COUNT + t] && (!optional || k.has_res)) { delete u; return DT_E_NULL; }
    }
    for (int slot = 0; slot < 3; ++slot) {
      ConvW &c = k.c[slot];
      c = slot == 2 ? ConvW{k.cout, k.cout_p, k.cout, k.cout_p} : ConvW{k.cin, k.cin_p, k.split_c, k.split_cp};
      c.cin_w = pack_chunks(c.cin_p) * 16;
      c.ksize = slot == 0 ? 1 : 3;
      const size_t taps = (size_t)c.ksize * c.ksize;
      if (has_launch(u, j, slot)) {   // a tile-GEMM / strip launch of its own: both packs (bf16x3: 6 bytes per weight = 1.5 floats)
        o_c[j][slot].w = bump.take(taps * c.cin_p * k.n_p);
        o_c[j][slot].wb = bump.take(taps * c.cin_w * k.n_p * 3 / 2);
      }
      if (has_launch(u, j, slot) || slot == 1) o_c[j][slot].ss = bump.take((size_t)2 * k.n_p);
    }
    if (j == 0) {   // enc1: conv1 is the direct first-layer kernel over wf[9C][cout_p]; the skip is w3[n_p][4] in conv2's epilogue
      o_c[0][1].w = bump.take((size_t)9 * C * k.cout_p);
      if (k.has_res) o_w3 = bump.take((size_t)4 * k.n_p);
    }
    k.tb_off = tb;
    tb += k.cout_p;
  }
  u->share_enc1 = getenv("DT_NO_SHARED_ENC1") == nullptr;
  const int c0p = u->blk[0].cout_p;
  u->tb_cols = tb;
  u->tb_stride = tb + (u->share_enc1 ? 9 * c0p : 0);          // [projected channels | nine class-bias vectors of enc1.conv2]
  const size_t o_w2t = u->share_enc1 ? bump.take((size_t)9 * c0p * c0p) : 0;
  const int half = (D / 2 > 1 ? D / 2 : 1);
  const size_t o_wt = bump.take((size_t)tb * D), o_bt = bump.take(tb);
  const size_t o_w1g = bump.take((size_t)D * D), o_b1g = bump.take(D), o_wc0 = bump.take(D), o_bc0 = bump.take(D);
  const size_t o_wc2 = bump.take((size_t)D * D), o_bc2 = bump.take(D), o_fr = bump.take(half);
  const size_t o_fw = bump.take((size_t)C * d[0]), o_fb = bump.take(C);
  u->slab_floats = bump.off;
  hipError_t e = hipMalloc((void **)&u->slab, u->slab_floats * sizeof(float));
  if (e != hipSuccess) { delete u; return (int)e; }
  float *S = u->slab;
  int st = DT_OK;
  auto copy = [&](size_t off, const float *src, size_t n) {
    if (st == DT_OK) {
      hipError_t ee = hipMemcpyAsync(S + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, s);
      if (ee != hipSuccess) st = (int)ee;
    }
  };
  for (int j = 0; j < kBlocks && st == DT_OK; ++j) {
    BlockW &k = u->blk[j];
    const float *const *t = bt + j * DT_BT_COUNT;
    // a slot's conv bias and eval-BatchNorm tensors (the skip is a plain conv)
    const float *const bn[3][5] = {{t[DT_BT_RES_B], nullptr, nullptr, nullptr, nullptr},
                                   {t[DT_BT_CONV1_B], t[DT_BT_BN1_G], t[DT_BT_BN1_B], t[DT_BT_BN1_MEAN], t[DT_BT_BN1_VAR]},
                                   {t[DT_BT_CONV2_B], t[DT_BT_BN2_G], t[DT_BT_BN2_B], t[DT_BT_BN2_MEAN], t[DT_BT_BN2_VAR]}};
    for (int slot = 0; slot < 3 && st == DT_OK; ++slot) {
      ConvW &c = k.c[slot];
      const bool conv = has_launch(u, j, slot);
      if (conv || (j == 0 && slot == 1)) {
        c.w = S + o_c[j][slot].w;
        c.scale = S + o_c[j][slot].ss; c.shift = c.scale + k.n_p;
        st = launch_fold_bn(bn[slot][0], bn[slot][1], bn[slot][2], bn[slot][3], bn[slot][4], c.scale, c.shift, k.cout, k.n_p, s);
      }
      if (!conv) continue;
      c.wb = S + o_c[j][slot].wb;
      if (!st) st = launch_pack_conv(t[kSlotWeight[slot]], c.w, k.cout, c.cin, c.ksize, c.cin_p, k.n_p, c.split_c, c.split_cp, s);
      if (!st) st = launch_pack_conv_bf16x3(t[kSlotWeight[slot]], c.wb, k.cout, c.cin, c.ksize, c.cin_p, c.cin_w, k.n_p, c.split_c, c.split_cp, s);
    }
    if (j == 0) {   // enc1's exceptions: conv1's own pack; the image skip's weights; conv2 tap-major for the class-bias columns
      k.w3 = S + o_w3;
      if (!st) st = launch_pack_first_conv(t[DT_BT_CONV1_W], k.c[1].w, k.cout, C, k.cout_p, s);
      if (!st) st = launch_pack_res3(t[DT_BT_RES_W], t[DT_BT_RES_B], k.w3, k.cout, C, k.n_p, s);
      if (!st && u->share_enc1) st = launch_pack_tap_major(t[DT_BT_CONV2_W], S + o_w2t, k.cout, k.cout, k.cout_p, s);
    }
    if (!st) st = launch_pack_linear_rows(t[DT_BT_TIME_W], t[DT_BT_TIME_B], S + o_wt + (size_t)k.tb_off * D,
                                          S + o_bt + k.tb_off, k.cout, D, k.cout_p, s);
  }
  copy(o_w1g, gt[DT_GT_TIME1_W], (size_t)D * D); copy(o_b1g, gt[DT_GT_TIME1_B], D);
  copy(o_wc0, gt[DT_GT_COND0_W], D); copy(o_bc0, gt[DT_GT_COND0_B], D);
  copy(o_wc2, gt[DT_GT_COND2_W], (size_t)D * D); copy(o_bc2, gt[DT_GT_COND2_B], D);
  copy(o_fr, gt[DT_GT_FREQS], half);
  copy(o_fw, gt[DT_GT_FINAL_W], (size_t)C * d[0]); copy(o_fb, gt[DT_GT_FINAL_B], C);
  if (st != DT_OK) { (void)hipFree(u->slab); delete u; return st; }
  u->tw = TembWeights{S + o_fr, S + o_w1g, S + o_b1g, S + o_wc0, S + o_bc0, S + o_wc2, S + o_bc2, S + o_wt, S + o_bt,
                      D, half, u->tb_stride, tb, u->share_enc1 ? S + o_w2t : nullptr, c0p};
  u->final_w = S + o_fw; u->final_b = S + o_fb;
  st = build_fused(u, bt, s);
  if (st != DT_OK) { (void)hipFree(u->slab); if (u->fused_slab) (void)hipFree(u->fused_slab); delete u; return st; }
  *out = u;
  return DT_OK;
}

void dt_unet_destroy(dt_unet *h) {
  if (!h) return;
  drop_graphs(h);
  if (h->slab) (void)hipFree(h->slab);
  if (h->fused_slab) (void)hipFree(h->fused_slab);
  delete h;
}

int dt_unet_time_bias_stride(const dt_unet *h) { return h ? h->tb_stride : DT_E_NULL; }

int dt_unet_time_bias(const dt_unet *h, const int32_t *t, const float *cond, const uint8_t *present, int rows,
                      float *out, void *stream) {
  if (!h || !t || !out) return DT_E_NULL;
  if (rows < 0) return DT_E_ARG;
  return launch_time_bias(h->tw, t, cond, present, rows, out, (hipStream_t)stream);
}

size_t dt_unet_workspace_bytes(const dt_unet *h, int batch_total, int H, int W) {
  const FwdShape sh = FwdShape::rows_only(batch_total, H, W);
  if (!h || sh.validate() != DT_OK) return 0;
  return make_plan(h, sh).total * sizeof(float);
}

int dt_unet_forward(const dt_unet *h, const float *x, int B, int n_pass, int H, int W, const float *tb, int tb_div,
                    float *eps, void *ws, size_t ws_bytes, void *stream) {
  const BatchSplit b{B, n_pass, 0, tb_div};
  if (const int bad = forward_status(h, x, b, H, W, tb, eps, ws)) return bad;
  return forward_impl(h, x, b, H, W, tb, eps, (float *)ws, ws_bytes, (hipStream_t)stream);
}

// launches are timed on an otherwise idle GPU, where extra workgroups are free, whereas in the sampler other streams fill idle
// CUs: a split launch (slab traffic + one more launch) must be this much faster to be taken
constexpr float kSplitMargin = 1.05f;

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
  const Plan pl = make_plan(h, t.shape);
  if (pl.total * sizeof(float) > ws_bytes) return DT_E_WORKSPACE;
  float *ws = (float *)workspace;
  ConvTimer timer;
  if (const int bad = timer.create()) return bad;
  const ResolvedForward f = resolve_forward(h, t.shape, nullptr);   // candidates start from the defaults
  const float *tb = h->slab;   // any readable floats: only timing matters here
  int st = DT_OK;
  {   // The clocks of an idle GPU take tens of milliseconds of load to settle (the same launch measures 15 % slower
      // cold): run one mid-sized layer for a while first so that the first candidates are not timed against a ramp.
    const ConvParams wp = bind_conv(h, f, 1, 1, f.c[1][1], ws + pl.pool[0], ws, pl, tb, batch_total);
    for (int rep = 0; rep < 200 && st == DT_OK; ++rep) st = launch_conv(wp, s);
    if (hipStreamSynchronize(s) != hipSuccess) st = (int)hipGetLastError();
  }
  for (int j = 0; j < kBlocks && st == DT_OK; ++j) {
    const float *in = j == 0 ? ws + pl.h[0] : (j <= 4 ? ws + pl.pool[j - 1] : ws + pl.cat[j - 5]);   // (enc1: stands in for the image)
    float skip_ms = 0.f;
    for (int slot = 0; slot < 3 && st == DT_OK; ++slot) {
      if (!has_launch(h, j, slot)) continue;
      ConvChoice best = f.c[j][slot];
      best.fuse = 0;               // candidates start from the UNFUSED launch (the default may have folded the skip in)
      const ConvLayer L = conv_layer(h, f, j, slot);
      float best_ms = 1e30f;
      // the timed average of one candidate; < 0: the launch cannot run here
      auto measure = [&](const ConvParams &q, int reps) -> float {
        float ms;
        const int lst = timer.time(q, reps, s, &ms);
        if (lst != DT_OK && lst != DT_E_SHAPE && lst != DT_E_ARG) st = lst;
        return lst == DT_OK ? ms : -1.f;
      };
      struct Cand { ConvChoice c; ConvParams q; float cost; };
      std::vector<Cand> cands;
      // a fused conv2 also saves the separate skip launch measured for slot 0; a split must win by kSplitMargin
      auto cost_of = [&](float ms, const ConvChoice &c) {
        return (ms + (c.fuse ? 0.f : (L.foldable ? skip_ms : 0.f))) * (c.splits > 1 ? kSplitMargin : 1.0f);
      };
      // Search policy (the search is paid once per model and shape, so it is pruned to what the per-layer tables show can
      // win): exact-fp32 mode -> the fp32-MFMA kind only; otherwise the strip kinds for full 3x3 walks that some strip tile
      // reaches and the plain split-bf16 kind for everything else.  Which candidates can run at all is conv_admissible's.
      const bool strip_ok = L.taps == 9 && strip_reaches(L.W);
      for (const int kind : {KIND_FP32, KIND_BF16, KIND_STRIP, KIND_STRIP2, KIND_STRIPK}) {
        if (h->precision == DT_PREC_FP32 ? kind != KIND_FP32 : kind == KIND_FP32) continue;
        if (is_strip(kind) ? !strip_ok : (kind == KIND_BF16 && strip_ok)) continue;
        for (int bm = 64; bm <= 256; bm *= 2)
          for (int bn = 64; bn <= 128; bn += 64) {
            // dec1.conv2 with one N tile also evaluates the head (saves the head launch and dec1's output round trip)
            if (j == kBlocks - 1 && slot == 2 && h->head_fusion && h->desc.channels <= 3 && L.n_p <= 128 && bn != L.n_p) continue;
            // 3x3 walks split by taps 1/3/9; the strip kernel and single-tap layers by channel chunks 1/2/4/8
            const long long tiles = (long long)((L.M + bm - 1) / bm) * (L.n_p / bn);
            for (int sp = 1; sp <= (L.splittable ? 9 : 1); sp *= ((is_strip(kind) || L.taps != 9) ? 2 : 3))
              for (int fuse = 0; fuse <= ((L.foldable && sp == 1) ? 1 : 0); ++fuse) {
                if (sp > 1 && tiles * (sp / 2) >= 1024) continue;          // already >= 4 workgroups per CU without this split
                const ConvChoice c{bm, bn, sp, kind, fuse};
                const ConvParams q = bind_conv(h, f, j, slot, c, in, ws, pl, tb, batch_total);
                if (conv_admissible(q) != DT_OK) continue;
                const float ms = measure(q, 3);
                if (ms < 0.f) continue;
                cands.push_back(Cand{c, q, cost_of(ms, c)});
              }
          }
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
  TunedShape *old = const_cast<TunedShape *>(find_tuned(h, t.shape));
  if (old) *old = t;
  else h->tuned.push_back(t);
  drop_graphs(h);
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
  const Plan pl = make_plan(h, req.shape);
  if (pl.total * sizeof(float) > ws_bytes) return DT_E_WORKSPACE;
  float *ws = (float *)workspace;
  const float *in = block == 0 ? ws + pl.h[0] : (block <= 4 ? ws + pl.pool[block - 1] : ws + pl.cat[block - 5]);
  if (!has_launch(h, block, slot)) { *ms = 0.f; *flops = 0.0; return DT_OK; }
  // every slot asks for the choice: (block, slot) is bound with what follows from its own resolution only
  std::fill_n(&req.c[0][0], kBlocks * 3, ConvChoice{bm, bn, splits, prec, fuse});
  const ResolvedForward f = resolve_forward(h, req.shape, &req);
  const ConvParams p = bind_conv(h, f, block, slot, f.c[block][slot], in, ws, pl, h->slab, batch_total);
  *flops = 2.0 * p.M * (double)p.cout_real * ((double)p.cin_real * p.ksize * p.ksize + (p.in2 ? p.cin2_real : 0));
  ConvTimer timer;
  if (const int bad = timer.create()) return bad;
  return timer.time(p, reps, (hipStream_t)stream, ms);
}

int dt_unet_set_precision(dt_unet *h, int precision) {
  if (!h) return DT_E_NULL;
  if (precision < DT_PREC_FP32 || precision > DT_PREC_AUTO) return DT_E_ARG;
  h->tuned.clear();                               // choices are per arithmetic mode: back to the heuristic plan
  drop_graphs(h);
  h->precision = precision;
  return DT_OK;
}

int dt_unet_set_head_fusion(dt_unet *h, int on) {
  if (!h) return DT_E_NULL;
  h->head_fusion = on != 0;
  drop_graphs(h);
  return DT_OK;
}

int dt_unet_set_fused(dt_unet *h, int on) {
  if (!h) return DT_E_NULL;
  h->fused_on = on != 0 && h->fused_ok;
  drop_graphs(h);
  return DT_OK;
}

int dt_unet_fused_active(const dt_unet *h, int H, int W) {
  if (!h) return DT_E_NULL;
  return use_fused(h, H, W) ? 1 : 0;
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
  *bm = c.bm; *bn = c.bn; *splits = c.splits; *prec = c.kind + (c.fuse ? 8 : 0); *tuned = t && has_launch(h, block, slot);
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
  if (!conv_choice_valid(c, slot, h->blk[block].n_p)) return DT_E_ARG;
  TunedShape *t = const_cast<TunedShape *>(find_tuned(h, sh));
  if (!t) {   // start from what an untuned forward would launch
    TunedShape fresh{sh, {}};
    memcpy(fresh.c, resolve_forward(h, sh, nullptr).c, sizeof(fresh.c));
    h->tuned.push_back(fresh);
    t = &h->tuned.back();
  }
  t->c[block][slot] = c;
  drop_graphs(h);
  return DT_OK;
}

int dt_unet_debug_activation(const dt_unet *h, int batch_total, int H, int W, int which, size_t *off, int *cp,
                             int *oh, int *ow) {
  if (!h || !off || !cp || !oh || !ow) return DT_E_NULL;
  if (which < 0 || which > kBlocks) return DT_E_ARG;
  const FwdShape sh = FwdShape::rows_only(batch_total, H, W);
  if (const int bad = sh.validate()) return bad;
  const Plan pl = make_plan(h, sh);
  if (which == kBlocks) { *off = pl.slab; *cp = 0; *oh = 0; *ow = 0; return DT_OK; }   // the split-K slab (diagnostics)
  *off = pl.o[which]; *cp = h->blk[which].cout_p; *oh = pl.H[which]; *ow = pl.W[which];
  return DT_OK;
}

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
static int sample_loop(const dt_unet *h, const SampleArgs &a) {
  const int B = a.b.B, H = a.H, W = a.W;
  const int E = h->desc.channels * H * W;
  const size_t slot = (size_t)B * E;
  const int tb_rows = a.b.tb_rows();            // time-bias rows per step
  const Plan pl = make_plan(h, a.b.shape(H, W));
  if (pl.total * sizeof(float) > a.ws_bytes) return DT_E_WORKSPACE;
  if (use_fused(h, H, W)) {
    // small model: forward + CFG mix + update of up to kFusedMaxSteps timesteps per launch, images resident in LDS
    for (int i0 = 0; i0 < a.n_steps; i0 += kFusedMaxSteps) {
      const int n = a.n_steps - i0 < kFusedMaxSteps ? a.n_steps - i0 : kFusedMaxSteps;
      FusedArgs fa{};
      fused_common(h, fa, a.b, a.tb + (size_t)i0 * tb_rows * h->tb_stride);
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
      int st = forward_impl(h, x, a.b, H, W, a.tb + (size_t)i * tb_rows * h->tb_stride, nullptr, (float *)a.ws, a.ws_bytes, a.s);
      if (st) return st;
    }
    // second-pass rows start at row B and belong to images B_single .. B-1: indexed by image through a pointer shifted back
    int st = launch_cfg_update_lowres(a.rule, x, lowres, a.b.n_pass == 2 ? lowres + (size_t)(B - a.b.B_single) * (H / 2) * (W / 2) * 4 : nullptr, a.z,
                                      a.z_row, a.z_shift ? (long long)a.z_shift[i] : 0, a.coef + 4 * i, a.has_noise[i], a.w, a.w_scalar, xn,
                                      B, h->desc.channels, H, W, a.b.B_single, a.s, a.mk);
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
static int run_or_replay(const dt_unet *h, const SampleArgs &a) {
  const char *genv = getenv("DT_GRAPH");
  const bool use_graph = genv && atoi(genv) != 0;
  if (!use_graph || g_prof.on.load() || a.n_steps < 4) return sample_loop(h, a);
  std::vector<unsigned char> key = a.key();
  std::lock_guard<std::mutex> lock(h->graph_mu);
  for (const LoopGraph &g : h->graphs)
    if (g.key == key) return (int)hipGraphLaunch(g.exec, a.s);
  // ---- first call with these arguments: capture the loop, instantiate, keep (at most 8 per handle)
  hipError_t e = hipStreamBeginCapture(a.s, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {   // stream cannot be captured (e.g. the legacy default stream): plain launches
    (void)hipGetLastError();
    return sample_loop(h, a);
  }
  const int st = sample_loop(h, a);
  LoopGraph g{};
  e = hipStreamEndCapture(a.s, &g.graph);
  if (st != DT_OK) { if (e == hipSuccess && g.graph) (void)hipGraphDestroy(g.graph); return st; }
  if (e != hipSuccess) return (int)e;
  e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g.graph); return (int)e; }
  g.key = std::move(key);
  if (h->graphs.size() >= 8) { (void)hipGraphExecDestroy(h->graphs.front().exec); (void)hipGraphDestroy(h->graphs.front().graph); h->graphs.erase(h->graphs.begin()); }
  h->graphs.push_back(std::move(g));
  if (getenv("DT_GRAPH_DEBUG")) fprintf(stderr, "[dt_hip] captured sampler loop: %d steps, batch %d -> graph #%zu\n", a.n_steps, a.b.B, h->graphs.size());
  return (int)hipGraphLaunch(h->graphs.back().exec, a.s);
}

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
  if (const int bad = sample_mixed_status(h, rule, a.b, H, W, n_steps, tb, coef, has_noise, w, traj, ws, h && h->share_enc1)) return bad;
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
  if (const int bad = sample_masked_status(h, rule, a.b, H, W, n_steps, tb, coef, has_noise, w, mask, known, traj, ws, h && h->share_enc1)) return bad;
  a.b = a.b.normalised();                      // every image takes one pass: a one-pass batch
  return sample_loop(h, a);
}
#undef DT_LOOP_ARGS

int dt_unet_forward_mixed(const dt_unet *h, const float *x, int B, int B_single, int H, int W, const float *tb, int tb_div,
                          float *eps, void *ws, size_t ws_bytes, void *stream) {
  const BatchSplit b{B, 2, B_single, tb_div};
  if (const int bad = forward_mixed_status(h, x, b, H, W, tb, eps, ws, h && h->share_enc1)) return bad;
  return forward_impl(h, x, b, H, W, tb, eps, (float *)ws, ws_bytes, (hipStream_t)stream);
}

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
