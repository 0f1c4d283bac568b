// The U-Net handle and what its translation units share: dt_unet.hip (create / destroy, the fused pack, the switches),
// dt_unet_forward.hip (launch resolution and the forward), dt_unet_tune.hip (the tuner and the plan hooks) and dt_sample.hip
// (the sampler loop and its graph replay).  The integers of the model are in dt_unet_layout.h; here are the pointers.
#pragma once
#include <mutex>
#include <vector>

#include "dt_conv_strip_pair.h"
#include "dt_fused.h"

namespace dt {

// the device pointers of one convolution slot (ConvGeom): nullptr where the slot has no such pack
struct ConvW {
  float *w, *wb;          // packed weights: fp32 tiles (dt_conv.hip), three bf16 planes (dt_conv_bf16.hip)
  float *scale, *shift;   // folded BN (a plain conv: 1 and its bias)
};
struct BlockW {
  ConvW c[3];             // enc1: c[1].w is the direct first-layer kernel's pack, c[0] is empty (w3 instead)
  float *w3;              // enc1 only: skip weights for the in-epilogue 1x1 (n_p x 4)
};

// (tile, split) choice of the three conv slots (0 = 1x1 skip, 1 = conv1, 2 = conv2) of every block for one forward shape:
// measured by dt_unet_autotune or pinned slot by slot through dt_unet_set_conv_choice; absent shapes use the heuristic
struct TunedShape {
  FwdShape shape;
  ConvChoice c[kBlocks][3];
};

// an instantiated hipGraph of one dt_sample_trajectory call (every launch of the loop), keyed by all its arguments
struct LoopGraph {
  std::vector<unsigned char> key;
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  LoopGraph() = default;
  LoopGraph(LoopGraph &&o) noexcept : key(std::move(o.key)), exec(o.exec), graph(o.graph) { o.exec = nullptr; o.graph = nullptr; }
  LoopGraph &operator=(LoopGraph &&o) noexcept {
    std::swap(key, o.key); std::swap(exec, o.exec); std::swap(graph, o.graph);
    return *this;
  }
  ~LoopGraph() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
  }
};

// the replay cache of a handle's sampler loop: at most kMax graphs, the oldest leaves first
class GraphCache {
 public:
  static constexpr size_t kMax = 8;
  std::mutex mu;   // the sampler holds it from its lookup to the launch of what it found or inserted; clear() takes it itself
  const LoopGraph *find(const std::vector<unsigned char> &key) const {
    for (const LoopGraph &g : graphs)
      if (g.key == key) return &g;
    return nullptr;
  }
  const LoopGraph &insert(LoopGraph &&g) {
    if (graphs.size() >= kMax) graphs.erase(graphs.begin());
    graphs.push_back(std::move(g));
    return graphs.back();
  }
  size_t size() const { return graphs.size(); }
  void clear() {
    std::lock_guard<std::mutex> lock(mu);
    graphs.clear();
  }
 private:
  std::vector<LoopGraph> graphs;
};

}  // namespace dt

struct dt_unet {
  dt_unet() = default;
  dt_unet(const dt_unet &) = delete;
  dt_unet &operator=(const dt_unet &) = delete;
  ~dt_unet() {
    graphs.clear();
    if (slab) (void)hipFree(slab);
    if (fused_slab) (void)hipFree(fused_slab);
  }
  std::vector<dt::TunedShape> tuned;
  // replay cache of the sampler loop (not part of the handle's logical state, hence mutable + its own lock: the
  // sampler may be entered from several host threads); cleared whenever the launch plan changes
  mutable dt::GraphCache graphs;
  int precision = DT_PREC_AUTO;   // DT_PREC_*: which convolution arithmetic the heuristic / autotuner may use
  bool head_fusion = true;   // dec1.conv2's epilogue evaluates the final 1x1 head (dt_unet_set_head_fusion)
  bool strip_pair = true;    // 256 x 64 K = 32 strip launches run the pair kernel where it serves them (dt_conv_strip_pair.h; DT_NO_STRIP_PAIR=1 at create time: off)
  bool concat_in_place = true;   // decoder strip launches read the concat's skip half from the encoder's output (resolve_forward; test hook, DT_NO_CONCAT_IN_PLACE=1 at create time: off)
  dt::UnetGeom geo{};
  dt::BlockW blk[dt::kBlocks] = {};
  float *slab = nullptr;     // one device allocation holding every pointer of blk, tw and the head (SlabLayout)
  dt::TembWeights tw{};
  const float *final_w = nullptr, *final_b = nullptr;   // the final 1x1 head, in the slab
  // Small models (padded dims <= 32 / 64) at 16 x 16: the whole forward -- and the whole sampler loop -- is ONE launch of
  // unet_fused_kernel (dt_fused.hip) with every activation in LDS.  fused_ok: the packs below exist; fused_on: the switch
  // (dt_unet_set_fused; DT_NO_FUSED=1 at create time starts with it off).
  bool fused_ok = false, fused_on = false;
  int fused_G = 2;
  float *fused_slab = nullptr;      // packed fp32 weights of the fused kernel + its layer table
  dt::FusedOp *fused_ops_dev = nullptr;
  int fused_n_ops = 0;
  dt::FusedLds fused_lds{};
  int fused_par = 0, fused_n_par = 0;   // the parameter block inside the fused slab
};

namespace dt {

const TunedShape *find_tuned(const dt_unet *u, const FwdShape &sh);
TunedShape *tuned_for(dt_unet *u, const FwdShape &sh);   // the same record, to be written

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
ConvLayer conv_layer(const dt_unet *u, const ResolvedForward &f, int j, int slot);
ResolvedForward resolve_forward(const dt_unet *u, const FwdShape &sh, const TunedShape *tuned);
// Parameters of slot `slot` of block j under choice c (the resolved one, or an autotuning candidate), bound to the workspace;
// `in` is the block input (enc1: the NCHW image).  The pool / head epilogues follow f's choice of the slot.
ConvParams bind_conv(const dt_unet *u, const ResolvedForward &f, int j, int slot, const ConvChoice &c, const float *in, float *ws,
                     const Plan &pl, const float *tb, int tb_div);
// One forward of the batch b (dt_batch.h), which the caller has checked: forward_status, forward_mixed_status or loop_status.
// eps == nullptr: the forward stops at the low-resolution head output.
int forward_impl(const dt_unet *u, const float *x, const BatchSplit &b, int H, int W, const float *tb, float *eps, float *ws,
                 size_t ws_bytes, hipStream_t s);
// the fused small-model path: whether a forward at H x W takes it, and the launch arguments every use of it shares
bool use_fused(const dt_unet *u, int H, int W);
void fused_common(const dt_unet *u, FusedArgs &a, const BatchSplit &b, const float *tb);

}  // namespace dt
