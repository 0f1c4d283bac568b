// The U-Net's geometry and its three layouts: what follows from a dt_unet_desc and a forward shape by integer arithmetic
// alone -- the channels of every block and convolution slot, the float offsets of everything in the handle's weight slab, and
// the activation buffers of one forward in the workspace.  Plain C++ with no HIP in it and no pointer into device memory:
// tests/host_sanitize/unet_layout_check.cpp compares every field below with the text of dt_unet_create and make_plan that it
// replaced, over a grid of models and forward shapes.  dt_unet.h holds the pointers that go with the geometry.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

#include "../../include/dt_hip.h"
#include "dt_batch.h"

namespace dt {

constexpr int kChanPad = 16;   // activation channel granularity (= BK of the conv GEMM)
constexpr int kNPad = 64;      // packed-weight N granularity (smallest BN tile)
constexpr int kBlocks = 8;
constexpr int kChunkPad = 4;   // chunk granularity of the split-bf16 weight packs (see ConvParams::ccw)
constexpr int kSplitMaxRows = 32768;   // split-K candidates only below this many GEMM rows (bounds the slab)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// 16-channel weight chunks per tap of a split-bf16 pack of cin_p input channels (zero chunks up to a multiple of kChunkPad)
inline int pack_chunks(int cin_p) { return round_up(cin_p, 16 * kChunkPad) >> 4; }

// level (power-of-two divisor of the image size) of the 8 blocks
constexpr int kDiv[kBlocks] = {1, 2, 4, 8, 16, 8, 4, 2};
// the encoder block whose output decoder block j (5..7) concatenates: dec3<-enc4(3), dec2<-enc3(2), dec1<-enc2(1)
inline int skip_block(int j) { return 8 - j; }

// ---------------------------------------------------------------------------------------------------------- geometry
// One convolution of a block, under its slot: 0 = the 1x1 skip, 1 = conv1 (both over the block input), 2 = conv2 (over
// conv1's output) -- the key of ResolvedForward::c, has_launch, conv_layer and every plan hook.
struct ConvGeom {
  int cin, cin_p;         // real / padded input channels
  int split_c, split_cp;  // concat split of the input channels (== cin, cin_p when no concat)
  int cin_w;              // input channels per tap of the split-bf16 pack: cin_p padded to kChunkPad chunks
  int ksize;              // 1 or 3
};
struct BlockGeom {
  int cin, cout;          // real channels
  int cin_p, cout_p, n_p; // padded
  int split_c, split_cp;  // concat split of the block input
  bool has_res;           // the skip is a 1x1 convolution (cin != cout), not the identity
  int tb_off;             // channel offset of this block in a time-bias row
  ConvGeom c[3];
};
struct UnetGeom {
  dt_unet_desc desc;
  // enc1 runs ONCE per step for all CFG passes (they share x): conv1 without the time bias over the B images, conv2 over the
  // B images with the passes' time biases entering as class-bias rows in its epilogue (tap_bias_kernel); DT_NO_SHARED_ENC1=1
  // at create time keeps the per-pass formulation (A/B runs, and the form the reference's operation order follows literally)
  bool share_enc1;
  BlockGeom blk[kBlocks];
  int cp[4];              // padded dims
  int tb_cols;            // projected channels of a time-bias row; the class-bias columns follow
  int tb_stride;          // floats of a time-bias row: [projected channels | nine class-bias vectors of enc1.conv2]
  // whether slot `slot` of block j is a convolution of its own: enc1.conv1 is the direct first-layer kernel and enc1's skip is
  // recomputed in conv2's epilogue; identity skips have none
  bool has_launch(int j, int slot) const { return slot == 2 || (j > 0 && (slot == 1 || blk[j].has_res)); }
};

// DT_OK, or the DT_E_SHAPE of a description no model has
inline int unet_geometry(const dt_unet_desc &desc, bool share_enc1, UnetGeom *out) {
  if (desc.channels < 1 || desc.channels > 3 || desc.temb_dim < 2) return DT_E_SHAPE;
  for (int i = 0; i < 4; ++i)
    if (desc.dims[i] < 1) return DT_E_SHAPE;
  UnetGeom g{};
  g.desc = desc;
  g.share_enc1 = share_enc1;
  const int C = desc.channels;
  const int32_t *d = desc.dims;
  for (int i = 0; i < 4; ++i) g.cp[i] = round_up(d[i], kChanPad);
  // (cin, cout) and the concat split of the eight blocks -- models.py:138-154
  const int cin[kBlocks] = {C, d[0], d[1], d[2], d[3], d[3] + d[3], d[2] + d[2], d[1] + d[1]};
  const int cout[kBlocks] = {d[0], d[1], d[2], d[3], d[3], d[2], d[1], d[0]};
  const int up_c[kBlocks] = {0, 0, 0, 0, 0, d[3], d[2], d[1]};   // channels coming from the upsampled branch
  int tb = 0;
  for (int j = 0; j < kBlocks; ++j) {
    BlockGeom &k = g.blk[j];
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
    for (int slot = 0; slot < 3; ++slot) {
      ConvGeom &c = k.c[slot];
      c = slot == 2 ? ConvGeom{k.cout, k.cout_p, k.cout, k.cout_p, 0, 0} : ConvGeom{k.cin, k.cin_p, k.split_c, k.split_cp, 0, 0};
      c.cin_w = pack_chunks(c.cin_p) * 16;
      c.ksize = slot == 0 ? 1 : 3;
    }
    k.tb_off = tb;
    tb += k.cout_p;
  }
  g.tb_cols = tb;
  g.tb_stride = tb + (share_enc1 ? 9 * g.blk[0].cout_p : 0);
  *out = g;
  return DT_OK;
}

// ---------------------------------------------------------------------------------------------------------- layouts
// Regions of one allocation in floats, each on a 256-byte boundary.  `log` (the layout check's): every (offset, floats) taken.
struct Bump {
  size_t off = 0;
  std::vector<std::pair<size_t, size_t>> *log = nullptr;
  size_t take(size_t n) {
    const size_t o = off;
    off += (n + 63) / 64 * 64;
    if (log) log->emplace_back(o, n);
    return o;
  }
};

// The weight slab of a handle, as float offsets; a region that a model does not have stays 0.
struct SlabLayout {
  struct { size_t w, wb, ss; } c[kBlocks][3];   // a slot's fp32 pack, bf16x3 pack, scale + shift (n_p floats each); enc1.conv1's w
                                                // is the direct first-layer kernel's pack wf[9C][cout_p]
  size_t w3;                                    // enc1's image-skip weights [n_p][4] for conv2's epilogue
  size_t w2t;                                   // enc1.conv2 tap-major, for the class-bias columns (share_enc1 only)
  size_t wt, bt;                                // the time tower: the blocks' time_mlp rows [tb_cols][D], their biases,
  size_t w1g, b1g, wc0, bc0, wc2, bc2, fr;      // time_mlp.1, cond_emb.0, cond_emb.2, the sinusoid frequencies [half]
  size_t fw, fb;                                // the final 1x1 head [C][dims[0]], [C]
  size_t total;
  int half;                                     // max(D / 2, 1)
};

inline SlabLayout slab_layout(const UnetGeom &g, std::vector<std::pair<size_t, size_t>> *log = nullptr) {
  SlabLayout L{};
  Bump bump;
  bump.log = log;
  const int C = g.desc.channels, D = g.desc.temb_dim;
  for (int j = 0; j < kBlocks; ++j) {
    const BlockGeom &k = g.blk[j];
    for (int slot = 0; slot < 3; ++slot) {
      const ConvGeom &c = k.c[slot];
      const size_t taps = (size_t)c.ksize * c.ksize;
      if (g.has_launch(j, slot)) {   // a tile-GEMM / strip launch of its own: both packs (bf16x3: 6 bytes per weight = 1.5 floats)
        L.c[j][slot].w = bump.take(taps * c.cin_p * k.n_p);
        L.c[j][slot].wb = bump.take(taps * c.cin_w * k.n_p * 3 / 2);
      }
      if (g.has_launch(j, slot) || slot == 1) L.c[j][slot].ss = bump.take((size_t)2 * k.n_p);
    }
    if (j == 0) {   // enc1: conv1 is the direct first-layer kernel over wf[9C][cout_p]; the skip is w3[n_p][4] in conv2's epilogue
      L.c[0][1].w = bump.take((size_t)9 * C * k.cout_p);
      if (k.has_res) L.w3 = bump.take((size_t)4 * k.n_p);
    }
  }
  const int c0p = g.blk[0].cout_p, tb = g.tb_cols;
  if (g.share_enc1) L.w2t = bump.take((size_t)9 * c0p * c0p);
  L.half = D / 2 > 1 ? D / 2 : 1;
  L.wt = bump.take((size_t)tb * D); L.bt = bump.take(tb);
  L.w1g = bump.take((size_t)D * D); L.b1g = bump.take(D); L.wc0 = bump.take(D); L.bc0 = bump.take(D);
  L.wc2 = bump.take((size_t)D * D); L.bc2 = bump.take(D); L.fr = bump.take(L.half);
  L.fw = bump.take((size_t)C * g.desc.dims[0]); L.fb = bump.take(C);
  L.total = bump.off;
  return L;
}

// activation buffers of one forward, as float offsets into the workspace
struct Plan {
  size_t h[kBlocks], r[kBlocks], o[kBlocks];   // conv1 out, skip out, block out
  size_t pool[4], cat[3];
  size_t slab, lowres;                         // split-K partial sums; low-resolution head output
  size_t total;
  int H[kBlocks], W[kBlocks];                  // spatial size of each block
  // the input buffer of block j: the pooled output of the encoder block before it, or the decoder's concat.  enc1 reads the
  // NCHW image itself; where a buffer must stand in for it (the tuner's timed launches) it is conv1's output.
  size_t input(int j) const { return j == 0 ? h[0] : (j <= 4 ? pool[j - 1] : cat[j - 5]); }
};

inline Plan make_plan(const UnetGeom &g, const FwdShape &sh, std::vector<std::pair<size_t, size_t>> *log = nullptr) {
  const int Bt = sh.Bt, H = sh.H, W = sh.W;
  Plan p{};
  Bump b;
  b.log = log;
  size_t slab = 0;
  for (int j = 0; j < kBlocks; ++j) {
    const BlockGeom &k = g.blk[j];
    const int h = H / kDiv[j], w = W / kDiv[j];
    p.H[j] = h; p.W[j] = w;
    const size_t px = (size_t)Bt * h * w;
    if (j >= 1 && j <= 4) p.pool[j - 1] = b.take(px * k.cin_p);
    if (j >= 5) p.cat[j - 5] = b.take(px * k.cin_p);
    p.h[j] = b.take(px * k.cout_p);
    p.r[j] = (k.has_res && j > 0) ? b.take(px * k.cout_p) : 0;
    p.o[j] = b.take(px * k.cout_p);
    if (j > 0 && px <= (size_t)kSplitMaxRows) {
      const size_t need = (size_t)9 * px * k.cout_p;    // room for the deepest split
      if (need > slab) slab = need;
    }
  }
  p.slab = b.take(slab);
  p.lowres = b.take((size_t)Bt * (H / 2) * (W / 2) * 4);
  p.total = b.off;
  return p;
}

}  // namespace dt
