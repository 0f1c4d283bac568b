// The forward of a U-Net handle: which launches a forward shape resolves to, how one convolution slot is bound to the
// workspace, and the launch sequence itself.
//
// Plan of one forward (reference models.py:159-224), NHWC activations with channels padded to 16:
//   x(NCHW) -> enc1.conv1 (direct fp32 conv, shared by the passes)
//   enc1 @H      -> pool -> enc2 @H/2 -> pool -> enc3 @H/4 -> pool -> enc4 @H/8 -> pool -> bottleneck @H/16
//   up+cat(enc4) -> dec3 @H/8 -> up+cat(enc3) -> dec2 @H/4 -> up+cat(enc2) -> dec1 @H/2 -> up + 1x1 head @H
// Each residual block is up to three implicit-GEMM launches (1x1 skip, conv1, conv2) whose epilogues
// carry BN/ReLU/time-bias/residual, so a forward is 8 blocks * (2..3) + 4 pools + 3 upcats + 2 = ~32 launches.
#include "dt_unet.h"

namespace dt {

const TunedShape *find_tuned(const dt_unet *u, const FwdShape &sh) {
  for (const TunedShape &t : u->tuned)
    if (t.shape == sh) return &t;
  return nullptr;
}

TunedShape *tuned_for(dt_unet *u, const FwdShape &sh) {
  for (TunedShape &t : u->tuned)
    if (t.shape == sh) return &t;
  return nullptr;
}

ConvLayer conv_layer(const dt_unet *u, const ResolvedForward &f, int j, int slot) {
  const BlockGeom &k = u->geo.blk[j];
  const int h = f.shape.H / kDiv[j], w = f.shape.W / kDiv[j];
  const int M = (j == 0 && f.shared_enc1 ? f.shape.imgs : f.shape.Bt) * h * w;
  const int taps = slot == 0 || (h == 1 && w == 1) ? 1 : 9;   // a 1x1 image only ever sees the centre tap of a padded 3x3 kernel
  return ConvLayer{M, w, k.n_p, k.c[slot].cin_p, taps, j > 0 && M <= kSplitMaxRows, slot == 2 && j > 0 && k.has_res};
}

ResolvedForward resolve_forward(const dt_unet *u, const FwdShape &sh, const TunedShape *tuned) {
  const UnetGeom &g = u->geo;
  ResolvedForward f{};
  f.shape = sh;
  f.shared_enc1 = g.share_enc1 && (sh.Bt + sh.single) % sh.imgs == 0;
  for (int j = 0; j < kBlocks; ++j)
    for (int slot = 0; slot < 3; ++slot)
      if (g.has_launch(j, slot)) f.c[j][slot] = resolve_conv_choice(conv_layer(u, f, j, slot), tuned ? &tuned->c[j][slot] : nullptr, u->precision);
  for (int j = 0; j < kBlocks; ++j) {
    const ConvChoice &c2 = f.c[j][2];
    const int h = sh.H / kDiv[j], w = sh.W / kDiv[j];
    // encoder blocks enc1..enc4 feed a 2x2 max pool: folded into conv2's staged epilogue where a 32-row tile holds whole row
    // pairs (W a power of two <= 16); split launches pool in their slab-summing epilogue kernel instead
    f.pool_fused[j] = j <= 3 && h % 2 == 0 && w % 2 == 0 && (c2.splits > 1 || (w <= 16 && (w & (w - 1)) == 0));
    // a decoder block reads the concat [upsampled | skip]: when both of its readers are strip launches (conv1, and the 1x1 skip
    // folded into conv2) they fetch the skip half straight from the encoder's output and the concat holds the upsampled half only
    // (the handle's switch is a test hook: off, the same launches read the skip half from the concat buffer)
    f.concat_in_place[j] = u->concat_in_place && j >= 5 && g.blk[j].has_res && is_strip(f.c[j][1].kind) && is_strip(c2.kind) && c2.fuse;
  }
  // dec1.conv2 also evaluates the final 1x1 head when its workgroups hold whole rows (one N tile, no split): the head is dec1's
  // only consumer, so dec1's own output is then never written
  const ConvChoice &last = f.c[kBlocks - 1][2];
  f.head_fused = u->head_fusion && last.splits == 1 && g.blk[kBlocks - 1].n_p == last.bn && g.desc.channels <= 3;
  return f;
}

ConvParams bind_conv(const dt_unet *u, const ResolvedForward &f, int j, int slot, const ConvChoice &c, const float *in, float *ws,
                     const Plan &pl, const float *tb, int tb_div) {
  const UnetGeom &g = u->geo;
  const BlockGeom &k = g.blk[j];
  const ConvGeom &cg = k.c[slot];
  const ConvW &cw = u->blk[j].c[slot];
  const ConvLayer L = conv_layer(u, f, j, slot);
  const int h = pl.H[j], w = pl.W[j];
  ConvParams p{};
  p.M = L.M; p.H = h; p.W = w;
  p.cin_p = L.cin_p; p.cout_p = k.cout_p; p.n_p = k.n_p;
  p.cin_real = cg.cin; p.cout_real = k.cout;
  p.tb_stride = g.tb_stride; p.m_per_tb = h * w * tb_div;
  p.slab = ws + pl.slab;
  p.in = slot == 2 ? ws + pl.h[j] : in;
  p.ksize = cg.ksize;
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
      p.x3 = in; p.w3 = u->blk[0].w3; p.x3_hw = h * w; p.x3_imgs = f.shape.imgs; p.x3_c = g.desc.channels;
      if (f.shared_enc1) {   // one launch over the images for all their passes
        p.n_dup = (f.shape.Bt + f.shape.single) / f.shape.imgs; p.dup_rows = p.M; p.dup_skip = f.shape.single * h * w; p.tbc = tb + g.tb_cols;
        p.skip_out = u->head_fusion && p.pool_out ? 1 : 0;   // only the pool reads enc1's output (else a pooling launch does)
      }
    } else {
      p.add = k.has_res ? ws + pl.r[j] : in;   // identity skip: cin_p == cout_p
    }
    if (j == kBlocks - 1 && f.head_fused) {
      p.head_w = u->final_w; p.head_b = u->final_b; p.head_out = ws + pl.lowres;
      p.head_c = g.desc.channels; p.head_cin = g.desc.dims[0];
    }
  }
  // the choice: tile, kind, the weight pack of the kind (and its chunk width), the folded skip walk where c folds it
  const bool fp32 = c.kind == KIND_FP32;
  p.bm = c.bm; p.bn = c.bn; p.splits = c.splits; p.kind = c.kind;
  p.w = fp32 ? cw.w : cw.wb;
  p.ccw = (fp32 ? cg.cin_p : cg.cin_w) >> 4;
  if (c.fuse) {   // conv2 with the block's 1x1 skip (slot 0) folded into its K walk (the slot-0 launch is then skipped)
    const ConvGeom &sg = k.c[0];
    const ConvW &sk = u->blk[j].c[0];
    p.add = nullptr;
    p.in2 = in; p.w2 = fp32 ? sk.w : sk.wb; p.bias2 = sk.shift; p.cin2_p = sg.cin_p; p.cin2_real = sg.cin;
    p.ccw2 = (fp32 ? sg.cin_p : sg.cin_w) >> 4;
  }
  return p;
}

namespace {

int run_block(const dt_unet *u, const ResolvedForward &f, int j, const float *in, float *ws, const Plan &pl, const float *tb,
              int tb_div, hipStream_t s) {
  const UnetGeom &g = u->geo;
  if (j == 0) {
    const BlockGeom &k = g.blk[0];
    const ConvW &c1 = u->blk[0].c[1];
    if (!f.shared_enc1 && f.shape.single) return DT_E_ARG;   // mixed batches exist in the shared-enc1 formulation only
    // (shared: the passes' time biases enter in conv2's epilogue)
    const int st = launch_first_conv(in, c1.w, c1.scale, c1.shift, f.shared_enc1 ? nullptr : tb + k.tb_off, g.tb_stride, tb_div, ws + pl.h[0],
                                     f.shape.imgs, f.shared_enc1 ? 1 : f.shape.Bt / f.shape.imgs, g.desc.channels, pl.H[0], pl.W[0], k.cout, k.cout_p, s);
    if (st) return st;
  }
  for (int slot = 0; slot < 3; ++slot) {
    if (!g.has_launch(j, slot) || (slot == 0 && f.c[j][2].fuse)) continue;
    ConvParams p = bind_conv(u, f, j, slot, f.c[j][slot], in, ws, pl, tb, tb_div);
    if (f.concat_in_place[j]) {
      const int skip = skip_block(j);
      p.cc_a = g.blk[j].split_cp >> 4;
      p.b_stride = g.blk[skip].cout_p;
      if (slot == 1) p.in_b = ws + pl.o[skip];
      if (slot == 2) p.in2_b = ws + pl.o[skip];
    }
    const int st = launch_conv(p, s, u->strip_pair);
    if (st) return st;
  }
  return DT_OK;
}

}  // namespace

int forward_impl(const dt_unet *u, const float *x, const BatchSplit &b, int H, int W, const float *tb, float *eps, float *ws,
                 size_t ws_bytes, hipStream_t s) {
  const UnetGeom &g = u->geo;
  const FwdShape sh = b.shape(H, W);
  const int Bt = sh.Bt, tb_div = b.tb_div;
  const Plan pl = make_plan(g, sh);
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
  for (int j = 0; j < kBlocks; ++j) {
    if (j >= 1 && j <= 4) {        // encoder: pool the previous block's output (unless its conv2 already did)
      if (!f.pool_fused[j - 1])
      st = launch_maxpool(ws + pl.o[j - 1], ws + pl.pool[j - 1], Bt,
                          pl.H[j - 1], pl.W[j - 1], g.blk[j - 1].cout_p, s);
      if (st) return st;
    } else if (j >= 5) {           // decoder: upsample previous output, concat the matching encoder output
      const int skip = skip_block(j);
      st = launch_upcat(ws + pl.o[j - 1], f.concat_in_place[j] ? nullptr : ws + pl.o[skip], ws + pl.cat[j - 5],
                        Bt, pl.H[j - 1], pl.W[j - 1], g.blk[j - 1].cout_p, g.blk[skip].cout_p, s);
      if (st) return st;
    }
    // enc1 reads the NCHW image itself (first-layer kernel, skip in conv2's epilogue)
    st = run_block(u, f, j, j == 0 ? x : ws + pl.input(j), ws, pl, tb, tb_div, s);
    if (st) return st;
  }
  if (!f.head_fused) {   // head at the low resolution (unless dec1.conv2's epilogue already produced it), then the 3-channel upsample
    st = launch_head(ws + pl.o[7], u->final_w, u->final_b, ws + pl.lowres, Bt, pl.H[7], pl.W[7], g.blk[7].cout_p,
                     g.desc.channels, g.desc.dims[0], s);
    if (st) return st;
  }
  if (!eps) return DT_OK;                  // the sampler's fused update interpolates the low-resolution output itself
  return launch_head_upsample(ws + pl.lowres, eps, Bt, pl.H[7], pl.W[7], g.desc.channels, s);
}

// (head fusion off = the test hook that materialises every block output in the workspace: only the layered path has those)
bool use_fused(const dt_unet *u, int H, int W) { return u->fused_ok && u->fused_on && u->head_fusion && H == 16 && W == 16; }

void fused_common(const dt_unet *u, FusedArgs &a, const BatchSplit &b, const float *tb) {
  const UnetGeom &g = u->geo;
  a.ops = u->fused_ops_dev; a.n_ops = u->fused_n_ops; a.fbase = u->fused_slab; a.par = u->fused_par; a.n_par = u->fused_n_par;
  a.head_w = u->final_w; a.head_b = u->final_b;
  a.tb = tb; a.tb_stride = g.tb_stride; a.tb_div = b.tb_div;
  a.lds = u->fused_lds; a.G = u->fused_G;
  a.C = g.desc.channels; a.c0 = g.desc.dims[0]; a.c0p = g.cp[0];
  a.B = b.B; a.n_pass = b.n_pass; a.B_single = b.B_single;
  a.tb_rows = b.tb_rows();
  a.flops_per_row = fused_flops_per_row(a.C, g.desc.dims[0], g.desc.dims[1]);
}

}  // namespace dt

extern "C" {

int dt_unet_forward(const dt_unet *h, const float *x, int B, int n_pass, int H, int W, const float *tb, int tb_div,
                    float *eps, void *ws, size_t ws_bytes, void *stream) {
  const dt::BatchSplit b{B, n_pass, 0, tb_div};
  if (const int bad = dt::forward_status(h, x, b, H, W, tb, eps, ws)) return bad;
  return dt::forward_impl(h, x, b, H, W, tb, eps, (float *)ws, ws_bytes, (hipStream_t)stream);
}

int dt_unet_forward_mixed(const dt_unet *h, const float *x, int B, int B_single, int H, int W, const float *tb, int tb_div,
                          float *eps, void *ws, size_t ws_bytes, void *stream) {
  const dt::BatchSplit b{B, 2, B_single, tb_div};
  if (const int bad = dt::forward_mixed_status(h, x, b, H, W, tb, eps, ws, h && h->geo.share_enc1)) return bad;
  return dt::forward_impl(h, x, b, H, W, tb, eps, (float *)ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
