// The U-Net handle of libdt_hip.so: create (geometry -> slab layout -> allocate -> pack -> the fused small-model pack) and
// destroy, the time-bias rows, the workspace size and the handle's switches.  The forward is dt_unet_forward.hip, the tuner
// and plan hooks dt_unet_tune.hip, the sampler loop dt_sample.hip; what they share is dt_unet.h.
#include <cstdlib>
#include <memory>
#include <new>

#include "dt_unet.h"

using namespace dt;

namespace {

constexpr int kSlotWeight[3] = {DT_BT_RES_W, DT_BT_CONV1_W, DT_BT_CONV2_W};   // a slot's OIHW weights among a block's tensors

// Writes into one device slab on one stream and keeps the first error of what it and its user launched.
struct SlabWriter {
  float *base;
  hipStream_t s;
  int st = DT_OK;
  float *at(size_t off) const { return base + off; }
  void copy(size_t off, const float *src, size_t n) {
    if (st != DT_OK) return;
    const hipError_t e = hipMemcpyAsync(base + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) st = (int)e;
  }
};

// packs every tensor of the model into the slab u->slab laid out as L, and points the handle at the regions
int pack_slab(dt_unet *u, const SlabLayout &L, const float *const *bt, const float *const *gt, hipStream_t s) {
  const UnetGeom &g = u->geo;
  const int C = g.desc.channels, D = g.desc.temb_dim;
  SlabWriter wr{u->slab, s};
  int &st = wr.st;
  for (int j = 0; j < kBlocks && st == DT_OK; ++j) {
    const BlockGeom &k = g.blk[j];
    const float *const *t = bt + j * DT_BT_COUNT;
    // a slot's conv bias and eval-BatchNorm tensors (the skip is a plain conv)
    const float *const bn[3][5] = {{t[DT_BT_RES_B], nullptr, nullptr, nullptr, nullptr},
                                   {t[DT_BT_CONV1_B], t[DT_BT_BN1_G], t[DT_BT_BN1_B], t[DT_BT_BN1_MEAN], t[DT_BT_BN1_VAR]},
                                   {t[DT_BT_CONV2_B], t[DT_BT_BN2_G], t[DT_BT_BN2_B], t[DT_BT_BN2_MEAN], t[DT_BT_BN2_VAR]}};
    for (int slot = 0; slot < 3 && st == DT_OK; ++slot) {
      const ConvGeom &cg = k.c[slot];
      ConvW &c = u->blk[j].c[slot];
      const bool conv = g.has_launch(j, slot);
      if (conv || (j == 0 && slot == 1)) {
        c.w = wr.at(L.c[j][slot].w);
        c.scale = wr.at(L.c[j][slot].ss); c.shift = c.scale + k.n_p;
        st = launch_fold_bn(bn[slot][0], bn[slot][1], bn[slot][2], bn[slot][3], bn[slot][4], c.scale, c.shift, k.cout, k.n_p, s);
      }
      if (!conv) continue;
      c.wb = wr.at(L.c[j][slot].wb);
      if (!st) st = launch_pack_conv(t[kSlotWeight[slot]], c.w, k.cout, cg.cin, cg.ksize, cg.cin_p, k.n_p, cg.split_c, cg.split_cp, s);
      if (!st) st = launch_pack_conv_bf16x3(t[kSlotWeight[slot]], c.wb, k.cout, cg.cin, cg.ksize, cg.cin_p, cg.cin_w, k.n_p, cg.split_c, cg.split_cp, s);
    }
    if (j == 0) {   // enc1's exceptions: conv1's own pack; the image skip's weights; conv2 tap-major for the class-bias columns
      BlockW &b0 = u->blk[0];
      b0.w3 = wr.at(L.w3);
      if (!st) st = launch_pack_first_conv(t[DT_BT_CONV1_W], b0.c[1].w, k.cout, C, k.cout_p, s);
      if (!st) st = launch_pack_res3(t[DT_BT_RES_W], t[DT_BT_RES_B], b0.w3, k.cout, C, k.n_p, s);
      if (!st && g.share_enc1) st = launch_pack_tap_major(t[DT_BT_CONV2_W], wr.at(L.w2t), k.cout, k.cout, k.cout_p, s);
    }
    if (!st) st = launch_pack_linear_rows(t[DT_BT_TIME_W], t[DT_BT_TIME_B], wr.at(L.wt) + (size_t)k.tb_off * D,
                                          wr.at(L.bt) + k.tb_off, k.cout, D, k.cout_p, s);
  }
  wr.copy(L.w1g, gt[DT_GT_TIME1_W], (size_t)D * D); wr.copy(L.b1g, gt[DT_GT_TIME1_B], D);
  wr.copy(L.wc0, gt[DT_GT_COND0_W], D); wr.copy(L.bc0, gt[DT_GT_COND0_B], D);
  wr.copy(L.wc2, gt[DT_GT_COND2_W], (size_t)D * D); wr.copy(L.bc2, gt[DT_GT_COND2_B], D);
  wr.copy(L.fr, gt[DT_GT_FREQS], L.half);
  wr.copy(L.fw, gt[DT_GT_FINAL_W], (size_t)C * g.desc.dims[0]); wr.copy(L.fb, gt[DT_GT_FINAL_B], C);
  u->tw = TembWeights{wr.at(L.fr), wr.at(L.w1g), wr.at(L.b1g), wr.at(L.wc0), wr.at(L.bc0), wr.at(L.wc2), wr.at(L.bc2), wr.at(L.wt), wr.at(L.bt),
                      D, L.half, g.tb_stride, g.tb_cols, g.share_enc1 ? wr.at(L.w2t) : nullptr, g.blk[0].cout_p};
  u->final_w = wr.at(L.fw); u->final_b = wr.at(L.fb);
  return st;
}

// ---- the fused small-model path (dt_fused.hip): packs + layer table at create time, one launch per forward / sampler call.
// DT_OK without fused_ok: the model is not one the kernel runs.
int build_fused(dt_unet *u, const float *const *bt, hipStream_t s) {
  const UnetGeom &g = u->geo;
  const int C = g.desc.channels, c0p = g.cp[0], c1p = g.cp[1];
  if (g.cp[2] != c1p || g.cp[3] != c1p || g.desc.dims[2] != g.desc.dims[1] || g.desc.dims[3] != g.desc.dims[1]) return DT_OK;
  if (!fused_eligible(C, c0p, c1p)) return DT_OK;
  const int G = u->fused_G;
  const FusedLds lds = fused_lds(G, c0p, c1p);
  if ((size_t)lds.total * sizeof(float) > kFusedLdsLimit) return DT_OK;
  // one slab: the parameter block (dt_fused.h: the kernel copies it into LDS), the packed weights of conv1 (blocks 1..7), conv2
  // (all) and the 1x1 skip convs (enc1's image skip aside), enc1.conv1 as two K chunks, and the layer table
  Bump bump;
  const int n_par = fused_par_floats(lds.tb_cols, c0p), par_w3 = fused_par_w3(lds.tb_cols);
  const size_t o_par = bump.take(n_par);
  size_t o_w[kBlocks][3] = {};
  for (int j = 0; j < kBlocks; ++j)
    for (int slot = 0; slot < 3; ++slot) {
      const ConvGeom &c = g.blk[j].c[slot];
      if (g.has_launch(j, slot)) o_w[j][slot] = bump.take((size_t)c.ksize * c.ksize * c.cin_p * g.blk[j].cout_p);
    }
  const size_t o_wf = bump.take((size_t)2 * (c0p / 16) * 256);
  const size_t o_ops = bump.take((sizeof(FusedOp) * kFusedMaxOps + 3) / 4);
  if (bump.off >= (1u << 30)) return DT_OK;                     // offsets are ints
  DT_HIP_TRY(hipMalloc((void **)&u->fused_slab, bump.off * sizeof(float)));
  SlabWriter wr{u->fused_slab, s};
  int &st = wr.st;
  FusedModel m{};
  m.c0p = c0p; m.c1p = c1p; m.wf = (int)o_wf; m.w3 = par_w3;
  st = launch_pack_fused_first(bt[DT_BT_CONV1_W], wr.at(o_wf), g.blk[0].cout, C, c0p / 16, s);
  wr.copy(o_par + par_w3, u->blk[0].w3, (size_t)4 * c0p);
  int pj = 0;                                                   // the block's offset inside the parameter block
  for (int j = 0; j < kBlocks && st == DT_OK; ++j) {
    const BlockGeom &k = g.blk[j];
    const float *const *t = bt + j * DT_BT_COUNT;
    FusedBlockW &f = m.blk[j];
    const int cp = k.cout_p;
    f.tb_off = k.tb_off;
    // the block's five vectors in the parameter block: conv1's scale and shift, conv2's, the skip conv's bias
    FusedConvW *const fc[3] = {&f.cr, &f.c1, &f.c2};
    const int at_scale[3] = {-1, 0, 2}, at_shift[3] = {4, 1, 3};
    for (int slot = 0; slot < 3 && st == DT_OK; ++slot) {
      const ConvGeom &cg = k.c[slot];
      const ConvW &c = u->blk[j].c[slot];
      const int scale = slot ? pj + at_scale[slot] * cp : 0, shift = pj + at_shift[slot] * cp;
      if (slot && c.scale) wr.copy(o_par + scale, c.scale, cp);
      if (c.shift) wr.copy(o_par + shift, c.shift, cp);
      *fc[slot] = FusedConvW{(int)o_w[j][slot], scale, shift};
      if (st == DT_OK && g.has_launch(j, slot))
        st = launch_pack_fused_conv(t[kSlotWeight[slot]], wr.at(o_w[j][slot]), k.cout, cg.cin, cg.ksize * cg.ksize, cg.cin_p / 16, k.cout_p / 16,
                                    cg.split_c, cg.split_cp, s);
    }
    pj += 5 * cp;
  }
  if (st == DT_OK && hipMemsetAsync(wr.at(o_par + 4 * c0p), 0, sizeof(float) * c0p, s) != hipSuccess) st = (int)hipGetLastError();   // (enc1 has no skip-conv bias)
  u->fused_par = (int)o_par; u->fused_n_par = n_par;
  if (st != DT_OK) return st;
  FusedOp ops[kFusedMaxOps];
  u->fused_n_ops = fused_ops(m, G, ops);
  u->fused_ops_dev = reinterpret_cast<FusedOp *>(wr.at(o_ops));
  // (a synchronous copy: `ops` lives on this stack frame)
  DT_HIP_TRY(hipMemcpy(u->fused_ops_dev, ops, sizeof(FusedOp) * u->fused_n_ops, hipMemcpyHostToDevice));
  u->fused_lds = lds;
  u->fused_ok = true;
  u->fused_on = getenv("DT_NO_FUSED") == nullptr;
  return DT_OK;
}

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

// The handle frees what it owns when it goes (dt_unet.h), so every error below is a plain return.
int dt_unet_create(const dt_unet_desc *desc, const float *const *bt, const float *const *gt, void *stream,
                   dt_unet **out) {
  if (!desc || !bt || !gt || !out) return DT_E_NULL;
  UnetGeom geo;
  if (const int bad = unet_geometry(*desc, getenv("DT_NO_SHARED_ENC1") == nullptr, &geo)) return bad;
  for (int i = 0; i < DT_GT_COUNT; ++i)
    if (!gt[i]) return DT_E_NULL;
  for (int j = 0; j < kBlocks; ++j)
    for (int t = 0; t < DT_BT_COUNT; ++t) {
      const bool optional = t == DT_BT_RES_W || t == DT_BT_RES_B;   // an identity skip has no weights
      if (!bt[j * DT_BT_COUNT + t] && (!optional || geo.blk[j].has_res)) return DT_E_NULL;
    }
  hipStream_t s = (hipStream_t)stream;
  std::unique_ptr<dt_unet> u(new (std::nothrow) dt_unet());
  if (!u) return (int)hipErrorOutOfMemory;
  u->geo = geo;
  u->strip_pair = getenv("DT_NO_STRIP_PAIR") == nullptr;
  u->concat_in_place = getenv("DT_NO_CONCAT_IN_PLACE") == nullptr;
  const SlabLayout L = slab_layout(geo);
  DT_HIP_TRY(hipMalloc((void **)&u->slab, L.total * sizeof(float)));
  if (const int st = pack_slab(u.get(), L, bt, gt, s)) return st;
  if (const int st = build_fused(u.get(), bt, s)) return st;
  *out = u.release();
  return DT_OK;
}

void dt_unet_destroy(dt_unet *h) { delete h; }

int dt_unet_time_bias_stride(const dt_unet *h) { return h ? h->geo.tb_stride : DT_E_NULL; }

int dt_unet_time_bias(const dt_unet *h, const int32_t *t, const float *cond, const uint8_t *present, int rows,
                      float *out, void *stream) {
  if (!h || !t || !out) return DT_E_NULL;
  if (rows < 0) return DT_E_ARG;
  return launch_time_bias(h->tw, t, cond, present, rows, out, (hipStream_t)stream);
}

size_t dt_unet_workspace_bytes(const dt_unet *h, int batch_total, int H, int W) {
  const FwdShape sh = FwdShape::rows_only(batch_total, H, W);
  if (!h || sh.validate() != DT_OK) return 0;
  return make_plan(h->geo, sh).total * sizeof(float);
}

int dt_unet_debug_activation(const dt_unet *h, int batch_total, int H, int W, int which, size_t *off, int *cp,
                             int *oh, int *ow) {
  if (!h || !off || !cp || !oh || !ow) return DT_E_NULL;
  if (which < 0 || which > kBlocks + 3) return DT_E_ARG;
  const FwdShape sh = FwdShape::rows_only(batch_total, H, W);
  if (const int bad = sh.validate()) return bad;
  const Plan pl = make_plan(h->geo, sh);
  if (which == kBlocks) { *off = pl.slab; *cp = 0; *oh = 0; *ow = 0; return DT_OK; }   // the split-K slab (diagnostics)
  if (which > kBlocks) {   // the concat [upsampled | skip] that dec3 / dec2 / dec1 read
    const int j = which - kBlocks + 4;
    *off = pl.cat[j - 5]; *cp = h->geo.blk[j].cin_p; *oh = pl.H[j]; *ow = pl.W[j];
    return DT_OK;
  }
  *off = pl.o[which]; *cp = h->geo.blk[which].cout_p; *oh = pl.H[which]; *ow = pl.W[which];
  return DT_OK;
}

int dt_unet_set_precision(dt_unet *h, int precision) {
  if (!h) return DT_E_NULL;
  if (precision < DT_PREC_FP32 || precision > DT_PREC_AUTO) return DT_E_ARG;
  h->tuned.clear();                               // choices are per arithmetic mode: back to the heuristic plan
  h->graphs.clear();
  h->precision = precision;
  return DT_OK;
}

int dt_unet_set_head_fusion(dt_unet *h, int on) {
  if (!h) return DT_E_NULL;
  h->head_fusion = on != 0;
  h->graphs.clear();
  return DT_OK;
}

int dt_unet_set_fused(dt_unet *h, int on) {
  if (!h) return DT_E_NULL;
  h->fused_on = on != 0 && h->fused_ok;
  h->graphs.clear();
  return DT_OK;
}

int dt_unet_fused_active(const dt_unet *h, int H, int W) {
  if (!h) return DT_E_NULL;
  return use_fused(h, H, W) ? 1 : 0;
}

}  // extern "C"
