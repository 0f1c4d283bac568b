// Host-only check of csrc/dt_unet_layout.h (plain C++, no HIP; built with -fsanitize=address,undefined by
// tests/test_unet_layout.py).  The channel geometry of the eight blocks, the offsets of the handle's weight slab and the
// workspace plan of a forward were written inside dt_unet_create and make_plan, between the allocations and the launches.
// That text is kept here, in namespace `before`, as it was written (the device pointers, the null tests and the launches
// taken out; the offsets that were locals of dt_unet_create gathered in a struct): it gives the expected values and must never
// be rewritten in terms of the header.  Over a grid of models and forward shapes every geometry field, every slab offset and
// every Plan member is compared with the header's; the program prints the number of comparisons and of mismatches.
// Independently of the old text, every region of both layouts (as the header's Bump logs them) must start on a 256-byte
// boundary, lie inside the total and be disjoint from every other, and every offset the layouts name must be such a region.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "dt_unet_layout.h"

namespace before {

constexpr int kChanPad = 16;
constexpr int kNPad = 64;
constexpr int kBlocks = 8;
constexpr int kChunkPad = 4;
constexpr int kSplitMaxRows = 32768;
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int pack_chunks(int cin_p) { return round_up(cin_p, 16 * kChunkPad) >> 4; }

struct FwdShape { int Bt, H, W, imgs, single; };

struct ConvW {
  int cin, cin_p;
  int split_c, split_cp;
  int cin_w;
  int ksize;
};

struct BlockW {
  int cin, cout;
  int cin_p, cout_p, n_p;
  int split_c, split_cp;
  bool has_res;
  ConvW c[3];
  int tb_off;
};

struct dt_unet {
  bool share_enc1 = true;
  int tb_cols = 0;
  dt_unet_desc desc;
  BlockW blk[kBlocks];
  int cp[4];
  int tb_stride;
  size_t slab_floats;
};

struct Bump {
  size_t off = 0;
  size_t take(size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; }   // 256-B aligned
};

struct Plan {
  size_t h[kBlocks], r[kBlocks], o[kBlocks];   // conv1 out, skip out, block out
  size_t pool[4], cat[3];
  size_t slab, lowres;                         // split-K partial sums; low-resolution head output
  size_t total;
  int H[kBlocks], W[kBlocks];                  // spatial size of each block
};

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

bool has_launch(const dt_unet *u, int j, int slot) { return slot == 2 || (j > 0 && (slot == 1 || u->blk[j].has_res)); }

// the locals of dt_unet_create that held the slab offsets
struct Offsets {
  struct { size_t w, wb, ss; } o_c[kBlocks][3] = {};
  size_t o_w3 = 0;
  size_t o_w2t, o_wt, o_bt, o_w1g, o_b1g, o_wc0, o_bc0, o_wc2, o_bc2, o_fr, o_fw, o_fb;
  int half;
};

// dt_unet_create, from its shape tests down to the hipMalloc of the slab; share_enc1 stands for the DT_NO_SHARED_ENC1 test
int create(const dt_unet_desc *desc, bool share_enc1, dt_unet *u, Offsets &O) {
  if (desc->channels < 1 || desc->channels > 3 || desc->temb_dim < 2) return DT_E_SHAPE;
  for (int i = 0; i < 4; ++i)
    if (desc->dims[i] < 1) return DT_E_SHAPE;
  u->desc = *desc;
  const int C = desc->channels, D = desc->temb_dim;
  const int *d = desc->dims;
  for (int i = 0; i < 4; ++i) u->cp[i] = round_up(d[i], kChanPad);
  // (cin, cout) and the concat split of the eight blocks -- models.py:138-154
  const int cin[kBlocks] = {C, d[0], d[1], d[2], d[3], d[3] + d[3], d[2] + d[2], d[1] + d[1]};
  const int cout[kBlocks] = {d[0], d[1], d[2], d[3], d[3], d[2], d[1], d[0]};
  const int up_c[kBlocks] = {0, 0, 0, 0, 0, d[3], d[2], d[1]};   // channels coming from the upsampled branch
  Bump bump;
  auto &o_c = O.o_c;
  size_t &o_w3 = O.o_w3;
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
    for (int slot = 0; slot < 3; ++slot) {
      ConvW &c = k.c[slot];
      c = slot == 2 ? ConvW{k.cout, k.cout_p, k.cout, k.cout_p, 0, 0} : ConvW{k.cin, k.cin_p, k.split_c, k.split_cp, 0, 0};
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
  u->share_enc1 = share_enc1;
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
  O.o_w2t = o_w2t; O.o_wt = o_wt; O.o_bt = o_bt; O.o_w1g = o_w1g; O.o_b1g = o_b1g; O.o_wc0 = o_wc0; O.o_bc0 = o_bc0;
  O.o_wc2 = o_wc2; O.o_bc2 = o_bc2; O.o_fr = o_fr; O.o_fw = o_fw; O.o_fb = o_fb; O.half = half;
  return DT_OK;
}

}  // namespace before

namespace {

long long g_compared = 0, g_mismatches = 0, g_region_faults = 0;

template <class A, class B>
void same(const char *what, A a, B b, const dt_unet_desc &d, int share, int j = -1, int slot = -1) {
  ++g_compared;
  if ((long long)a == (long long)b) return;
  if (++g_mismatches <= 20)
    printf("MISMATCH %s: before %lld, header %lld (channels %d dims %d %d %d %d temb %d share_enc1 %d block %d slot %d)\n", what,
           (long long)a, (long long)b, d.channels, d.dims[0], d.dims[1], d.dims[2], d.dims[3], d.temb_dim, share, j, slot);
}

typedef std::vector<std::pair<size_t, size_t>> Log;

// every logged region on a 256-byte boundary, inside the total, disjoint from the others; every named offset a logged region
void regions_ok(const char *what, Log log, size_t total, const std::vector<size_t> &named) {
  auto fault = [&](const char *why, size_t a, size_t b) {
    if (++g_region_faults <= 20) printf("REGION %s: %s (%zu, %zu; total %zu)\n", what, why, a, b, total);
  };
  if (log.size() != named.size()) fault("the layout names another number of regions than it takes", log.size(), named.size());
  for (const size_t off : named) {
    bool found = false;
    for (const auto &r : log) found = found || r.first == off;
    if (!found) fault("a named offset is no region", off, 0);
  }
  std::sort(log.begin(), log.end());
  for (size_t i = 0; i < log.size(); ++i) {
    if (log[i].first * sizeof(float) % 256) fault("not on a 256-byte boundary", log[i].first, log[i].second);
    if (log[i].first + log[i].second > total) fault("ends beyond the total", log[i].first, log[i].second);
    if (i + 1 < log.size() && log[i].second > 0 && log[i].first + log[i].second > log[i + 1].first) fault("overlaps the next region", log[i].first, log[i + 1].first);
  }
}

}  // namespace

int main() {
  const int dims[][4] = {
      {16, 32, 32, 32}, {32, 64, 64, 64}, {38, 76, 76, 76}, {51, 102, 102, 102}, {64, 128, 128, 128}, {128, 256, 256, 256},   // size factors 0.1, 0.25, 0.3, 0.4, 0.5, 1.0
      {13, 29, 51, 100}, {100, 51, 29, 13}, {20, 40, 72, 136},                                                              // not multiples of 16
      {16, 16, 16, 16}, {3, 3, 3, 3}, {1, 1, 1, 1}, {48, 48, 96, 96}, {24, 40, 40, 80}};                                    // equal neighbours: identity skips
  const int tembs[] = {2, 7, 64, 128};
  const int rows[] = {1, 2, 5, 41, 82, 512, 4096};
  const int pics[][2] = {{16, 16}, {16, 48}, {48, 16}, {32, 32}, {64, 64}};
  long long models = 0, shapes = 0, res_true = 0, res_false = 0, split_below = 0, split_above = 0, share_on = 0, share_off = 0;

  for (int C = 1; C <= 3; ++C)
    for (const auto &dm : dims)
      for (const int D : tembs)
        for (int share = 0; share <= 1; ++share) {
          const dt_unet_desc desc{C, {dm[0], dm[1], dm[2], dm[3]}, D};
          before::dt_unet old{};
          before::Offsets O;
          dt::UnetGeom g{};
          const int st_old = before::create(&desc, share != 0, &old, O);
          const int st_new = dt::unet_geometry(desc, share != 0, &g);
          same("status", st_old, st_new, desc, share);
          if (st_old != DT_OK || st_new != DT_OK) continue;
          ++models;
          ++(share ? share_on : share_off);
          // ---- geometry
          same("share_enc1", old.share_enc1, g.share_enc1, desc, share);
          same("tb_cols", old.tb_cols, g.tb_cols, desc, share);
          same("tb_stride", old.tb_stride, g.tb_stride, desc, share);
          same("desc.channels", old.desc.channels, g.desc.channels, desc, share);
          same("desc.temb_dim", old.desc.temb_dim, g.desc.temb_dim, desc, share);
          for (int i = 0; i < 4; ++i) {
            same("cp", old.cp[i], g.cp[i], desc, share, i);
            same("desc.dims", old.desc.dims[i], g.desc.dims[i], desc, share, i);
          }
          for (int j = 0; j < dt::kBlocks; ++j) {
            const before::BlockW &a = old.blk[j];
            const dt::BlockGeom &b = g.blk[j];
            same("cin", a.cin, b.cin, desc, share, j); same("cout", a.cout, b.cout, desc, share, j);
            same("cin_p", a.cin_p, b.cin_p, desc, share, j); same("cout_p", a.cout_p, b.cout_p, desc, share, j);
            same("n_p", a.n_p, b.n_p, desc, share, j);
            same("split_c", a.split_c, b.split_c, desc, share, j); same("split_cp", a.split_cp, b.split_cp, desc, share, j);
            same("has_res", a.has_res, b.has_res, desc, share, j); same("tb_off", a.tb_off, b.tb_off, desc, share, j);
            if (j > 0) ++(a.has_res ? res_true : res_false);
            for (int slot = 0; slot < 3; ++slot) {
              same("c.cin", a.c[slot].cin, b.c[slot].cin, desc, share, j, slot);
              same("c.cin_p", a.c[slot].cin_p, b.c[slot].cin_p, desc, share, j, slot);
              same("c.split_c", a.c[slot].split_c, b.c[slot].split_c, desc, share, j, slot);
              same("c.split_cp", a.c[slot].split_cp, b.c[slot].split_cp, desc, share, j, slot);
              same("c.cin_w", a.c[slot].cin_w, b.c[slot].cin_w, desc, share, j, slot);
              same("c.ksize", a.c[slot].ksize, b.c[slot].ksize, desc, share, j, slot);
              same("has_launch", before::has_launch(&old, j, slot), g.has_launch(j, slot), desc, share, j, slot);
            }
          }
          same("skip_block(5)", 8 - 5, dt::skip_block(5), desc, share); same("skip_block(6)", 8 - 6, dt::skip_block(6), desc, share);
          same("skip_block(7)", 8 - 7, dt::skip_block(7), desc, share);
          // ---- the weight slab
          Log slab_log;
          const dt::SlabLayout L = dt::slab_layout(g, &slab_log);
          std::vector<size_t> named;
          for (int j = 0; j < dt::kBlocks; ++j)
            for (int slot = 0; slot < 3; ++slot) {
              same("slab c.w", O.o_c[j][slot].w, L.c[j][slot].w, desc, share, j, slot);
              same("slab c.wb", O.o_c[j][slot].wb, L.c[j][slot].wb, desc, share, j, slot);
              same("slab c.ss", O.o_c[j][slot].ss, L.c[j][slot].ss, desc, share, j, slot);
              const bool conv = g.has_launch(j, slot);
              if (conv || (j == 0 && slot == 1)) named.push_back(L.c[j][slot].w);
              if (conv) named.push_back(L.c[j][slot].wb);
              if (conv || slot == 1) named.push_back(L.c[j][slot].ss);
            }
          same("slab w3", O.o_w3, L.w3, desc, share); same("slab w2t", O.o_w2t, L.w2t, desc, share);
          same("slab wt", O.o_wt, L.wt, desc, share); same("slab bt", O.o_bt, L.bt, desc, share);
          same("slab w1g", O.o_w1g, L.w1g, desc, share); same("slab b1g", O.o_b1g, L.b1g, desc, share);
          same("slab wc0", O.o_wc0, L.wc0, desc, share); same("slab bc0", O.o_bc0, L.bc0, desc, share);
          same("slab wc2", O.o_wc2, L.wc2, desc, share); same("slab bc2", O.o_bc2, L.bc2, desc, share);
          same("slab fr", O.o_fr, L.fr, desc, share); same("slab fw", O.o_fw, L.fw, desc, share);
          same("slab fb", O.o_fb, L.fb, desc, share); same("slab half", O.half, L.half, desc, share);
          same("slab total", old.slab_floats, L.total, desc, share);
          if (g.blk[0].has_res) named.push_back(L.w3);
          if (g.share_enc1) named.push_back(L.w2t);
          for (const size_t off : {L.wt, L.bt, L.w1g, L.b1g, L.wc0, L.bc0, L.wc2, L.bc2, L.fr, L.fw, L.fb}) named.push_back(off);
          regions_ok("slab", slab_log, L.total, named);
          // ---- the workspace plan
          for (const int Bt : rows)
            for (const auto &hw : pics) {
              ++shapes;
              const before::Plan a = before::make_plan(&old, before::FwdShape{Bt, hw[0], hw[1], Bt, 0});
              Log plan_log;
              const dt::Plan b = dt::make_plan(g, dt::FwdShape::rows_only(Bt, hw[0], hw[1]), &plan_log);
              std::vector<size_t> pn;
              for (int j = 0; j < dt::kBlocks; ++j) {
                same("plan h", a.h[j], b.h[j], desc, share, j); same("plan r", a.r[j], b.r[j], desc, share, j);
                same("plan o", a.o[j], b.o[j], desc, share, j);
                same("plan H", a.H[j], b.H[j], desc, share, j); same("plan W", a.W[j], b.W[j], desc, share, j);
                // "the input buffer of block j", as forward_impl's `cur` chain, dt_unet_autotune and dt_unet_time_conv spelled it
                same("plan input", j == 0 ? a.h[0] : (j <= 4 ? a.pool[j - 1] : a.cat[j - 5]), b.input(j), desc, share, j);
                pn.push_back(b.h[j]); pn.push_back(b.o[j]);
                if (j > 0) pn.push_back(b.input(j));
                if (j > 0 && g.blk[j].has_res) pn.push_back(b.r[j]);
                if (j > 0) ++((long long)Bt * b.H[j] * b.W[j] <= dt::kSplitMaxRows ? split_below : split_above);
              }
              for (int i = 0; i < 4; ++i) same("plan pool", a.pool[i], b.pool[i], desc, share, i);
              for (int i = 0; i < 3; ++i) same("plan cat", a.cat[i], b.cat[i], desc, share, i);
              same("plan slab", a.slab, b.slab, desc, share); same("plan lowres", a.lowres, b.lowres, desc, share);
              same("plan total", a.total, b.total, desc, share);
              pn.push_back(b.slab); pn.push_back(b.lowres);
              regions_ok("plan", plan_log, b.total, pn);
            }
        }
  // descriptions no model has: the status alone
  const dt_unet_desc bad[] = {{0, {16, 32, 32, 32}, 64}, {4, {16, 32, 32, 32}, 64}, {3, {16, 32, 32, 32}, 1}, {3, {0, 32, 32, 32}, 64},
                              {3, {16, 32, 32, -1}, 64}, {3, {16, 32, 0, 32}, 64}};
  long long refused = 0;
  for (const dt_unet_desc &desc : bad) {
    before::dt_unet old{};
    before::Offsets O;
    dt::UnetGeom g{};
    const int st_old = before::create(&desc, true, &old, O);
    same("status", st_old, dt::unet_geometry(desc, true, &g), desc, 1);
    if (st_old == DT_E_SHAPE) ++refused;
  }
  printf("models %lld  forward shapes %lld  refused descriptions %lld\n", models, shapes, refused);
  printf("blocks 1..7: has_res true %lld  has_res false %lld\n", res_true, res_false);
  printf("blocks 1..7 of a shape: rows at most kSplitMaxRows %lld  above %lld\n", split_below, split_above);
  printf("share_enc1: on %lld  off %lld\n", share_on, share_off);
  printf("compared %lld values: %lld mismatches, %lld region faults\n", g_compared, g_mismatches, g_region_faults);
  if (g_mismatches || g_region_faults) return 1;
  printf("unet layout check ok\n");
  return 0;
}
