// Host-only check of csrc/dt_conv_forms.h (plain C++, no HIP; built with -fsanitize=address,undefined by
// tests/test_conv_forms.py).  For every form of the table and every picture width 1..64 the members of ConvForm are
// compared with the expressions the launch rules and the strip launcher held before the table existed.  Those are kept
// here, in namespace `before`, as they were written (strip_kc, strip_lds_bytes, strip_lds_limit, kind_has_tile, the width
// tests of conv_admissible, rows1 / rows2 / need of launch_conv_strip, epilogue_stage_floats): they are the expected
// values and must never be rewritten in terms of the header.  sizeof(__bf16) is spelled sizeof(bf16_t).
// The same for conv_real_channel, the padded-channel map of the weight packs: pack_conv_kernel, pack_conv_bf16x3_kernel and
// pack_fused_conv_kernel each spelled it out (before::channel_fp32 / channel_bf16x3 / channel_fused, verbatim); for every
// cin in 1..130 and every concat split of it the map over a pack's padded channels hits each real channel exactly once.
#include <stdint.h>
#include <stdio.h>

#include "dt_conv_forms.h"

namespace before {

typedef uint16_t bf16_t;
enum ConvKind { KIND_FP32 = 0, KIND_BF16 = 1, KIND_STRIP = 3, KIND_STRIP2 = 4, KIND_STRIPK = 5 };
inline bool is_strip(int kind) { return kind >= KIND_STRIP; }
inline int strip_halo(int W, int bm) { return bm % W == 0 ? W : W + 1; }

int strip_kc(int kind, int bm, int bn) { return kind == KIND_STRIPK ? (bm == 64 && bn == 64 ? 4 : 2) : (kind == KIND_STRIP2 ? 2 : 1); }

size_t strip_lds_bytes(int W, int bm, int bn, int kind) {
  const int kc = strip_kc(kind, bm, bn);
  const int R = bm + 2 * strip_halo(W, bm);
  const size_t loop = (size_t)kc * ((size_t)3 * (((R + 7) & ~7) + 8) * 16 + (kind == KIND_STRIPK ? 0 : (size_t)2 * 3 * bn * 16)) * sizeof(bf16_t);
  const size_t stage = (size_t)(bm == 256 || (kind == KIND_STRIPK && bn == 64) ? 128 : 64) * (bn + 4) * sizeof(float);
  return loop > stage ? loop : stage;
}

inline size_t strip_lds_limit(int kind) { return kind == KIND_STRIP ? 65536u : 98304u; }

bool strip_reaches(int W) { return W + 1 <= 64 && strip_lds_bytes(W, 64, 64, KIND_STRIP) <= strip_lds_limit(KIND_STRIP); }

static bool kind_has_tile(int kind, int bm, int bn) {
  if (kind < KIND_FP32 || kind > KIND_STRIPK || kind == 2) return false;
  if ((bm != 64 && bm != 128 && !(bm == 256 && bn == 64 && is_strip(kind))) || (bn != 64 && bn != 128)) return false;
  return !(kind == KIND_STRIPK && (bm > 128 || (bm == 128 && bn == 128)));
}

// conv_admissible: `if (kc == 4 && p.W + 1 > 32) return DT_E_SHAPE;` and `if (p.W + 1 > 64) return DT_E_SHAPE;`
bool width_in_reach(int kc, int W) { return !(kc == 4 && W + 1 > 32) && !(W + 1 > 64); }

// launch_conv_strip, the second epilogue stage
struct Stages { size_t rows1, rows2, need; };
Stages stages(int kind, int bm, int bn) {
  const int kc = strip_kc(kind, bm, bn);
  const size_t rows1 = bm == 256 || kc == 4 || (kind == KIND_STRIPK && bm == 128) ? 128 : 64;   // WK * WM * 32
  const size_t rows2 = bm == 256 ? 128 : (bm == 128 ? 64 : 32);                                 // WM * 32
  const size_t need = (rows1 + (kind == KIND_STRIPK ? rows2 : rows1)) * (bn + 4) * sizeof(float);
  return {rows1, rows2, need};
}

// dt_conv_epilogue.h, the two GEMM kernels' stage (WM = 2)
constexpr int epilogue_stage_floats(int BN, int WM = 2) { return WM * 32 * (BN + 4); }

// pack_conv_kernel (dt_conv.hip), cp in [0, cin_p)
int channel_fp32(int cp, int cin, int split_c, int split_cp) {
  int c = -1;
  if (cp < split_cp) { if (cp < split_c) c = cp; }
  else { const int cc = split_c + (cp - split_cp); if (cc < cin) c = cc; }
  return c;
}
// pack_conv_bf16x3_kernel (dt_conv_bf16.hip), cp in [0, cin_w)
int channel_bf16x3(int cp, int cin, int cin_p, int split_c, int split_cp) {
  int c = -1;
  if (cp < split_cp) { if (cp < split_c) c = cp; }
  else if (cp < cin_p) { const int cc = split_c + (cp - split_cp); if (cc < cin) c = cc; }
  return c;
}
// pack_fused_conv_kernel (dt_fused.hip), cp in [0, kc * 16) = [0, cin_p)
int channel_fused(int cp, int cin, int split_c, int split_cp) {
  int ci;
  if (cp < split_cp) ci = cp < split_c ? cp : -1;
  else ci = cp - split_cp + split_c < cin ? cp - split_cp + split_c : -1;
  return ci;
}

}  // namespace before

static long checks = 0, failures = 0;
#define EXPECT_EQ(got, want, ...)                                                     \
  do {                                                                                \
    ++checks;                                                                         \
    if ((long long)(got) != (long long)(want)) {                                      \
      ++failures;                                                                     \
      printf("MISMATCH %s = %lld, expected %lld at ", #got, (long long)(got), (long long)(want)); \
      printf(__VA_ARGS__);                                                            \
      printf("\n");                                                                   \
    }                                                                                 \
  } while (0)

int main() {
  using namespace dt;
  // ---- which (kind, bm, bn) exist; every row is found under its own key (no duplicates)
  int found = 0;
  const int bms[] = {64, 96, 128, 256}, bns[] = {64, 128};
  for (int kind = 0; kind <= 6; ++kind)
    for (int bm : bms)
      for (int bn : bns) {
        const ConvForm *f = find_conv_form(kind, bm, bn);
        EXPECT_EQ(f != nullptr, before::kind_has_tile(kind, bm, bn), "kind %d tile %d x %d", kind, bm, bn);
        found += f != nullptr;
      }
  const int rows = (int)(sizeof(kConvForms) / sizeof(kConvForms[0]));
  EXPECT_EQ(rows, 21, "rows of the table");
  EXPECT_EQ(found, rows, "rows reached by find_conv_form");
  for (const ConvForm &f : kConvForms) {
    EXPECT_EQ(find_conv_form(f.kind, f.bm, f.bn) == &f, 1, "kind %d tile %d x %d is listed once", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.cls >= 0 && f.cls < KC_CONV_COUNT, 1, "class of kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(is_strip(f.kind), before::is_strip(f.kind), "kind %d", f.kind);
    EXPECT_EQ(f.wm() * f.wn() * f.wk, 4, "four waves, kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.mi() * 32 * f.wm(), f.bm, "rows of kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.ni() * 32 * f.wn(), f.bn, "columns of kind %d tile %d x %d", f.kind, f.bm, f.bn);
    if (!is_strip(f.kind)) {
      EXPECT_EQ(f.kc, 1, "kind %d", f.kind);
      EXPECT_EQ(f.wk, 1, "kind %d", f.kind);
      EXPECT_EQ(f.wm(), 2, "kind %d", f.kind);
      EXPECT_EQ(f.stage_floats(), before::epilogue_stage_floats(f.bn), "kind %d tile %d x %d", f.kind, f.bm, f.bn);
      continue;
    }
    // ---- strip forms
    const before::Stages st = before::stages(f.kind, f.bm, f.bn);
    EXPECT_EQ(f.kc, before::strip_kc(f.kind, f.bm, f.bn), "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.kc % f.wk, 0, "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.lds_limit(), before::strip_lds_limit(f.kind), "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.needs_lds_attribute(), f.kind != before::KIND_STRIP, "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.stage_rows(), st.rows1, "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.stage_bytes(), st.rows1 * (f.bn + 4) * sizeof(float), "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.copy_rows(), f.kind == before::KIND_STRIPK ? st.rows2 : st.rows1, "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.dup_stage_bytes(), st.need, "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(f.dup_stage_bytes() <= f.lds_limit(), st.need <= before::strip_lds_limit(f.kind), "kind %d tile %d x %d", f.kind, f.bm, f.bn);
    EXPECT_EQ(2 * (f.bm + 2 * (f.max_w() + 1)) <= f.ap() * 256, 1, "staging reach of kind %d tile %d x %d", f.kind, f.bm, f.bn);
    for (int W = 1; W <= 64; ++W) {
      const size_t want = before::strip_lds_bytes(W, f.bm, f.bn, f.kind);
      const bool fits = want <= before::strip_lds_limit(f.kind), reach = before::width_in_reach(before::strip_kc(f.kind, f.bm, f.bn), W);
      EXPECT_EQ(f.lds_bytes(W), want, "kind %d tile %d x %d W %d", f.kind, f.bm, f.bn, W);
      EXPECT_EQ(f.lds_bytes(W) <= f.lds_limit(), fits, "kind %d tile %d x %d W %d", f.kind, f.bm, f.bn, W);
      EXPECT_EQ(W <= f.max_w(), reach, "kind %d tile %d x %d W %d", f.kind, f.bm, f.bn, W);
      EXPECT_EQ(f.reaches(W), fits && reach, "kind %d tile %d x %d W %d", f.kind, f.bm, f.bn, W);
      // the kernel's carve-up stays inside what the host allocates: strip, then weights; stage copies; the second stage
      const int plane_a = f.plane_a(f.zero_row(f.strip_rows(strip_halo(W, f.bm))));
      EXPECT_EQ(strip_halo(W, f.bm), before::strip_halo(W, f.bm), "W %d bm %d", W, f.bm);
      EXPECT_EQ((size_t)(f.strip_elems(plane_a) + f.weight_elems()) * 2 <= f.lds_bytes(W), 1, "kind %d tile %d x %d W %d", f.kind, f.bm, f.bn, W);
      EXPECT_EQ((size_t)f.wk * f.copy_floats() * 4 <= f.lds_bytes(W), 1, "kind %d tile %d x %d W %d", f.kind, f.bm, f.bn, W);
    }
  }
  for (int W = 1; W <= 64; ++W)
    EXPECT_EQ(find_conv_form(KIND_STRIP, 64, 64)->reaches(W), before::strip_reaches(W), "strip_reaches(%d)", W);
  // ---- the padded-channel map: a plain input (split_c == cin) and every concat split of cin channels, padded as
  // dt_unet_create pads them (each tensor to 16 channels, the split-bf16 pack to 64 per tap)
  for (int cin = 1; cin <= 130; ++cin)
    for (int split_c = 1; split_c <= cin; ++split_c) {
      const int pad16 = 16, pad64 = 64;
      const int split_cp = (split_c + pad16 - 1) / pad16 * pad16;
      const int cin_p = split_c == cin ? split_cp : split_cp + (cin - split_c + pad16 - 1) / pad16 * pad16;
      const int cin_w = (cin_p + pad64 - 1) / pad64 * pad64;
      int hits[130] = {0};
      long outside = 0;
      for (int cp = 0; cp < cin_w; ++cp) {
        const int c = conv_real_channel(cp, cin, cin_p, split_c, split_cp);
        if (c >= 0 && c < cin) ++hits[c];
        else outside += c != -1;
        EXPECT_EQ(c, before::channel_bf16x3(cp, cin, cin_p, split_c, split_cp), "bf16x3 pack, cin %d split %d cp %d", cin, split_c, cp);
        if (cp < cin_p) {
          EXPECT_EQ(c, before::channel_fp32(cp, cin, split_c, split_cp), "fp32 pack, cin %d split %d cp %d", cin, split_c, cp);
          EXPECT_EQ(c, before::channel_fused(cp, cin, split_c, split_cp), "fused pack, cin %d split %d cp %d", cin, split_c, cp);
        } else {
          EXPECT_EQ(c, -1, "zero chunk, cin %d split %d cp %d", cin, split_c, cp);
        }
      }
      EXPECT_EQ(outside, 0, "values other than a real channel or -1, cin %d split %d", cin, split_c);
      for (int c = 0; c < cin; ++c) EXPECT_EQ(hits[c], 1, "real channel %d of cin %d split %d", c, cin, split_c);
    }
  printf("%s: %ld checks, %ld mismatches\n", failures ? "conv forms FAILED" : "conv forms ok", checks, failures);
  return failures ? 1 : 0;
}
