// The forms of a convolution launch: every (kind, tile) that is compiled, and everything that follows from one -- wave
// layout, strip staging, dynamic LDS and its carve-up, launch bounds, profiler class.  The kernels take their constants
// from a form, the launch rules and the launchers (dt_conv.hip, dt_conv_bf16.hip, dt_conv_strip.hip) read the same table.
// A new form is one row below, plus its kernel code if the layout is new.  No HIP here: plain C++14 `constexpr`, which
// host and device code (and the host-only check tests/host_sanitize/conv_forms_check.cpp) evaluate alike.
#pragma once
#include <stddef.h>

namespace dt {

// Launch kinds of a convolution.  The numbers are part of the ABI (dt_unet_conv_choice / dt_unet_set_conv_choice, the plan
// table plans/gfx950.json); 2 (round 1's LDS-DMA variant) is retired and rejected.
enum ConvKind {
  KIND_FP32 = 0,     // exact fp32 MFMA implicit GEMM (conv_gemm_kernel)
  KIND_BF16 = 1,     // split-bf16 implicit GEMM (conv_gemm_bf16x6_kernel)
  KIND_STRIP = 3,    // split-bf16 strip kernel (full 3x3 walks): one 16-channel chunk per step
  KIND_STRIP2 = 4,   // strip kernel, two chunks (K = 32) per step
  KIND_STRIPK = 5,   // strip kernel, the step's chunks split across the waves (tiles below 128 x 128)
};
constexpr bool is_strip(int kind) { return kind >= KIND_STRIP; }

// Halo rows either side of a strip tile.  The corner taps reach W + 1 pixels back / ahead; when the tile starts at x = 0 and
// ends at x = W - 1 (BM a multiple of W) those two reads are out-of-picture taps of the first / last row and go to the
// zero rows anyway, so W rows are enough -- which is what lets the K = 32 tile fit twice per CU at W = 16.
constexpr int strip_halo(int W, int bm) { return bm % W == 0 ? W : W + 1; }

// The padded-channel map of every weight pack: the real input channel behind padded channel cp of a tap, or -1 where cp is
// padding.  The activations' channels are padded to 16 per tensor and a decoder block reads the concat of two tensors, so
// real channels [0, split_c) live at [0, split_c) and real channels [split_c, cin) from split_cp on (split_c == cin,
// split_cp == cin_p without a concat); the zero chunks [cin_p, cin_w) of a split-bf16 pack (ConvParams::ccw) are padding too.
constexpr int conv_real_channel(int cp, int cin, int cin_p, int split_c, int split_cp) {
  return cp < split_cp ? (cp < split_c ? cp : -1) : (cp < cin_p && split_c + (cp - split_cp) < cin ? split_c + (cp - split_cp) : -1);
}

// Profiler classes of the convolution launches (KernelClass, dt_internal.h, continues the numbering).  The benchmark groups
// kernels by their printed names: their number and order are fixed.
enum ConvClass {
  KC_CONV_128x128 = 0, KC_CONV_128x64, KC_CONV_64x128, KC_CONV_64x64,
  KC_CONVB_128x128, KC_CONVB_128x64, KC_CONVB_64x128, KC_CONVB_64x64,
  KC_CONVS_128x128, KC_CONVS_128x64, KC_CONVS_64x128, KC_CONVS_64x64, KC_CONVS_256x64, KC_CONVS_K128x64, KC_CONVS_K64x64, KC_CONVS_K64x128,
  KC_CONV_COUNT
};

// X(profiler class, kind, BM, BN, KC, WK).  KC = 16-channel chunks per step, WK = waves that split them (strip kernel,
// conv_strip_bf16x6_kernel<BM, BN, KC, WK>; 1, 1 for the two GEMM kernels).  A KIND_STRIP2 form shares the class of the
// KIND_STRIP form of its tile.  (The kernels of a code object are emitted in the order of its rows.)
#define DT_CONV_FORMS_FP32(X)                    \
  X(KC_CONV_128x128, KIND_FP32, 128, 128, 1, 1)  \
  X(KC_CONV_128x64, KIND_FP32, 128, 64, 1, 1)    \
  X(KC_CONV_64x128, KIND_FP32, 64, 128, 1, 1)    \
  X(KC_CONV_64x64, KIND_FP32, 64, 64, 1, 1)
#define DT_CONV_FORMS_BF16(X)                    \
  X(KC_CONVB_128x128, KIND_BF16, 128, 128, 1, 1) \
  X(KC_CONVB_128x64, KIND_BF16, 128, 64, 1, 1)   \
  X(KC_CONVB_64x128, KIND_BF16, 64, 128, 1, 1)   \
  X(KC_CONVB_64x64, KIND_BF16, 64, 64, 1, 1)
#define DT_CONV_FORMS_STRIPK(X)                   \
  X(KC_CONVS_K64x128, KIND_STRIPK, 64, 128, 2, 2) \
  X(KC_CONVS_K64x64, KIND_STRIPK, 64, 64, 4, 4)   \
  X(KC_CONVS_K128x64, KIND_STRIPK, 128, 64, 2, 2)
#define DT_CONV_FORMS_STRIP2(X)                    \
  X(KC_CONVS_256x64, KIND_STRIP2, 256, 64, 2, 1)   \
  X(KC_CONVS_128x128, KIND_STRIP2, 128, 128, 2, 1) \
  X(KC_CONVS_128x64, KIND_STRIP2, 128, 64, 2, 1)   \
  X(KC_CONVS_64x128, KIND_STRIP2, 64, 128, 2, 1)   \
  X(KC_CONVS_64x64, KIND_STRIP2, 64, 64, 2, 1)
#define DT_CONV_FORMS_STRIP(X)                    \
  X(KC_CONVS_256x64, KIND_STRIP, 256, 64, 1, 1)   \
  X(KC_CONVS_128x128, KIND_STRIP, 128, 128, 1, 1) \
  X(KC_CONVS_128x64, KIND_STRIP, 128, 64, 1, 1)   \
  X(KC_CONVS_64x128, KIND_STRIP, 64, 128, 1, 1)   \
  X(KC_CONVS_64x64, KIND_STRIP, 64, 64, 1, 1)
#define DT_CONV_FORMS_ALL_STRIP(X) DT_CONV_FORMS_STRIPK(X) DT_CONV_FORMS_STRIP2(X) DT_CONV_FORMS_STRIP(X)

// Four wave64 per workgroup, WM x WN x WK over (rows, columns, the step's chunks); each wave holds MI x NI accumulator
// tiles of 32 x 32.  The members below are the only place these facts are computed.
struct ConvForm {
  int kind, bm, bn, kc, wk, cls;

  // 2 x 2 over the tile; 4 x 1 for the 256 x 64 tile (64 x 64 wave tiles on layers with 64 output channels); with the K
  // split every wave keeps a 64 x 64 tile, WM x WN x WK
  constexpr int wn() const { return wk > 1 ? bn / 64 : (bm == 256 ? 1 : 2); }
  constexpr int wm() const { return 4 / (wn() * wk); }
  constexpr int mi() const { return bm / (32 * wm()); }
  constexpr int ni() const { return bn / (32 * wn()); }
  constexpr int kw() const { return kc / wk; }                       // chunks of a step one wave multiplies

  // ---- strip staging: AP items (strip row, k-half) per thread of 256 cover the tile and its halo on rows of at most
  // max_w() pixels.  The limit is stated, not derived: the KC = 4 form stops at 31 although rows of 32 pixels (halo 32)
  // would fit its one item per thread.
  constexpr int ap() const { return bm == 256 ? 3 : (kc == 4 ? 1 : 2); }
  constexpr int max_w() const { return kc == 4 ? 31 : 63; }

  // ---- dynamic LDS of a strip launch, in the order the kernel lays it out.  bf16 elements from offset 0: the strip,
  // [KC][3 planes][zero_row + 8][16] -- the tile's rows and a halo either side, then zero rows from the next multiple of 8
  // on; then the weight tiles [2][KC][3][BN][16], absent with the K split (those waves take their fragments from global
  // memory).  Each part is a function of the one before, so that the kernel derives its offsets by the same steps.
  constexpr int strip_rows(int halo) const { return bm + 2 * halo; }
  constexpr int zero_row(int rows) const { return (rows + 7) & ~7; }
  constexpr int plane_a(int zero_row) const { return (zero_row + 8) * 16; }
  constexpr int plane_b() const { return bn * 16; }
  constexpr int strip_elems(int plane_a) const { return kc * 3 * plane_a; }
  constexpr int weight_elems() const { return wk > 1 ? 0 : 2 * kc * 3 * plane_b(); }
  // Floats from offset 0 again, once the walk is over: the epilogue stage, one copy of WM * 32 rows per K-split wave
  // (the same copies hold the partial tiles where they meet before a fused skip walk), at a pitch of BN + 4; behind
  // them the second stage of a two-pass epilogue (ConvParams::dup_stage2), one copy.
  constexpr int pitch() const { return bn + 4; }
  constexpr int copy_rows() const { return wm() * 32; }
  constexpr int stage_rows() const { return wk * copy_rows(); }
  constexpr int copy_floats() const { return copy_rows() * pitch(); }
  constexpr int stage_floats() const { return stage_rows() * pitch(); }
  constexpr size_t walk_bytes(int W) const { return (size_t)(strip_elems(plane_a(zero_row(strip_rows(strip_halo(W, bm))))) + weight_elems()) * 2; }
  constexpr size_t stage_bytes() const { return (size_t)stage_floats() * 4; }
  constexpr size_t lds_bytes(int W) const { return walk_bytes(W) > stage_bytes() ? walk_bytes(W) : stage_bytes(); }
  constexpr size_t dup_stage_bytes() const { return (size_t)(stage_floats() + copy_floats()) * 4; }   // both stages of a two-pass epilogue
  // what a launch may take: 64 KB at three waves per SIMD (KC = 1), 96 KB (two workgroups per CU) at two
  constexpr size_t lds_limit() const { return kc == 1 ? 65536u : 98304u; }
  constexpr int waves_per_simd() const { return kc == 1 ? 3 : 2; }   // the strip kernel's __launch_bounds__
  constexpr bool needs_lds_attribute() const { return lds_limit() > 65536; }   // above what a kernel may take by default
  // whether a strip form runs on picture rows of W pixels (staging reach, LDS)
  constexpr bool reaches(int W) const { return W <= max_w() && lds_bytes(W) <= lds_limit(); }

  // ---- a strip workgroup that walks NH adjacent N tiles of the form over ONE staged strip (conv_strip_bf16x6_kernel's NH,
  // dt_conv_strip_kernel.h; NH = 2 is the pair kernel, dt_conv_strip_pair.h): 256 threads per half, all of them stage the
  // strip, the halves' weight tiles lie side by side, and each half has an epilogue stage of its own, far enough from
  // the next for the second stage of a two-pass epilogue whether the launch has one or not.  Kernel and launcher both
  // read these.
  constexpr int threads(int nh) const { return 256 * nh; }
  constexpr int ap(int nh) const { return nh == 1 ? ap() : (2 * (bm + 2 * (max_w() + 1)) + threads(nh) - 1) / threads(nh); }
  constexpr int plane_b(int nh) const { return plane_b() * nh; }
  constexpr int half_stage_floats() const { return stage_floats() + copy_floats(); }
};

#define DT_X(cls, kind, bm, bn, kc, wk) {kind, bm, bn, kc, wk, cls},
constexpr ConvForm kConvForms[] = {DT_CONV_FORMS_FP32(DT_X) DT_CONV_FORMS_BF16(DT_X) DT_CONV_FORMS_ALL_STRIP(DT_X)};
#undef DT_X

// the form of a launch choice, or nullptr where (kind, bm, bn) is not compiled
constexpr const ConvForm *find_conv_form(int kind, int bm, int bn) {
  for (const ConvForm &f : kConvForms)
    if (f.kind == kind && f.bm == bm && f.bn == bn) return &f;
  return nullptr;
}
// some form of the tile bm x bn with the K split wk: nothing else decides the wave layout and the epilogue stage
constexpr const ConvForm *find_conv_layout(int bm, int bn, int wk) {
  for (const ConvForm &f : kConvForms)
    if (f.bm == bm && f.bn == bn && f.wk == wk) return &f;
  return nullptr;
}
// the form behind conv_strip_bf16x6_kernel<bm, bn, kc, wk> (an instantiation outside the table does not compile)
constexpr const ConvForm *find_strip_form(int bm, int bn, int kc, int wk) {
  for (const ConvForm &f : kConvForms)
    if (is_strip(f.kind) && f.bm == bm && f.bn == bn && f.kc == kc && f.wk == wk) return &f;
  return nullptr;
}

}  // namespace dt
