// The pair kernel of the strip convolutions (dt_conv_strip_pair.hip): the NH = 2 instantiation of the K = 32 strip form of
// the 256 x 64 tile (KIND_STRIP2: conv_strip_bf16x6_kernel<256,64,2,1>, dt_conv_strip_kernel.h), in which one workgroup of
// eight waves walks TWO adjacent tiles over one staged activation strip.  It is not a form of its own: no row in
// dt_conv_forms.h, no kind, no plan-table entry.  A resolved launch of that form is served by it where strip_pair_serves()
// says so, and computes the same bits.  What the host needs beyond the form table -- its LDS footprint, its routing rule --
// is here.
#pragma once
#include "dt_internal.h"

namespace dt {

struct StripPairForm {
  // the form each half runs as: wave layout (4 x 1 waves of 64 x 64), K = 32 steps, halo rule, epilogue stage
  static constexpr ConvForm half() { return *find_conv_form(KIND_STRIP2, 256, 64); }
  static constexpr int kNh = 2, kBm = 256, kBn = 128;       // two halves: the workgroup's tile
  static constexpr int threads() { return half().threads(kNh); }
  // ---- dynamic LDS, bf16 elements from offset 0: the strip exactly as the half's form lays it out,
  // [KC][3][zero_row + 8][16], then the weight tiles of both halves side by side, [2 stages][KC][3][128][16]
  static constexpr int weight_elems() { return 2 * half().kc * 3 * half().plane_b(kNh); }
  static constexpr size_t walk_bytes(int W) {
    return (size_t)(half().strip_elems(half().plane_a(half().zero_row(half().strip_rows(strip_halo(W, kBm))))) + weight_elems()) * 2;
  }
  // floats from offset 0 once the walk is over: half h stages its epilogue at h * half_stage_floats()
  static constexpr size_t stage_bytes(bool dup_stage2) {
    return (size_t)(half().half_stage_floats() + half().stage_floats() + (dup_stage2 ? half().copy_floats() : 0)) * 4;
  }
  static constexpr size_t lds_bytes(int W, bool dup_stage2) {
    return walk_bytes(W) > stage_bytes(dup_stage2) ? walk_bytes(W) : stage_bytes(dup_stage2);
  }
  static constexpr size_t lds_limit() { return 163840; }   // one workgroup per CU: all of its LDS
  static constexpr bool reaches(int W) { return half().reaches(W) && lds_bytes(W, true) <= lds_limit(); }
};
static_assert(StripPairForm::kBm == StripPairForm::half().bm && StripPairForm::kBn == StripPairForm::kNh * StripPairForm::half().bn, "two halves side by side");

// whether the pair kernel serves the launch p (which passed conv_admissible): the K = 32 strip form of the 256 x 64 tile on a
// layer whose N tiles pair up, at a picture width whose strip and both halves' weight tiles fit one CU's LDS
inline bool strip_pair_serves(const ConvParams &p) {
  return p.kind == KIND_STRIP2 && p.bm == 256 && p.bn == 64 && p.n_p % StripPairForm::kBn == 0 && StripPairForm::reaches(p.W);
}
int launch_conv_strip_pair(const ConvParams &p, hipStream_t s);
// launch_conv for a U-Net handle: strip_pair is the handle's switch (off with DT_NO_STRIP_PAIR=1 at create time); without
// it, as in launch_conv(p, s), every launch runs the kernel of its own form
int launch_conv(const ConvParams &p, hipStream_t s, bool strip_pair);

}  // namespace dt
