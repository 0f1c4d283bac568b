// The strip kernel for TWO adjacent 256 x 64 tiles at once (NH = 2, dt_conv_strip_kernel.h) in a code object of its own,
// and its launcher.  Routing and LDS footprint: dt_conv_strip_pair.h.
#include "dt_conv_strip_kernel.h"
#include "dt_conv_strip_pair.h"

namespace dt {

constexpr ConvForm kHalf = StripPairForm::half();
static void (*const kPairKernel)(ConvParams) = conv_strip_bf16x6_kernel<kHalf.bm, kHalf.bn, kHalf.kc, kHalf.wk, StripPairForm::kNh>;

// p passed conv_admissible and strip_pair_serves
int launch_conv_strip_pair(const ConvParams &p_in, hipStream_t s) {
  ConvParams p = p_in;
  p.dup_stage2 = p.n_dup == 2 && p.pool_out;                       // a second epilogue stage behind each half's first
  const size_t lds = StripPairForm::lds_bytes(p.W, p.dup_stage2);
  static const LdsLimit limit = {reinterpret_cast<const void *>(kPairKernel), StripPairForm::lds_limit()};
  static LdsLimitOnce lds_limit;
  if (const int st = lds_limit.raise(&limit, 1)) return st;
  kPairKernel<<<dim3((p.M + p.bm - 1) / p.bm, p.n_p / StripPairForm::kBn, p.splits), StripPairForm::threads(), lds, s>>>(p);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace dt
