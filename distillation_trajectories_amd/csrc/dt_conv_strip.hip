// The strip convolution's forms (dt_conv_forms.h) as compiled kernels, and their launcher.  The kernel itself:
// dt_conv_strip_kernel.h.
#include <vector>

#include "dt_conv_strip_kernel.h"

namespace dt {

#define DT_STRIP_ROW(cls, kind, bm, bn, kc, wk) {{kind, bm, bn, kc, wk, cls}, conv_strip_bf16x6_kernel<bm, bn, kc, wk>},
static const ConvKernel kStripKernels[] = {DT_CONV_FORMS_ALL_STRIP(DT_STRIP_ROW)};

// The forms with more than one chunk per step take up to 96 KB of dynamic LDS (128x128: 80 KB)
static int strip_lds_attribute() {
  static const std::vector<LdsLimit> limits = [] {
    std::vector<LdsLimit> v;
    for (const ConvKernel &k : kStripKernels)
      if (k.form.needs_lds_attribute()) v.push_back({reinterpret_cast<const void *>(k.fn), k.form.lds_limit()});
    return v;
  }();
  static LdsLimitOnce once;
  return once.raise(limits.data(), limits.size());
}

// p passed conv_admissible (dt_conv.hip): a full 3x3 walk whose tile, chunk groups and LDS footprint the form supports
int launch_conv_strip(const ConvParams &p_in, hipStream_t s) {
  ConvParams p = p_in;
  const ConvKernel &k = conv_kernel_of(kStripKernels, p);
  size_t lds = k.form.lds_bytes(p.W);
  // a second epilogue stage behind the first (and its K-split copies), if it fits this launch's LDS class
  p.dup_stage2 = p.n_dup == 2 && p.pool_out && k.form.dup_stage_bytes() <= k.form.lds_limit();
  if (p.dup_stage2 && k.form.dup_stage_bytes() > lds) lds = k.form.dup_stage_bytes();
  if (const int st = k.form.needs_lds_attribute() ? strip_lds_attribute() : DT_OK) return st;
  k.fn<<<dim3((p.M + p.bm - 1) / p.bm, p.n_p / p.bn, p.splits), 256, lds, s>>>(p);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace dt
