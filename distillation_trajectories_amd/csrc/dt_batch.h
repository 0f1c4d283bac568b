// The batch of one forward / sampler call, and what the five entries that take one answer before they look at the workspace
// (dt_unet_forward, dt_unet_forward_mixed, dt_sample_trajectory, dt_sample_trajectory_mixed, dt_sample_trajectory_masked).
// Plain C++ with no HIP in it: tests/host_sanitize/batch_check.cpp compares every status function below with the condition
// list its entry held before, over a grid of arguments.  Pointers enter as const void * and are never dereferenced.
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "../../include/dt_hip.h"

namespace dt {

// One forward shape, the key of every launch plan: Bt batch rows of H x W pictures made of imgs images -- every image once
// (pass 0), then the images from `single` on a second time (pass 1), or all of them Bt / imgs times when single == 0.  The
// split is part of the key because enc1's launches run over the images, not the rows.
struct FwdShape {
  int Bt, H, W, imgs, single;
  static FwdShape rows_only(int Bt, int H, int W) { return FwdShape{Bt, H, W, Bt, 0}; }   // for what the split does not change (the workspace layout)
  bool operator==(const FwdShape &o) const { return Bt == o.Bt && H == o.H && W == o.W && imgs == o.imgs && single == o.single; }
  // DT_OK, DT_E_SHAPE (rows, images or picture size the kernels do not run) or DT_E_ARG (rows and images that do not fit together)
  int validate() const {
    if (Bt < 1 || imgs < 1 || H < 16 || W < 16 || H % 16 || W % 16) return DT_E_SHAPE;
    if (single < 0 || single >= imgs || (single ? Bt != 2 * imgs - single : Bt % imgs != 0)) return DT_E_ARG;
    return DT_OK;
  }
};

// B images; the first B_single of them take one pass, the others n_pass (B_single > 0 needs n_pass == 2): rows
// [pass 0 of all B images | pass 1 of images B_single .. B-1].  tb_div rows in a row share one time-bias row.
struct BatchSplit {
  int B, n_pass, B_single, tb_div;
  int rows() const { return B * n_pass - B_single * (n_pass - 1); }
  FwdShape shape(int H, int W) const { return FwdShape{rows(), H, W, B, B_single}; }
  int tb_rows() const { return rows() / tb_div; }   // time-bias rows of one forward
  // every image takes one pass: the one-pass batch it is
  BatchSplit normalised() const { return B_single == B ? BatchSplit{B, 1, 0, tb_div} : *this; }
  // a mixed batch the kernels run: some but not all images take one pass, a time-bias row never straddles the single / CFG
  // boundary, and enc1 runs in the shared formulation (the only one that has mixed batches)
  bool mixed_ok(bool share_enc1) const {
    return n_pass == 2 && B_single >= 1 && B_single < B && tb_div >= 1 && rows() % tb_div == 0 && B_single % tb_div == 0 && share_enc1;
  }
};

inline bool any_null(std::initializer_list<const void *> ptrs) {
  for (const void *p : ptrs)
    if (!p) return true;
  return false;
}

inline bool loop_counts_ok(int rule, int n_steps) { return n_steps >= 0 && rule >= 0 && rule <= DT_RULE_MANAGER; }

// what the sampler loop itself asks of its batch, after the entry's own tests
inline int loop_status(const BatchSplit &b, int H, int W) {
  if (const int bad = b.shape(H, W).validate()) return bad;
  if (b.tb_div < 1 || b.rows() % b.tb_div) return DT_E_ARG;
  return DT_OK;
}

// ---- one function per entry: the status the entry returns before it sizes the workspace, the tests in the entry's order

// dt_unet_forward (rows that tb_div does not divide are the fused path's to refuse: the layered path runs them)
inline int forward_status(const void *h, const void *x, const BatchSplit &b, int H, int W, const void *tb, const void *eps, const void *ws) {
  if (any_null({eps, h, x, tb, ws})) return DT_E_NULL;
  if (b.n_pass < 1 || b.tb_div < 1) return DT_E_SHAPE;
  return b.shape(H, W).validate();
}

// dt_unet_forward_mixed: the batch is judged before x, tb and ws are looked at
inline int forward_mixed_status(const void *h, const void *x, const BatchSplit &b, int H, int W, const void *tb, const void *eps, const void *ws,
                                bool share_enc1) {
  if (any_null({eps, h})) return DT_E_NULL;
  if (!b.mixed_ok(share_enc1)) return DT_E_ARG;
  if (any_null({x, tb, ws})) return DT_E_NULL;
  return b.shape(H, W).validate();
}

// dt_sample_trajectory (b.tb_div == b.B: one time-bias row per pass)
inline int sample_status(const void *h, int rule, const BatchSplit &b, int H, int W, int n_steps, const void *tb, const void *coef,
                         const void *has_noise, const void *traj, const void *ws) {
  if (any_null({h, tb, coef, has_noise, traj, ws})) return DT_E_NULL;
  if (b.n_pass < 1 || b.n_pass > 2 || !loop_counts_ok(rule, n_steps)) return DT_E_ARG;
  return loop_status(b, H, W);
}

// dt_sample_trajectory_mixed
inline int sample_mixed_status(const void *h, int rule, const BatchSplit &b, int H, int W, int n_steps, const void *tb, const void *coef,
                               const void *has_noise, const void *w, const void *traj, const void *ws, bool share_enc1) {
  if (any_null({h, tb, coef, has_noise, traj, ws, w})) return DT_E_NULL;
  if (!loop_counts_ok(rule, n_steps) || !b.mixed_ok(share_enc1)) return DT_E_ARG;
  return loop_status(b, H, W);
}

// dt_sample_trajectory_masked, b as the caller gave it: a batch whose images all take one pass is judged as normalised()
inline int sample_masked_status(const void *h, int rule, const BatchSplit &b, int H, int W, int n_steps, const void *tb, const void *coef,
                                const void *has_noise, const void *w, const void *mask, const void *known, const void *traj, const void *ws,
                                bool share_enc1) {
  if (any_null({h, tb, coef, has_noise, traj, ws, mask, known})) return DT_E_NULL;
  if (b.n_pass < 1 || b.n_pass > 2 || !loop_counts_ok(rule, n_steps) || b.tb_div < 1) return DT_E_ARG;
  if (b.B < 1 || b.B_single < 0 || b.B_single > b.B || (b.n_pass == 1 && b.B_single)) return DT_E_ARG;
  const BatchSplit n = b.normalised();
  if (n.B_single) {
    if (!w) return DT_E_NULL;
    if (!n.mixed_ok(share_enc1)) return DT_E_ARG;
  }
  if (((uintptr_t)mask | (uintptr_t)known | (uintptr_t)traj) & 15) return DT_E_ARG;   // float4 reads of the layered update
  return loop_status(n, H, W);
}

}  // namespace dt
