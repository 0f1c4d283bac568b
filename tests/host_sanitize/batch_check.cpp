// Host-only check of csrc/dt_batch.h (plain C++, no HIP; built with -fsanitize=address,undefined by tests/test_batch_check.py).
// The five entries that take a batch -- dt_unet_forward, dt_unet_forward_mixed, dt_sample_trajectory,
// dt_sample_trajectory_mixed, dt_sample_trajectory_masked -- each held a condition list of its own, followed by the tests at
// the head of forward_impl or sample_loop (rows, FwdShape::validate, tb_div, rows % tb_div), up to the workspace-size test.
// Those lists are kept here, in namespace `before`, as they were written: they are the expected values and must never be
// rewritten in terms of the header.  Every one is compared with the header's status function of the entry over a grid of
// arguments; the program prints how many grid points gave each status, per entry, and the number of mismatches.
#include <stdint.h>
#include <stdio.h>

#include "dt_batch.h"

namespace before {

struct dt_unet { bool share_enc1; };

struct FwdShape {
  int Bt, H, W, imgs, single;
  int validate() const {
    if (Bt < 1 || imgs < 1 || H < 16 || W < 16 || H % 16 || W % 16) return DT_E_SHAPE;
    if (single < 0 || single >= imgs || (single ? Bt != 2 * imgs - single : Bt % imgs != 0)) return DT_E_ARG;
    return DT_OK;
  }
};

// forward_impl, down to the workspace test
int forward_impl(const dt_unet *u, const float *x, int B, int n_pass, int H, int W, const float *tb, int tb_div, float *ws, int B_single = 0) {
  if (!u || !x || !tb || !ws) return DT_E_NULL;
  if (n_pass < 1 || tb_div < 1) return DT_E_SHAPE;
  const int Bt = B * n_pass - B_single * (n_pass - 1);
  const FwdShape sh{Bt, H, W, B, B_single};
  if (const int bad = sh.validate()) return bad;
  return DT_OK;
}

struct SampleArgs { int B, n_pass, B_single, H, W, tb_div; };

// sample_loop, down to the workspace test
int sample_loop(const SampleArgs &a) {
  const int B = a.B, H = a.H, W = a.W;
  const FwdShape sh{B * a.n_pass - a.B_single * (a.n_pass - 1), H, W, B, a.B_single};
  if (const int bad = sh.validate()) return bad;
  if (a.tb_div < 1 || sh.Bt % a.tb_div) return DT_E_ARG;
  return DT_OK;
}

int old_forward(const dt_unet *h, const float *x, int B, int n_pass, int H, int W, const float *tb, int tb_div, float *eps, float *ws) {
  if (!eps) return DT_E_NULL;
  return forward_impl(h, x, B, n_pass, H, W, tb, tb_div, ws);
}

int old_forward_mixed(const dt_unet *h, const float *x, int B, int B_single, int H, int W, const float *tb, int tb_div, float *eps, float *ws) {
  if (!eps || !h) return DT_E_NULL;
  if (B_single < 1 || B_single >= B || tb_div < 1 || (2 * B - B_single) % tb_div || B_single % tb_div || !h->share_enc1) return DT_E_ARG;
  return forward_impl(h, x, B, 2, H, W, tb, tb_div, ws, B_single);
}

int old_sample(const dt_unet *h, int rule, int B, int n_pass, int H, int W, int n_steps, const float *tb, const float *coef,
               const int32_t *has_noise, float *traj, void *ws) {
  if (!h || !tb || !coef || !has_noise || !traj || !ws) return DT_E_NULL;
  if (n_pass < 1 || n_pass > 2 || n_steps < 0 || rule < 0 || rule > DT_RULE_MANAGER) return DT_E_ARG;
  return sample_loop(SampleArgs{B, n_pass, 0, H, W, B});
}

int old_sample_mixed(const dt_unet *h, int rule, int B, int B_single, int H, int W, int n_steps, const float *tb, int tb_div,
                     const float *coef, const int32_t *has_noise, const float *w, float *traj, void *ws) {
  if (!h || !tb || !coef || !has_noise || !traj || !ws || !w) return DT_E_NULL;
  if (n_steps < 0 || rule < 0 || rule > DT_RULE_MANAGER || B < 2 || B_single < 1 || B_single >= B || tb_div < 1) return DT_E_ARG;
  if ((2 * B - B_single) % tb_div || B_single % tb_div || !h->share_enc1) return DT_E_ARG;   // a time-bias row never straddles the single / CFG boundary
  return sample_loop(SampleArgs{B, 2, B_single, H, W, tb_div});
}

int old_sample_masked(const dt_unet *h, int rule, int B, int n_pass, int B_single, int H, int W, int n_steps, const float *tb, int tb_div,
                      const float *coef, const int32_t *has_noise, const float *w, const float *mask, const float *known, float *traj,
                      void *ws) {
  if (!h || !tb || !coef || !has_noise || !traj || !ws || !mask || !known) return DT_E_NULL;
  if (n_pass < 1 || n_pass > 2 || n_steps < 0 || rule < 0 || rule > DT_RULE_MANAGER || tb_div < 1) return DT_E_ARG;
  if (B < 1 || B_single < 0 || B_single > B || (n_pass == 1 && B_single)) return DT_E_ARG;
  if (B_single == B) { n_pass = 1; B_single = 0; }                       // every image takes one pass
  if (B_single) {                                                        // a mixed batch: dt_sample_trajectory_mixed's conditions
    if (!w) return DT_E_NULL;
    if ((2 * B - B_single) % tb_div || B_single % tb_div || !h->share_enc1) return DT_E_ARG;
  }
  if (((uintptr_t)mask | (uintptr_t)known | (uintptr_t)traj) & 15) return DT_E_ARG;   // float4 reads of the layered update
  return sample_loop(SampleArgs{B, n_pass, B_single, H, W, tb_div});
}

}  // namespace before

// the pointers of one call; nothing is read through them
struct Ptrs {
  const before::dt_unet *h;
  float *x, *tb, *eps, *ws, *coef, *traj, *w, *mask, *known;
  int32_t *has_noise;
};

enum Entry { FORWARD, FORWARD_MIXED, SAMPLE, SAMPLE_MIXED, SAMPLE_MASKED, N_ENTRIES };
static const char *const kEntry[N_ENTRIES] = {"dt_unet_forward", "dt_unet_forward_mixed", "dt_sample_trajectory", "dt_sample_trajectory_mixed",
                                              "dt_sample_trajectory_masked"};
static const char *const kStatus[5] = {"DT_OK", "DT_E_NULL", "DT_E_SHAPE", "DT_E_ARG", "DT_E_WORKSPACE"};
static long seen[N_ENTRIES][5], points = 0, mismatches = 0;

static void expect(int entry, int got, int want, int rule, const dt::BatchSplit &b, int H, int W, int n_steps, int variant) {
  ++points;
  if (want <= 0 && want >= -4) ++seen[entry][-want];
  if (got == want) return;
  if (++mismatches <= 20)
    printf("MISMATCH %s: %d, expected %d at rule %d B %d n_pass %d B_single %d tb_div %d H %d W %d n_steps %d pointers %d\n", kEntry[entry], got,
           want, rule, b.B, b.n_pass, b.B_single, b.tb_div, H, W, n_steps, variant);
}

int main() {
  alignas(16) static float mem[16];
  static int32_t imem[4];
  static const before::dt_unet unet[2] = {{false}, {true}};
  const int rules[] = {-1, 0, 2, 3}, hw[][2] = {{16, 16}, {16, 24}, {8, 16}, {32, 48}}, steps[] = {-1, 0, 2};
  for (int share = 0; share < 2; ++share) {
    // every pointer set, each required pointer (and w) null in turn, then mask, known and traj one float off 16-byte alignment
    const Ptrs good{&unet[share], mem, mem, mem, mem, mem, mem, mem, mem, mem, imem};
    Ptrs variants[15];
    for (Ptrs &v : variants) v = good;
    variants[1].h = nullptr; variants[2].x = nullptr; variants[3].tb = nullptr; variants[4].eps = nullptr; variants[5].ws = nullptr;
    variants[6].coef = nullptr; variants[7].has_noise = nullptr; variants[8].traj = nullptr; variants[9].w = nullptr;
    variants[10].mask = nullptr; variants[11].known = nullptr;
    variants[12].mask = mem + 1; variants[13].known = mem + 1; variants[14].traj = mem + 1;
    for (int v = 0; v < 15; ++v) {
      const Ptrs &p = variants[v];
      const bool sh = p.h && p.h->share_enc1;
      for (int rule : rules)
        for (int B = 0; B <= 5; ++B)
          for (int n_pass = 0; n_pass <= 3; ++n_pass)
            for (int B_single = -1; B_single <= 6; ++B_single)
              for (int tb_div = 0; tb_div <= 6; ++tb_div)
                for (const int *s : hw)
                  for (int n_steps : steps) {
                    const int H = s[0], W = s[1];
                    const dt::BatchSplit plain{B, n_pass, 0, tb_div}, loop{B, n_pass, 0, B}, mixed{B, 2, B_single, tb_div},
                        masked{B, n_pass, B_single, tb_div};
                    expect(FORWARD, dt::forward_status(p.h, p.x, plain, H, W, p.tb, p.eps, p.ws),
                           before::old_forward(p.h, p.x, B, n_pass, H, W, p.tb, tb_div, p.eps, p.ws), rule, plain, H, W, n_steps, v);
                    expect(FORWARD_MIXED, dt::forward_mixed_status(p.h, p.x, mixed, H, W, p.tb, p.eps, p.ws, sh),
                           before::old_forward_mixed(p.h, p.x, B, B_single, H, W, p.tb, tb_div, p.eps, p.ws), rule, mixed, H, W, n_steps, v);
                    expect(SAMPLE, dt::sample_status(p.h, rule, loop, H, W, n_steps, p.tb, p.coef, p.has_noise, p.traj, p.ws),
                           before::old_sample(p.h, rule, B, n_pass, H, W, n_steps, p.tb, p.coef, p.has_noise, p.traj, p.ws), rule, loop, H, W,
                           n_steps, v);
                    expect(SAMPLE_MIXED, dt::sample_mixed_status(p.h, rule, mixed, H, W, n_steps, p.tb, p.coef, p.has_noise, p.w, p.traj, p.ws, sh),
                           before::old_sample_mixed(p.h, rule, B, B_single, H, W, n_steps, p.tb, tb_div, p.coef, p.has_noise, p.w, p.traj, p.ws),
                           rule, mixed, H, W, n_steps, v);
                    expect(SAMPLE_MASKED,
                           dt::sample_masked_status(p.h, rule, masked, H, W, n_steps, p.tb, p.coef, p.has_noise, p.w, p.mask, p.known, p.traj,
                                                    p.ws, sh),
                           before::old_sample_masked(p.h, rule, B, n_pass, B_single, H, W, n_steps, p.tb, tb_div, p.coef, p.has_noise, p.w,
                                                     p.mask, p.known, p.traj, p.ws),
                           rule, masked, H, W, n_steps, v);
                  }
    }
  }
  // ---- rows(), shape(), tb_rows() and normalised() against the expressions they replaced
  long members = 0;
  for (int B = 0; B <= 5; ++B)
    for (int n_pass = 0; n_pass <= 3; ++n_pass)
      for (int B_single = -1; B_single <= 6; ++B_single)
        for (int tb_div = 1; tb_div <= 6; ++tb_div) {
          const dt::BatchSplit b{B, n_pass, B_single, tb_div}, n = b.normalised();
          const int rows = B * n_pass - B_single * (n_pass - 1);
          int np = n_pass, bs = B_single;
          if (B_single == B) { np = 1; bs = 0; }
          const dt::FwdShape sh = b.shape(16, 32);
          const bool same = b.rows() == rows && b.tb_rows() == rows / tb_div && sh.Bt == rows && sh.H == 16 && sh.W == 32 && sh.imgs == B &&
                            sh.single == B_single && n.B == B && n.n_pass == np && n.B_single == bs && n.tb_div == tb_div;
          ++members;
          if (!same) { ++mismatches; printf("MISMATCH members at B %d n_pass %d B_single %d tb_div %d\n", B, n_pass, B_single, tb_div); }
        }
  for (int e = 0; e < N_ENTRIES; ++e) {
    printf("%s:", kEntry[e]);
    for (int st = 0; st < 5; ++st) printf(" %s %ld", kStatus[st], seen[e][st]);
    printf("\n");
  }
  printf("%s: %ld grid points, %ld member checks, %ld mismatches\n", mismatches ? "batch check FAILED" : "batch check ok", points, members, mismatches);
  return mismatches ? 1 : 0;
}
