// Host-side walk of include/dt_hip_cka.h under AddressSanitizer and UndefinedBehaviorSanitizer: the workspace arithmetic and
// every argument error of the three entry points.  All of them return before any HIP call, so the program needs no GPU.
// Built by csrc/build.py::build_cka_sanitizer_driver from csrc/dt_cka.hip and this file alone (host code instrumented);
// run by tests/test_cka_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/dt_hip_cka.h"
#define EXPECT(expr, want) do { long long g = (long long)(expr); if (g != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #expr, g, (long long)(want)); ++bad; } } while (0)
int main() {
  int bad = 0;
  std::vector<double> buf(64);
  void *p = buf.data();
  float *f = (float *)p; double *d = (double *)p; int *i = (int *)p;
  for (int n : {4, 5, 64, 65, 130, 2048}) for (int pm : {1, 3, 1023, 1024, 1025, 32768, 1 << 24}) {
    const size_t nt = (size_t)(n + 63) / 64, tiles = nt * (nt + 1) / 2, slab = tiles * 4096 * 8;
    const size_t head = ((size_t)pm * 8 + 255) / 256 * 256, slabs = ((size_t)pm + DT_CKA_SLAB - 1) / DT_CKA_SLAB;
    const size_t least = dt_cka_min_workspace_bytes(n, pm), full = dt_cka_workspace_bytes(1, n, pm);
    EXPECT(least, head + slab);
    if (full < least || (full - head) % slab || (full - head) / slab > slabs || full % 16) { std::printf("FAIL ws %d %d\n", n, pm); ++bad; }
    EXPECT(dt_cka_workspace_bytes(DT_CKA_MAX_LAYERS, n, pm), full);
  }
  EXPECT(dt_cka_workspace_bytes(0, 8, 8), 0);
  EXPECT(dt_cka_workspace_bytes(DT_CKA_MAX_LAYERS + 1, 8, 8), 0);
  EXPECT(dt_cka_workspace_bytes(1, 3, 8), 0);
  EXPECT(dt_cka_workspace_bytes(1, DT_CKA_MAX_N + 1, 8), 0);
  EXPECT(dt_cka_workspace_bytes(1, 8, 0), 0);
  EXPECT(dt_cka_workspace_bytes(1, 8, DT_CKA_MAX_P + 1), 0);
  EXPECT(dt_cka_min_workspace_bytes(3, 8), 0);
  EXPECT(dt_cka_min_workspace_bytes(8, -1), 0);
  const float *base[2] = {f, f};
  long long rs[2] = {8, 8};
  int groups[2] = {1, 2}, c[2] = {8, 3}, pitch[2] = {8, 4};
  const size_t big = 1 << 20;
  EXPECT(dt_cka_gram(nullptr, rs, groups, c, pitch, 2, 4, d, d, i, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, 4, nullptr, d, i, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, 4, d, d, i, nullptr, big, nullptr), DT_E_NULL);
  { const float *hole[2] = {f, nullptr}; EXPECT(dt_cka_gram(hole, rs, groups, c, pitch, 2, 4, d, d, i, p, big, nullptr), DT_E_NULL); }
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 0, 4, d, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, 3, d, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, DT_CKA_MAX_N + 1, d, d, i, p, big, nullptr), DT_E_SHAPE);
  { int wide[2] = {8, 5}; EXPECT(dt_cka_gram(base, rs, groups, wide, pitch, 2, 4, d, d, i, p, big, nullptr), DT_E_SHAPE); }       // c > pitch
  { int none[2] = {1, 0}; EXPECT(dt_cka_gram(base, rs, none, c, pitch, 2, 4, d, d, i, p, big, nullptr), DT_E_SHAPE); }
  { int many[2] = {1, 1 << 23}; EXPECT(dt_cka_gram(base, rs, many, c, pitch, 2, 4, d, d, i, p, big, nullptr), DT_E_SHAPE); }   // groups * c > 2^24
  { long long back[2] = {8, -8}; EXPECT(dt_cka_gram(base, back, groups, c, pitch, 2, 4, d, d, i, p, big, nullptr), DT_E_SHAPE); }
  { const float *odd[2] = {f, (const float *)((char *)p + 2)}; EXPECT(dt_cka_gram(odd, rs, groups, c, pitch, 2, 4, d, d, i, p, big, nullptr), DT_E_ARG); }
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, 4, (double *)((char *)p + 4), d, i, p, big, nullptr), DT_E_ARG);
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, 4, d, d, i, (char *)p + 8, big, nullptr), DT_E_ARG);
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, 4, d, d, i, p, dt_cka_min_workspace_bytes(4, 8) - 1, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_cka_gram(base, rs, groups, c, pitch, 2, 4, d, d, i, p, 0, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_cka_scores(nullptr, d, i, 1, d, d, i, 1, 4, d, d, nullptr, nullptr), DT_E_NULL);
  EXPECT(dt_cka_scores(d, d, i, 1, d, d, i, 1, 4, d, nullptr, nullptr, nullptr), DT_E_NULL);
  EXPECT(dt_cka_scores(d, d, i, 0, d, d, i, 1, 4, d, d, nullptr, nullptr), DT_E_SHAPE);
  EXPECT(dt_cka_scores(d, d, i, 1, d, d, i, DT_CKA_MAX_LAYERS + 1, 4, d, d, nullptr, nullptr), DT_E_SHAPE);
  EXPECT(dt_cka_scores(d, d, i, 1, d, d, i, 1, 3, d, d, nullptr, nullptr), DT_E_SHAPE);
  EXPECT(dt_cka_scores(d, d, i, 1, d, d, i, 1, 4, d, d, (double *)((char *)p + 4), nullptr), DT_E_ARG);
  EXPECT(dt_cka(nullptr, rs, groups, c, pitch, 2, d, d, i, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 4, d, d, nullptr, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_cka(base, rs, groups, c, pitch, 2, d, d, i, base, rs, groups, c, pitch, 2, nullptr, d, i, 4, d, d, nullptr, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_cka(base, rs, groups, c, pitch, 2, d, d, i, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 4, nullptr, d, nullptr, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_cka(base, rs, groups, c, pitch, 2, d, d, i, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 3, d, d, nullptr, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_cka(base, rs, groups, c, pitch, 2, d, d, i, base, rs, groups, c, pitch, 65, d, d, i, 4, d, d, nullptr, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_cka(base, rs, groups, c, pitch, 2, d, d, i, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 4, d, d, nullptr, p, 16, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_cka(base, rs, groups, c, pitch, 2, d, d, i, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 4, d, d, nullptr, (char *)p + 4, big, nullptr), DT_E_ARG);
  std::printf(bad ? "%d failures\n" : "cka host checks clean (%d)\n", bad);
  return bad != 0;
}
