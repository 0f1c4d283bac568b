// Sampler noise on the device (include/dt_hip_rng.h): the torch CPU generator's stream, bit for bit.
//   mt19937_words_kernel  one workgroup per stream walks an mt19937 held in LDS and writes tempered words;
//   normal_kernel         the wide part: torch's vectorised Box-Muller over those words, one thread per pair (j, j + 8).
// The arithmetic of the transform is a pinned sequence of single fp32 operations and fused multiply-adds (the pairing the
// AVX512 build of torch 2.10 compiles ATen/native/cpu/avx_mathfun.h to: the capability the recorded vectors come from).
// Contraction is switched off for the file, whatever the build flags say, every fused pair is an explicit fmaf, and
// everything else is a plain operator, which then rounds once.
// (HIP's __fmul_rn / __fadd_rn are header inlines compiled with contraction on, so they are not used: see dt_update.hip.)
// fp32 denormals are kept (the default of the HIP compiler for gfx950; csrc/build.py FLAGS must not flush them): reduced
// arguments next to the octant boundaries are tiny.
#include "dt_internal.h"
#include "../../include/dt_hip_rng.h"

#pragma clang fp contract(off)

namespace dt {

constexpr int kMtN = DT_RNG_STATE_WORDS, kMtM = 397;
constexpr int kMaxStreams = 1 << 20, kMaxElements = 1 << 30;
constexpr long long kChunkWords = 16ll << 20;   // word rows of one dt_rng_randn chunk: 64 MiB, unless one draw per stream needs more
constexpr long long kMaxUnits = 1ll << 30;      // 64-pair wave units of one normal_kernel launch (32-bit index arithmetic)
constexpr long long kMaxB = (1ll << 31) - 1;    // inner draw count B (32-bit, with the unit limit: b0 + draw < 2^32)

struct WordsArgs {
  const uint64_t *seeds;
  const uint32_t *state_in;
  const int32_t *pos_in;
  long long skip, n, pitch;
  uint32_t *words, *state_out;
  int32_t *pos_out;
};

// the next block of 624 words in place.  Word i needs old i, i + 1 and i + 397 mod 624: span [0, 227) reads only old words,
// [227, 454) the new words of the first span and old ones, [454, 624) new words of the second span, old ones and the new word 0.
// Within a span every thread reads before any thread writes.
__device__ inline void mt_regenerate(uint32_t *st, int tid) {
  const int lo[3] = {0, 227, 454}, cnt[3] = {227, 227, 170};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    uint32_t v = 0;
    const int i = lo[k] + tid;
    if (tid < cnt[k]) {
      const int i1 = i + 1 == kMtN ? 0 : i + 1, im = i + kMtM >= kMtN ? i + kMtM - kMtN : i + kMtM;
      const uint32_t y = (st[i] & 0x80000000u) | (st[i1] & 0x7fffffffu);
      v = st[im] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    __syncthreads();
    if (tid < cnt[k]) st[i] = v;
    __syncthreads();
  }
}

__device__ inline uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__global__ __launch_bounds__(256) void mt19937_words_kernel(WordsArgs a) {
  __shared__ uint32_t st[kMtN];
  const int tid = threadIdx.x;
  const size_t s = blockIdx.x;
  int pos = kMtN;
  if (a.state_in) {
    for (int i = tid; i < kMtN; i += 256) st[i] = a.state_in[s * kMtN + i];
    pos = a.pos_in[s];
    pos = pos < 0 ? 0 : (pos > kMtN ? kMtN : pos);
  } else if (tid == 0) {   // init_genrand: a chain of 623 dependent steps
    uint32_t x = (uint32_t)a.seeds[s];
    st[0] = x;
    for (int i = 1; i < kMtN; ++i) {
      x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
      st[i] = x;
    }
  }
  __syncthreads();
  long long skip = a.skip, done = 0;   // uniform over the workgroup, like pos
  uint32_t *out = a.words + s * (size_t)a.pitch;
  while (skip > 0 || done < a.n) {
    if (pos == kMtN) {
      mt_regenerate(st, tid);
      pos = 0;
    }
    const int avail = kMtN - pos;
    if (skip > 0) {
      const int take = skip < avail ? (int)skip : avail;
      pos += take;
      skip -= take;
      continue;
    }
    const int take = a.n - done < avail ? (int)(a.n - done) : avail;
    for (int i = tid; i < take; i += 256) out[done + i] = mt_temper(st[pos + i]);   // done + i < n <= pitch
    pos += take;
    done += take;
  }
  if (a.state_out) {
    __syncthreads();
    for (int i = tid; i < kMtN; i += 256) a.state_out[s * kMtN + i] = st[i];
    if (tid == 0) a.pos_out[s] = pos;
  }
}

// log256_ps of avx_mathfun.h for x > 0
__device__ inline float rng_log(float x) {
  x = fmaxf(x, __uint_as_float(0x00800000u));
  const uint32_t bits = __float_as_uint(x);
  float e = (float)((int)(bits >> 23) - 0x7f);
  x = __uint_as_float((bits & 0x807fffffu) | 0x3f000000u);
  e = e + 1.0f;
  const bool small = x < 0.707106781186547524f;
  const float tmp = small ? x : 0.0f;
  x = x - 1.0f;
  e = e - (small ? 1.0f : 0.0f);
  x = x + tmp;
  const float z = x * x;
  float y = 7.0376836292E-2f;
  y = __builtin_fmaf(y, x, -1.1514610310E-1f);
  y = __builtin_fmaf(y, x, 1.1676998740E-1f);
  y = __builtin_fmaf(y, x, -1.2420140846E-1f);
  y = __builtin_fmaf(y, x, 1.4249322787E-1f);
  y = __builtin_fmaf(y, x, -1.6668057665E-1f);
  y = __builtin_fmaf(y, x, 2.0000714765E-1f);
  y = __builtin_fmaf(y, x, -2.4999993993E-1f);
  y = __builtin_fmaf(y, x, 3.3333331174E-1f);
  y = y * x;
  const float eq1 = e * -2.12194440e-4f;
  y = __builtin_fmaf(y, z, eq1);
  const float zh = z * 0.5f;
  y = y - zh;
  x = x + y;
  return __builtin_fmaf(e, 0.693359375f, x);
}

// sincos256_ps of avx_mathfun.h
__device__ inline void rng_sincos(float x, float &sn, float &cs) {
  uint32_t sign_sin = __float_as_uint(x) & 0x80000000u;
  x = __uint_as_float(__float_as_uint(x) & 0x7fffffffu);
  float y = x * 1.27323954473516f;
  int j = (int)y;                 // truncation, as cvttps
  j = (j + 1) & ~1;
  y = (float)j;
  sign_sin ^= (uint32_t)(j & 4) << 29;
  const bool poly = (j & 2) == 0;
  const uint32_t sign_cos = (uint32_t)(~(j - 2) & 4) << 29;
  x = __builtin_fmaf(y, -0.78515625f, x);
  x = __builtin_fmaf(y, -2.4187564849853515625e-4f, x);
  x = __builtin_fmaf(y, -3.77489497744594108e-8f, x);
  const float z = x * x;
  float c = 2.443315711809948E-005f;
  c = __builtin_fmaf(c, z, -1.388731625493765E-003f);
  c = __builtin_fmaf(c, z, 4.166664568298827E-002f);
  c = c * z;
  const float zh = z * 0.5f;
  c = __builtin_fmaf(c, z, -zh);
  c = c + 1.0f;
  float s = -1.9515295891E-4f;
  s = __builtin_fmaf(s, z, 8.3321608736E-3f);
  s = __builtin_fmaf(s, z, -1.6666654611E-1f);
  s = s * z;
  s = __builtin_fmaf(s, x, x);
  // the selection of the header, with its additions of zero
  const float ysin2 = poly ? s : 0.0f, ysin1 = poly ? 0.0f : c;
  const float s2 = s - ysin2, c2 = c - ysin1;
  const float xs = ysin1 + ysin2, xc = c2 + s2;
  sn = __uint_as_float(__float_as_uint(xs) ^ sign_sin);
  cs = __uint_as_float(__float_as_uint(xc) ^ sign_cos);
}

// two normals from the words of a pair (j, j + 8): normal_fill_16 of ATen with mean 0, std 1
__device__ inline void rng_pair(uint32_t w1, uint32_t w2, float &n1, float &n2) {
  const float u1 = 1.0f - (float)(w1 & 0xffffffu) * 5.9604644775390625e-08f;   // 2^-24
  const float u2 = (float)(w2 & 0xffffffu) * 5.9604644775390625e-08f;
  const float m = -2.0f * rng_log(u1);
  const float r = (float)__builtin_sqrt((double)m);   // correctly rounded in fp32: the fp64 root carries 53 >= 2 * 24 + 2 bits
  const float theta = 6.283185307179586f * u2;
  float sn, cs;
  rng_sincos(theta, sn, cs);
  n1 = r * cs + 0.0f;   // fma(n, 1, 0): a zero comes out as +0
  n2 = r * sn + 0.0f;
}

struct NormalArgs {
  const uint32_t *words;
  long long pitch;
  unsigned streams, nd, cpd;   // streams and draws per stream of this launch, 64-pair units per draw
  unsigned groups8;            // 8 * (E / 16): pairs of the full groups; the tail's 8 pairs follow
  int E, W, tail;
  long long a0;                // (a, b) of the launch's first draw
  unsigned b0, B;              // B <= kMaxB, draws <= kMaxUnits: b0 + draw fits 32 bits
  float *out;
  long long ss, sa, sb;
};

__global__ __launch_bounds__(256) void normal_kernel(NormalArgs p) {
  const unsigned u = blockIdx.x * 4u + (threadIdx.x >> 6);   // < kMaxUnits + 4
  const unsigned df = u / p.cpd, chunk = u - df * p.cpd;
  const unsigned s = df / p.nd, dl = df - s * p.nd;
  if (s >= p.streams) return;
  const unsigned pr = chunk * 64u + (threadIdx.x & 63);
  const unsigned pairs = p.groups8 + (p.tail ? 8u : 0u);
  if (pr >= pairs) return;
  const unsigned bb = p.b0 + dl, q = bb / p.B;
  const long long a = p.a0 + q, b = bb - q * p.B;
  const uint32_t *row = p.words + (size_t)s * (size_t)p.pitch + (size_t)dl * (size_t)p.W;
  int e0, i0;
  bool st0 = true, st1 = true;
  if (pr < p.groups8) {
    e0 = i0 = (int)((pr >> 3) * 16u + (pr & 7u));
    if (p.tail) {   // the last 16 elements belong to the tail words
      st0 = e0 < p.E - 16;
      st1 = e0 + 8 < p.E - 16;
    }
  } else {
    const int k = (int)(pr - p.groups8);
    i0 = p.E + k;
    e0 = p.E - 16 + k;
  }
  if (!st0 && !st1) return;
  float n1, n2;
  rng_pair(row[i0], row[i0 + 8], n1, n2);   // i0 + 8 < W
  float *o = p.out + s * p.ss + a * p.sa + b * p.sb;
  if (st0) o[e0] = n1;
  if (st1) o[e0 + 8] = n2;   // e0 + 8 < E
}

static inline long long words_per_draw(int E) { return E % 16 ? (long long)E + 16 : (long long)E; }

static int check_start(const uint64_t *seeds, const uint32_t *state_in, const int32_t *pos_in, const uint32_t *state_out,
                       const int32_t *pos_out, int S) {
  if (!seeds && !state_in) return DT_E_NULL;
  if (state_in && !pos_in) return DT_E_NULL;
  if ((state_out == nullptr) != (pos_out == nullptr)) return DT_E_NULL;
  if (S < 1 || S > kMaxStreams) return DT_E_ARG;
  return DT_OK;
}

static int launch_words(const WordsArgs &a, int S, hipStream_t s) {
  mt19937_words_kernel<<<S, 256, 0, s>>>(a);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

static inline long long units_per_draw(int E) { return (8ll * (E / 16) + (E % 16 ? 8 : 0) + 63) / 64; }

// draws [d0, d0 + nd) of every stream, the word rows starting at draw d0; S * nd * units_per_draw(E) <= kMaxUnits, B <= kMaxB
static int launch_normal(const uint32_t *words, long long pitch, int S, long long d0, long long nd, long long B, int E, float *out,
                         long long ss, long long sa, long long sb, hipStream_t s) {
  NormalArgs p;
  p.words = words;
  p.pitch = pitch;
  p.streams = (unsigned)S;
  p.nd = (unsigned)nd;
  p.cpd = (unsigned)units_per_draw(E);
  p.groups8 = 8u * (unsigned)(E / 16);
  p.E = E;
  p.W = (int)words_per_draw(E);
  p.tail = E % 16 != 0;
  p.a0 = d0 / B;
  p.b0 = (unsigned)(d0 % B);
  p.B = (unsigned)B;
  p.out = out;
  p.ss = ss, p.sa = sa, p.sb = sb;
  const long long units = (long long)S * nd * p.cpd;
  normal_kernel<<<(unsigned)((units + 3) / 4), 256, 0, s>>>(p);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

static int check_normal(int S, long long A, long long B, int E) {
  if (E < 16 || E > kMaxElements) return DT_E_ARG;
  if (S < 0 || S > kMaxStreams || A < 0 || B < 0 || B > kMaxB) return DT_E_ARG;
  if (A > 0 && B > (1ll << 62) / A) return DT_E_ARG;
  if ((long long)S * units_per_draw(E) > kMaxUnits) return DT_E_ARG;   // one draw per stream is the least a launch covers
  return DT_OK;
}

extern "C" int dt_rng_mt19937_words(const uint64_t *seeds, const uint32_t *state_in, const int32_t *pos_in, int S, long long skip,
                                    long long n, uint32_t *words, long long word_pitch, uint32_t *state_out, int32_t *pos_out,
                                    void *stream) {
  if (int rc = check_start(seeds, state_in, pos_in, state_out, pos_out, S)) return rc;
  if (skip < 0 || n < 0 || word_pitch < n) return DT_E_ARG;
  if (n > 0 && !words) return DT_E_NULL;
  return launch_words(WordsArgs{seeds, state_in, pos_in, skip, n, word_pitch, words, state_out, pos_out}, S, (hipStream_t)stream);
}

extern "C" int dt_rng_normal_from_words(const uint32_t *words, long long word_pitch, int S, long long A, long long B, int E,
                                        float *out, long long stride_s, long long stride_a, long long stride_b, void *stream) {
  if (int rc = check_normal(S, A, B, E)) return rc;
  if (S == 0 || A == 0 || B == 0) return DT_OK;
  if (A * B > kMaxUnits / ((long long)S * units_per_draw(E))) return DT_E_ARG;   // one launch
  if (!words || !out) return DT_E_NULL;
  if (A * B > (1ll << 62) / words_per_draw(E) || word_pitch < A * B * words_per_draw(E)) return DT_E_ARG;
  return launch_normal(words, word_pitch, S, 0, A * B, B, E, out, stride_s, stride_a, stride_b, (hipStream_t)stream);
}

// workspace: [S][624] running states, [S] positions, then the word rows of a chunk
static inline size_t state_block_bytes(int S) { return (size_t)S * (kMtN + 1) * sizeof(uint32_t); }

extern "C" size_t dt_rng_workspace_bytes(int S, long long draws, int E) {
  if (S < 1 || S > kMaxStreams || draws < 0 || E < 16 || E > kMaxElements) return 0;
  const long long W = words_per_draw(E);
  long long per = kChunkWords / ((long long)S * W);   // draws per stream and chunk
  per = per < 1 ? 1 : per;
  per = per > draws ? (draws < 1 ? 1 : draws) : per;
  return state_block_bytes(S) + (size_t)S * (size_t)per * (size_t)W * sizeof(uint32_t);
}

extern "C" int dt_rng_randn(const uint64_t *seeds, const uint32_t *state_in, const int32_t *pos_in, int S, long long skip, long long A,
                            long long B, int E, float *out, long long stride_s, long long stride_a, long long stride_b,
                            uint32_t *state_out, int32_t *pos_out, void *workspace, size_t workspace_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_start(seeds, state_in, pos_in, state_out, pos_out, S)) return rc;
  if (int rc = check_normal(S, A, B, E)) return rc;
  if (skip < 0) return DT_E_ARG;
  const long long W = words_per_draw(E), draws = A * B;
  if (draws > (1ll << 62) / W) return DT_E_ARG;
  if (draws == 0) {   // no workspace needed; a pure skip still moves the end state
    if (!state_out) return DT_OK;
    return launch_words(WordsArgs{seeds, state_in, pos_in, skip, 0, 0, nullptr, state_out, pos_out}, S, s);
  }
  if (!out) return DT_E_NULL;
  if (!workspace || ((uintptr_t)workspace & 3)) return workspace ? DT_E_ARG : DT_E_NULL;
  const size_t row_bytes = (size_t)S * (size_t)W * sizeof(uint32_t);
  if (workspace_bytes < state_block_bytes(S) + row_bytes) return DT_E_WORKSPACE;
  uint32_t *run_state = (uint32_t *)workspace;
  int32_t *run_pos = (int32_t *)(run_state + (size_t)S * kMtN);
  uint32_t *rows = run_state + (size_t)S * (kMtN + 1);
  long long per = (long long)((workspace_bytes - state_block_bytes(S)) / row_bytes);
  const long long cap = kChunkWords / ((long long)S * W) < 1 ? 1 : kChunkWords / ((long long)S * W);
  const long long unit_cap = kMaxUnits / ((long long)S * units_per_draw(E));   // >= 1 after check_normal
  per = per > cap ? cap : per;
  per = per > unit_cap ? unit_cap : per;
  for (long long d = 0; d < draws; d += per) {
    const long long nd = draws - d < per ? draws - d : per;
    const bool first = d == 0, last = d + nd == draws;
    WordsArgs w{first ? seeds : nullptr, first ? state_in : run_state, first ? pos_in : run_pos, first ? skip : 0, nd * W, per * W, rows,
                last ? state_out : run_state, last ? pos_out : run_pos};
    if (int rc = launch_words(w, S, s)) return rc;
    if (int rc = launch_normal(rows, per * W, S, d, nd, B, E, out, stride_s, stride_a, stride_b, s)) return rc;
  }
  return DT_OK;
}

}  // namespace dt
