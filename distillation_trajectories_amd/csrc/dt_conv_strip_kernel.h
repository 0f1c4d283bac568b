// 3x3 convolution on the split-bf16 arithmetic of dt_conv_bf16.hip with the activation tile staged ONCE per
// 16-channel chunk and reused by all nine taps ("strip" kernel).
//
// The plain implicit-GEMM kernel re-stages its BM x 16 activation tile for every (tap, chunk): nine global
// loads, nine 3-way bf16 splits and nine LDS writes of (nearly) the same pixels.  Here a workgroup keeps the
// tile's rows PLUS a halo of W+1 pixels on either side in LDS as three bf16 planes:
//      strip row s  <->  pixel m0 - (W+1) + s,      s in [0, BM + 2(W+1))
// and tap (dy, dx) of output row r reads strip row r + (W+1) + dy*W + dx -- the same LDS image at a shifted row
// (halo W instead of W+1 when the tile covers whole picture rows, see strip_halo).
// Taps that fall outside the picture (zero padding, also across picture boundaries inside a tile) read one of
// eight all-zero rows instead (the one with the same bank as the real row would have: no conflicts); validity
// is a 9-bit mask per fragment row, computed once.
// Per chunk: one strip load/split/write, then nine steps that only stage the 3 x BN x 16 weight tile of their
// tap (double buffered) and run 24 MFMAs per wave.  ds_read_b128 stays conflict-free at any shift because the
// half-swap swizzle is a function of the strip row (rows 8 apart always differ in it).
//
// (Measured and not kept: weight fragments straight from global memory -- no weight LDS traffic, no barrier per
// tap, double-buffered strip -- 3-8 % slower (181 vs 186, 149 vs 156, 171 vs 181 TF/s); the weight tile through
// global_load_lds into a ring of three, prefetched two taps ahead with counted vmcnt -- 1-5 % slower.)
//
// Split-K runs over channel chunks (grid.z slabs, summed in z order by splitk_epilogue_kernel); the block's
// fused 1x1 skip walk follows as single-tap chunks over in2 / w2, as in the plain kernel.
//
// This header is the kernel and nothing else.  dt_conv_strip.hip compiles the forms of dt_conv_forms.h from it (NH = 1),
// dt_conv_strip_pair.hip the one NH = 2 instantiation, each into a code object of its own.
#pragma once
#include <type_traits>

#include "dt_conv_epilogue.h"

namespace dt {

extern __shared__ __attribute__((aligned(16))) __bf16 strip_lds[];

// KC = 16-channel chunks staged and multiplied per step (1 or 2): KC = 2 halves the barriers and doubles the
// MFMAs between them at twice the LDS footprint and staging registers (2 waves/SIMD instead of 3).
// WK = waves that share one output tile and split the step's KC chunks between them (1, 2 or 4): small layers need
// small workgroup tiles to fill the chip, and a 64 x 64 tile cut 2 x 2 leaves each wave 32 x 32 (6 fragment reads per
// 6 MFMAs, ~100 TF/s).  With WK = 4 every wave keeps a 64 x 64 accumulator (12 reads per 24 MFMAs) over a quarter of
// the channels and the four partial tiles are summed in wave order in the staged epilogue -- split-K without slabs.
// NH = adjacent BM x BN tiles along N that one workgroup of 4 NH waves walks over ONE staged strip (1, or 2 for
// <256,64,2,1>: the pair kernel, routed by dt_conv_strip_pair.h).  With N tiled in 64s every one of the 2-4 N tiles of an M
// tile loads, splits and stages the same fp32 strip, and the two workgroups that share a CU run their tap loops
// independently, so that the launch lasts as long as the slower one.  With NH = 2 the strip is staged once per chunk
// group for all eight waves, the weight tiles of both halves (adjacent in the pack: one 3-plane x 128-column x 16 tile
// per tap and chunk) are double buffered as one, and both halves move tap by tap behind the same barriers.  A half is
// a virtual BM x BN workgroup: waves 4 hn .. 4 hn + 3 with the form's wave layout, its own first channel n0h and its own
// epilogue stage in LDS, on which it runs conv_midpoint and conv_epilogue of the form; the order of the operations
// behind every output element is the NH = 1 kernel's, so the results are bit-identical to it.  The folded 1x1 skip walk
// goes through the strip there (DIRECT is false for <256,64,2,1>): taken straight from global memory, both halves
// would load and split the same rows, which is the work NH = 2 removes.
template <int BM, int BN, int KC, int WK, int NH = 1>
__global__ __launch_bounds__(256 * NH, find_strip_form(BM, BN, KC, WK)->waves_per_simd()) void conv_strip_bf16x6_kernel(const ConvParams p) {
  // four waves (per half): 2 x 2 over the tile, or 4 x 1 for the 256 x 64 tile (a 64 x 64 wave tile -- 12 fragment reads per 24
  // MFMAs, like the 128 x 128 tile -- for layers with 64 output channels, where 128 x 64 leaves each wave 64 x 32),
  // or WM x 1 x WK with the K split
  constexpr ConvForm F = *find_strip_form(BM, BN, KC, WK);
  constexpr int WN = F.wn(), WM = F.wm(), NT = F.threads(NH);
  constexpr int MI = F.mi(), NI = F.ni();
  constexpr int KW = F.kw();                                       // chunks of a step one wave multiplies
  static_assert(WM * WN * WK * 64 * NH == NT && KC % WK == 0 && MI * 32 * WM == BM && NI * 32 * WN == BN && (WK == 1 || (MI == 2 && NI == 2)), "wave layout");
  static_assert(NH == 1 || (NH == 2 && WK == 1 && WN == 1 && F.waves_per_simd() == 2), "two halves, each a column of four waves: eight waves, one workgroup per CU");
  constexpr int BNW = BN * NH;                                     // columns of the weight tile: the halves' tiles side by side
  constexpr int PLANE_B = F.plane_b(NH), STAGE_B = 3 * PLANE_B;   // bf16 elements
  constexpr int AP = F.ap(NH);                                     // strip items (row, k-half) per thread
  static_assert(2 * (BM + 2 * (F.max_w() + 1)) <= AP * NT, "strip staging reach");
  const int halo = strip_halo(p.W, BM);
  const int R = F.strip_rows(halo);
  const int RZ = F.zero_row(R);                                    // 8 all-zero rows start here (multiple of 8)
  const int PLANE_A = F.plane_a(RZ);
  __bf16 *As = strip_lds;                                          // [KC][3][RZ+8][16]
  __bf16 *Bs = strip_lds + F.strip_elems(PLANE_A);                 // [2][KC][3][BNW][16]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: chunk and tile offsets stay in scalar registers
  // (The wave indices of NH = 2 are spelled out, and DB is tested with `if constexpr` in the steps below.  With
  // `(wave & 3) % WK` and so on, and the K-split weight path left for the optimiser to remove, the NH = 2 kernel computes the
  // same but comes out under another scalar register allocation, 0.4-1.3 % slower per launch: DESIGN 9ab.)
  const int hn = NH == 1 ? 0 : wave >> 2;                          // the wave's half
  const int wk = NH == 1 ? wave % WK : 0, wm = NH == 1 ? (wave / WK) / WN : wave & 3, wn = NH == 1 ? (wave / WK) % WN : 0;
  const int half = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BNW;
  const int n0h = n0 + hn * BN;                                    // this half's first output channel
  const int HW = p.H * p.W;
  const int CC = p.cin_p >> 4;

  // ---- strip staging: item -> (strip row, k-half), 32 contiguous bytes of one pixel
  bool s_in[AP], s_ok[AP], s_core[AP];
  int s_off[AP], s_off2[AP], s_offb[AP], s_lds[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int item = tid + i * NT;
    const int srow = item >> 1, hh = item & 1;
    const int m = m0 - halo + srow;
    s_in[i] = item < 2 * R;
    s_ok[i] = s_in[i] && m >= 0 && m < p.M;
    s_core[i] = s_ok[i] && srow >= halo && srow < halo + BM;       // rows the single-tap skip walk needs
    const int mm = s_ok[i] ? m : 0;
    s_off[i] = mm * p.cin_p + hh * 8;
    s_off2[i] = mm * p.cin2_p + hh * 8;
    s_offb[i] = mm * p.b_stride + hh * 8;                             // two-source block input (decoder concat)
    s_lds[i] = srow * 16 + ((hh ^ ((srow >> 3) & 1)) << 3);
  }
  // ---- weight staging: the three plane tiles of one (tap, chunk) are contiguous [BNW][16] bf16 runs
  // (with the K split and BN = 64, and with two halves, both thread halves stage: even / odd (chunk, plane) tiles)
  constexpr bool B_ALL = (WK > 1 || NH > 1) && BNW * 4 == NT;
  constexpr int NB = B_ALL ? KC * 3 / 2 : KC * 3, SB = B_ALL ? 2 : 1;
  static_assert(!B_ALL || (KC * 3) % 2 == 0, "weight staging");
  static_assert(NH == 1 || B_ALL, "weight staging of two halves");
  const bool b_thread = B_ALL || tid < BNW * 2;
  const int bt = B_ALL ? (tid & (BNW * 2 - 1)) : tid, bsub = B_ALL ? tid / (BNW * 2) : 0;
  const size_t w_plane = (size_t)p.n_p * 16;
  const __bf16 *wbase = reinterpret_cast<const __bf16 *>(p.w) + (size_t)n0 * 16 + bt * 8 + bsub * w_plane;
  const __bf16 *wbase2 = reinterpret_cast<const __bf16 *>(p.w2) + (size_t)n0 * 16 + bt * 8 + bsub * w_plane;
  const int b_lds = bsub * PLANE_B + bt * 8;

  // ---- fragment rows: strip row of the centre tap and the 9-bit tap-validity mask
  int a_row[MI];
  unsigned a_mask[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int row_i = wm * (MI * 32) + mi * 32 + l31;
    const int m = m0 + row_i;
    a_row[mi] = row_i + halo;
    const ConvRowMath rm = kernarg_row_math();                    // (not p.rm: these pairs would then hold scalar registers through the walk)
    unsigned mask = 0;
    if (m < p.M) {
      const RowPixel px = row_pixel(m, HW, p.W, rm);
      mask = pixel_tap_mask(px.y, px.x, p.H, p.W);
    }
    a_mask[mi] = mask;
  }
  int b_frag[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int row = (hn * WN + wn) * (NI * 32) + ni * 32 + l31;      // column of the weight tile
    b_frag[ni] = row * 16 + ((half ^ ((row >> 3) & 1)) << 3);
  }

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  // steps-worth of KC channel chunks in this z slice; the walk may run past the layer's CC chunks (odd chunk counts): the
  // weight pack holds zero chunks there (p.ccw per tap, checked by the launcher) and the activation loads are skipped
  const int n_main = (CC + p.splits * KC - 1) / (p.splits * KC);
  const int cc0 = blockIdx.z * n_main * KC;
  const int CC2 = p.cin2_p >> 4;
  const int n_chunks = n_main + (p.in2 ? (CC2 + KC - 1) / KC : 0);

  f32x4 sa0[KC][AP], sa1[KC][AP];
  u32x4 rb[NB];
  auto load_strip = [&](int ch) __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      sa0[kk][i] = f32x4{0.f, 0.f, 0.f, 0.f}; sa1[kk][i] = sa0[kk][i];
      if (ch < n_main) {
        const int cc = cc0 + ch * KC + kk;
        if (s_ok[i] && cc < CC) {
          const float *src = (p.in_b && cc >= p.cc_a) ? p.in_b + s_offb[i] + (cc - p.cc_a) * 16 : p.in + s_off[i] + cc * 16;
          sa0[kk][i] = *reinterpret_cast<const f32x4 *>(src);
          sa1[kk][i] = *reinterpret_cast<const f32x4 *>(src + 4);
        }
      } else if (s_core[i] && (ch - n_main) * KC + kk < CC2) {
        const int c2 = (ch - n_main) * KC + kk;
        const float *src = (p.in2_b && c2 >= p.cc_a) ? p.in2_b + s_offb[i] + (c2 - p.cc_a) * 16 : p.in2 + s_off2[i] + c2 * 16;
        sa0[kk][i] = *reinterpret_cast<const f32x4 *>(src);
        sa1[kk][i] = *reinterpret_cast<const f32x4 *>(src + 4);
      }
    }
  };
  auto write_strip = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
    for (int i = 0; i < AP; ++i)
      if (s_in[i]) {
        bf16x8 p1, p2, p3;
        split8(sa0[kk][i], sa1[kk][i], p1, p2, p3);
        __bf16 *A = As + kk * 3 * PLANE_A;
        *reinterpret_cast<bf16x8 *>(A + s_lds[i]) = p1;
        *reinterpret_cast<bf16x8 *>(A + PLANE_A + s_lds[i]) = p2;
        *reinterpret_cast<bf16x8 *>(A + 2 * PLANE_A + s_lds[i]) = p3;
      }
  };
  // The weight tiles are visited in a fixed order, so a running pointer replaces per-step index arithmetic:
  // next tap of the chunk group (+tap_stride), first tap of the next group, the skip weights, next skip group.
  const size_t tap_stride = (size_t)p.ccw * 3 * w_plane, group_stride = (size_t)KC * 3 * w_plane;
  const __bf16 *wrun = wbase + (size_t)cc0 * 3 * w_plane;
  enum { ADV_NONE = 0, ADV_TAP, ADV_GROUP, ADV_SKIP0, ADV_SKIP };
  auto load_b = [&](int adv) __attribute__((always_inline)) {
    if (adv == ADV_TAP) wrun += tap_stride;
    else if (adv == ADV_GROUP) wrun = wrun - 8 * tap_stride + group_stride;
    else if (adv == ADV_SKIP0) wrun = wbase2;
    else if (adv == ADV_SKIP) wrun += group_stride;
    if (b_thread) {
#pragma unroll
      for (int i = 0; i < NB; ++i)                                 // tile i = (chunk, plane): consecutive chunks of one tap are 3 planes apart
        rb[i] = *reinterpret_cast<const u32x4 *>(wrun + (SB * i) * w_plane);
    }
  };
  auto write_b = [&](int stage) __attribute__((always_inline)) {
    if (b_thread) {
      __bf16 *B = Bs + stage * KC * STAGE_B;
#pragma unroll
      for (int i = 0; i < NB; ++i) *reinterpret_cast<u32x4 *>(B + (SB * i) * PLANE_B + b_lds) = rb[i];
    }
  };

  // ---- K-split kernels: weight fragments straight from global memory.  With the step's chunks split across the waves a
  // weight tile is multiplied by ONE wave (64 x 64 tile) or two (128 x 64, 64 x 128): staging it through LDS shares nothing
  // and costs a barrier per tap.  The packed tile in global memory IS the LDS image (half-swap swizzle included), so a lane's
  // B fragment is one 16-byte load; the fragments of step s + 1 are requested before the MFMAs of step s, and the only
  // barriers left are the two around a strip restage.
  constexpr bool DB = WK > 1;
  bf16x8 fbn[KW][NI][3];
  auto load_bd = [&](int adv) __attribute__((always_inline)) {
    if (adv == ADV_TAP) wrun += tap_stride;
    else if (adv == ADV_GROUP) wrun = wrun - 8 * tap_stride + group_stride;
    else if (adv == ADV_SKIP0) wrun = wbase2;
    else if (adv == ADV_SKIP) wrun += group_stride;
    const __bf16 *wt = wrun - (bt * 8 + bsub * w_plane);           // the tile's first element (wrun carries this thread's staging offset)
#pragma unroll
    for (int kw = 0; kw < KW; ++kw)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          fbn[kw][ni][pl] = *reinterpret_cast<const bf16x8 *>(wt + ((wk * KW + kw) * 3 + pl) * w_plane + b_frag[ni]);
  };

  // ---- prologue: strip of chunk 0, weights of step 0, the zero row
  load_strip(0);
  if constexpr (DB) load_bd(ADV_NONE); else load_b(ADV_NONE);
  if (tid < 48 * KC) *reinterpret_cast<u32x4 *>(As + (tid >> 4) * PLANE_A + RZ * 16 + (tid & 15) * 8) = u32x4{0u, 0u, 0u, 0u};
  write_strip();
  if (!DB) write_b(0);
  __syncthreads();

  // One step = one tap of one (KC-chunk) group.  TT is the tap as a compile-time constant: the nine taps of a main
  // chunk are unrolled, so shifts, mask bits and the whole walk bookkeeping fold away and only the chunk loop is
  // left as scalar control.
  int step = 0;
  bool stage_next_strip = true;            // false: the next step is a skip step that takes its activations straight from global memory
  auto do_step = [&](auto TT, int ch, bool first_tap, bool last_tap, bool next_chunk, int adv) __attribute__((always_inline)) {
    constexpr int tt = decltype(TT)::value;
    const bool more = !last_tap || next_chunk;
    if (first_tap && next_chunk && stage_next_strip) load_strip(ch + 1);   // lands while this chunk's taps run
    bf16x8 fbc[KW][NI][3];                                         // DB: this step's weight fragments (requested during the previous step)
    if constexpr (DB) {
#pragma unroll
      for (int kw = 0; kw < KW; ++kw)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) fbc[kw][ni][pl] = fbn[kw][ni][pl];
      if (more) load_bd(adv);
    } else if (more) load_b(adv);
    {
      int wv = p.W;
      asm volatile("" : "+s"(wv));           // likewise: do not keep nine precomputed shifts in SGPRs
      const int shift = (tt / 3 - 1) * wv + (tt % 3 - 1);
      int a_e[MI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        // an out-of-picture tap reads zero row RZ + (srow & 7) at the same physical half (a row's 16-B slot in the 256-B
        // bank row depends on srow & 7 and, through the half swap, on bit 3 -- which `half ^ ...` below keeps): the bank a lane hits is
        // the one its in-picture read would hit, so any mix of the two stays conflict-free
        int row0 = a_row[mi];
        asm volatile("" : "+v"(row0));       // keeps the nine taps' addresses from being hoisted out of the chunk loop (18+ VGPRs)
        const int srow = row0 + shift;
        const int lrow = ((a_mask[mi] >> tt) & 1u) ? srow : RZ + (srow & 7);
        a_e[mi] = lrow * 16 + ((half ^ ((srow >> 3) & 1)) << 3);
      }
#pragma unroll
      for (int kw = 0; kw < KW; ++kw) {
        const int kk = wk * KW + kw;                                // this wave's chunk of the step (all of them without the K split)
        const __bf16 *A = As + kk * 3 * PLANE_A;
        const __bf16 *B = Bs + ((step & 1) * KC + kk) * STAGE_B;
        bf16x8 fb[NI][3];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            if constexpr (DB) fb[ni][pl] = fbc[kw][ni][pl];
            else fb[ni][pl] = *reinterpret_cast<const bf16x8 *>(B + pl * PLANE_B + b_frag[ni]);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          bf16x8 fa[3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            fa[pl] = *reinterpret_cast<const bf16x8 *>(A + pl * PLANE_A + a_e[mi]);
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) mfma_bf16x6(acc[mi][ni], fa, fb[ni]);
        }
      }
    }
    if (!DB && more) write_b((step + 1) & 1);
    const bool restage = last_tap && next_chunk && stage_next_strip;
    if (restage) {
      __syncthreads();                                             // every wave is done with this chunk's strip
      write_strip();
    }
    if (!DB || restage) __syncthreads();
    ++step;
  };

  // ---- fused 1x1 skip walk with the activations taken straight from global memory (wave tiles of at most 2 x 32 rows x
  // chunks per step): a lane's A fragment of a 32 x 32 x 16 MFMA is 8 consecutive channels of ONE pixel, so two float4 loads
  // and the three-way split give it without LDS.  The strip path restaged the tile per step behind two barriers with the loads
  // of step s + 1 issued only one (single-tap) step ahead: 25-40 us per layer for 2-4 GFLOP.  Here the loads of step s + 2 are
  // issued when step s has consumed its registers (two register sets, the strip staging registers being idle), the weight
  // tile keeps its double buffer and a step has one barrier.
  constexpr bool DIRECT = MI * KW <= 2 && KC >= 2;   // (K = 16 steps: 3 waves per SIMD leave no registers for the two sets)
  f32x4 ga0[KW][MI][2], ga1[KW][MI][2];
  const int n_skip = p.in2 ? (CC2 + KC - 1) / KC : 0;
  auto load_a = [&](f32x4 (&g)[KW][MI][2], int s2) __attribute__((always_inline)) {
#pragma unroll
    for (int kw = 0; kw < KW; ++kw)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int c2 = s2 * KC + wk * KW + kw;
        const int m = m0 + wm * (MI * 32) + mi * 32 + l31;
        g[kw][mi][0] = f32x4{0.f, 0.f, 0.f, 0.f}; g[kw][mi][1] = g[kw][mi][0];
        if (m < p.M && c2 < CC2) {
          const float *src = (p.in2_b && c2 >= p.cc_a) ? p.in2_b + (size_t)m * p.b_stride + (c2 - p.cc_a) * 16 + half * 8
                                                       : p.in2 + (size_t)m * p.cin2_p + c2 * 16 + half * 8;
          g[kw][mi][0] = *reinterpret_cast<const f32x4 *>(src);
          g[kw][mi][1] = *reinterpret_cast<const f32x4 *>(src + 4);
        }
      }
  };
  auto skip_step = [&](f32x4 (&g)[KW][MI][2], int s2) __attribute__((always_inline)) {
    const bool more = s2 + 1 < n_skip;
    bf16x8 fbc[KW][NI][3];
    if (DB) {
#pragma unroll
      for (int kw = 0; kw < KW; ++kw)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) fbc[kw][ni][pl] = fbn[kw][ni][pl];
      if (more) load_bd(ADV_SKIP);
    } else if (more) load_b(ADV_SKIP);
#pragma unroll
    for (int kw = 0; kw < KW; ++kw) {
      const int kk = wk * KW + kw;
      const __bf16 *B = Bs + ((step & 1) * KC + kk) * STAGE_B;
      bf16x8 fb[NI][3];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) fb[ni][pl] = DB ? fbc[kw][ni][pl] : *reinterpret_cast<const bf16x8 *>(B + pl * PLANE_B + b_frag[ni]);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        bf16x8 fa[3];
        split8(g[kw][mi][0], g[kw][mi][1], fa[0], fa[1], fa[2]);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) mfma_bf16x6(acc[mi][ni], fa, fb[ni]);
      }
    }
    if (s2 + 2 < n_skip) load_a(g, s2 + 2);
    if (!DB) {
      if (more) write_b((step + 1) & 1);
      __syncthreads();
    }
    ++step;
  };

  // Two workgroups share a CU (and each SIMD) on the big layers, and the SIMD's arbiter favours the older wave: left
  // alone, the older workgroup finishes its loop well before the younger one, which then runs the rest by itself at one
  // wave per SIMD.  Blocks b and b + 256 are the pair that usually shares a CU (round-robin dispatch; a guess that only
  // affects speed): they take the high priority in alternate chunk groups.
  // (Only for grids of at most two workgroups per CU: with three resident ones two would share a priority -- measured
  // 11 % slower on enc1.conv2's 1024 workgroups -- and larger grids refill CUs at arbitrary times anyway.)
  // (Not with NH = 2: that workgroup has its CU to itself.)
  const int prio_grp = ((blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) >> 8) & 1;
  const bool use_prio = NH == 1 && gridDim.x * gridDim.y * gridDim.z <= 512;
  for (int ch = 0; ch < n_main; ++ch) {                            // 3x3 walk: nine unrolled taps per chunk group
    if (use_prio) {
      if ((ch ^ prio_grp) & 1) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    // (with the K split the fused skip walk starts from a fresh prologue after the mid-kernel reduction below)
    const bool next_chunk = ch + 1 < ((WK > 1 && p.in2) ? n_main : n_chunks);
    if (DIRECT && WK == 1 && p.in2 && ch + 1 == n_main) {          // the skip walk's first two steps load during this chunk's taps
      stage_next_strip = false;
      load_a(ga0, 0);
      if (n_skip > 1) load_a(ga1, 1);
    }
    do_step(std::integral_constant<int, 0>{}, ch, true, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 1>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 2>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 3>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 4>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 5>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 6>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 7>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 8>{}, ch, false, true, next_chunk, ch + 1 < n_main ? ADV_GROUP : ADV_SKIP0);
    if constexpr (WK == 1) {
      if (ch + 1 == n_main && p.in2) conv_midpoint<MI, NI>(p, acc, n0h, wn, l31);
    }
  }
  if constexpr (WK > 1) {
    // After the loop, not in its last trip: inside it, what the skip walk's prologue loads (the next weight fragments and the
    // two activation sets, up to 56 registers) counts as live around the loop's back edge, i.e. through every tap of every
    // chunk group -- <64,64,4,4> then kept 62 registers in scratch and reloaded them around the ninth tap and the restage.
    if (p.in2) {
      // BN + ReLU apply to the COMPLETE 3x3 sum: the WK partial tiles meet in LDS (free after the last step's barrier), wave
      // 0 of each group continues with relu(bn(sum)) and the others with zero, and the skip walk restarts the pipeline
      constexpr int P = F.pitch(), COPY = F.copy_floats();
      float *red = reinterpret_cast<float *>(strip_lds);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        if (mi || DB) __syncthreads();                             // (DB: the last step ended without a barrier; the strip is still being read)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            red[wk * COPY + (wm * 32 + 4 * half + (r & 3) + 8 * (r >> 2)) * P + wn * (NI * 32) + ni * 32 + l31] = acc[mi][ni][r];
        __syncthreads();
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float *src = red + (wm * 32 + 4 * half + (r & 3) + 8 * (r >> 2)) * P + wn * (NI * 32) + ni * 32 + l31;
            float v = src[0];
#pragma unroll
            for (int c = 1; c < WK; ++c) v += src[c * COPY];
            acc[mi][ni][r] = wk == 0 ? v : 0.f;
          }
      }
      if (wk == 0) conv_midpoint<MI, NI>(p, acc, n0h, wn, l31);
      __syncthreads();
      if (DB) load_bd(ADV_SKIP0); else load_b(ADV_SKIP0);
      if (DIRECT) {
        load_a(ga0, 0);
        if (n_skip > 1) load_a(ga1, 1);
      } else {
        load_strip(n_main);
        if (tid < 48 * KC) *reinterpret_cast<u32x4 *>(As + (tid >> 4) * PLANE_A + RZ * 16 + (tid & 15) * 8) = u32x4{0u, 0u, 0u, 0u};
        write_strip();
      }
      if (!DB) write_b(step & 1);
      __syncthreads();
    }
  }
  if (NH == 1) __builtin_amdgcn_s_setprio(0);
  if (DIRECT) {                                                    // fused 1x1 skip walk, activations from global memory
    for (int s2 = 0; s2 < n_skip; s2 += 2) {
      skip_step(ga0, s2);
      if (s2 + 1 < n_skip) skip_step(ga1, s2 + 1);
    }
  } else {
    for (int ch = n_main; ch < n_chunks; ++ch)                     // fused 1x1 skip walk through the strip: centre tap only
      do_step(std::integral_constant<int, 4>{}, ch, true, true, ch + 1 < n_chunks, ADV_SKIP);
  }
  // (each half is a BM x BN workgroup of 256 threads to the epilogue: its own channels, its own stage)
  float *stage = reinterpret_cast<float *>(strip_lds) + hn * F.half_stage_floats();
  conv_epilogue<BM, BN, WK, WK == 1, false, NH == 1 ? 0 : 255>(p, acc, stage, m0, n0h, wm, wn, half, l31, wk);
}

}  // namespace dt
