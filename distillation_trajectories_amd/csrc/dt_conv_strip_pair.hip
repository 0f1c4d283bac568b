// The strip convolution of dt_conv_strip.hip for TWO adjacent 256 x 64 tiles at once: one workgroup of eight waves, 4 (M) x
// 2 (N), covers 256 rows x 128 output channels.
//
// With N tiled in 64s, conv_strip_bf16x6_kernel<256,64,2,1> loads, splits and stages the same fp32 activation strip once
// per N tile (2-4 times per M tile on the layers it runs), and the two workgroups that share a CU run their tap loops
// independently, so that the launch lasts as long as the slower one.  Here the strip is staged once per chunk group for
// all eight waves, the weight tiles of both N halves (adjacent in the pack: one 3-plane x 128-column x 16 tile per tap and
// chunk) are double buffered as there, and both halves move tap by tap behind the same barriers.
//
// The two N halves are two virtual 256 x 64 workgroups: half wn = wave / 4 has its own n0, its own epilogue stage in LDS
// and the wave row wm = wave % 4, and runs conv_midpoint<2,2> and conv_epilogue<256,64,1> of the 256 x 64 form on them.
// Halo rule, zero rows, half-swap swizzle, tap masks and row arithmetic are those of dt_conv_strip.hip, and so is the order
// of the operations behind every output element (chunk groups, taps, chunks of a step, the six plane products, the
// epilogue's expressions): the results are bit-identical to the 256 x 64 kernel's.  Routing: dt_conv_strip_pair.h.
#include <mutex>
#include <type_traits>

#include "dt_conv_strip_pair.h"

// conv_epilogue_on (dt_conv_epilogue.h) is written for workgroups of 256 threads and takes its thread index from
// threadIdx.x.  Each half of this workgroup is such a workgroup to it -- threads 256 h .. 256 h + 255, in the same order
// -- so inside that header, and only there, threadIdx reads as the index within the half.  (This holds while the header
// reads nothing of the workgroup but threadIdx.x and every barrier in it is uniform over the workgroup: a use of blockDim,
// of the workitem id itself or of a barrier under a per-half condition would break this kernel alone.  Passing the index
// as an argument is the clean form, once that header may change.)
namespace dt {
struct PairHalfThread { int x; };
__device__ inline PairHalfThread pair_half_thread() { return PairHalfThread{(int)(__builtin_amdgcn_workitem_id_x() & 255u)}; }
}  // namespace dt
#define threadIdx dt::pair_half_thread()
#include "dt_conv_epilogue.h"
#undef threadIdx

namespace dt {

extern __shared__ __attribute__((aligned(16))) __bf16 pair_lds[];

__global__ __launch_bounds__(StripPairForm::kThreads, 2) void conv_strip_pair_bf16x6_kernel(const ConvParams p) {
  constexpr ConvForm F = StripPairForm::half();
  constexpr int NT = StripPairForm::kThreads, BM = StripPairForm::kBm, KC = StripPairForm::kKc, AP = StripPairForm::kAp;
  constexpr int MI = F.mi(), NI = F.ni();
  static_assert(F.wm() == 4 && F.wn() == 1 && MI == 2 && NI == 2 && F.kc == KC && F.bm == BM && 2 * F.bn == StripPairForm::kBn, "two 4 x 1 halves of 64 x 64 wave tiles");
  static_assert(2 * (BM + 2 * (F.max_w() + 1)) <= AP * NT, "strip staging reach");
  constexpr int PLANE_B = StripPairForm::plane_b(), STAGE_B = 3 * PLANE_B;     // bf16 elements
  const int halo = strip_halo(p.W, BM);
  const int R = F.strip_rows(halo);
  const int RZ = F.zero_row(R);                                    // 8 all-zero rows start here (multiple of 8)
  const int PLANE_A = F.plane_a(RZ);
  __bf16 *As = pair_lds;                                           // [KC][3][RZ+8][16]
  __bf16 *Bs = pair_lds + F.strip_elems(PLANE_A);                  // [2][KC][3][128][16]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: chunk and tile offsets stay in scalar registers
  const int wm = wave & 3, wn = wave >> 2;
  const int half = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * StripPairForm::kBn;
  const int n0h = n0 + wn * F.bn;                                  // this half's first output channel
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
  // ---- weight staging: the plane tiles of one (tap, chunk) are contiguous [128][16] bf16 runs, 256 threads each; the thread
  // halves stage the even / odd (chunk, plane) tiles
  constexpr int NB = KC * 3 / 2;
  const int bt = tid & 255, bsub = tid >> 8;
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
    const int row = wn * (NI * 32) + ni * 32 + l31;                // column of the 128-wide weight tile
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
#pragma unroll
    for (int i = 0; i < NB; ++i)                                   // tile 2 i + bsub = (chunk, plane): consecutive chunks of one tap are 3 planes apart
      rb[i] = *reinterpret_cast<const u32x4 *>(wrun + (2 * i) * w_plane);
  };
  auto write_b = [&](int stage) __attribute__((always_inline)) {
    __bf16 *B = Bs + stage * KC * STAGE_B;
#pragma unroll
    for (int i = 0; i < NB; ++i) *reinterpret_cast<u32x4 *>(B + (2 * i) * PLANE_B + b_lds) = rb[i];
  };

  // ---- prologue: strip of chunk 0, weights of step 0, the zero row
  load_strip(0);
  load_b(ADV_NONE);
  if (tid < 48 * KC) *reinterpret_cast<u32x4 *>(As + (tid >> 4) * PLANE_A + RZ * 16 + (tid & 15) * 8) = u32x4{0u, 0u, 0u, 0u};
  write_strip();
  write_b(0);
  __syncthreads();

  // One step = one tap of one (KC-chunk) group, as in dt_conv_strip.hip: TT is the tap as a compile-time constant, the
  // nine taps of a main chunk are unrolled and only the chunk loop is left as scalar control.
  int step = 0;
  auto do_step = [&](auto TT, int ch, bool first_tap, bool last_tap, bool next_chunk, int adv) __attribute__((always_inline)) {
    constexpr int tt = decltype(TT)::value;
    const bool more = !last_tap || next_chunk;
    if (first_tap && next_chunk) load_strip(ch + 1);               // lands while this chunk's taps run
    if (more) load_b(adv);
    {
      int wv = p.W;
      asm volatile("" : "+s"(wv));           // do not keep nine precomputed shifts in SGPRs
      const int shift = (tt / 3 - 1) * wv + (tt % 3 - 1);
      int a_e[MI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        // an out-of-picture tap reads zero row RZ + (srow & 7) at the same physical half: the bank a lane hits is the one its
        // in-picture read would hit, so any mix of the two stays conflict-free
        int row0 = a_row[mi];
        asm volatile("" : "+v"(row0));       // keeps the nine taps' addresses from being hoisted out of the chunk loop
        const int srow = row0 + shift;
        const int lrow = ((a_mask[mi] >> tt) & 1u) ? srow : RZ + (srow & 7);
        a_e[mi] = lrow * 16 + ((half ^ ((srow >> 3) & 1)) << 3);
      }
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        const __bf16 *A = As + kk * 3 * PLANE_A;
        const __bf16 *B = Bs + ((step & 1) * KC + kk) * STAGE_B;
        bf16x8 fb[NI][3];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            fb[ni][pl] = *reinterpret_cast<const bf16x8 *>(B + pl * PLANE_B + b_frag[ni]);
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
    if (more) write_b((step + 1) & 1);
    const bool restage = last_tap && next_chunk;
    if (restage) {
      __syncthreads();                                             // every wave is done with this chunk's strip
      write_strip();
    }
    __syncthreads();
    ++step;
  };

  for (int ch = 0; ch < n_main; ++ch) {                            // 3x3 walk: nine unrolled taps per chunk group
    const bool next_chunk = ch + 1 < n_chunks;
    do_step(std::integral_constant<int, 0>{}, ch, true, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 1>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 2>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 3>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 4>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 5>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 6>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 7>{}, ch, false, false, next_chunk, ADV_TAP);
    do_step(std::integral_constant<int, 8>{}, ch, false, true, next_chunk, ch + 1 < n_main ? ADV_GROUP : ADV_SKIP0);
    if (ch + 1 == n_main && p.in2) conv_midpoint<MI, NI>(p, acc, n0h, 0, l31);
  }
  for (int ch = n_main; ch < n_chunks; ++ch)                       // fused 1x1 skip walk through the strip: centre tap only
    do_step(std::integral_constant<int, 4>{}, ch, true, true, ch + 1 < n_chunks, ADV_SKIP);
  // each half is a 256 x 64 workgroup to the epilogue: its own channels, its own stage, wave row wm of four
  float *stage = reinterpret_cast<float *>(pair_lds) + wn * StripPairForm::half_stage_floats();
  conv_epilogue<BM, F.bn, 1, true>(p, acc, stage, m0, n0h, wm, 0, half, l31, 0);
}

// The kernel takes up to all of a CU's LDS.  The runtime keeps that attribute per device: it is set on the first launch on
// each device, not once per process.
static int pair_lds_attribute() {
  constexpr int kMaxDevices = 64;
  static std::mutex mu;                    // launches come from several host threads
  static int status[kMaxDevices];          // 0 not set yet, 1 set, otherwise -(hip error)
  int dev = 0;
  DT_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) return DT_E_ARG;
  std::lock_guard<std::mutex> lock(mu);
  if (status[dev] == 0) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(conv_strip_pair_bf16x6_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)StripPairForm::lds_limit());
    status[dev] = e == hipSuccess ? 1 : -(int)e;
  }
  return status[dev] == 1 ? DT_OK : -status[dev];
}

// p passed conv_admissible and strip_pair_serves
int launch_conv_strip_pair(const ConvParams &p_in, hipStream_t s) {
  ConvParams p = p_in;
  p.dup_stage2 = p.n_dup == 2 && p.pool_out;                       // a second epilogue stage behind each half's first
  const size_t lds = StripPairForm::lds_bytes(p.W, p.dup_stage2);
  if (const int st = pair_lds_attribute()) return st;
  conv_strip_pair_bf16x6_kernel<<<dim3((p.M + p.bm - 1) / p.bm, p.n_p / StripPairForm::kBn, p.splits), StripPairForm::kThreads, lds, s>>>(p);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace dt
