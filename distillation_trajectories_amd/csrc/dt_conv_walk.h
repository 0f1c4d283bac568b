// The K walk of the two tile-GEMM convolution kernels (conv_gemm_kernel, dt_conv.hip; conv_gemm_bf16x6_kernel,
// dt_conv_bf16.hip): what they share of it, written once.  A 256-thread workgroup owns a BM x BN output tile and walks K in
// chunks of 16 channels of one tap:
//   - split-K: grid.z slices the (tap, channel chunk) walk into equal runs of whole chunks; where a slice starts, how
//     it steps, how many chunks the fused 1x1 skip walk adds, where conv_midpoint stands between the two    KWalk
//   - the accumulator clear                                                                         DT_CLEAR_ACC
// Both kernels run the same software pipeline over these, one barrier per chunk: iteration `it` issues the global loads
// of chunk it+1 into registers (chunk it+1 - n_main of the skip walk once it+1 >= n_main, else chunk (tap, cc) and
// k.next()), runs the MFMAs of chunk it from LDS stage it&1 (conv_midpoint first where k.at_midpoint), then parks the
// registers in the other stage; it == -1 is the prologue (loads chunk 0, no compute).
// That loop, the decode of a staged row into (valid, y, x, offsets) and a tap's (dy, dx), bounds test and address shift
// stay spelled out in each kernel, next to what its arithmetic dictates (how many consecutive k an item holds, the LDS
// image and its swizzle, the address of a weight tile in its pack, the fragment reads and the MFMAs).  They were shared
// too -- as one function template over an arithmetic policy, then as small structs both loops used -- and each form
// changed the machine code of the fp32 kernels: more spilled registers in the first, and in the second the same
// registers but 1x1 skip launches 2 % slower in two rounds of measurements.  With what is here the
// eight kernels compile to their earlier instructions, one for one.  (The strip kernel, dt_conv_strip.hip, stages whole
// strips and shares none of this.)
#pragma once
#include "dt_conv_epilogue.h"

namespace dt {

// The accumulator clear (a macro: through a function, or as `= {}`, the 64 x 64 fp32 kernel keeps five more registers in scratch)
#define DT_CLEAR_ACC(acc, MI, NI)                                  \
  _Pragma("unroll") for (int mi_ = 0; mi_ < MI; ++mi_)             \
  _Pragma("unroll") for (int ni_ = 0; ni_ < NI; ++ni_)             \
  _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) acc[mi_][ni_][r_] = 0.f

// Chunks of the walk of slice blockIdx.z: n_main chunks of the (tap, channel chunk) walk from (tap, cc) on, then -- with a
// fused skip (p.in2, splits == 1) -- the cin2_p / 16 chunks of the 1x1 skip walk
struct KWalk {
  int CC, n_main, n_iter;   // chunks per tap; chunks of the main walk of this slice; with the skip walk's
  int tap, cc;              // the next chunk of the main walk
  __device__ __forceinline__ explicit KWalk(const ConvParams &p) {
    CC = p.cin_p >> 4;
    n_main = (p.tap_hi - p.tap_lo) * CC / p.splits;
    n_iter = n_main + (p.in2 ? (p.cin2_p >> 4) : 0);
    tap = p.tap_lo + (blockIdx.z * n_main) / CC;
    cc = (blockIdx.z * n_main) % CC;
  }
  __device__ __forceinline__ void next() { if (++cc == CC) { cc = 0; ++tap; } }
  // before the MFMAs of chunk `it`: conv_midpoint turns the main walk's sums into relu(acc * scale + shift), the skip walk goes on
  __device__ __forceinline__ bool at_midpoint(const ConvParams &p, int it) const { return it == n_main && p.in2; }
};

}  // namespace dt
