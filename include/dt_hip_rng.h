/*
 * dt_hip_rng.h -- entry points of libdt_hip.so for sampler noise made on the device: the stream of the torch CPU generator,
 * bit for bit (what torch.manual_seed / torch.randn on the host give), added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, a stream argument, asynchronous, int status (0 ok, <0 DT_E_*,
 * >0 a hipError_t); nothing is allocated, every buffer is the caller's.
 *
 * The stream.  A generator is an mt19937: 624 untempered state words and a position pos in 0..624, the index of the next
 * word in the state (624: the block is used up and is regenerated before the next word).  torch.manual_seed(s) is the key
 * init_genrand(s mod 2^32) at position 624.  Word k of a stream is the k-th tempered output from there on.
 * A contiguous fp32 torch.randn of E >= 16 elements takes words(E) consecutive words of the stream:
 *     words(E) = E            if E % 16 == 0
 *              = E + 16       otherwise
 * With u[i] = (word[i] & 0xFFFFFF) * 2^-24, every full group of 16 elements (base = 16 g, j = 0..7) is
 *     r = sqrt(-2 log(1 - u[base + j])),  theta = 2 pi u[base + j + 8],  out[base + j] = r cos theta,  out[base + j + 8] = r sin theta
 * and, if E % 16 != 0, the last 16 elements out[E - 16 .. E) are computed the same way from the 16 extra words
 * word[E .. E + 16) instead.  log and sincos are the cephes single-precision polynomials as the AVX512 build of torch 2.10
 * evaluates them (ATen/native/cpu/avx_mathfun.h, with that build's fused multiply-adds; the capability the recorded vectors of
 * tests/golden/torch_randn_vectors.npz come from, and the only one checked), sqrt is correctly rounded, and every zero comes out
 * as +0.  Draw d of a stream (d = 0, 1, ...) starts at word d * words(E).
 * So an output depends on nothing but (seed or state + position, skip, E, draw index, element): not on the number of streams
 * in a call, the chunking, the strides or the launch shape.
 *
 * Limits: 1 <= S <= 2^20 streams per call; counts are 64-bit and >= 0; E >= 16 (torch takes a double-precision scalar path
 * below that, which is not provided: DT_E_ARG) and E <= 2^30; B < 2^31; with units(E) = ceil(pairs / 64) wave units per draw
 * (pairs = 8 floor(E / 16), + 8 with a tail), S * units(E) <= 2^30, and one dt_rng_normal_from_words call covers at most 2^30
 * units: S * A * B * units(E) <= 2^30 (dt_rng_randn chunks, so only the first of the two binds it).  Beyond them: DT_E_ARG.
 */
#ifndef DT_HIP_RNG_H
#define DT_HIP_RNG_H

#include "dt_hip.h"
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DT_RNG_STATE_WORDS 624

/* n tempered words of each of S independent streams, one workgroup per stream (the walk of one stream is serial):
 *   words_dev[s * word_pitch + k], k < n, = word skip + k of stream s          (word_pitch in words, >= n)
 * Stream s starts from seeds_dev[s] (uint64, taken mod 2^32) when state_in_dev is NULL, else from the explicit generator
 * state_in_dev[s][624] at position pos_in_dev[s] (0..624); that is how the host generator's current state gets in.
 * state_out_dev / pos_out_dev (both or neither; may alias the inputs) receive each stream's state and position after word
 * skip + n - 1, from which a later call continues the same walk.  words_dev may be NULL when n == 0 (a pure skip).
 * DT_E_NULL: no start, or one of a pair missing; DT_E_ARG: S outside the limits, n or skip negative, word_pitch < n. */
int dt_rng_mt19937_words(const uint64_t *seeds_dev, const uint32_t *state_in_dev, const int32_t *pos_in_dev, int S,
                         long long skip, long long n, uint32_t *words_dev, long long word_pitch, uint32_t *state_out_dev,
                         int32_t *pos_out_dev, void *stream);

/* The transform: for each of S streams, A * B consecutive draws of E elements from the word row
 * words_dev[s * word_pitch ...] (draw a * B + b at word (a * B + b) * words(E) of the row; word_pitch >= A * B * words(E)), written
 *   out_dev[s * stride_s + a * stride_a + b * stride_b + e],  e < E                (strides in floats)
 * and nothing else of out_dev.  With a = sample, b = step, stride_a = E and stride_b = n * E, the sample-major draw order of a
 * sampler lands in the step-major [T][n][E] layout its kernels read.  One thread per pair (j, j + 8).
 * DT_E_ARG: E < 16 or above the limit, S / A / B negative or above their limits, more than 2^30 units, word_pitch too small; a
 * zero count is a no-op. */
int dt_rng_normal_from_words(const uint32_t *words_dev, long long word_pitch, int S, long long A, long long B, int E,
                             float *out_dev, long long stride_s, long long stride_a, long long stride_b, void *stream);

/* Workspace of dt_rng_randn for S streams of `draws` draws of E elements: the streams' running states plus a chunk of word
 * rows, bounded whatever `draws` is.  dt_rng_randn accepts any workspace of at least dt_rng_workspace_bytes(S, 1, E) bytes
 * (one draw per stream and chunk) and uses what it is given up to this size.  0 for S, draws or E outside their own limits. */
size_t dt_rng_workspace_bytes(int S, long long draws, int E);

/* Both kernels, chunked through workspace_dev (4-byte aligned): A * B draws per stream after skipping `skip` words, placed as by
 * dt_rng_normal_from_words; starts and end states as by dt_rng_mt19937_words.  DT_E_WORKSPACE if workspace_bytes is below the
 * minimum above; argument errors as the two entries'.  Nothing is launched when a status other than DT_OK comes back from the
 * argument checks.  With A * B == 0 no workspace is needed (it may be NULL): the call only skips, and launches the word kernel
 * when an end state is asked for. */
int dt_rng_randn(const uint64_t *seeds_dev, const uint32_t *state_in_dev, const int32_t *pos_in_dev, int S, long long skip,
                 long long A, long long B, int E, float *out_dev, long long stride_s, long long stride_a, long long stride_b,
                 uint32_t *state_out_dev, int32_t *pos_out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_RNG_H */
