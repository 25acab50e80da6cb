// Workgroup reductions: the join of per-wave values through LDS (gfx950, wave64).
//
// The caller reduces within its wave first (wave_sum, wave_sum_fast, wave_max, wave_sum_d, an integer shuffle sum: the two float wave sums
// associate differently, so the choice stays at the call site) and hands the wave's value in; NW is the number of waves of the workgroup.  Every
// helper: barrier (red may still be read from the previous call), lane 0 of each wave stores, barrier, every thread joins and returns the
// result.  All threads of the workgroup must call it.
//
// The associations are part of the contract (bit-equal tests hold group-norm statistics, cache rows and codes to them):
//   NW == 4       (r0 + r1) + (r2 + r3), respectively fmaxf(fmaxf(r0, r1), fmaxf(r2, r3))
//   any other NW  serially from index 0 (a sum starts from zero)
// A max is order-independent, so sites that used to join four maxima serially see the same bits.  The arg-max joins serially for every NW.
//
// Left alone on purpose: rows_pipe.hip (two statistics in disjoint halves of one buffer, to save a barrier on the decode path), rvq.hip (arg-max
// with runner-up), ecapa.hip (per-column joins), norm.hip (float64 tiles), flash_attn.hip.
#pragma once
#include "common.h"

template <int NW, typename T>
__device__ __forceinline__ T block_join_sum(T wave_value, T* red) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave_value;
  __syncthreads();
  if constexpr (NW == 4) return (red[0] + red[1]) + (red[2] + red[3]);
  T r = T(0);
#pragma unroll
  for (int i = 0; i < NW; ++i) r += red[i];
  return r;
}

// R sums at once (the per-row statistics of a tile: one barrier pair for all of them instead of one per row): red holds NW * R floats, the
// association per sum is block_join_sum's.
template <int NW, int R>
__device__ __forceinline__ void block_join_sum_rows(const float (&wave_values)[R], float* red, float (&out)[R]) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < R; ++i) red[(threadIdx.x >> 6) * R + i] = wave_values[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < R; ++i) {
    if constexpr (NW == 4) {
      out[i] = (red[i] + red[R + i]) + (red[2 * R + i] + red[3 * R + i]);
    } else {
      float r = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) r += red[w * R + i];
      out[i] = r;
    }
  }
}

template <int NW>
__device__ __forceinline__ float block_join_max(float wave_value, float* red) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave_value;
  __syncthreads();
  if constexpr (NW == 4) return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float r = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) r = fmaxf(r, red[i]);
  return r;
}

struct ArgMax { float v; int i; };

__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {
  // larger value wins; on ties the smaller index (mx.argmax returns the first maximum)
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

// takes the lane's candidate (the wave step is part of it: there is one way to do it)
template <int NW>
__device__ __forceinline__ ArgMax block_argmax(ArgMax x, float* redv, int* redi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ArgMax y;
    y.v = __shfl_xor(x.v, o, 64);
    y.i = __shfl_xor(x.i, o, 64);
    x = better(x, y);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = x.v; redi[threadIdx.x >> 6] = x.i; }
  __syncthreads();
  ArgMax r;
  r.v = redv[0]; r.i = redi[0];
  for (int i = 1; i < NW; ++i) { ArgMax y; y.v = redv[i]; y.i = redi[i]; r = better(r, y); }
  return r;
}

// Tail of the fake-quant extrema passes (256 threads): {-min, max} >= 0 of the workgroup, then thread 0 raises the stored pair.  Both are
// non-negative, so the integer order of their bit patterns is their float order, and a max is order-independent: deterministic atomics.
// only_if_raises: read the stored pair first and skip an atomic that would not change it (a stale read is a smaller value and merely lets the
// atomic run) -- for grids of many thousand workgroups that meet in the same two words.
__device__ __forceinline__ void block_extrema_atomic_max(float nmn, float mx, float* red8, int* dst_pair, bool only_if_raises) {
  nmn = wave_max(nmn);
  mx = wave_max(mx);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red8[2 * w] = nmn; red8[2 * w + 1] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { nmn = fmaxf(nmn, red8[2 * i]); mx = fmaxf(mx, red8[2 * i + 1]); }
    volatile const float* cur = (volatile const float*)dst_pair;
    if (!only_if_raises || nmn > cur[0]) atomicMax(dst_pair, __float_as_int(nmn));
    if (!only_if_raises || mx > cur[1]) atomicMax(dst_pair + 1, __float_as_int(mx));
  }
}
