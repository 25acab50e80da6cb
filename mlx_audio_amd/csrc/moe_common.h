// What the two grouped expert GEMMs (moe.hip on float images, moe_quant.hip on packed codes) share on the host: the workspace layout behind
// mi355_moe_plan, its check, and the launch of the weighted combine (the kernel itself is in moe.hip).
#pragma once
#include "common.h"

struct Layout {
  int64_t h, y, counts, offsets, perm, tiles, total, max_tiles;
};

inline bool moe_layout(int64_t N, int64_t k, int64_t E, int64_t D, int64_t I, Layout* L) {
  if (N < 1 || k < 1 || E < 1 || D < 1 || I < 1 || N * k > (1 << 30) / 4 || N * k * (D > I ? D : I) > ((int64_t)1 << 40)) return false;
  const int64_t P = N * k;
  auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
  L->max_tiles = (P + MI355_MOE_TILE_ROWS - 1) / MI355_MOE_TILE_ROWS + E;
  L->h = 0;
  L->y = L->h + up(P * I * 4);
  L->counts = L->y + up(P * D * 4);
  L->offsets = L->counts + up(E * 4);
  L->perm = L->offsets + up((E + 1) * 4);
  L->tiles = L->perm + up(P * 4);
  L->total = L->tiles + up(L->max_tiles * 16);
  return true;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline int moe_workspace_check(const char* who, int N, int k, int E, int D, int I, const void* ws, int64_t bytes, Layout* L) {
  MI355_REQUIRE(moe_layout(N, k, E, D, I, L), "%s: bad sizes (N = %d, k = %d, E = %d, D = %d, I = %d)", who, N, k, E, D, I);
  MI355_REQUIRE(ws && aligned16(ws), "%s: the workspace must be a 16-byte aligned device buffer", who);
  MI355_REQUIRE(bytes >= L->total, "%s: workspace of %lld bytes is short of mi355_moe_workspace_bytes = %lld", who, (long long)bytes, (long long)L->total);
  return MI355_OK;
}

// out[t] = sum_slot weights[t, slot] * y[t k + slot] + shared[t] + res[t]: one launch of moe_combine_kernel (moe.hip), unchecked
void moe_combine_launch(const float* y, const float* weights, int N, int k, int D, const float* shared, int64_t ld_shared, const float* res, int64_t ld_res,
                        float* out, int64_t ldo, hipStream_t stream);
