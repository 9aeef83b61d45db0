// ag_collect_slots.hip -- the record collectors of multi-slot rounds (ag_simulate_slots):
// what Agent.update reads from the logs of src/Auction.py:68-74 (src/Agent.py:70-94,
// src/Bidder.py:62-63), appended to the stores the one-slot collectors fill (ag_lrts.hip,
// ag_shading.hip); every update downstream of the stores is slot-agnostic.
//
//  k_lrts_collect_slots     one record per FILLED slot whose winner is an LR-TS allocator: up to
//                           max_slots records per auction.
//  k_shading_collect_slots  one record per participation of a non-truthful bidder; it won iff
//                           won_slot >= 0, its utility is value * click_k - log_price (the logged
//                           price of the round, not the winner's own price_k).
//
// One lane per auction, grid-stride. A lane owns several records, so a wave reserves its store
// slots in one step: every lane counts its records, the wave takes the exclusive prefix sum of the
// counts, one lane adds the total to `count`, and each lane writes its records at consecutive
// slots -- the records of a wave are one contiguous span of every store column. Records at a slot
// >= capacity are dropped while `count` still advances (the update reports the overflow).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ag_host.h"

namespace {

constexpr int kCsThreads = 256;

// Exclusive prefix sum of n over the wave's lanes; *total = the wave's sum. Every lane of the
// wave must call it.
__device__ __forceinline__ int wave_excl_scan(int n, int lane, int *total) {
  int incl = n;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  *total = __shfl(incl, 63, 64);
  return incl - n;
}

// The wave's first store slot for `total` records (one atomic), broadcast to its lanes.
__device__ __forceinline__ int64_t wave_reserve(unsigned long long *count, int total, int lane) {
  unsigned long long first = 0;
  if (lane == 0) first = atomicAdd(count, (unsigned long long)total);
  return (int64_t)__shfl(first, 0, 64);
}

__global__ __launch_bounds__(kCsThreads) void k_lrts_collect_slots(
    int64_t B, int P, int S, int OE, const double *__restrict__ ctx, const int32_t *__restrict__ part,
    const int32_t *__restrict__ winner, const uint8_t *__restrict__ outcome, const int32_t *__restrict__ num_filled,
    const int32_t *__restrict__ item, const int32_t *__restrict__ akind, uint32_t *__restrict__ key,
    float *__restrict__ x, int64_t cap, unsigned long long *__restrict__ count) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * kCsThreads; base < B; base += (int64_t)gridDim.x * kCsThreads) {
    const int64_t i = base + threadIdx.x;
    uint32_t keys[AG_MAX_SLOTS];
    int n = 0;
    if (i < B) {
      int F = num_filled[i];  // min(n, P - 1): 0 at P == 1, where nobody is charged
      F = F < S ? F : S;
#pragma unroll
      for (int k = 0; k < AG_MAX_SLOTS; ++k) {
        uint32_t kk = 0;
        bool take = false;
        if (k < F) {
          const int w = winner[(size_t)k * B + i];
          if (w >= 0 && w < P) {
            const int a = part[(size_t)w * B + i];
            take = akind[a] == AG_ALLOCATOR_LRTS;
            kk = ((uint32_t)a << 16) | ((uint32_t)item[(size_t)w * B + i] << 1) |
                 (outcome[(size_t)k * B + i] != 0 ? 1u : 0u);
          }
        }
        // the lane's records packed to the front of keys[] (static indices: registers)
#pragma unroll
        for (int j = 0; j <= k; ++j)
          if (take && j == n) keys[j] = kk;
        n += take ? 1 : 0;
      }
    }
    int total;
    const int excl = wave_excl_scan(n, lane, &total);
    if (total == 0) continue;
    const int64_t slot0 = wave_reserve(count, total, lane) + excl;
    if (n == 0) continue;
#pragma unroll
    for (int j = 0; j < AG_MAX_SLOTS; ++j)
      if (j < n && slot0 + j < cap) key[slot0 + j] = keys[j];
    for (int d = 0; d <= OE; ++d) {  // the context row once per auction, whatever its records
      const float v = d < OE ? (float)ctx[(size_t)d * B + i] : 1.0f;
      for (int j = 0; j < n; ++j)
        if (slot0 + j < cap) x[(size_t)d * cap + slot0 + j] = v;
    }
  }
}

struct ShSlotsIn {
  const int32_t *part;     // [P][B]
  const int8_t *won_slot;  // [P][B]
  const double *log_price; // [B]
  const uint8_t *outcome;  // [S][B]
  const int32_t *item;     // [P][B]
  const double *gamma, *est_ctr, *propensity;  // [P][B]
};

__global__ __launch_bounds__(kCsThreads) void k_shading_collect_slots(
    int64_t first, int64_t B, int P, int S, int K, ShSlotsIn in, const int32_t *__restrict__ bkind,
    const double *__restrict__ values, ag_shading_samples st, unsigned long long *__restrict__ count) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * kCsThreads; base < B; base += (int64_t)gridDim.x * kCsThreads) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < B;
    int n = 0;
    if (live)
      for (int s = 0; s < P; ++s) n += bkind[in.part[(size_t)s * B + i]] != AG_BIDDER_TRUTHFUL ? 1 : 0;
    int total;
    const int excl = wave_excl_scan(n, lane, &total);
    if (total == 0) continue;
    int64_t slot = wave_reserve(count, total, lane) + excl;
    if (n == 0) continue;
    const double lp = in.log_price[i];  // NaN when F = 0: then nobody won and it is not used
    for (int s = 0; s < P; ++s) {
      const size_t o = (size_t)s * B + i;
      const int a = in.part[o];
      if (bkind[a] == AG_BIDDER_TRUTHFUL) continue;  // Empirical, ValueLearning, PolicyLearning, DR
      const int64_t at = slot++;
      if (at >= st.capacity) continue;  // overflow: reported by the update
      const int k = in.won_slot[o];
      const bool won = k >= 0 && k < S;
      const double v = values[(size_t)a * K + in.item[o]];
      const double oc = won && in.outcome[(size_t)k * B + i] != 0 ? 1.0 : 0.0;
      st.agent[at] = a;
      st.gamma[at] = in.gamma[o];
      st.utility[at] = won ? v * oc - lp : 0.0;  // src/Bidder.py:62-63 on the logged price
      if (st.ctr) st.ctr[at] = in.est_ctr[o];
      if (st.value) st.value[at] = v;
      if (st.propensity) st.propensity[at] = in.propensity[o];
      if (st.won) st.won[at] = won ? 1 : 0;
      if (st.order) st.order[at] = (uint64_t)(first + i) * (uint64_t)P + (uint64_t)s;
    }
  }
}

int grid_over(int64_t n) { return agtrain::grid_over(n, kCsThreads); }

}  // namespace

extern "C" {

int ag_lrts_collect_slots(ag_ctx *c, int64_t B, const ag_batch_in *in, const ag_slots_out *out,
                          const ag_lrts_samples *s, void *stream) {
  const char *who = "ag_lrts_collect_slots";
  if (!c || !s || !in || !out) return ag_set_error(AG_ERR_INVALID, "%s: null argument", who);
  AG_CHECK_STRUCT(s, who, "ag_lrts_samples");
  AG_CHECK_STRUCT(in, who, "ag_batch_in");
  AG_CHECK_STRUCT(out, who, "ag_slots_out");
  if (!s->key || !s->x || !s->count || s->capacity < 0)
    return ag_set_error(AG_ERR_INVALID, "%s: sample store needs key, x, count and capacity >= 0", who);
  if (B < 0) return ag_set_error(AG_ERR_INVALID, "%s: B < 0", who);
  if (B == 0 || !c->has_lrts) return AG_OK;
  if (c->shape.num_agents > 65536 || c->shape.num_items > 32768)
    return ag_set_error(AG_ERR_UNSUPPORTED, "%s: sample keys hold N <= 65536, K <= 32768", who);
  if (!in->ctx || !in->part || !out->winner || !out->outcome || !out->num_filled || !out->item)
    return ag_set_error(AG_ERR_INVALID, "%s: needs in.ctx, in.part, out.winner, out.outcome, out.num_filled "
                                        "and out.item", who);
  AgDeviceGuard g(c->device);
  hipLaunchKernelGGL(k_lrts_collect_slots, dim3(grid_over(B)), dim3(kCsThreads), 0, (hipStream_t)stream, B,
                     c->shape.num_participants, c->shape.num_slots, c->shape.obs_embedding_size, in->ctx, in->part,
                     out->winner, out->outcome, out->num_filled, out->item, c->d_akind, s->key, s->x, s->capacity,
                     (unsigned long long *)s->count);
  AG_HIP(hipGetLastError());
  return AG_OK;
}

int ag_shading_collect_slots(ag_ctx *c, int64_t first, int64_t B, const ag_batch_in *in, const ag_slots_out *out,
                             const ag_shading_samples *s, void *stream) {
  const char *who = "ag_shading_collect_slots";
  if (!c || !s || !in || !out) return ag_set_error(AG_ERR_INVALID, "%s: null argument", who);
  AG_CHECK_STRUCT(s, who, "ag_shading_samples");
  AG_CHECK_STRUCT(in, who, "ag_batch_in");
  AG_CHECK_STRUCT(out, who, "ag_slots_out");
  if (!s->agent || !s->gamma || !s->utility || !s->count || s->capacity < 0)
    return ag_set_error(AG_ERR_INVALID, "%s: sample store needs agent, gamma, utility, count, capacity", who);
  if (B < 0) return ag_set_error(AG_ERR_INVALID, "%s: B < 0", who);
  if (B == 0 || !c->has_shading) return AG_OK;
  if (!in->part || !out->won_slot || !out->log_price || !out->outcome || !out->item || !out->gamma)
    return ag_set_error(AG_ERR_INVALID, "%s: needs in.part, out.won_slot, out.log_price, out.outcome, out.item "
                                        "and out.gamma", who);
  if ((s->ctr && !out->est_ctr) || (s->propensity && !out->propensity))
    return ag_set_error(AG_ERR_INVALID, "%s: the store's ctr / propensity need out.est_ctr / out.propensity", who);
  AgDeviceGuard g(c->device);
  const ShSlotsIn ki{in->part, out->won_slot, out->log_price, out->outcome, out->item, out->gamma, out->est_ctr,
                     out->propensity};
  hipLaunchKernelGGL(k_shading_collect_slots, dim3(grid_over(B)), dim3(kCsThreads), 0, (hipStream_t)stream, first, B,
                     c->shape.num_participants, c->shape.num_slots, c->shape.num_items, ki, c->d_bkind, c->d_values,
                     *s, (unsigned long long *)s->count);
  AG_HIP(hipGetLastError());
  return AG_OK;
}

}  // extern "C"
