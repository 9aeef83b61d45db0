// ag_collect.hip -- the record collectors: what Agent.update reads from the logs of a launch
// (src/Auction.py:68-74, src/Agent.py:70-94, src/Bidder.py:62-63), appended to caller-owned
// stores. The updates downstream of the stores (ag_lrts.hip, ag_shading.hip, ag_dr.hip) do not
// know how many slots a round had.
//
//  k_lrts_collect     one record per filled slot whose winner is an LR-TS allocator: (agent, item,
//                     click) packed into a key, and the observed context + 1.
//  k_shading_collect  one record per participation of a non-truthful bidder: (agent, gamma, net
//                     utility) and, where the store has them, ctr, value, propensity, won, order.
//
// Each kernel is a template over an output view: OneSlotView reads ag_simulate's ag_batch_out
// (ag_lrts_collect, ag_shading_collect), SlotsView reads ag_simulate_slots' ag_slots_out
// (ag_lrts_collect_slots, ag_shading_collect_slots). A view says how many LR-TS records a lane may
// own, who won a rank (or which rank a participant won) and whether it was clicked, and which
// price the utility is taken on.
//
// One lane per auction, grid-stride. A wave reserves its store slots in one step: every lane
// counts its records, the wave takes the exclusive prefix sum of the counts, one lane adds the
// total to `count`, and each lane writes its records at consecutive slots -- the records of a
// wave are one contiguous span of every store column. Records at a slot >= capacity are dropped
// while `count` still advances (the update reports the overflow).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ag_host.h"

namespace {

constexpr int kThreads = 256;

// ag_simulate's outputs: one slot, so at most one winner per auction, and nobody wins at P == 1
// (nobody is charged, src/Auction.py:68). Winner and click from their arrays, or from the ABI 17
// packed word (bit 31 is the click).
struct OneSlotView {
  using Out = ag_batch_out;
  static constexpr int kMaxWon = 1;  // LR-TS records a lane may own
  const int32_t *winner;             // [B], with outcome [B]; NULL: the packed word is read
  const uint8_t *outcome;
  const uint32_t *winner_outcome;    // [B]
  const double *price_;              // [B]
  int P;

  static OneSlotView make(const Out &o, int64_t, const ag_shape &sh) {
    const bool fields = o.winner && o.outcome;
    return {fields ? o.winner : nullptr, fields ? o.outcome : nullptr, o.winner_outcome, o.price, sh.num_participants};
  }
  static bool has_winners(const Out &o) { return (o.winner && o.outcome) || o.winner_outcome; }
  static bool lrts_ready(const Out &o) { return o.item && has_winners(o); }
  static bool shading_ready(const Out &o) { return has_winners(o) && o.item && o.price && o.gamma; }
  static constexpr const char *kLrtsNeeds = "in.ctx, in.part, out.item and out.winner + out.outcome (or "
                                            "out.winner_outcome)";
  static constexpr const char *kShadingNeeds = "in.part, out.winner + out.outcome (or out.winner_outcome), "
                                               "out.item, out.price, out.gamma";

  struct Round {  // an auction's winner and click, read once
    int w;
    bool clicked;
  };
  __device__ Round round(int64_t i) const {
    if (winner) return {winner[i], outcome[i] != 0};
    const uint32_t wo = winner_outcome[i];
    return {(int)(wo & 0x7fffffffu), (wo >> 31) != 0};
  }
  __device__ int filled(int64_t) const { return P >= 2 ? 1 : 0; }
  // the participant slot that won rank k (0 here)
  __device__ int winner_of(const Round &r, int, int64_t, bool *clicked) const {
    *clicked = r.clicked;
    return r.w;
  }
  // the rank participant slot s won, or -1
  __device__ int rank_of(const Round &r, int s, int64_t, bool *clicked) const {
    *clicked = r.clicked;
    return (r.w == s && P >= 2) ? 0 : -1;
  }
  __device__ double price(int64_t i) const { return price_[i]; }
};

// ag_simulate_slots' outputs: up to min(max_slots, P - 1) winners per auction; utilities on the
// logged price of the round, not the winner's own price_k.
struct SlotsView {
  using Out = ag_slots_out;
  static constexpr int kMaxWon = AG_MAX_SLOTS;
  const int32_t *winner;      // [S][B]
  const uint8_t *outcome;     // [S][B]
  const int32_t *num_filled;  // [B]
  const int8_t *won_slot;     // [P][B]
  const double *log_price;    // [B]
  int64_t B;
  int S;

  static SlotsView make(const Out &o, int64_t B, const ag_shape &sh) {
    return {o.winner, o.outcome, o.num_filled, o.won_slot, o.log_price, B, sh.num_slots};
  }
  static bool lrts_ready(const Out &o) { return o.winner && o.outcome && o.num_filled && o.item; }
  static bool shading_ready(const Out &o) { return o.won_slot && o.log_price && o.outcome && o.item && o.gamma; }
  static constexpr const char *kLrtsNeeds = "in.ctx, in.part, out.winner, out.outcome, out.num_filled and out.item";
  static constexpr const char *kShadingNeeds = "in.part, out.won_slot, out.log_price, out.outcome, out.item and "
                                               "out.gamma";

  __device__ int filled(int64_t i) const {  // min(n, P - 1): 0 at P == 1
    const int F = num_filled[i];
    return F < S ? F : S;
  }
  struct Round {};  // every read is per rank or per participant
  __device__ Round round(int64_t) const { return {}; }
  __device__ int winner_of(const Round &, int k, int64_t i, bool *clicked) const {
    *clicked = outcome[(size_t)k * B + i] != 0;
    return winner[(size_t)k * B + i];
  }
  __device__ int rank_of(const Round &, int s, int64_t i, bool *clicked) const {
    const int k = won_slot[(size_t)s * B + i];
    const bool won = k >= 0 && k < S;
    *clicked = won && outcome[(size_t)k * B + i] != 0;
    return won ? k : -1;
  }
  __device__ double price(int64_t i) const { return log_price[i]; }  // NaN when no slot was filled: not used then
};

// A wave's store slots for its lanes' records: lane l of the wave gets n_l consecutive slots from
// the returned one (meaningless where n == 0); *total = the wave's records. One atomic per wave.
// Every lane of the wave must call it.
__device__ __forceinline__ int64_t wave_reserve(unsigned long long *count, int n, int *total) {
  const int lane = threadIdx.x & 63;
  int incl = n;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  *total = __shfl(incl, 63, 64);
  if (*total == 0) return 0;
  unsigned long long first = 0;
  if (lane == 0) first = atomicAdd(count, (unsigned long long)*total);
  return (int64_t)__shfl(first, 0, 64) + (incl - n);
}

template <class View>
__global__ __launch_bounds__(kThreads) void k_lrts_collect(
    int64_t B, int P, int OE, const double *__restrict__ ctx, const int32_t *__restrict__ part,
    const int32_t *__restrict__ item, View v, const int32_t *__restrict__ akind, uint32_t *__restrict__ key,
    float *__restrict__ x, int64_t cap, unsigned long long *__restrict__ count) {
  for (int64_t base = (int64_t)blockIdx.x * kThreads; base < B; base += (int64_t)gridDim.x * kThreads) {
    const int64_t i = base + threadIdx.x;
    uint32_t keys[View::kMaxWon];
    int n = 0;
    if (i < B) {
      const int F = v.filled(i);
      const typename View::Round r = v.round(i);
#pragma unroll
      for (int k = 0; k < View::kMaxWon; ++k) {
        uint32_t kk = 0;
        bool take = false;
        if (k < F) {
          bool clicked;
          const int w = v.winner_of(r, k, i, &clicked);
          if (w >= 0 && w < P) {
            const int a = part[(size_t)w * B + i];
            take = akind[a] == AG_ALLOCATOR_LRTS;
            kk = ((uint32_t)a << 16) | ((uint32_t)item[(size_t)w * B + i] << 1) | (clicked ? 1u : 0u);
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
    const int64_t slot0 = wave_reserve(count, n, &total);
    if (n == 0) continue;
#pragma unroll
    for (int j = 0; j < View::kMaxWon; ++j)
      if (j < n && slot0 + j < cap) key[slot0 + j] = keys[j];
    for (int d = 0; d <= OE; ++d) {  // the context row once per auction, whatever its records
      const float c = d < OE ? (float)ctx[(size_t)d * B + i] : 1.0f;
      for (int j = 0; j < n; ++j)
        if (slot0 + j < cap) x[(size_t)d * cap + slot0 + j] = c;
    }
  }
}

struct ShadingIn {  // per participation, [P][B]
  const int32_t *part, *item;
  const double *gamma, *est_ctr, *propensity;
};

template <class View>
__global__ __launch_bounds__(kThreads) void k_shading_collect(
    int64_t first, int64_t B, int P, int K, View v, ShadingIn in, const int32_t *__restrict__ bkind,
    const double *__restrict__ values, ag_shading_samples st) {
  for (int64_t base = (int64_t)blockIdx.x * kThreads; base < B; base += (int64_t)gridDim.x * kThreads) {
    const int64_t i = base + threadIdx.x;
    int n = 0;
    if (i < B)
      for (int s = 0; s < P; ++s) n += bkind[in.part[(size_t)s * B + i]] != AG_BIDDER_TRUTHFUL ? 1 : 0;
    int total;
    int64_t slot = wave_reserve((unsigned long long *)st.count, n, &total);
    if (n == 0) continue;
    const double price = v.price(i);
    const typename View::Round r = v.round(i);
    for (int s = 0; s < P; ++s) {
      const size_t o = (size_t)s * B + i;
      const int a = in.part[o];
      if (bkind[a] == AG_BIDDER_TRUTHFUL) continue;  // Empirical, ValueLearning, PolicyLearning, DR
      const int64_t at = slot++;
      if (at >= st.capacity) continue;  // overflow: reported by the update
      bool clicked;
      const bool won = v.rank_of(r, s, i, &clicked) >= 0;
      const double val = values[(size_t)a * K + in.item[o]];
      st.agent[at] = a;
      st.gamma[at] = in.gamma[o];
      st.utility[at] = won ? val * (clicked ? 1.0 : 0.0) - price : 0.0;  // src/Bidder.py:62-63
      if (st.ctr) st.ctr[at] = in.est_ctr[o];
      if (st.value) st.value[at] = val;
      if (st.propensity) st.propensity[at] = in.propensity[o];
      if (st.won) st.won[at] = won ? 1 : 0;
      if (st.order) st.order[at] = (uint64_t)(first + i) * (uint64_t)P + (uint64_t)s;
    }
  }
}

// ag_batch_out in either of its layouts, ag_slots_out in its one
int read_out(const ag_batch_out *p, ag_batch_out *v, const char *who) { return ag_read_out(p, v, who); }
int read_out(const ag_slots_out *p, ag_slots_out *v, const char *who) {
  if (int rc = ag_check_struct(p, who, "ag_slots_out")) return rc;
  *v = *p;
  return AG_OK;
}

template <class View>
int lrts_collect(const char *who, ag_ctx *c, int64_t B, const ag_batch_in *in, const typename View::Out *out_arg,
                 const ag_lrts_samples *s, void *stream) {
  if (int rc = ag_check_store(c, s, who)) return rc;
  if (!in || !out_arg) return ag_set_error(AG_ERR_INVALID, "%s: null argument", who);
  AG_CHECK_STRUCT(in, who, "ag_batch_in");
  typename View::Out out;
  if (int rc = read_out(out_arg, &out, who)) return rc;
  if (B < 0) return ag_set_error(AG_ERR_INVALID, "%s: B < 0", who);
  if (B == 0 || !c->has_lrts) return AG_OK;
  if (c->shape.num_agents > 65536 || c->shape.num_items > 32768)
    return ag_set_error(AG_ERR_UNSUPPORTED, "%s: sample keys hold N <= 65536, K <= 32768", who);
  if (!in->ctx || !in->part || !View::lrts_ready(out))
    return ag_set_error(AG_ERR_INVALID, "%s: needs %s", who, View::kLrtsNeeds);
  AgDeviceGuard g(c->device);
  hipLaunchKernelGGL(k_lrts_collect<View>, dim3(agtrain::grid_over(B, kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, B, c->shape.num_participants, c->shape.obs_embedding_size, in->ctx, in->part,
                     out.item, View::make(out, B, c->shape), c->d_akind, s->key, s->x, s->capacity,
                     (unsigned long long *)s->count);
  AG_HIP(hipGetLastError());
  return AG_OK;
}

template <class View>
int shading_collect(const char *who, ag_ctx *c, int64_t first, int64_t B, const ag_batch_in *in,
                    const typename View::Out *out_arg, const ag_shading_samples *s, void *stream) {
  if (int rc = ag_check_store(c, s, who)) return rc;
  if (!in || !out_arg) return ag_set_error(AG_ERR_INVALID, "%s: null argument", who);
  AG_CHECK_STRUCT(in, who, "ag_batch_in");
  typename View::Out out;
  if (int rc = read_out(out_arg, &out, who)) return rc;
  if (B < 0) return ag_set_error(AG_ERR_INVALID, "%s: B < 0", who);
  if (B == 0 || !c->has_shading) return AG_OK;
  if (!in->part || !View::shading_ready(out)) return ag_set_error(AG_ERR_INVALID, "%s: needs %s", who, View::kShadingNeeds);
  if ((s->ctr && !out.est_ctr) || (s->propensity && !out.propensity))
    return ag_set_error(AG_ERR_INVALID, "%s: the store's ctr / propensity need out.est_ctr / out.propensity", who);
  AgDeviceGuard g(c->device);
  const ShadingIn ki{in->part, out.item, out.gamma, out.est_ctr, out.propensity};
  hipLaunchKernelGGL(k_shading_collect<View>, dim3(agtrain::grid_over(B, kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, first, B, c->shape.num_participants, c->shape.num_items,
                     View::make(out, B, c->shape), ki, c->d_bkind, c->d_values, *s);
  AG_HIP(hipGetLastError());
  return AG_OK;
}

}  // namespace

extern "C" {

int ag_lrts_collect(ag_ctx *c, int64_t B, const ag_batch_in *in, const ag_batch_out *out, const ag_lrts_samples *s,
                    void *stream) {
  if (int rc = ag_one_slot_only(c, "ag_lrts_collect")) return rc;
  return lrts_collect<OneSlotView>("ag_lrts_collect", c, B, in, out, s, stream);
}

int ag_lrts_collect_slots(ag_ctx *c, int64_t B, const ag_batch_in *in, const ag_slots_out *out,
                          const ag_lrts_samples *s, void *stream) {
  return lrts_collect<SlotsView>("ag_lrts_collect_slots", c, B, in, out, s, stream);
}

int ag_shading_collect(ag_ctx *c, int64_t first, int64_t B, const ag_batch_in *in, const ag_batch_out *out,
                       const ag_shading_samples *s, void *stream) {
  if (int rc = ag_one_slot_only(c, "ag_shading_collect")) return rc;
  return shading_collect<OneSlotView>("ag_shading_collect", c, first, B, in, out, s, stream);
}

int ag_shading_collect_slots(ag_ctx *c, int64_t first, int64_t B, const ag_batch_in *in, const ag_slots_out *out,
                             const ag_shading_samples *s, void *stream) {
  return shading_collect<SlotsView>("ag_shading_collect_slots", c, first, B, in, out, s, stream);
}

}  // extern "C"
