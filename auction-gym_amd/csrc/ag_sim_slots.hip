// ag_sim_slots.hip -- the multi-slot kernels: k_simulate's SLOTS builds (ag_simulate_slots) and
// k_allocate_slots (ag_allocate_slots). A build ranks up to SM + 1 bids per lane in registers
// (ag_sim.h TopList); SM is 2, 4 or 8 and the host picks the smallest that holds the context's
// max_slots; the Makefile compiles this file once per SM (-DAG_SM), in parallel. 256-lane
// workgroups, D = E + 1 = 2..8, screened and exact item search, OracleAllocator + TruthfulBidder
// populations (kGenOracle) and any population (kGenAll); and their generate-mode builds
// (ag_simulate_slots_generated), which draw every input in the kernel.
#include "ag_sim.h"

#ifndef AG_SM
#error "compile with -DAG_SM=<2, 4 or 8>"
#endif

namespace ag {
namespace {

template <int SM, bool PRUNE, int G>
SimKernel pick_d(int D) {
  switch (D) {
    case 2: return k_simulate<0, 2, PRUNE, G, kThreads, 0, false, SM>;
    case 3: return k_simulate<0, 3, PRUNE, G, kThreads, 0, false, SM>;
    case 4: return k_simulate<0, 4, PRUNE, G, kThreads, 0, false, SM>;
    case 5: return k_simulate<0, 5, PRUNE, G, kThreads, 0, false, SM>;
    case 6: return k_simulate<0, 6, PRUNE, G, kThreads, 0, false, SM>;
    case 7: return k_simulate<0, 7, PRUNE, G, kThreads, 0, false, SM>;
    case 8: return k_simulate<0, 8, PRUNE, G, kThreads, 0, false, SM>;
    default: return nullptr;
  }
}

// the generate-mode builds (ag_simulate_slots_generated): Oracle + Truthful populations at every
// D; general populations at the shipped width only (the generate mode's LR-TS noise is drawn at a
// compile-time width, ts_gen_item)
template <int SM, bool PRUNE>
SimKernel pick_gen_d(int D, int general) {
  if (general) return D == 6 ? k_simulate<0, 6, PRUNE, kGenAll, kThreads, kShipDo, true, SM> : nullptr;
  switch (D) {
    case 2: return k_simulate<0, 2, PRUNE, kGenOracle, kThreads, 0, true, SM>;
    case 3: return k_simulate<0, 3, PRUNE, kGenOracle, kThreads, 0, true, SM>;
    case 4: return k_simulate<0, 4, PRUNE, kGenOracle, kThreads, 0, true, SM>;
    case 5: return k_simulate<0, 5, PRUNE, kGenOracle, kThreads, 0, true, SM>;
    case 6: return k_simulate<0, 6, PRUNE, kGenOracle, kThreads, 0, true, SM>;
    case 7: return k_simulate<0, 7, PRUNE, kGenOracle, kThreads, 0, true, SM>;
    case 8: return k_simulate<0, 8, PRUNE, kGenOracle, kThreads, 0, true, SM>;
    default: return nullptr;
  }
}

template <int SM>
SimKernel pick_sm(int D, bool prune, int general, bool gen) {
  if (gen) return prune ? pick_gen_d<SM, true>(D, general) : pick_gen_d<SM, false>(D, general);
  if (general) return prune ? pick_d<SM, true, kGenAll>(D) : pick_d<SM, false, kGenAll>(D);
  return prune ? pick_d<SM, true, kGenOracle>(D) : pick_d<SM, false, kGenOracle>(D);
}

// Batched AllocationMechanism.allocate(bids, num_slots) (src/AuctionAllocation.py:18-35): one
// auction per lane over the coalesced [P][B] rows, the ranking of ag_sim.h TopList; the arrays
// the reference returns, padded to max_slots rows with -1 / NaN.
template <int SM>
__global__ __launch_bounds__(kThreads) void k_allocate_slots(const double *__restrict__ bids,
                                                             const int32_t *__restrict__ num_slots, int max_slots,
                                                             int64_t B, int P, int mech, int32_t *winner,
                                                             double *price, double *second) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < B; i += (int64_t)gridDim.x * kThreads) {
    int n = num_slots ? num_slots[i] : max_slots;
    n = n < 1 ? 1 : (n > max_slots ? max_slots : n);
    TopList<SM, false> top;
    top.init();
    for (int s = 0; s < P; ++s) top.insert(s, bids[(int64_t)s * B + i], 0.0);
    const int nw = n < P ? n : P;          // winners, and FirstPrice prices: sorted[:n]
    const int ns = n < P - 1 ? n : P - 1;  // sorted[1:n + 1]
#pragma unroll
    for (int k = 0; k < SM; ++k) {
      if (k < max_slots) {
        const int64_t o = (int64_t)k * B + i;
        if (winner) winner[o] = k < nw ? top.slot[k] : -1;
        if (price)
          price[o] = mech == AG_FIRST_PRICE ? (k < nw ? top.bid[k] : (double)NAN)
                                            : (k < ns ? top.bid[k + 1] : (double)NAN);
        if (second) second[o] = k < ns ? top.bid[k + 1] : (double)NAN;
      }
    }
  }
}

}  // namespace

template <>
SimKernel pick_slots_for<AG_SM>(int D, bool prune, int general, bool gen) {
  return pick_sm<AG_SM>(D, prune, general, gen);
}

template <>
hipError_t launch_allocate_slots_for<AG_SM>(const double *bids, const int32_t *num_slots, int max_slots, int64_t B,
                                            int P, int mech, int32_t *winner, double *price, double *second,
                                            hipStream_t st) {
  const int64_t tiles = (B + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)(tiles < 8 * kMinGrid ? tiles : 8 * kMinGrid)), block(kThreads);
  hipLaunchKernelGGL(k_allocate_slots<AG_SM>, grid, block, 0, st, bids, num_slots, max_slots, B, P, mech, winner,
                     price, second);
  return hipGetLastError();
}

}  // namespace ag
