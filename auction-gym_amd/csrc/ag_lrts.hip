// ag_lrts.hip -- LR-TS allocator update on the GPU (Agent.update -> PyTorchLogistic-
// RegressionAllocator.update, src/Agent.py:79-91, src/BidderAllocation.py:29-65,
// src/Models.py:35-48), on the won samples k_lrts_collect (ag_collect.hip) appended to a
// caller-owned store: (agent, item, outcome, observed context + 1).
//
//  1. bucket           histogram -> exclusive scan -> scatter: samples grouped by agent.
//  2. k_lrts_train     one workgroup per agent, persistent over the epochs: forward, BCE +
//                      prior loss, gradient, Adam, ReduceLROnPlateau and the early stop all
//                      on the device (no host round trip per epoch), then the Laplace
//                      update of q and prev_m = m.
//
// Every sum over samples is exact (fixed-point terms added as integers: oracle/ag_oracle.c
// ora_lrts_update states the arithmetic), so results do not depend on sample order,
// bucket order or the lane a sample lands on: the update is bit-identical to the oracle
// and identical on every rank of a multi-GPU job that trains on the gathered samples.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ag_exp.h"
#include "ag_exp_table.h"
#include "ag_host.h"
#include "ag_coop.h"
#include "ag_train_math.h"

namespace {

using namespace agtm;

constexpr int kLrThreads = 256;        // 4 waves; one sample per lane per pass
constexpr int kLrEpochs = AG_LRTS_MAX_EPOCHS;
constexpr int kLrMaxKD = 64;           // K * (OE + 1) columns of the accumulator tile
constexpr int kLrAccStride = 144;      // int64 per accumulator row: 2 (KD + 1) <= 130, 128-B multiple
constexpr int kLrCache = 16;           // samples per lane kept in registers (1 workgroup / CU)
constexpr int kAccStride = kLrThreads + 1;  // [column][lane] int64 tile, padded: the column
                                            // reduction (lanes = columns) is conflict-free
constexpr int kHistory = 100;          // losses[-100] of the early stop
constexpr int64_t kLo24 = (int64_t(1) << 24) - 1;

// fx_round, kGradScale / kLossScale and the BCE term lr_bce_term: ag_train_math.h
// (hi, lo) partial sums of values split at bit 24 -> the exact sum S read back as
// (double)(S >> 24) * 2^24 + (double)(S & (2^24 - 1)) (ora_lrts_update's fx_read).
__device__ __forceinline__ double fx_read(int64_t hi, int64_t lo, double inv_scale) {
  hi += lo >> 24;
  lo &= kLo24;
  return ((double)hi * 0x1p24 + (double)lo) * inv_scale;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------
// 1. bucket by agent
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLrThreads) void k_lrts_hist(const uint32_t *__restrict__ key, int64_t n, int N,
                                                          int64_t *__restrict__ counts) {
  extern __shared__ unsigned int s_hist[];
  for (int a = threadIdx.x; a < N; a += kLrThreads) s_hist[a] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kLrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLrThreads)
    atomicAdd(&s_hist[key[i] >> 16], 1u);
  __syncthreads();
  for (int a = threadIdx.x; a < N; a += kLrThreads)
    if (s_hist[a]) atomicAdd((unsigned long long *)&counts[a], (unsigned long long)s_hist[a]);
}

// counts [N] -> offsets [N + 1] (exclusive scan) and cursors [N] = offsets; one block.
__global__ __launch_bounds__(kLrThreads) void k_lrts_scan(int64_t *__restrict__ counts, int N,
                                                          int64_t *__restrict__ offsets,
                                                          int64_t *__restrict__ cursors) {
  __shared__ int64_t s_carry;
  __shared__ int64_t s_w[kLrThreads / 64];
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int base = 0; base < N; base += kLrThreads) {
    const int a = base + threadIdx.x;
    const int64_t v = a < N ? counts[a] : 0;
    int64_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int64_t pre = s_carry;
    for (int j = 0; j < wv; ++j) pre += s_w[j];
    if (a < N) {
      offsets[a] = pre + incl - v;
      cursors[a] = pre + incl - v;
    }
    __syncthreads();
    if (threadIdx.x == kLrThreads - 1) s_carry = pre + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[N] = s_carry;
}

__global__ __launch_bounds__(kLrThreads) void k_lrts_scatter(const uint32_t *__restrict__ key,
                                                             const float *__restrict__ x, int64_t n,
                                                             int64_t cap_in, int Do,
                                                             int64_t *__restrict__ cursors,
                                                             uint32_t *__restrict__ okey,
                                                             float *__restrict__ ox, int64_t cap_out) {
  for (int64_t i = (int64_t)blockIdx.x * kLrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLrThreads) {
    const uint32_t k = key[i];
    const int64_t pos = (int64_t)atomicAdd((unsigned long long *)&cursors[k >> 16], 1ull);
    okey[pos] = k;
    for (int d = 0; d < Do; ++d) ox[(size_t)d * cap_out + pos] = x[(size_t)d * cap_in + i];
  }
}

// ---------------------------------------------------------------------------------------
// 2. training: up to kLrCache * 256 samples per workgroup, several workgroups per agent
// ---------------------------------------------------------------------------------------
struct LrSample {
  float x[AG_LRTS_MAX_DO];
  int item;
  int y;
};

template <int DO>
__device__ __forceinline__ float lr_logit(const float *__restrict__ w, const float (&x)[AG_LRTS_MAX_DO]) {
  float z = w[0] * x[0];
#pragma unroll
  for (int d = 1; d < DO; ++d) z = z + w[d] * x[d];
  return z;
}

template <int DO>
__device__ __forceinline__ void lr_load(const uint32_t *__restrict__ key, const float *__restrict__ x,
                                        int64_t cap, int64_t i, LrSample &s) {
  const uint32_t k = key[i];
  s.item = (int)((k >> 1) & 0x7fffu);
  s.y = (int)(k & 1u);
#pragma unroll
  for (int d = 0; d < DO; ++d) s.x[d] = x[(size_t)d * cap + i];
}

// One sample's contribution to the epoch: BCE term (fixed point, returned) and gradient
// terms added to this lane's accumulator column.
template <int DO>
__device__ __forceinline__ int64_t lr_epoch_sample(const LrSample &s, const float *__restrict__ sm,
                                                   int64_t *__restrict__ acc, const uint64_t *tab) {
  const float z = lr_logit<DO>(sm + s.item * DO, s.x);
  const float p = 1.0f / (1.0f + (float)agexp::exp_fast(-(double)z, tab));
  const double t = lr_bce_term(p, s.y);
  const double gz = (double)p - (double)s.y;
#pragma unroll
  for (int d = 0; d < DO; ++d) acc[(s.item * DO + d) * kAccStride] += fx_round(gz * (double)s.x[d], kGradScale);
  return fx_round(t, kLossScale);
}

template <int DO>
__device__ __forceinline__ void lr_laplace_sample(const LrSample &s, const float *__restrict__ sm,
                                                  int64_t *__restrict__ acc, const uint64_t *tab) {
  const float z = lr_logit<DO>(sm + s.item * DO, s.x);
  const float P = 1.0f / (1.0f + (float)agexp::exp_fast((double)(1.0f - z), tab));
  const float w = P * (1.0f - P);
#pragma unroll
  for (int d = 0; d < DO; ++d)
    acc[(s.item * DO + d) * kAccStride] += fx_round((double)w * (double)(s.x[d] * s.x[d]), kGradScale);
}

// Per-block column sums of the lane accumulator tile (thread = column c, row group r;
// each value split at bit 24 so no partial can overflow) into the block's slot of the
// agent's partials [rank][KD + 1][2] (column KD: the loss); the tile is zeroed for reuse.
__device__ __forceinline__ void lr_block_partials(int64_t *__restrict__ s_acc, int KD, int64_t lsum_hi,
                                                  int64_t lsum_lo, int64_t (*s_hi)[kLrMaxKD + 1],
                                                  int64_t (*s_lo)[kLrMaxKD + 1], int64_t *__restrict__ dst) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  {
    const int64_t h = wave_sum(lsum_hi), l = wave_sum(lsum_lo);
    if (lane == 0) {
      s_hi[wv][KD] = h;
      s_lo[wv][KD] = l;
    }
  }
  const int c = tid & 63, r = tid >> 6;
  if (c < KD) {
    int64_t h = 0, l = 0;
    int64_t *col = s_acc + c * kAccStride + r * 64;
    for (int j = 0; j < 64; ++j) {
      const int64_t v = col[j];
      col[j] = 0;
      h += v >> 24;
      l += v & kLo24;
    }
    s_hi[r][c] = h;
    s_lo[r][c] = l;
  }
  __syncthreads();
  if (tid <= KD) {
    dst[2 * tid] = s_hi[0][tid] + s_hi[1][tid] + s_hi[2][tid] + s_hi[3][tid];
    dst[2 * tid + 1] = s_lo[0][tid] + s_lo[1][tid] + s_lo[2][tid] + s_lo[3][tid];
  }
}

// The training of one LR-TS agent is spread over `nblk` co-resident workgroups, each
// owning a contiguous chunk of the agent's samples (the first kLrCache per lane in
// registers). Every epoch each workgroup writes its exact partial sums; after the agent
// barrier EVERY workgroup adds all partials (integers: identical totals everywhere) and
// runs the same Adam / scheduler / early-stop step on its LDS copy of the parameters, so
// the workgroups stay in lockstep without a second barrier. Partials are double-buffered
// by epoch parity.
template <int DO>
__global__ __launch_bounds__(kLrThreads) void k_lrts_train(
    int K, const int32_t *__restrict__ blk_agent, const int32_t *__restrict__ blk_rank,
    const int32_t *__restrict__ agent_nblk, const int64_t *__restrict__ agent_pbase,
    const int64_t *__restrict__ offsets, const uint32_t *__restrict__ key, const float *__restrict__ xs,
    int64_t cap, float *__restrict__ gm, float *__restrict__ gq, float *__restrict__ gpm,
    const double *__restrict__ adam_tab, int32_t *__restrict__ epochs_out, float *__restrict__ loss_trace,
    int64_t *__restrict__ partials, unsigned *__restrict__ barriers, const int32_t *__restrict__ bar_off) {
  const int a = blk_agent[blockIdx.x], rank = blk_rank[blockIdx.x], nblk = agent_nblk[a];
  const int tid = threadIdx.x;
  const int64_t s0 = offsets[a], n = offsets[a + 1] - s0;
  const int KD = K * DO;
  const int PW = 2 * (KD + 1);  // int64 per partial record
  // the agent's accumulator rows [bar_lines(nblk)][kLrAccStride] (agcoop::agent_allreduce_i64)
  int64_t *accrows = partials + agent_pbase[a];
  unsigned *bar = barriers + (size_t)bar_off[a] * agcoop::kBarLineWords;
  // this workgroup's samples: [c0, c1) of the agent's n
  const int64_t per = (n + nblk - 1) / nblk;
  const int64_t c0 = (int64_t)rank * per, c1 = c0 + per < n ? c0 + per : n;
  const int64_t nb = c1 > c0 ? c1 - c0 : 0;

  extern __shared__ int64_t s_acc[];  // [KD][kAccStride]
  __shared__ uint64_t s_tab[256];
  __shared__ float s_m[kLrMaxKD], s_pm[kLrMaxKD], s_q[kLrMaxKD], s_ea[kLrMaxKD], s_es[kLrMaxKD];
  __shared__ int64_t s_hi[4][kLrMaxKD + 1], s_lo[4][kLrMaxKD + 1];
  __shared__ float s_hist[kHistory];
  __shared__ float s_loss, s_negstep, s_bc2;
  __shared__ double s_lr, s_best;
  __shared__ int s_bad, s_stop, s_flag;
  __shared__ int64_t s_part[2 * (kLrMaxKD + 1)], s_tot[2 * (kLrMaxKD + 1)];

  for (int i = tid; i < 256; i += kLrThreads) s_tab[i] = ag_exp_tab[i];
  float *m_g = gm + (size_t)a * KD, *q_g = gq + (size_t)a * KD, *pm_g = gpm + (size_t)a * KD;
  for (int c = tid; c < KD; c += kLrThreads) {
    s_m[c] = m_g[c];
    s_pm[c] = pm_g[c];
    s_q[c] = q_g[c];
    s_ea[c] = 0.0f;
    s_es[c] = 0.0f;
  }
  for (int i = tid; i < KD * kAccStride; i += kLrThreads) s_acc[i] = 0;
  if (tid == 0) {
    s_lr = 2e-3;
    s_best = INFINITY;
    s_bad = 0;
    s_stop = 0;
  }
  LrSample cache[kLrCache];
  int ncached = 0;
#pragma unroll
  for (int j = 0; j < kLrCache; ++j) {
    const int64_t i = (int64_t)j * kLrThreads + tid;
    if (i < nb) {
      lr_load<DO>(key, xs, cap, s0 + c0 + i, cache[j]);
      ncached = j + 1;
    }
  }
  const int64_t stream_from = (int64_t)kLrCache * kLrThreads;
  int64_t *acc = s_acc + tid;
  __syncthreads();

  int epoch = 0;
  for (; epoch < kLrEpochs; ++epoch) {
    // ---- A: forward + BCE + gradient terms of this lane's samples
    int64_t lsum = 0;
#pragma unroll
    for (int j = 0; j < kLrCache; ++j)
      if (j < ncached) lsum += lr_epoch_sample<DO>(cache[j], s_m, acc, s_tab);
    for (int64_t i = stream_from + tid; i < nb; i += kLrThreads) {
      LrSample sm;
      lr_load<DO>(key, xs, cap, s0 + c0 + i, sm);
      lsum += lr_epoch_sample<DO>(sm, s_m, acc, s_tab);
    }
    __syncthreads();
    // ---- B: this workgroup's exact partials, summed over the agent's workgroups up the
    // barrier tree (exact integer atomics; every workgroup gets the same totals)
    lr_block_partials(s_acc, KD, lsum >> 24, lsum & kLo24, s_hi, s_lo, s_part);
    agcoop::agent_allreduce_i64(bar, accrows, kLrAccStride, rank, nblk, s_part, PW, s_tot, &s_flag);
    // ---- C: totals (identical in every workgroup), loss, Adam; scheduler on thread 0
    if (tid == 0) {
      const int64_t h = s_tot[2 * KD], l = s_tot[2 * KD + 1];
      double prior = 0.0;
      for (int k = 0; k < K; ++k)
        for (int d = 0; d < DO - 1; ++d) {
          const double df = (double)s_pm[k * DO + d] - (double)s_m[k * DO + d];
          prior += (double)s_q[k * DO + d] * (df * df);
        }
      s_loss = (float)(0.5 * prior + fx_read(h, l, 1.0 / kLossScale));
      s_negstep = (float)(-(s_lr / adam_tab[epoch]));
      s_bc2 = (float)adam_tab[kLrEpochs + epoch];
    }
    __syncthreads();
    if (tid < KD) {
      const int c = tid;
      const int64_t h = s_tot[2 * c], l = s_tot[2 * c + 1];
      const double gp = (c % DO) < DO - 1 ? -(double)s_q[c] * ((double)s_pm[c] - (double)s_m[c]) : 0.0;
      const float g = (float)(fx_read(h, l, 1.0 / kGradScale) + gp);
      const float ea = s_ea[c] + 0.1f * (g - s_ea[c]);
      const float es = s_es[c] * 0.999f + (0.001f * g) * g;
      // float32 sqrt correctly rounded (as the CPU sqrtss): via the refined FP64 sqrt --
      // double rounding is innocuous for sqrt (53 >= 2 * 24 + 2); v_sqrt_f32 is 1 ulp.
      const float den = (float)__builtin_sqrt((double)es) / s_bc2 + 1e-8f;
      s_ea[c] = ea;
      s_es[c] = es;
      s_m[c] = s_m[c] + s_negstep * (ea / den);
    }
    if (tid == 0) {
      const float loss = s_loss;
      if (loss_trace && rank == 0) loss_trace[(size_t)a * kLrEpochs + epoch] = loss;
      s_hist[epoch % kHistory] = loss;
      if ((double)loss < s_best * (1.0 - 1e-4)) {
        s_best = (double)loss;
        s_bad = 0;
      } else {
        s_bad += 1;
      }
      if (s_bad > 10) {
        const double nl = s_lr * 0.5;
        if (s_lr - nl > 1e-8) s_lr = nl;
        s_bad = 0;
      }
      if (epoch > 1024 && fabs((double)s_hist[(epoch - 99) % kHistory] - (double)loss) < 1e-6) s_stop = 1;
    }
    __syncthreads();
    if (s_stop) {
      ++epoch;
      break;
    }
  }

  // ---- Laplace approximation of q (src/Models.py:43-45), then prev_m = m
#pragma unroll
  for (int j = 0; j < kLrCache; ++j)
    if (j < ncached) lr_laplace_sample<DO>(cache[j], s_m, acc, s_tab);
  for (int64_t i = stream_from + tid; i < nb; i += kLrThreads) {
    LrSample sm;
    lr_load<DO>(key, xs, cap, s0 + c0 + i, sm);
    lr_laplace_sample<DO>(sm, s_m, acc, s_tab);
  }
  __syncthreads();
  lr_block_partials(s_acc, KD, 0, 0, s_hi, s_lo, s_part);
  agcoop::agent_allreduce_i64(bar, accrows, kLrAccStride, rank, nblk, s_part, PW, s_tot, &s_flag);
  if (rank == 0) {
    if (tid < KD) {
      const int c = tid;
      const int64_t h = s_tot[2 * c], l = s_tot[2 * c + 1];
      q_g[c] = s_q[c] + (float)fx_read(h, l, 1.0 / kGradScale);
      m_g[c] = s_m[c];
      pm_g[c] = s_m[c];
    }
    if (tid == 0) epochs_out[a] = epoch;
  }
}

// ---------------------------------------------------------------------------------------
// 3. resumable / record-parallel training (ag_lrts_rp_*): the same fit as k_lrts_train, one
//    launch per epoch, each agent's state (m, Adam moments, scheduler, loss history, phase) in
//    HBM between launches. Launch k steps the state with the totals of launch k - 1 (this
//    rank's workgroups summed up the agent's combining tree without waiting, then -- G ranks --
//    the caller's int64 all-reduce), then adds the next epoch's exact partials at the new m:
//    every rank holding a shard of an agent's won samples steps to the posterior one process
//    computes from all of them (ag_dr.hip k_bidder_epoch has the same structure).
// ---------------------------------------------------------------------------------------
enum { kLrTrain = 0, kLrLaplace, kLrDone };
struct LrSt {
  int32_t phase, epoch, have_tot, bad;
  double lr, best;
  float m[kLrMaxKD], ea[kLrMaxKD], es[kLrMaxKD];
  float hist[kHistory];
};

// Both parities of the state ([2][N]) are initialised: k_lrts_epoch writes st_out only for
// the masked agents, so an unmasked agent's parity-1 row must already read Done when
// ag_lrts_rp_poll looks at it after an odd number of launches.
__global__ void k_lrts_rp_init(int N, int KD, const int32_t *__restrict__ mask, const float *__restrict__ gm,
                               LrSt *__restrict__ st) {
  const int a = blockIdx.x;
  if (a >= N) return;
  for (int par = 0; par < 2; ++par) {
    LrSt &f = st[(size_t)par * N + a];
    for (int c = threadIdx.x; c < kLrMaxKD; c += blockDim.x) {
      f.m[c] = c < KD ? gm[(size_t)a * KD + c] : 0.0f;
      f.ea[c] = f.es[c] = 0.0f;
    }
    for (int c = threadIdx.x; c < kHistory; c += blockDim.x) f.hist[c] = 0.0f;
    if (threadIdx.x == 0) {
      f.phase = mask[a] ? kLrTrain : kLrDone;
      f.epoch = f.have_tot = f.bad = 0;
      f.lr = 2e-3;
      f.best = INFINITY;
    }
  }
}

template <int DO>
__global__ __launch_bounds__(kLrThreads) void k_lrts_epoch(
    int K, const int32_t *__restrict__ blk_agent, const int32_t *__restrict__ blk_rank,
    const int32_t *__restrict__ agent_nblk, const int64_t *__restrict__ offsets, const uint32_t *__restrict__ key,
    const float *__restrict__ xs, int64_t cap, float *__restrict__ gm, float *__restrict__ gq,
    float *__restrict__ gpm, const double *__restrict__ adam_tab, int32_t *__restrict__ epochs_out,
    const LrSt *__restrict__ st_in, LrSt *__restrict__ st_out, const int64_t *__restrict__ tot_in,
    int64_t *__restrict__ tot_out, int64_t *__restrict__ acc_rows, unsigned *__restrict__ bars,
    const int32_t *__restrict__ bar_off) {
  const int a = blk_agent[blockIdx.x], rank = blk_rank[blockIdx.x], nblk = agent_nblk[a];
  const int tid = threadIdx.x;
  const int KD = K * DO;
  const int PW = 2 * (KD + 1);
  extern __shared__ int64_t s_acc[];  // [KD][kAccStride]
  __shared__ uint64_t s_tab[256];
  __shared__ LrSt st;
  __shared__ float s_q[kLrMaxKD], s_pm[kLrMaxKD];
  __shared__ int64_t s_hi[4][kLrMaxKD + 1], s_lo[4][kLrMaxKD + 1];
  __shared__ float s_loss, s_negstep, s_bc2;
  __shared__ int s_flag;
  __shared__ int64_t s_part[2 * (kLrMaxKD + 1)];
  for (int i = tid; i < 256; i += kLrThreads) s_tab[i] = ag_exp_tab[i];
  for (int i = tid; i < (int)(sizeof(LrSt) / 4); i += kLrThreads)
    reinterpret_cast<uint32_t *>(&st)[i] = reinterpret_cast<const uint32_t *>(st_in + a)[i];
  float *q_g = gq + (size_t)a * KD, *pm_g = gpm + (size_t)a * KD, *m_g = gm + (size_t)a * KD;
  for (int c = tid; c < KD; c += kLrThreads) {
    s_q[c] = q_g[c];
    s_pm[c] = pm_g[c];
  }
  for (int i = tid; i < KD * kAccStride; i += kLrThreads) s_acc[i] = 0;
  __syncthreads();
  const int64_t *T = tot_in + (size_t)a * kLrAccStride;
  if (st.phase == kLrTrain && st.have_tot) {
    // k_lrts_train's step C from the summed partials of epoch st.epoch
    const int epoch = st.epoch;
    if (tid == 0) {
      double prior = 0.0;
      for (int k = 0; k < K; ++k)
        for (int d = 0; d < DO - 1; ++d) {
          const double df = (double)s_pm[k * DO + d] - (double)st.m[k * DO + d];
          prior += (double)s_q[k * DO + d] * (df * df);
        }
      s_loss = (float)(0.5 * prior + fx_read(T[2 * KD], T[2 * KD + 1], 1.0 / kLossScale));
      s_negstep = (float)(-(st.lr / adam_tab[epoch]));
      s_bc2 = (float)adam_tab[kLrEpochs + epoch];
    }
    __syncthreads();
    if (tid < KD) {
      const int c = tid;
      const double gp = (c % DO) < DO - 1 ? -(double)s_q[c] * ((double)s_pm[c] - (double)st.m[c]) : 0.0;
      const float g = (float)(fx_read(T[2 * c], T[2 * c + 1], 1.0 / kGradScale) + gp);
      const float ea = st.ea[c] + 0.1f * (g - st.ea[c]);
      const float es = st.es[c] * 0.999f + (0.001f * g) * g;
      const float den = (float)__builtin_sqrt((double)es) / s_bc2 + 1e-8f;
      st.ea[c] = ea;
      st.es[c] = es;
      st.m[c] = st.m[c] + s_negstep * (ea / den);
    }
    __syncthreads();
    if (tid == 0) {
      const float loss = s_loss;
      st.hist[epoch % kHistory] = loss;
      if ((double)loss < st.best * (1.0 - 1e-4)) {
        st.best = (double)loss;
        st.bad = 0;
      } else {
        st.bad += 1;
      }
      if (st.bad > 10) {
        const double nl = st.lr * 0.5;
        if (st.lr - nl > 1e-8) st.lr = nl;
        st.bad = 0;
      }
      const bool stop = epoch > 1024 && fabs((double)st.hist[(epoch - 99) % kHistory] - (double)loss) < 1e-6;
      st.epoch = epoch + 1;
      if (stop || st.epoch >= kLrEpochs) st.phase = kLrLaplace;
      st.have_tot = 0;
    }
    __syncthreads();
  } else if (st.phase == kLrLaplace && st.have_tot) {
    // the Laplace q from the summed terms, then prev_m = m (src/Models.py:43-48)
    if (rank == 0) {
      for (int c = tid; c < KD; c += kLrThreads) {
        q_g[c] = s_q[c] + (float)fx_read(T[2 * c], T[2 * c + 1], 1.0 / kGradScale);
        m_g[c] = st.m[c];
        pm_g[c] = st.m[c];
      }
      if (tid == 0) epochs_out[a] = st.epoch;
    }
    __syncthreads();
    if (tid == 0) {
      st.phase = kLrDone;
      st.have_tot = 0;
    }
    __syncthreads();
  }
  const bool active = st.phase != kLrDone;
  if (active) {
    const int64_t s0 = offsets[a], n = offsets[a + 1] - s0;
    const int64_t per = (n + nblk - 1) / nblk;
    const int64_t c0 = (int64_t)rank * per < n ? (int64_t)rank * per : n;
    const int64_t c1 = c0 + per < n ? c0 + per : n;
    int64_t *acc = s_acc + tid;
    int64_t lsum = 0;
    const bool train = st.phase == kLrTrain;
    for (int64_t i = c0 + tid; i < c1; i += kLrThreads) {
      LrSample sm;
      lr_load<DO>(key, xs, cap, s0 + i, sm);
      if (train)
        lsum += lr_epoch_sample<DO>(sm, st.m, acc, s_tab);
      else
        lr_laplace_sample<DO>(sm, st.m, acc, s_tab);
    }
    __syncthreads();
    lr_block_partials(s_acc, KD, lsum >> 24, lsum & kLo24, s_hi, s_lo, s_part);
    agcoop::agent_reduce_nowait(bars + (size_t)bar_off[a] * agcoop::kBarLineWords,
                                acc_rows + (size_t)bar_off[a] * kLrAccStride, kLrAccStride, rank, nblk, s_part, PW,
                                tot_out + (size_t)a * kLrAccStride, &s_flag);
  }
  if (rank == 0 && tid == 0) {
    st.have_tot = active ? 1 : 0;
    st_out[a] = st;
  }
}

using EpochKernel = void (*)(int, const int32_t *, const int32_t *, const int32_t *, const int64_t *,
                             const uint32_t *, const float *, int64_t, float *, float *, float *, const double *,
                             int32_t *, const LrSt *, LrSt *, const int64_t *, int64_t *, int64_t *, unsigned *,
                             const int32_t *);
EpochKernel pick_epoch(int Do) {
  switch (Do) {
    case 1: return k_lrts_epoch<1>;
    case 2: return k_lrts_epoch<2>;
    case 3: return k_lrts_epoch<3>;
    case 4: return k_lrts_epoch<4>;
    case 5: return k_lrts_epoch<5>;
    case 6: return k_lrts_epoch<6>;
    case 7: return k_lrts_epoch<7>;
    case 8: return k_lrts_epoch<8>;
    default: return nullptr;
  }
}

using TrainKernel = void (*)(int, const int32_t *, const int32_t *, const int32_t *, const int64_t *,
                             const int64_t *, const uint32_t *, const float *, int64_t, float *, float *,
                             float *, const double *, int32_t *, float *, int64_t *, unsigned *, const int32_t *);

TrainKernel pick_train(int Do) {
  switch (Do) {
    case 1: return k_lrts_train<1>;
    case 2: return k_lrts_train<2>;
    case 3: return k_lrts_train<3>;
    case 4: return k_lrts_train<4>;
    case 5: return k_lrts_train<5>;
    case 6: return k_lrts_train<6>;
    case 7: return k_lrts_train<7>;
    case 8: return k_lrts_train<8>;
    default: return nullptr;
  }
}

int grid_over(int64_t n) { return agtrain::grid_over(n, kLrThreads); }

}  // namespace

void ag_lrts_release(ag_ctx *c) {
  ag_lrts_ws &w = c->lrts;
  (void)hipFree(w.key);
  (void)hipFree(w.x);
  (void)hipFree(w.offsets);
  (void)hipFree(w.adam_tab);
  (void)hipFree(w.epochs);
  (void)hipFree(w.tables);
  (void)hipFree(w.partials);
  (void)hipFree(w.rp.st);
  (void)hipFree(w.rp.acc);
  (void)hipFree(w.rp.tables);
  w = ag_lrts_ws();
}

extern "C" {

// The won samples of a store bucketed by agent into the workspace (w.key, w.x with stride
// w.cap; w.offsets [N + 1]): histogram -> exclusive scan -> scatter. Shared by ag_lrts_update
// and ag_lrts_rp_begin. Synchronises for the count.
static int bucket_samples(ag_ctx *c, const ag_lrts_samples *s, hipStream_t st, const char *who) {
  const int N = c->shape.num_agents, Do = c->shape.obs_embedding_size + 1;
  uint64_t n = 0;
  if (int rc = agtrain::read_store_count(s->count, s->capacity, who, "won samples", st, &n)) return rc;
  ag_lrts_ws &w = c->lrts;
  if (!w.adam_tab) {
    const std::vector<double> tab = agtrain::adam_bias_table(kLrEpochs);
    hipError_t e = hipMalloc(&w.adam_tab, sizeof(double) * tab.size());
    if (e == hipSuccess) e = hipMemcpy(w.adam_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&w.offsets, sizeof(int64_t) * (3 * (size_t)N + 1));
    if (e == hipSuccess) e = hipMalloc(&w.epochs, sizeof(int32_t) * N);
    if (e != hipSuccess) {
      ag_lrts_release(c);
      return ag_set_error(AG_ERR_HIP, "%s: workspace: %s", who, hipGetErrorString(e));
    }
  }
  if ((int64_t)n > w.cap) {  // key and x share the capacity (x's row stride): both again
    const int64_t cap = (int64_t)n + ((int64_t)n >> 2) + 1024;
    size_t none = 0;
    w.cap = 0;
    hipError_t e = agtrain::dev_reserve(&w.key, &none, sizeof(uint32_t) * cap);
    none = 0;
    if (e == hipSuccess) e = agtrain::dev_reserve(&w.x, &none, sizeof(float) * (size_t)Do * cap);
    if (e != hipSuccess) return ag_set_error(AG_ERR_HIP, "%s: sample workspace: %s", who, hipGetErrorString(e));
    w.cap = cap;
  }
  int64_t *counts = w.offsets + N + 1, *cursors = counts + N;
  AG_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * N, st));
  if (n > 0) {
    if ((size_t)N * 4 > 64 * 1024)
      return ag_set_error(AG_ERR_UNSUPPORTED, "%s: N=%d agents > 16384", who, N);
    hipLaunchKernelGGL(k_lrts_hist, dim3(grid_over((int64_t)n)), dim3(kLrThreads), (size_t)N * 4, st, s->key,
                       (int64_t)n, N, counts);
    AG_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_lrts_scan, dim3(1), dim3(kLrThreads), 0, st, counts, N, w.offsets, cursors);
  AG_HIP(hipGetLastError());
  if (n > 0) {
    hipLaunchKernelGGL(k_lrts_scatter, dim3(grid_over((int64_t)n)), dim3(kLrThreads), 0, st, s->key, s->x,
                       (int64_t)n, s->capacity, Do, cursors, w.key, w.x, w.cap);
    AG_HIP(hipGetLastError());
  }
  return AG_OK;
}

int ag_lrts_update(ag_ctx *c, const ag_lrts_samples *s, int32_t *epochs, float *loss_trace, void *stream) {
  if (int rc = ag_check_store(c, s, "ag_lrts_update")) return rc;
  if (!c->has_lrts) return AG_OK;
  if (!c->lrts_loaded) return ag_set_error(AG_ERR_STATE, "ag_lrts_update: ag_load_lrts not called");
  const int N = c->shape.num_agents, K = c->shape.num_items, Do = c->shape.obs_embedding_size + 1;
  TrainKernel train = pick_train(Do);
  if (!train || K * Do > kLrMaxKD)
    return ag_set_error(AG_ERR_UNSUPPORTED, "ag_lrts_update: needs OE+1 <= %d and K*(OE+1) <= %d (K=%d, OE+1=%d)",
                        AG_LRTS_MAX_DO, kLrMaxKD, K, Do);
  AgDeviceGuard g(c->device);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = bucket_samples(c, s, st, "ag_lrts_update")) return rc;
  ag_lrts_ws &w = c->lrts;
  // agents' sample counts -> workgroups per agent (kLrCache samples per lane each)
  std::vector<int64_t> h_off((size_t)N + 1);
  AG_HIP(hipMemcpyAsync(h_off.data(), w.offsets, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  const size_t lds = sizeof(int64_t) * (size_t)K * Do * kAccStride;
  AG_HIP(hipFuncSetAttribute((const void *)train, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  AG_HIP(agtrain::resident_blocks((const void *)train, kLrThreads, lds, c->device, &w.coop_blocks));
  agtrain::BlockTables T;
  T.nblk.assign(N, 0);
  const int64_t chunk = c->lrts_chunk > 0 ? c->lrts_chunk : (int64_t)kLrCache * kLrThreads;
  for (int a = 0; a < N; ++a) {
    const int64_t na = h_off[a + 1] - h_off[a];
    if (c->h_akind[a] != AG_ALLOCATOR_LRTS || na < 2) continue;
    T.nblk[a] = (int32_t)((na + chunk - 1) / chunk);
  }
  agtrain::share_out(T.nblk, w.coop_blocks);  // more samples than the resident grid caches
  agtrain::block_tables(T, [](int nb) { return agcoop::bar_lines(nb); });
  const int G = T.G(), lines = T.lines;
  const int64_t pwords = (int64_t)lines * kLrAccStride;  // accumulator rows, one per barrier line
  std::vector<int64_t> pbase(N);
  for (int a = 0; a < N; ++a) pbase[a] = (int64_t)T.bar_off[a] * kLrAccStride;
  AG_HIP(hipMemsetAsync(w.epochs, 0, sizeof(int32_t) * N, st));
  if (G > 0) {
    // (room for 256 more workgroups, 64 more lines and 4096 more words before the buffers grow again)
    hipError_t e = agtrain::dev_reserve(&w.tables, &w.tables_bytes, agtrain::layout_bytes(agtrain::lrts_layout, N, G, lines),
                                        agtrain::layout_bytes(agtrain::lrts_layout, N, G + 256, lines + 64));
    if (e == hipSuccess)
      e = agtrain::dev_reserve(&w.partials, &w.partials_bytes, sizeof(int64_t) * pwords, sizeof(int64_t) * (pwords + 4096));
    if (e != hipSuccess) return ag_set_error(AG_ERR_HIP, "ag_lrts_update: tables: %s", hipGetErrorString(e));
    agtrain::Carve carve(w.tables);
    const agtrain::LrtsTables D = agtrain::lrts_layout(carve, N, G, lines);
    AG_HIP(hipMemcpyAsync(D.bagent, T.blk_agent.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
    AG_HIP(hipMemcpyAsync(D.brank, T.blk_rank.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
    AG_HIP(hipMemcpyAsync(D.nblk, T.nblk.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
    AG_HIP(hipMemcpyAsync(D.pbase, pbase.data(), sizeof(int64_t) * N, hipMemcpyHostToDevice, st));
    AG_HIP(hipMemcpyAsync(D.baroff, T.bar_off.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
    if (lines) AG_HIP(hipMemsetAsync(D.bar, 0, sizeof(unsigned) * agcoop::kBarLineWords * lines, st));
    if (pwords) AG_HIP(hipMemsetAsync(w.partials, 0, sizeof(int64_t) * pwords, st));  // accumulator rows
    AG_HIP(agtrain::launch_group(train, T.multi(), G, kLrThreads, lds, st, K, D.bagent, D.brank, D.nblk, D.pbase,
                                 w.offsets, w.key, w.x, w.cap, c->d_tsm, c->d_tsq, c->d_tsprev, w.adam_tab, w.epochs,
                                 loss_trace, w.partials, D.bar, D.baroff));
  }
  if (epochs) {
    AG_HIP(hipMemcpyAsync(epochs, w.epochs, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    AG_HIP(hipStreamSynchronize(st));
  }
  return AG_OK;
}

// ---- resumable / record-parallel LR-TS training (k_lrts_epoch) ----
int ag_lrts_rp_begin(ag_ctx *c, const ag_lrts_samples *s, const int32_t *agents, const int64_t *samples_total,
                     int64_t *totals, void *stream) {
  if (int rc = ag_check_store(c, s, "ag_lrts_rp_begin")) return rc;
  if (!totals) return ag_set_error(AG_ERR_INVALID, "ag_lrts_rp_begin: null totals");
  if (!c->lrts_loaded) return ag_set_error(AG_ERR_STATE, "ag_lrts_rp_begin: ag_load_lrts not called");
  const int N = c->shape.num_agents, K = c->shape.num_items, Do = c->shape.obs_embedding_size + 1;
  EpochKernel kern = pick_epoch(Do);
  if (!kern || K * Do > kLrMaxKD)
    return ag_set_error(AG_ERR_UNSUPPORTED, "ag_lrts_rp_begin: needs OE+1 <= %d and K*(OE+1) <= %d", AG_LRTS_MAX_DO,
                        kLrMaxKD);
  AgDeviceGuard g(c->device);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = bucket_samples(c, s, st, "ag_lrts_rp_begin")) return rc;
  ag_lrts_ws &w = c->lrts;
  auto &rp = w.rp;
  std::vector<int64_t> off((size_t)N + 1);
  AG_HIP(hipMemcpyAsync(off.data(), w.offsets, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  // agents trained: LR-TS allocators in the mask with >= 2 won samples over all ranks (the
  // reference skips the update below that, src/BidderAllocation.py:33-34)
  constexpr int64_t kRpChunk = 2048;
  std::vector<int32_t> mask(N, 0);
  agtrain::BlockTables T;
  T.nblk.assign(N, 0);
  for (int a = 0; a < N; ++a) {
    const int64_t na = off[a + 1] - off[a], nt = samples_total ? samples_total[a] : na;
    if (c->h_akind[a] != AG_ALLOCATOR_LRTS || (agents && !agents[a]) || nt < 2) continue;
    mask[a] = 1;
    T.nblk[a] = (int32_t)std::max<int64_t>(1, (na + kRpChunk - 1) / kRpChunk);
  }
  agtrain::block_tables(T, [](int nb) { return std::max(1, agcoop::bar_lines(nb)); });
  const int G = T.G(), lines = T.lines;
  // (room for 64 more workgroups and 16 more lines before the buffers grow again)
  AG_HIP(agtrain::dev_reserve(&rp.st, &rp.st_bytes, sizeof(LrSt) * 2 * (size_t)N));
  AG_HIP(agtrain::dev_reserve(&rp.acc, &rp.acc_bytes, agtrain::layout_bytes(agtrain::rp_acc_layout, lines, kLrAccStride),
                              agtrain::layout_bytes(agtrain::rp_acc_layout, lines + 16, kLrAccStride)));
  AG_HIP(agtrain::dev_reserve(&rp.tables, &rp.tables_bytes, agtrain::layout_bytes(agtrain::rp_tables_layout, N, G, 0),
                              agtrain::layout_bytes(agtrain::rp_tables_layout, N, G + 64, 0)));
  agtrain::Carve carve_acc(rp.acc), carve_tables(rp.tables);
  rp.A = agtrain::rp_acc_layout(carve_acc, lines, kLrAccStride);
  rp.T = agtrain::rp_tables_layout(carve_tables, N, G, 0);
  if (G) {
    AG_HIP(hipMemcpyAsync(rp.T.bagent, T.blk_agent.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
    AG_HIP(hipMemcpyAsync(rp.T.brank, T.blk_rank.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
  }
  AG_HIP(hipMemcpyAsync(rp.T.nblk, T.nblk.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(rp.T.baroff, T.bar_off.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(rp.T.mask, mask.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  if (lines) AG_HIP(hipMemsetAsync(rp.acc, 0, carve_acc.bytes(), st));
  AG_HIP(hipMemsetAsync(totals, 0, sizeof(int64_t) * 2 * kLrAccStride * (size_t)N, st));
  AG_HIP(hipMemsetAsync(w.epochs, 0, sizeof(int32_t) * N, st));
  hipLaunchKernelGGL(k_lrts_rp_init, dim3(N), dim3(64), 0, st, N, K * Do, rp.T.mask, c->d_tsm, (LrSt *)rp.st);
  AG_HIP(hipGetLastError());
  const size_t lds = sizeof(int64_t) * (size_t)K * Do * kAccStride;
  AG_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  rp.G = G;
  rp.k = 0;
  rp.totals = totals;
  rp.active = true;
  return AG_OK;
}

int ag_lrts_rp_epoch(ag_ctx *c, int32_t launches, int64_t *launch_index, void *stream) {
  if (!c || !c->lrts.rp.active) return ag_set_error(AG_ERR_STATE, "ag_lrts_rp_epoch: no ag_lrts_rp_begin");
  if (launches < 0) return ag_set_error(AG_ERR_INVALID, "ag_lrts_rp_epoch: launches < 0");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents, K = c->shape.num_items, Do = c->shape.obs_embedding_size + 1;
  ag_lrts_ws &w = c->lrts;
  auto &rp = w.rp;
  EpochKernel kern = pick_epoch(Do);
  const size_t lds = sizeof(int64_t) * (size_t)K * Do * kAccStride;
  LrSt *S = (LrSt *)rp.st;
  hipStream_t st = (hipStream_t)stream;
  for (int32_t l = 0; l < launches; ++l) {
    const int64_t k = rp.k;
    if (rp.G > 0)
      hipLaunchKernelGGL(kern, dim3(rp.G), dim3(kLrThreads), lds, st, K, rp.T.bagent, rp.T.brank, rp.T.nblk, w.offsets, w.key,
                         w.x, w.cap, c->d_tsm, c->d_tsq, c->d_tsprev, w.adam_tab, w.epochs, S + (size_t)(k & 1) * N,
                         S + (size_t)((k + 1) & 1) * N, rp.totals + (size_t)((k + 1) & 1) * kLrAccStride * N,
                         rp.totals + (size_t)(k & 1) * kLrAccStride * N, rp.A.acc, rp.A.bar, rp.T.baroff);
    AG_HIP(hipGetLastError());
    rp.k = k + 1;
  }
  if (launch_index) *launch_index = rp.k - 1;
  return AG_OK;
}

int ag_lrts_rp_poll(ag_ctx *c, int32_t *training, void *stream) {
  if (!c || !c->lrts.rp.active) return ag_set_error(AG_ERR_STATE, "ag_lrts_rp_poll: no ag_lrts_rp_begin");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents;
  auto &rp = c->lrts.rp;
  hipStream_t st = (hipStream_t)stream;
  std::vector<int32_t> ph(N);
  // the phase word of every agent's latest state (LrSt starts with it)
  AG_HIP(hipMemcpy2DAsync(ph.data(), sizeof(int32_t), (LrSt *)rp.st + (size_t)(rp.k & 1) * N, sizeof(LrSt),
                          sizeof(int32_t), N, hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  int32_t n = 0;
  for (int a = 0; a < N; ++a) n += ph[a] != kLrDone;
  if (training) *training = n;
  return AG_OK;
}

int ag_lrts_rp_end(ag_ctx *c, int32_t *epochs, void *stream) {
  if (!c || !c->lrts.rp.active) return ag_set_error(AG_ERR_STATE, "ag_lrts_rp_end: no ag_lrts_rp_begin");
  int32_t training = 0;
  if (int rc = ag_lrts_rp_poll(c, &training, stream)) return rc;
  c->lrts.rp.active = false;
  if (training) return ag_set_error(AG_ERR_STATE, "ag_lrts_rp_end: %d agents still training", training);
  if (epochs) {
    AG_HIP(hipMemcpyAsync(epochs, c->lrts.epochs, sizeof(int32_t) * c->shape.num_agents, hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
    AG_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  return AG_OK;
}

int ag_lrts_read(ag_ctx *c, float *m, float *q, float *prev_m) {
  if (!c) return ag_set_error(AG_ERR_INVALID, "ag_lrts_read: null ctx");
  AgDeviceGuard g(c->device);
  const size_t n = (size_t)c->shape.num_agents * c->shape.num_items * (c->shape.obs_embedding_size + 1);
  AG_HIP(hipDeviceSynchronize());
  if (m) AG_HIP(hipMemcpy(m, c->d_tsm, n * sizeof(float), hipMemcpyDeviceToHost));
  if (q) AG_HIP(hipMemcpy(q, c->d_tsq, n * sizeof(float), hipMemcpyDeviceToHost));
  if (prev_m) AG_HIP(hipMemcpy(prev_m, c->d_tsprev, n * sizeof(float), hipMemcpyDeviceToHost));
  return AG_OK;
}

}  // extern "C"
