// ag_dr.hip -- DoublyRobustBidder.update on the GPU (Agent.update -> src/Bidder.py:473-615,
// models src/Models.py:51-62, :92-218).
//
// One workgroup per DR agent, persistent over the three fits the reference runs one after
// the other: the win-rate model (BCE on the logs + the gamma = 0 augmentation, <= 32768
// epochs), the policy's imitation of the logging policy (first update only, <= 16384) and
// the doubly robust policy fit (<= 32768, rsample noise per epoch supplied by the caller).
// Everything a fit needs per epoch (Adam with weight decay + AMSGrad, ReduceLROnPlateau,
// the reference's early stop) runs on the device. Sums over the agent's records are exact
// (fixed-point terms added as integers), so the result is independent of record order and
// lane assignment; the arithmetic is oracle/ag_oracle_dr.c ora_dr_update, bit for bit.
//
// Three kernels drive the same fits and give the same models bit for bit (tests/test_gpu_rp.py):
//   k_bidder_train<PH>  persistent, a group of workgroups per learner, the fits as loops
//                       (fit_winrate, fit_imitation, fit_dr, fit_dm, fit_pl): ag_bidder_update;
//   k_bidder_epoch      one launch per epoch, the learner's state (FitSt) in HBM: the record-
//                       parallel multi-GPU update, the drop-in update's noise windows;
//   k_bidder_pipe<PH>   persistent, every learner in every workgroup, FitSt in LDS:
//                       ag_bidder_rp_run, AG_BIDDER_PIPE=1.
// What they share stands once: the per-record terms (wr_pair, imit_rec, dr_rec, dm_rec), the
// hyper-parameters (fit_hyper), a workgroup's slice of the records (wg_slice), the estimated
// utilities (estimated_utilities), the words per fit and the trace rows (fit_words, trace_row);
// the last two kernels also the FitSt machine (fit_enter, fit_after, fit_step) and a
// workgroup's sums of an epoch (epoch_partial). On the host, block_tables lays out the
// workgroups and barrier lines of ag_bidder_update's and ag_bidder_rp_begin's launches.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "ag_exp.h"
#include "ag_exp_table.h"
#include "ag_host.h"
#include "ag_log1p.h"
#include "ag_philox.h"
#include "ag_coop.h"
#include "ag_div.h"
#include "ag_train_math.h"

namespace {

using namespace agtm;

using agcoop::agent_barrier;
using agcoop::bar_lines;
using agcoop::kBarLineWords;
constexpr int kDrThreads = 256;
constexpr int kWrEpochs = 32768, kInitEpochs = 16384, kDrEpochs = 32768;
constexpr int64_t kBidderChunk = 8192;  // records per workgroup of a PolicyLearningBidder (default)
constexpr int64_t kMinChunk = 1024;     // fewest records per workgroup of an exact-sum learner's split
#ifndef AG_DR_REC_LDS0
#define AG_DR_REC_LDS0 (32 * 1024)
#endif
constexpr size_t kRecLdsBytes0 = AG_DR_REC_LDS0;  // record cache per workgroup, win-rate phase (4 per CU)
#ifndef AG_DR_REC_LDS
#define AG_DR_REC_LDS (48 * 1024)  // (3 workgroups per CU: profiles/r04r_ab_trainer_*.log)
#endif
#ifndef AG_DR_PH0_MIN_WAVES
#define AG_DR_PH0_MIN_WAVES 4  // the win-rate fits: <= 128 VGPRs
#endif
#ifndef AG_DR_PH1_MIN_WAVES
#define AG_DR_PH1_MIN_WAVES 3  // the later fits: <= 168 VGPRs, 3 waves per SIMD (FP_DR_TS update 1.96 -> 1.69 s)
#endif
constexpr size_t kRecLdsBytes = AG_DR_REC_LDS;  // record cache per workgroup, later fits
constexpr int64_t kLo24 = (int64_t(1) << 24) - 1;

// the fixed-point terms and their biased forms (fxb, fxb_fast, fxb_x, fx_in): ag_train_math.h
__device__ __forceinline__ void addw(int64_t &a, int64_t t) { a = (int64_t)((uint64_t)a + (uint64_t)t); }
__device__ __forceinline__ void fx_unbias(int64_t &a, int64_t n) {
  a = (int64_t)((uint64_t)a - (uint64_t)n * kFxMagic);
}

__device__ __forceinline__ double fxv(int64_t hi, int64_t lo) {
  hi += lo >> 24;
  lo &= kLo24;
  return ((double)hi * 0x1p24 + (double)lo) * kInv;
}

// softplus(u) = u > 20 ? u : log1p(exp(u)) and its derivative exp(u) / (exp(u) + 1), from
// e = exp(u) (the forward pass keeps it for the backward pass)
__device__ __forceinline__ double dsoftplus_e(double u, double e) { return u > 20.0 ? 1.0 : e / (e + 1.0); }
// SharedDiv (log1p_main's divisions from a shared reciprocal) and softplus_fast: ag_train_math.h
using agexp::exp_fast;

// Exact block sum of NV per-lane int64 accumulators (each split at bit 24 so nothing can
// overflow): every thread gets the totals as (hi, lo) pairs in s_out.
template <int NV>
__device__ __forceinline__ void block_sums(const int64_t (&v)[NV], int64_t (*s_w)[32], int64_t *s_out) {
  static_assert(2 * NV <= 32, "block_sums: at most 16 sums");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    int64_t h = v[j] >> 24, l = v[j] & kLo24;
    for (int o = 32; o > 0; o >>= 1) {
      h += __shfl_xor(h, o, 64);
      l += __shfl_xor(l, o, 64);
    }
    if (lane == 0) {
      s_w[wv][2 * j] = h;
      s_w[wv][2 * j + 1] = l;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * NV) {
    int64_t t = 0;
    for (int w = 0; w < kDrThreads / 64; ++w) t += s_w[w][threadIdx.x];
    s_out[threadIdx.x] = t;
  }
  __syncthreads();
}

// torch.optim.Adam single-tensor step with weight decay and AMSGrad (thread j: param j)
struct AdamState {
  float ea[16], es[16], mx[16];
};

__device__ __forceinline__ void adam_param(float &p, float grad, int j, AdamState &a, float neg_step, float bc2f,
                                           float wdf) {
  const float g = grad + wdf * p;
  a.ea[j] = a.ea[j] + 0.1f * (g - a.ea[j]);
  a.es[j] = a.es[j] * 0.999f + (0.001f * g) * g;
  a.mx[j] = a.mx[j] > a.es[j] ? a.mx[j] : a.es[j];
  // float32 sqrt correctly rounded (as the CPU's sqrtss): via the refined FP64 sqrt
  const float den = (float)__builtin_sqrt((double)a.mx[j]) / bc2f + 1e-8f;
  p = p + neg_step * (a.ea[j] / den);
}

struct Plateau {
  double best, threshold, factor, min_lr;
  int bad, patience;
};
__device__ __forceinline__ void plateau_step(Plateau &s, float loss, double &lr) {
  if ((double)loss < s.best * (1.0 - s.threshold)) {
    s.best = (double)loss;
    s.bad = 0;
  } else {
    s.bad += 1;
  }
  if (s.bad > s.patience) {
    double nl = lr * s.factor;
    if (nl < s.min_lr) nl = s.min_lr;
    if (lr - nl > 1e-8) lr = nl;
    s.bad = 0;
  }
}
struct Stopper {
  double best;
  int best_epoch, wait;
};
__device__ __forceinline__ bool stop_step(Stopper &s, int epoch, float loss) {
  if (s.best - (double)loss > 1e-6) {
    s.best_epoch = epoch;
    s.best = (double)loss;
    return false;
  }
  return epoch - s.best_epoch > s.wait;
}

// The exact-sum learners' fits in the reference's order (src/Bidder.py:229-325, :500-615): the
// ValueLearningBidder's win count, the win-rate fit, DoublyRobustBidder's estimated utilities
// (no fit: one pass), the imitation of the logging policy, the policy fit (DR or DM).
enum { kFitWins = 0, kFitWr, kFitEu, kFitInit, kFitPol, kFitDone };
// the row of a fit in epochs [3] and traces [3][kDrEpochs]: win-rate, imitation, policy fit
__device__ __forceinline__ int fit_slot(int fit) { return fit == kFitWr ? 0 : (fit == kFitInit ? 1 : 2); }
__device__ __forceinline__ float *trace_row(float *traces, int a, int fit) {
  return traces + ((size_t)a * 3 + fit_slot(fit)) * kDrEpochs;
}
// words (hi, lo pairs) of a fit's per-epoch sums: the win count, the win-rate fit's loss and 4
// gradient terms, the 12-parameter fits' 16 sums
__device__ __forceinline__ constexpr int fit_words(int fit) {
  return fit == kFitWins ? 2 : (fit == kFitWr ? 10 : 32);
}

// A fit's hyper-parameters, by fit and bidder kind -- the one statement of them, read by the
// persistent fits (fit_winrate, fit_imitation, fit_dr, fit_dm) and by the FitSt machine:
// Adam(lr, weight decay, AMSGrad), ReduceLROnPlateau(threshold, factor, min_lr, patience; none
// for the imitation), early stop after `wait` epochs without a 1e-6 improvement, <= max_epochs.
//   win-rate (src/Bidder.py:229-252 ValueLearningBidder, :500-530 DoublyRobustBidder)
//   imitation (src/Models.py:106-137), any bidder kind
//   policy fit: DR (src/Bidder.py:562-590), DM (ValueLearningBidder 'policy', :258-303)
struct FitHyper {
  double lr;
  float wd;
  double threshold, factor, min_lr;
  int patience, wait, max_epochs;
};
__device__ __forceinline__ constexpr FitHyper fit_hyper(int fit, int bk) {
  const bool dr = bk == AG_BIDDER_DOUBLY_ROBUST;
  if (fit == kFitWr)
    return dr ? FitHyper{3e-3, (float)1e-6, 1e-4, 0.2, 1e-7, 256, 1024, kWrEpochs}
              : FitHyper{3e-3, (float)1e-6, 1e-4, 0.1, 1e-7, 100, 512, kWrEpochs};
  if (fit == kFitInit) return FitHyper{1e-3, (float)1e-4, 0.0, 0.0, 0.0, 0, 512, kInitEpochs};
  return dr ? FitHyper{7e-3, (float)1e-4, 5e-3, 0.2, 1e-8, 100, 512, kDrEpochs}
            : FitHyper{2e-3, (float)1e-6, 1e-4, 0.1, 1e-7, 100, 256, kInitEpochs};
}
__device__ __forceinline__ Plateau plateau_of(const FitHyper &H) {
  return Plateau{INFINITY, H.threshold, H.factor, H.min_lr, 0, H.patience};
}
__device__ __forceinline__ Stopper stopper_of(const FitHyper &H) { return Stopper{INFINITY, -1, H.wait}; }

// forward values of the policy; eh / eam / eas = exp of h / am / as, kept for the backward
// pass's softplus derivatives
struct PolF {
  double h[2], s[2], am, as, mu, sp_sigma, sigma, eh[2], eam, eas;
  double rh[2], ram, ras;  // policy_fwd_main only: the reciprocals of 1 + eh / eam / eas (ag_div.h)
};
__device__ __forceinline__ void policy_fwd(const float *p, double c, double v, PolF &f, const uint64_t *tab) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    f.h[j] = c * (double)p[2 * j] + v * (double)p[2 * j + 1] + (double)p[4 + j];
    f.s[j] = softplus_fast(f.h[j], f.eh[j], tab);
  }
  f.am = f.s[0] * (double)p[6] + f.s[1] * (double)p[7] + (double)p[8];
  f.as = f.s[0] * (double)p[9] + f.s[1] * (double)p[10] + (double)p[11];
  f.mu = softplus_fast(f.am, f.eam, tab);
  f.sp_sigma = softplus_fast(f.as, f.eas, tab);
  f.sigma = f.sp_sigma + 0.01;  // min_sigma (src/Models.py:104)
}
// softplus through the main paths alone (ok cleared when an input leaves them); r = the
// reciprocal of 1 + e, shared by log1p's c / (1 + e) and the backward pass's e / (e + 1)
// (ag_div.h; where ok holds and u <= 20, e is in [2^-29, 2^29]: div_safe's range)
__device__ __forceinline__ double softplus_main(double u, double &e, double &r, const uint64_t *tab, bool &ok) {
  e = agexp::exp_main(u, tab);
  bool lok;
  r = agdiv::recip(1.0 + e);
  const double l = aglog1p::log1p_main_t(e, lok, SharedDiv{r});
  ok = (int)ok & (int)agexp::exp_in_main(u) & ((int)lok | (int)(u > 20.0));
  return u > 20.0 ? u : l;
}
// dsoftplus_e from softplus_main's reciprocal (the same bits where its ok holds)
__device__ __forceinline__ double dsoftplus_r(double u, double e, double r) {
  return u > 20.0 ? 1.0 : agdiv::div_core(e, e + 1.0, r);
}
// policy_fwd through the main paths alone: true when they gave policy_fwd's values (every
// softplus input inside them), else the caller runs policy_fwd -- one rare branch per record
// instead of one per softplus
__device__ __forceinline__ bool policy_fwd_main(const float *p, double c, double v, PolF &f, const uint64_t *tab) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    f.h[j] = c * (double)p[2 * j] + v * (double)p[2 * j + 1] + (double)p[4 + j];
    f.s[j] = softplus_main(f.h[j], f.eh[j], f.rh[j], tab, ok);
  }
  f.am = f.s[0] * (double)p[6] + f.s[1] * (double)p[7] + (double)p[8];
  f.as = f.s[0] * (double)p[9] + f.s[1] * (double)p[10] + (double)p[11];
  f.mu = softplus_main(f.am, f.eam, f.ram, tab, ok);
  f.sp_sigma = softplus_main(f.as, f.eas, f.ras, tab, ok);
  f.sigma = f.sp_sigma + 0.01;
  return ok;
}
__device__ __forceinline__ void policy_fwd_fast(const float *p, double c, double v, PolF &f, const uint64_t *tab) {
  if (__builtin_expect(!policy_fwd_main(p, c, v, f, tab), 0)) policy_fwd(p, c, v, f, tab);
}
// policy_bwd's twelve gradient terms as doubles (d[j]: parameter j), the same expressions,
// from policy_fwd_main's values (used only where its ok holds)
__device__ __forceinline__ void policy_terms(const float *p, double c, double v, const PolF &f, double dmu,
                                             double dsigma, double *d) {
  const double dam = dmu * dsoftplus_r(f.am, f.eam, f.ram), das = dsigma * dsoftplus_r(f.as, f.eas, f.ras);
  double ds[2];
  ds[0] = dam * (double)p[6] + das * (double)p[9];
  ds[1] = dam * (double)p[7] + das * (double)p[10];
  d[6] = dam * f.s[0];
  d[7] = dam * f.s[1];
  d[8] = dam;
  d[9] = das * f.s[0];
  d[10] = das * f.s[1];
  d[11] = das;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double dh = ds[j] * dsoftplus_r(f.h[j], f.eh[j], f.rh[j]);
    d[2 * j] = dh * c;
    d[2 * j + 1] = dh * v;
    d[4 + j] = dh;
  }
}
// a record's N fixed-point terms through fxb's fast path when every one is in its range (ok
// in: the record's main-path test), added to acc[0..N); false (nothing added) otherwise
template <int N>
__device__ __forceinline__ bool fx_add_fast(int64_t (&acc)[16], const double (&d)[N], bool ok) {
  double x[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    x[k] = d[k] * kGrid;
    ok = (int)ok & (int)fx_in(x[k]);
  }
  if (__builtin_expect(!ok, 0)) return false;
#pragma unroll
  for (int k = 0; k < N; ++k) addw(acc[k], fxb_x(x[k]));
  return true;
}

__device__ __forceinline__ void policy_bwd(const float *p, double c, double v, const PolF &f, double dmu,
                                           double dsigma, int64_t (&G)[16], int off, const uint64_t *tab) {
  const double dam = dmu * dsoftplus_e(f.am, f.eam), das = dsigma * dsoftplus_e(f.as, f.eas);
  double ds[2];
  ds[0] = dam * (double)p[6] + das * (double)p[9];
  ds[1] = dam * (double)p[7] + das * (double)p[10];
  // biased terms (fxb): one per accumulator per record, fx_unbias'd by the caller
  addw(G[off + 6], fxb(dam * f.s[0]));
  addw(G[off + 7], fxb(dam * f.s[1]));
  addw(G[off + 8], fxb(dam));
  addw(G[off + 9], fxb(das * f.s[0]));
  addw(G[off + 10], fxb(das * f.s[1]));
  addw(G[off + 11], fxb(das));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double dh = ds[j] * dsoftplus_e(f.h[j], f.eh[j]);
    addw(G[off + 2 * j], fxb(dh * c));
    addw(G[off + 2 * j + 1], fxb(dh * v));
    addw(G[off + 4 + j], fxb(dh));
  }
}

__device__ __forceinline__ void bias_corrections(int step, const double *adam_tab, float &bc2f, double &bc1) {
  // adam_tab: [0, kDrEpochs): 1 - 0.9^t; [kDrEpochs, 2 kDrEpochs): (1 - 0.999^t)^0.5 (libm pow)
  bc1 = adam_tab[step];
  bc2f = (float)adam_tab[kDrEpochs + step];
}

// records of agent a: SoA, bucketed: ctr, value, gamma, prop, util (f64), won (u8)
struct DrRecords {
  const double *ctr, *value, *gamma, *prop, *util;
  const uint8_t *won;
};

// LDS of one workgroup
struct TrainLds {
  uint64_t tab[256];
  float wr[4], pol[12];
  int64_t w[kDrThreads / 64][32];
  int64_t tot[32];
  double wf[kDrThreads / 64][16];
  double ftot[16];
  AdamState adam;
  int stop;       // a NaN loss
  int exhausted;  // a noise-driven fit ran out of noise epochs before it stopped
  int flag;       // agent_allreduce_i64's broadcast
};

__device__ __forceinline__ void adam_reset(TrainLds &S) {
  if (threadIdx.x < 16) S.adam.ea[threadIdx.x] = S.adam.es[threadIdx.x] = S.adam.mx[threadIdx.x] = 0.0f;
  __syncthreads();
}

// The workgroups training one agent: each owns a contiguous chunk of the agent's records and
// exchanges its per-epoch partial sums through `part` ([2 parities][nblk][32] words) at an
// agent barrier; afterwards every workgroup holds the same totals and runs the same Adam /
// scheduler / early-stop step on its LDS copy of the parameters (the workgroups stay in
// lockstep without a second barrier: an exchange's parity buffer is only rewritten two
// exchanges later, after every workgroup has passed the barrier in between).
struct Coop {
  int rank, nblk;
  int64_t *part;
  unsigned *bar;  // the agent's barrier lines (bar_lines)
  int ph;         // exchanges so far (identical in every workgroup of the agent)
  int64_t *acc;   // exact_totals' accumulator rows [bar_lines][32] (row 0: the totals), zero
                  // between exchanges
};

// exact totals of NV fixed-point sums over the agent's records (S.tot: hi, lo pairs), summed
// up the agent barrier's combining tree with integer atomics: each workgroup adds its 2 NV
// words to its level-0 node's accumulator row and arrives; the last arriver at a node moves
// the node's row into its parent's (zeroing it) and arrives one level up; the root's last
// arriver publishes the totals in row 0 and releases everyone, who read that one row.
// Integer additions: the totals are exact whatever the order (round 1 had every workgroup
// read every other workgroup's partials after the barrier: nblk lines from other XCDs per
// workgroup per epoch).
template <int NV>
__device__ __forceinline__ void exact_totals(const int64_t (&acc)[NV], TrainLds &S, Coop &C) {
  block_sums<NV>(acc, S.w, S.tot);
  if (C.nblk > 1) {
    agcoop::agent_allreduce_i64(C.bar, C.acc, 32, C.rank, C.nblk, S.tot, 2 * NV, S.tot, &S.flag);
    ++C.ph;
  }
}

// Fixed-order double sums (the policy-learning fits: importance weights are unbounded, so
// their terms do not fit a fixed-point grid). In each workgroup, record c0 + j is added by
// thread j mod 256 in record order; each wave combines by the butterfly v + shfl_xor(v, o),
// o = 32 .. 1 (the same value on every lane); the wave totals are added to 0.0 in wave
// order; the workgroup totals are added to 0.0 in workgroup order. oracle/ag_oracle_dr.c
// pl_epoch is this order exactly.
template <int NV>
__device__ __forceinline__ void float_totals(const double (&v)[NV], TrainLds &S, Coop &C) {
  static_assert(NV <= 16, "float_totals: at most 16 sums");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double x = v[j];
    for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, 64);
    if (lane == 0) S.wf[wv][j] = x;
  }
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < NV)
    for (int w = 0; w < kDrThreads / 64; ++w) t += S.wf[w][threadIdx.x];
  if (C.nblk > 1) {
    double *pp = reinterpret_cast<double *>(C.part + (size_t)(C.ph & 1) * C.nblk * 32);
    if (threadIdx.x < NV) pp[C.rank * 32 + threadIdx.x] = t;
    agent_barrier(C.bar, C.rank, C.nblk);
    if (threadIdx.x < NV) {
      double T = 0.0;
      for (int b = 0; b < C.nblk; ++b) T += pp[b * 32 + threadIdx.x];
      S.ftot[threadIdx.x] = T;
    }
    ++C.ph;
  } else if (threadIdx.x < NV) {
    S.ftot[threadIdx.x] = 0.0 + t;
  }
  __syncthreads();
}

// one Adam step of the first np parameters of `par` (thread j: parameter j)
__device__ __forceinline__ void adam_step_block(TrainLds &S, float *par, int np, float grad, int step, double lr,
                                                float wd, const double *adam_tab) {
  double bc1;
  float bc2f;
  bias_corrections(step, adam_tab, bc2f, bc1);
  const float neg_step = (float)(-(lr / bc1));
  if ((int)threadIdx.x < np) {
    float p = par[threadIdx.x];
    adam_param(p, grad, threadIdx.x, S.adam, neg_step, bc2f, wd);
    par[threadIdx.x] = p;
  }
}

// The rsample noise of the DR / DM policy fits: the caller's draws (noise != NULL: agent's
// record i of epoch e at noise[e * n + i]) or synthetic ones -- a standard normal by
// Marsaglia's polar method on Philox4x32-10 (counter (i, e, attempt, agent), key = seed), two
// candidate pairs of 32-bit uniforms per call (a wave's 64 lanes then finish in ~2 calls
// instead of ~4 with one pair), its log through the restated log1p, so the host
// (oracle/ag_oracle_dr.c ora_fit_noise) draws the same bits.
struct FitNoise {
  const float *noise;  // agent's draws or NULL
  int64_t n;           // agent's record count
  uint64_t seed;
  uint32_t agent;
  int epochs;          // epochs available (synthetic: unlimited)
};

__device__ __forceinline__ double fit_eps(const FitNoise &F, int e, int64_t i) {
  if (F.noise) return (double)F.noise[(int64_t)e * F.n + i];
  // the rejection loop only finds the first accepted (u, s); the transform runs once after
  // it for every lane together (a wave's lanes accept at different attempts)
  double u = 0.0, s = 0.0;
  bool found = false;
  for (uint32_t t = 0; t < 32 && !found; ++t) {
    uint32_t w[4];
    philox((uint32_t)i, (uint32_t)e, t, F.agent, (uint32_t)F.seed, (uint32_t)(F.seed >> 32), w);
    const double u0 = (double)w[0] * 0x1p-31 - 1.0, v0 = (double)w[1] * 0x1p-31 - 1.0;
    const double u1 = (double)w[2] * 0x1p-31 - 1.0, v1 = (double)w[3] * 0x1p-31 - 1.0;
    const double s0 = u0 * u0 + v0 * v0, s1 = u1 * u1 + v1 * v1;
    const bool a0 = s0 > 0.0 && s0 < 1.0, a1 = s1 > 0.0 && s1 < 1.0;
    if (a0 || a1) {
      u = a0 ? u0 : u1;
      s = a0 ? s0 : s1;
      found = true;
    }
  }
  if (!found) return 0.0;
  return polar_transform(u, s);
}

// records of the workgroup: [c0, c0 + nb) of the agent's n
struct Chunk {
  int64_t c0, nb, n;
};
// workgroup `rank` of the G that share an agent's n records: a contiguous slice each
__device__ __forceinline__ Chunk wg_slice(int64_t n, int G, int rank) {
  const int64_t per = (n + G - 1) / G;
  const int64_t c0 = (int64_t)rank * per < n ? (int64_t)rank * per : n;
  return Chunk{c0, (c0 + per < n ? c0 + per : n) - c0, n};
}

// The workgroup's records as the fits read them, every epoch: the first `cap` of its chunk
// staged once in LDS as float32 fields (every fit consumes them through a float32 rounding,
// so the staged values are the ones it would compute: (float)ctr, (float)value, ...), the rest
// read from the global store. Local index j = record c0 + j of the agent. Fields [nf][cap]
// floats: ctr, value, gamma, propensity, utility, estimated utility; then won [cap] bytes.
enum { kFCtr = 0, kFVal, kFGam, kFProp, kFUtil, kFEu };
struct RecView {
  DrRecords R;       // the agent's records (global)
  const double *eu;  // the agent's estimated utilities (global, DoublyRobustBidder)
  int64_t c0;
  const float *lf;  // LDS fields
  const uint8_t *lw;
  int64_t cap;      // staged records (a multiple of kDrThreads, so j < cap is block-uniform)
  __device__ __forceinline__ double f(int fld, const double *g, int64_t j) const {
    return j < cap ? (double)lf[(int64_t)fld * cap + j] : (double)(float)g[c0 + j];
  }
  __device__ __forceinline__ double ctr(int64_t j) const { return f(kFCtr, R.ctr, j); }
  __device__ __forceinline__ double val(int64_t j) const { return f(kFVal, R.value, j); }
  __device__ __forceinline__ double gam(int64_t j) const { return f(kFGam, R.gamma, j); }
  __device__ __forceinline__ float prop(int64_t j) const {
    return j < cap ? lf[(int64_t)kFProp * cap + j] : (float)R.prop[c0 + j];
  }
  __device__ __forceinline__ double util(int64_t j) const { return f(kFUtil, R.util, j); }
  __device__ __forceinline__ double eut(int64_t j) const { return f(kFEu, eu, j); }
  __device__ __forceinline__ double won(int64_t j) const { return (double)(j < cap ? lw[j] : R.won[c0 + j]); }
  // the same fields with the LDS / global choice known at compile time (each_record's loops)
  template <bool L>
  __device__ __forceinline__ double fl(int fld, const double *g, int64_t j) const {
    if constexpr (L) return (double)lf[(int64_t)fld * cap + j];
    else return (double)(float)g[c0 + j];
  }
  template <bool L> __device__ __forceinline__ double ctr_(int64_t j) const { return fl<L>(kFCtr, R.ctr, j); }
  template <bool L> __device__ __forceinline__ double val_(int64_t j) const { return fl<L>(kFVal, R.value, j); }
  template <bool L> __device__ __forceinline__ double gam_(int64_t j) const { return fl<L>(kFGam, R.gamma, j); }
  template <bool L> __device__ __forceinline__ double util_(int64_t j) const { return fl<L>(kFUtil, R.util, j); }
  template <bool L> __device__ __forceinline__ double eut_(int64_t j) const { return fl<L>(kFEu, eu, j); }
  template <bool L> __device__ __forceinline__ float prop_(int64_t j) const {
    if constexpr (L) return lf[(int64_t)kFProp * cap + j];
    else return (float)R.prop[c0 + j];
  }
  template <bool L> __device__ __forceinline__ double won_(int64_t j) const {
    if constexpr (L) return (double)lw[j];
    else return (double)R.won[c0 + j];
  }
};

// f(j, std::true_type / std::false_type) for this thread's records j of [0, nb): the staged
// ones (j < cap, read from LDS) then the rest (global) -- two loops with the source known at
// compile time, instead of a per-field test (cap is a multiple of kDrThreads)
template <class F>
__device__ __forceinline__ void each_record(const RecView &V, int64_t nb, F &&f) {
  const int64_t ns = nb < V.cap ? nb : V.cap;
  int64_t j = threadIdx.x;
  for (; j < ns; j += kDrThreads) f(j, std::true_type());
  for (; j < nb; j += kDrThreads) f(j, std::false_type());
}

// One BCE row of the win-rate fit: wr_main (branch-free) and wr_patch (ag_train_math.h); wr_finish
// patches (rarely) and adds the terms.
__device__ __forceinline__ void wr_finish(int64_t (&acc)[5], WrMain m, double c, double v, double g, double y,
                                          bool aug, const uint64_t *tab) {
  int64_t t2, t3;
  if (__builtin_expect(m.ok, 1)) {
    t2 = fxb_x(m.x2);
    t3 = fxb_x(m.x3);
  } else {
    if (!m.main) wr_patch(m, y, tab);
    t2 = fxb(m.gz * v);
    t3 = fxb(m.gz * g);
  }
  addw(acc[0], fxb_fast(m.t));
  addw(acc[1], fxb_fast(m.gz * c));
  addw(acc[2], t2);
  if (!aug) addw(acc[3], t3);  // the augmentation row's g = 0 term is +-0: rounds to 0
  addw(acc[4], fxb_fast(m.gz));
}

// a record's logged row and its gamma = 0, y = 0 augmentation row, both main paths first
__device__ __forceinline__ void wr_pair(int64_t (&acc)[5], double c, double v, double g, double y, double w0,
                                        double w1, double w2, double w3, const uint64_t *tab) {
  const WrMain A = wr_main(c, v, g, y, false, w0, w1, w2, w3, tab);
  const WrMain B = wr_main(c, v, 0.0, 0.0, true, w0, w1, w2, w3, tab);
  if (__builtin_expect((int)A.ok & (int)B.ok, 1)) {  // one branch for both rows
    addw(acc[0], fxb_fast(A.t));
    addw(acc[1], fxb_fast(A.gz * c));
    addw(acc[2], fxb_x(A.x2));
    addw(acc[3], fxb_x(A.x3));
    addw(acc[4], fxb_fast(A.gz));
    addw(acc[0], fxb_fast(B.t));
    addw(acc[1], fxb_fast(B.gz * c));
    addw(acc[2], fxb_x(B.x2));
    addw(acc[4], fxb_fast(B.gz));
  } else {
    wr_finish(acc, A, c, v, g, y, false, tab);
    wr_finish(acc, B, c, v, 0.0, 0.0, true, tab);
  }
}

// a lane that ran wr_pair for nrec records (both rows each): its accumulators unbiased
__device__ __forceinline__ void wr_unbias(int64_t (&acc)[5], int64_t nrec) {
  fx_unbias(acc[0], 2 * nrec);
  fx_unbias(acc[1], 2 * nrec);
  fx_unbias(acc[2], 2 * nrec);
  fx_unbias(acc[3], nrec);
  fx_unbias(acc[4], 2 * nrec);
}

// PyTorchWinRateEstimator fit (src/Bidder.py:229-252 ValueLearningBidder, :500-530
// DoublyRobustBidder): BCE (mean) over the logs plus the gamma = 0, y = 0 augmentation;
// H = fit_hyper(kFitWr, the bidder's kind).
__device__ int fit_winrate(const RecView &V, const Chunk &K, TrainLds &S, Coop &C, const FitHyper H,
                           const double *adam_tab, float *tr) {
  const int tid = threadIdx.x;
  adam_reset(S);
  double lr = H.lr;
  Plateau pl = plateau_of(H);
  Stopper sp = stopper_of(H);
  const double M = 2.0 * (double)K.n;
  int e = 0;
  for (; e < H.max_epochs; ++e) {
    int64_t acc[5] = {0, 0, 0, 0, 0};
    const double w0 = (double)S.wr[0], w1 = (double)S.wr[1], w2 = (double)S.wr[2], w3 = (double)S.wr[3];
    // record j's logged row and its gamma = 0, y = 0 augmentation row together (two
    // independent chains for the scheduler; the sums are exact, so any order)
    int64_t nrec = 0;
    each_record(V, K.nb, [&](int64_t j, auto L) {
      constexpr bool l = decltype(L)::value;
      const double c = V.template ctr_<l>(j), v = V.template val_<l>(j);
      wr_pair(acc, c, v, V.template gam_<l>(j), V.template won_<l>(j), w0, w1, w2, w3, S.tab);
      ++nrec;
    });
    wr_unbias(acc, nrec);
    exact_totals<5>(acc, S, C);
    // every thread: the same loss; threads 0..3 step their parameter
    const float loss = (float)(fxv(S.tot[0], S.tot[1]) / M);
    const float g = tid < 4 ? (float)(fxv(S.tot[2 + 2 * tid], S.tot[3 + 2 * tid]) / M) : 0.0f;
    adam_step_block(S, S.wr, 4, g, e, lr, H.wd, adam_tab);
    if (tid == 0 && tr) tr[e] = loss;
    plateau_step(pl, loss, lr);  // every thread keeps the same scheduler state
    const bool stop = stop_step(sp, e, loss);
    __syncthreads();
    if (stop) return e + 1;
  }
  return e;
}

// one record of the imitation fit: MSE terms of mu to the logged gamma and of softplus(sigma)
// to 0.05 (acc[12], acc[13]) and their gradient (acc[0..11]), biased
__device__ __noinline__ void imit_rec_exact(int64_t (&acc)[16], const float *pol, double c, double v, double g,
                                            const uint64_t *tab) {
  PolF f;
  policy_fwd(pol, c, v, f, tab);
  const double dm = f.mu - g, dsg = f.sp_sigma - 0.05;
  addw(acc[12], fxb(dm * dm));
  addw(acc[13], fxb(dsg * dsg));
  policy_bwd(pol, c, v, f, 2.0 * dm, 2.0 * dsg, acc, 0, tab);
}
// the common path: main-path functions and fast fixed-point terms, imit_rec_exact (the same
// terms) when a record leaves them
__device__ __forceinline__ void imit_rec(int64_t (&acc)[16], const float *pol, double c, double v, double g,
                                         const uint64_t *tab) {
  PolF f;
  const bool ok = policy_fwd_main(pol, c, v, f, tab);
  const double dm = f.mu - g, dsg = f.sp_sigma - 0.05;
  double d[14];
  policy_terms(pol, c, v, f, 2.0 * dm, 2.0 * dsg, d);
  d[12] = dm * dm;
  d[13] = dsg * dsg;
  if (__builtin_expect(!fx_add_fast<14>(acc, d, ok), 0)) {  // (a separate array: acc stays in registers)
    int64_t t[16] = {};
    imit_rec_exact(t, pol, c, v, g, tab);
#pragma unroll
    for (int k = 0; k < 14; ++k) addw(acc[k], t[k]);
  }
}

// BidShadingContextualBandit.initialise_policy (src/Models.py:106-137): imitation of the
// logging policy, MSE of mu to the logged gammas + MSE of softplus(sigma) (without
// min_sigma) to 0.05; fit_hyper(kFitInit): no scheduler.
__device__ int fit_imitation(const RecView &V, const Chunk &K, TrainLds &S, Coop &C, const double *adam_tab,
                             float *tr) {
  constexpr FitHyper H = fit_hyper(kFitInit, AG_BIDDER_DOUBLY_ROBUST);  // (the same for every kind)
  const int tid = threadIdx.x;
  adam_reset(S);
  Stopper sp = stopper_of(H);
  const double n = (double)K.n;
  int e = 0;
  for (; e < H.max_epochs; ++e) {
    int64_t acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
    each_record(V, K.nb, [&](int64_t j, auto L) {
      constexpr bool l = decltype(L)::value;
      imit_rec(acc, S.pol, V.template ctr_<l>(j), V.template val_<l>(j), V.template gam_<l>(j), S.tab);
    });
    const int64_t nrec = K.nb > tid ? (K.nb - tid + kDrThreads - 1) / kDrThreads : 0;
#pragma unroll
    for (int q = 0; q < 14; ++q) fx_unbias(acc[q], nrec);
    exact_totals<16>(acc, S, C);
    const float loss = (float)(fxv(S.tot[24], S.tot[25]) / n + fxv(S.tot[26], S.tot[27]) / n);
    const float g = tid < 12 ? (float)(fxv(S.tot[2 * tid], S.tot[2 * tid + 1]) / n) : 0.0f;
    adam_step_block(S, S.pol, 12, g, e, H.lr, H.wd, adam_tab);
    if (tid == 0 && tr) tr[e] = loss;
    const bool stop = stop_step(sp, e, loss);
    __syncthreads();
    if (stop) return e + 1;
  }
  return e;
}

// one record of the DR policy fit (fit_dr): its loss term (acc[12]) and gradient (acc[0..11]),
// biased; du = utility - estimated utility, ep = the epoch's rsample draw
__device__ __noinline__ void dr_rec_exact(int64_t (&acc)[16], const float *pol, const float *wr, double c,
                                          double v, double g, float prop, double du, double ep, const uint64_t *tab) {
  const double inv_sqrt2pi = 1.0 / __builtin_sqrt(2.0 * 3.141592653589793);
  PolF f;
  policy_fwd(pol, c, v, f, tab);
  const double mu = f.mu, sg = f.sigma;
  const double zz = (mu - g) / sg;
  const double pdf_raw = exp_fast(-(zz * zz) / 2.0, tab) / sg * inv_sqrt2pi;
  const double pi = pdf_raw < 1e-30 ? 1e-30 : pdf_raw;
  const double p0 = (double)fmaxf(prop, 1e-15f);
  const double iw = pi / p0;
  const double iwc = iw < 1.0 / 50.0 ? 1.0 / 50.0 : (iw > 50.0 ? 50.0 : iw);
  const double raw = mu + sg * ep;
  const double gs = raw < 0.0 ? 0.0 : (raw > 1.0 ? 1.0 : raw);
  const double zw = c * (double)wr[0] + v * (double)wr[1] + gs * (double)wr[2] + (double)wr[3];
  const double Wv = 1.0 / (1.0 + exp_fast(-zw, tab));
  const double V = c * v;
  addw(acc[12], fxb(-(du * iwc + Wv * (V - V * gs))));
  double dpi_dmu = 0.0, dpi_dsg = 0.0;
  if (pdf_raw >= 1e-30 && iw >= 1.0 / 50.0 && iw <= 50.0) {
    const double k = du / p0;
    dpi_dmu = k * pdf_raw * (g - mu) / (sg * sg);
    dpi_dsg = k * pdf_raw * ((g - mu) * (g - mu) / (sg * sg * sg) - 1.0 / sg);
  }
  double ddm = 0.0;
  if (raw >= 0.0 && raw <= 1.0) ddm = -Wv * V + (V - V * gs) * Wv * (1.0 - Wv) * (double)wr[2];
  policy_bwd(pol, c, v, f, -(dpi_dmu + ddm), -(dpi_dsg + ddm * ep), acc, 0, tab);
}
// the common path of dr_rec_exact (main-path exp / softplus, fast fixed-point terms; the
// same expressions), dr_rec_exact when a record leaves it
__device__ __forceinline__ void dr_rec(int64_t (&acc)[16], const float *pol, const float *wr, double c, double v,
                                       double g, float prop, double du, double ep, const uint64_t *tab) {
  const double inv_sqrt2pi = 1.0 / __builtin_sqrt(2.0 * 3.141592653589793);
  PolF f;
  bool ok = policy_fwd_main(pol, c, v, f, tab);
  const double mu = f.mu, sg = f.sigma;
  const double p0 = (double)fmaxf(prop, 1e-15f);
  // three divisions by sg, two by p0: one reciprocal each (ag_div.h; a record whose operands
  // leave div_safe's range takes dr_rec_exact)
  const double rsg = agdiv::recip(sg), rp0 = agdiv::recip(p0);
  const double zz = agdiv::div_core(mu - g, sg, rsg);
  const double xp = -(zz * zz) / 2.0;
  const double ex = agexp::exp_main(xp, tab);
  const double pdf_raw = agdiv::div_core(ex, sg, rsg) * inv_sqrt2pi;
  const double pi = pdf_raw < 1e-30 ? 1e-30 : pdf_raw;
  const double iw = agdiv::div_core(pi, p0, rp0);
  ok = (int)ok & (int)agdiv::div_safe(mu - g, sg) & (int)agdiv::div_safe(ex, sg) & (int)agdiv::div_safe(pi, p0) &
       (int)agdiv::div_safe(du, p0);
  const double iwc = iw < 1.0 / 50.0 ? 1.0 / 50.0 : (iw > 50.0 ? 50.0 : iw);
  const double raw = mu + sg * ep;
  const double gs = raw < 0.0 ? 0.0 : (raw > 1.0 ? 1.0 : raw);
  const double zw = c * (double)wr[0] + v * (double)wr[1] + gs * (double)wr[2] + (double)wr[3];
  const double Wv = 1.0 / (1.0 + agexp::exp_main(-zw, tab));
  ok = (int)ok & (int)agexp::exp_in_main(xp) & (int)agexp::exp_in_main(-zw);
  const double V = c * v;
  double d[13];
  d[12] = -(du * iwc + Wv * (V - V * gs));
  double dpi_dmu = 0.0, dpi_dsg = 0.0;
  if (pdf_raw >= 1e-30 && iw >= 1.0 / 50.0 && iw <= 50.0) {
    const double k = agdiv::div_core(du, p0, rp0);
    dpi_dmu = k * pdf_raw * (g - mu) / (sg * sg);
    dpi_dsg = k * pdf_raw * ((g - mu) * (g - mu) / (sg * sg * sg) - agdiv::div_core(1.0, sg, rsg));
  }
  double ddm = 0.0;
  if (raw >= 0.0 && raw <= 1.0) ddm = -Wv * V + (V - V * gs) * Wv * (1.0 - Wv) * (double)wr[2];
  policy_terms(pol, c, v, f, -(dpi_dmu + ddm), -(dpi_dsg + ddm * ep), d);
  if (__builtin_expect(!fx_add_fast<13>(acc, d, ok), 0)) {
    int64_t t[16] = {};
    dr_rec_exact(t, pol, wr, c, v, g, prop, du, ep, tab);
#pragma unroll
    for (int k = 0; k < 13; ++k) addw(acc[k], t[k]);
  }
}

// DoublyRobustBidder's policy fit (src/Bidder.py:562-590, src/Models.py:201-218): loss
// -mean((u - u^) clip(pi / pi0, 1/50, 50) + W(ctr, value, g~) (V - V g~)), g~ = clip(mu +
// sigma eps, 0, 1); fit_hyper(kFitPol, DoublyRobust).
__device__ int fit_dr(const RecView &V, const Chunk &K, TrainLds &S, Coop &C,
                      const FitNoise &F, const double *adam_tab, float *tr) {
  constexpr FitHyper H = fit_hyper(kFitPol, AG_BIDDER_DOUBLY_ROBUST);
  const int tid = threadIdx.x;
  adam_reset(S);
  double lr = H.lr;
  Plateau pl = plateau_of(H);
  Stopper sp = stopper_of(H);
  const double n = (double)K.n;
  int e = 0;
  for (; e < H.max_epochs && e < F.epochs; ++e) {
    int64_t acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
    each_record(V, K.nb, [&](int64_t j, auto L) {
      constexpr bool l = decltype(L)::value;
      dr_rec(acc, S.pol, S.wr, V.template ctr_<l>(j), V.template val_<l>(j), V.template gam_<l>(j),
             V.template prop_<l>(j), V.template util_<l>(j) - V.template eut_<l>(j), fit_eps(F, e, K.c0 + j), S.tab);
    });
    const int64_t nrec = K.nb > tid ? (K.nb - tid + kDrThreads - 1) / kDrThreads : 0;
#pragma unroll
    for (int q = 0; q < 13; ++q) fx_unbias(acc[q], nrec);
    exact_totals<16>(acc, S, C);
    const float loss = (float)(fxv(S.tot[24], S.tot[25]) / n);
    const float g = tid < 12 ? (float)(fxv(S.tot[2 * tid], S.tot[2 * tid + 1]) / n) : 0.0f;
    adam_step_block(S, S.pol, 12, g, e, lr, H.wd, adam_tab);
    if (tid == 0 && tr) tr[e] = loss;
    plateau_step(pl, loss, lr);
    const bool stop = stop_step(sp, e, loss);
    if (tid == 0 && loss != loss) S.stop = 1;  // NaN: the reference exits (src/Bidder.py:592-600)
    __syncthreads();
    if (stop || S.stop) return e + 1;
  }
  if (e < H.max_epochs && tid == 0) S.exhausted = 1;
  return e;
}

// one record of the ValueLearningBidder policy fit (fit_dm), biased
__device__ __noinline__ void dm_rec_exact(int64_t (&acc)[16], const float *pol, const float *wr, double c,
                                          double v, double ep, const uint64_t *tab) {
  PolF f;
  policy_fwd(pol, c, v, f, tab);
  const double raw = f.mu + f.sigma * ep;
  const double gs = raw < 0.0 ? 0.0 : (raw > 1.0 ? 1.0 : raw);
  const double zw = c * (double)wr[0] + v * (double)wr[1] + gs * (double)wr[2] + (double)wr[3];
  const double Wv = 1.0 / (1.0 + exp_fast(-zw, tab));
  const double V = c * v;
  addw(acc[12], fxb(-(Wv * (V - V * gs))));
  double ddm = 0.0;
  if (raw >= 0.0 && raw <= 1.0) ddm = -Wv * V + (V - V * gs) * Wv * (1.0 - Wv) * (double)wr[2];
  policy_bwd(pol, c, v, f, -ddm, -(ddm * ep), acc, 0, tab);
}
// the common path of dm_rec_exact, dm_rec_exact when a record leaves it
__device__ __forceinline__ void dm_rec(int64_t (&acc)[16], const float *pol, const float *wr, double c, double v,
                                       double ep, const uint64_t *tab) {
  PolF f;
  bool ok = policy_fwd_main(pol, c, v, f, tab);
  const double raw = f.mu + f.sigma * ep;
  const double gs = raw < 0.0 ? 0.0 : (raw > 1.0 ? 1.0 : raw);
  const double zw = c * (double)wr[0] + v * (double)wr[1] + gs * (double)wr[2] + (double)wr[3];
  const double Wv = 1.0 / (1.0 + agexp::exp_main(-zw, tab));
  ok = (int)ok & (int)agexp::exp_in_main(-zw);
  const double V = c * v;
  double d[13];
  d[12] = -(Wv * (V - V * gs));
  double ddm = 0.0;
  if (raw >= 0.0 && raw <= 1.0) ddm = -Wv * V + (V - V * gs) * Wv * (1.0 - Wv) * (double)wr[2];
  policy_terms(pol, c, v, f, -ddm, -(ddm * ep), d);
  if (__builtin_expect(!fx_add_fast<13>(acc, d, ok), 0)) {
    int64_t t[16] = {};
    dm_rec_exact(t, pol, wr, c, v, ep, tab);
#pragma unroll
    for (int k = 0; k < 13; ++k) addw(acc[k], t[k]);
  }
}

// ValueLearningBidder's policy fit (inference 'policy', src/Bidder.py:258-303): loss
// -mean(W(ctr, value, g~) (V - V g~)), g~ = clip(mu + sigma eps, 0, 1); fit_hyper(kFitPol,
// ValueLearning). Exact fixed-point sums (bounded terms).
__device__ int fit_dm(const RecView &V, const Chunk &K, TrainLds &S, Coop &C, const FitNoise &F,
                      const double *adam_tab, float *tr) {
  constexpr FitHyper H = fit_hyper(kFitPol, AG_BIDDER_VALUE_LEARNING);
  const int tid = threadIdx.x;
  adam_reset(S);
  double lr = H.lr;
  Plateau pl = plateau_of(H);
  Stopper sp = stopper_of(H);
  const double n = (double)K.n;
  int e = 0;
  for (; e < H.max_epochs && e < F.epochs; ++e) {
    int64_t acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
    each_record(V, K.nb, [&](int64_t j, auto L) {
      constexpr bool l = decltype(L)::value;
      dm_rec(acc, S.pol, S.wr, V.template ctr_<l>(j), V.template val_<l>(j), fit_eps(F, e, K.c0 + j), S.tab);
    });
    const int64_t nrec = K.nb > tid ? (K.nb - tid + kDrThreads - 1) / kDrThreads : 0;
#pragma unroll
    for (int q = 0; q < 13; ++q) fx_unbias(acc[q], nrec);
    exact_totals<16>(acc, S, C);
    const float loss = (float)(fxv(S.tot[24], S.tot[25]) / n);
    const float g = tid < 12 ? (float)(fxv(S.tot[2 * tid], S.tot[2 * tid + 1]) / n) : 0.0f;
    adam_step_block(S, S.pol, 12, g, e, lr, H.wd, adam_tab);
    if (tid == 0 && tr) tr[e] = loss;
    plateau_step(pl, loss, lr);
    const bool stop = stop_step(sp, e, loss);
    __syncthreads();
    if (stop) return e + 1;
  }
  if (e < H.max_epochs && tid == 0) S.exhausted = 1;
  return e;
}

// DoublyRobustBidder's estimated utilities (src/Bidder.py:541-546) of the workgroup's slice
// [c0, c0 + nb) of the agent's records R, with the fitted win-rate model wr: written to eu
// (global, the agent's) and, the slice's first `cap`, to the LDS row lfe of the record cache
// (cap = 0: no cache). each_record's thread mapping: a thread reads back what it wrote.
__device__ __forceinline__ void estimated_utilities(const DrRecords &R, int64_t c0, int64_t nb, const float *wr,
                                                    double *eu, const uint64_t *tab, float *lfe = nullptr,
                                                    int64_t cap = 0) {
  for (int64_t j = threadIdx.x; j < nb; j += kDrThreads) {
    const int64_t i = c0 + j;
    const double c = (double)(float)R.ctr[i], v = (double)(float)R.value[i], g = (double)(float)R.gamma[i];
    const double z = c * (double)wr[0] + v * (double)wr[1] + g * (double)wr[2] + (double)wr[3];
    const float W = (float)(1.0 / (1.0 + agexp::exp(-z, tab)));
    const double Vv = R.ctr[i] * R.value[i], P = R.ctr[i] * R.value[i] * R.gamma[i];
    eu[i] = (double)W * (Vv - P);
    if (j < cap) lfe[j] = (float)eu[i];
  }
}

// per-record gradient of a policy loss term from d/dmu and d/dsigma (policy_bwd's order)
__device__ __forceinline__ void policy_grad(const float *p, double c, double v, const PolF &f, double dmu,
                                            double dsigma, double (&G)[14], const uint64_t *tab) {
  const double dam = dmu * dsoftplus_e(f.am, f.eam), das = dsigma * dsoftplus_e(f.as, f.eas);
  double ds[2];
  ds[0] = dam * (double)p[6] + das * (double)p[9];
  ds[1] = dam * (double)p[7] + das * (double)p[10];
  G[6] += dam * f.s[0];
  G[7] += dam * f.s[1];
  G[8] += dam;
  G[9] += das * f.s[0];
  G[10] += das * f.s[1];
  G[11] += das;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double dh = ds[j] * dsoftplus_e(f.h[j], f.eh[j]);
    G[2 * j] += dh * c;
    G[2 * j + 1] += dh * v;
    G[4 + j] += dh;
  }
}

// PolicyLearningBidder's policy fit (src/Bidder.py:376-407, the losses of src/Models.py:
// 174-199; AG_PL_LOSS_* kinds): Adam(lr 2e-3, wd 1e-4, AMSGrad), ReduceLROnPlateau
// (patience 100, factor 0.2, min_lr 1e-8), early stop after 512 epochs, <= 16384 epochs.
// oracle/ag_oracle_dr.c pl_epoch, term for term, with the same fixed-order sums.
__device__ int fit_pl(const RecView &V, const Chunk &K, TrainLds &S, Coop &C, int kind, const double *adam_tab,
                      float *tr) {
  const int tid = threadIdx.x;
  adam_reset(S);
  double lr = 2e-3;
  Plateau pl{INFINITY, 1e-4, 0.2, 1e-8, 0, 100};
  Stopper sp{INFINITY, -1, 512};
  const double inv_sqrt2pi = 1.0 / __builtin_sqrt(2.0 * 3.141592653589793);
  const double n = (double)K.n;
  int e = 0;
  for (; e < kInitEpochs; ++e) {
    double acc[14];
#pragma unroll
    for (int j = 0; j < 14; ++j) acc[j] = 0.0;
    for (int64_t j = tid; j < K.nb; j += kDrThreads) {
      const double c = V.ctr(j), v = V.val(j), g = V.gam(j);
      PolF f;
      policy_fwd_fast(S.pol, c, v, f, S.tab);
      const double mu = f.mu, sg = f.sigma;
      const double zz = (mu - g) / sg;
      const double pdf_raw = exp_fast(-(zz * zz) / 2.0, S.tab) / sg * inv_sqrt2pi;
      const double pi = pdf_raw < 1e-30 ? 1e-30 : pdf_raw;
      const double p0 = (double)fmaxf(V.prop(j), 1e-15f);
      const double u = V.util(j);
      double term = 0.0, kl = 0.0, dpi = 0.0, dmu = 0.0, dsg = 0.0;
      if (kind == AG_PL_LOSS_REINFORCE) {
        term = -(pi * u);
        dpi = -u;
      } else if (kind == AG_PL_LOSS_REINFORCE_OFFPOLICY || kind == AG_PL_LOSS_TRPO) {
        term = -((pi / p0) * u);
        dpi = -u / p0;
        if (kind == AG_PL_LOSS_TRPO) {
          kl = (sg * sg + (mu - g) * (mu - g)) / (2.0 * sg * sg) - 0.5;
          dmu = 5e-2 * ((mu - g) / (sg * sg));
          dsg = 5e-2 * (-((mu - g) * (mu - g)) / (sg * sg * sg));
        }
      } else {  // PPO
        const double iw = pi / p0;
        const bool in_range = iw >= 1.0 / 50.0 && iw <= 50.0;
        const double iwc = iw < 1.0 / 50.0 ? 1.0 / 50.0 : (iw > 50.0 ? 50.0 : iw);
        const double A = iw * u, Bc = iwc * u;
        term = -(A < Bc ? A : Bc);
        dpi = (in_range || A < Bc) ? -u / p0 : 0.0;
      }
      if (pdf_raw >= 1e-30 && dpi != 0.0) {
        dmu += dpi * pdf_raw * (g - mu) / (sg * sg);
        dsg += dpi * pdf_raw * ((g - mu) * (g - mu) / (sg * sg * sg) - 1.0 / sg);
      }
      double gr[14];
#pragma unroll
      for (int q = 0; q < 14; ++q) gr[q] = 0.0;
      policy_grad(S.pol, c, v, f, dmu, dsg, gr, S.tab);
#pragma unroll
      for (int q = 0; q < 12; ++q) acc[q] += gr[q];
      acc[12] += term;
      acc[13] += kl;
    }
    float_totals<14>(acc, S, C);
    const float loss = (float)(S.ftot[12] / n + (S.ftot[13] / n) * 5e-2);
    const float g = tid < 12 ? (float)(S.ftot[tid] / n) : 0.0f;
    adam_step_block(S, S.pol, 12, g, e, lr, (float)1e-4, adam_tab);
    if (tid == 0 && tr) tr[e] = loss;
    plateau_step(pl, loss, lr);
    const bool stop = stop_step(sp, e, loss);
    if (tid == 0 && loss != loss) S.stop = 1;  // NaN: the reference exits (src/Bidder.py:409-417)
    __syncthreads();
    if (stop || S.stop) return e + 1;
  }
  return e;
}

// The workgroups of the learning bidders (ValueLearning, PolicyLearning, DoublyRobust): block
// b trains agent blk_agent[b] as workgroup blk_rank[b] of agent_nblk[agent] over the agent's
// records, running its fits in the reference's order, in two launches:
//   PH = 0: the win-rate fits (ValueLearning, DoublyRobust; a ValueLearningBidder without
//           wins falls back, status 1) -> wr_ws, epochs [a][0]; a register-lean loop, 4 waves
//           per SIMD;
//   PH = 1: everything after (estimated utilities, imitation, the policy fits) from wr_ws,
//           then the agent's state.
// status: 0 trained, 1 ValueLearningBidder fallback (no wins: nothing trained), -1 no logs,
// -2 NaN loss, -3 out of noise epochs (state not written); epochs [3] = (win-rate,
// imitation, policy fit); traces [3][32768] (workgroup 0).
template <int PH>
__global__ __launch_bounds__(kDrThreads, PH == 0 ? AG_DR_PH0_MIN_WAVES : AG_DR_PH1_MIN_WAVES) void k_bidder_train(
    const int32_t *__restrict__ bkind, const int32_t *__restrict__ bmode, const int32_t *__restrict__ blk_agent,
    const int32_t *__restrict__ blk_rank, const int32_t *__restrict__ agent_nblk,
    const int64_t *__restrict__ offsets, DrRecords R0, double *__restrict__ eu_ws, float *__restrict__ state,
    float *__restrict__ wr_ws, const int32_t *__restrict__ initialised, const float *__restrict__ noise,
    const int64_t *__restrict__ noise_off, int noise_epochs, uint64_t noise_seed, const double *__restrict__ adam_tab,
    int32_t *__restrict__ epochs_out, int32_t *__restrict__ status, float *__restrict__ traces,
    int64_t *__restrict__ partials, unsigned *__restrict__ barriers, const int32_t *__restrict__ bar_off, int nf,
    int64_t cap) {
  const int a = blk_agent[blockIdx.x], rank = blk_rank[blockIdx.x], nblk = agent_nblk[a];
  const int tid = threadIdx.x;
  const int bk = bkind[a];
  const int64_t s0 = offsets[a], n = offsets[a + 1] - s0;
  const bool lead = rank == 0;
  const bool has_wr = bk == AG_BIDDER_DOUBLY_ROBUST || bk == AG_BIDDER_VALUE_LEARNING;
  if (n == 0) {
    // no logs: a ValueLearningBidder falls back (its won mask sums to 0, src/Bidder.py:206-
    // 211); the other learners fail in the reference
    if (PH == 1 && lead && tid == 0) {
      epochs_out[3 * a] = epochs_out[3 * a + 1] = epochs_out[3 * a + 2] = 0;
      status[a] = bk == AG_BIDDER_VALUE_LEARNING ? 1 : -1;
    }
    return;
  }
  if (PH == 1 && bk == AG_BIDDER_VALUE_LEARNING && status[a] == 1) return;  // fallback: state unchanged
  __shared__ TrainLds S;
  for (int i = tid; i < 256; i += kDrThreads) S.tab[i] = ag_exp_tab[i];
  float *st = state + (size_t)a * 16;
  if (tid < 4) S.wr[tid] = (PH == 1 && has_wr) ? wr_ws[(size_t)a * 4 + tid] : st[tid];
  if (tid < 12) S.pol[tid] = st[4 + tid];
  if (tid == 0) S.stop = S.exhausted = 0;
  __syncthreads();
  DrRecords R{R0.ctr + s0, R0.value + s0, R0.gamma + s0, R0.prop + s0, R0.util + s0, R0.won + s0};
  const Chunk K = wg_slice(n, nblk, rank);
  // the agent's exchange region (its workgroups have consecutive block indices): [2][nblk][32]
  // parity buffers, then [nblk][32] accumulator rows
  int64_t *preg = partials + (size_t)(blockIdx.x - rank) * 3 * 32;
  unsigned *abar = barriers + (size_t)bar_off[a] * kBarLineWords;
  Coop C{rank, nblk, preg, abar, 0, preg + (size_t)2 * nblk * 32};
  // stage the chunk's first `cap` records in LDS (the fields this phase's fits read)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  float *lf = reinterpret_cast<float *>(s_dyn);
  uint8_t *lw = reinterpret_cast<uint8_t *>(lf + (size_t)nf * cap);
  {
    const int64_t ns = K.nb < cap ? K.nb : cap;
    const bool full = PH == 1 && bk != AG_BIDDER_VALUE_LEARNING;  // propensity, utility
    const bool won = PH == 0 || bk == AG_BIDDER_DOUBLY_ROBUST;
    for (int64_t j = tid; j < ns; j += kDrThreads) {
      const int64_t i = K.c0 + j;
      lf[kFCtr * cap + j] = (float)R.ctr[i];
      lf[kFVal * cap + j] = (float)R.value[i];
      lf[kFGam * cap + j] = (float)R.gamma[i];
      if (full) {
        lf[kFProp * cap + j] = (float)R.prop[i];
        lf[kFUtil * cap + j] = (float)R.util[i];
      }
      if (won) lw[j] = R.won[i];
    }
    __syncthreads();
  }
  const RecView V{R, eu_ws + s0, K.c0, lf, lw, cap};
  // the agent's trace rows from one pointer (tr, tr + kDrEpochs, tr + 2 kDrEpochs: trace_row's
  // rows, kept as offsets -- a trace_row call per fit costs phase 1 four more spilled SGPRs)
  float *tr = (traces && lead) ? trace_row(traces, a, kFitWr) : nullptr;
  if constexpr (PH == 0) {
    int ep0 = 0, stat = 0;
    if (bk == AG_BIDDER_DOUBLY_ROBUST) {
      ep0 = fit_winrate(V, K, S, C, fit_hyper(kFitWr, AG_BIDDER_DOUBLY_ROBUST), adam_tab, tr);
    } else {  // ValueLearningBidder
      int64_t acc[1] = {0};
      each_record(V, K.nb, [&](int64_t j, auto L) { acc[0] += V.template won_<decltype(L)::value>(j) != 0.0 ? 1 : 0; });
      exact_totals<1>(acc, S, C);
      if (S.tot[0] == 0 && S.tot[1] == 0)
        stat = 1;  // src/Bidder.py:206-211: revert to Gaussian shading, nothing trained
      else
        ep0 = fit_winrate(V, K, S, C, fit_hyper(kFitWr, AG_BIDDER_VALUE_LEARNING), adam_tab, tr);
    }
    if (!lead) return;
    if (tid == 0) {
      epochs_out[3 * a] = ep0;
      status[a] = stat;
    }
    if (tid < 4) wr_ws[(size_t)a * 4 + tid] = S.wr[tid];
  } else {
    const FitNoise F{noise ? noise + noise_off[a] : nullptr, n, noise_seed, (uint32_t)a,
                     noise ? noise_epochs : 1 << 30};
    int ep1 = 0, ep2 = 0;
    int stat = 0;
    if (bk == AG_BIDDER_DOUBLY_ROBUST) {
      estimated_utilities(R, K.c0, K.nb, S.wr, eu_ws + s0, S.tab, lf + kFEu * cap, cap);
      __syncthreads();
      if (!initialised[a]) ep1 = fit_imitation(V, K, S, C, adam_tab, tr ? tr + kDrEpochs : nullptr);
      ep2 = fit_dr(V, K, S, C, F, adam_tab, tr ? tr + 2 * kDrEpochs : nullptr);
      stat = S.stop ? -2 : 0;
    } else if (bk == AG_BIDDER_VALUE_LEARNING) {
      if (bmode[a] == AG_VL_POLICY) ep2 = fit_dm(V, K, S, C, F, adam_tab, tr ? tr + 2 * kDrEpochs : nullptr);
    } else {  // PolicyLearningBidder
      if (!initialised[a]) ep1 = fit_imitation(V, K, S, C, adam_tab, tr ? tr + kDrEpochs : nullptr);
      ep2 = fit_pl(V, K, S, C, bmode[a], adam_tab, tr ? tr + 2 * kDrEpochs : nullptr);
      stat = S.stop ? -2 : 0;
    }
    __syncthreads();
    if (S.exhausted) stat = -3;  // not applied: the caller supplies more noise epochs
    if (!lead) return;
    if (tid == 0) {
      epochs_out[3 * a + 1] = ep1;
      epochs_out[3 * a + 2] = ep2;
      status[a] = stat;
    }
    if (stat == -3) return;
    if (tid < 4) st[tid] = S.wr[tid];
    if (tid < 12) st[4 + tid] = S.pol[tid];
  }
}

// ---------------------------------------------------------------------------------------
// Resumable, record-parallel training (ag_bidder_rp_*): the exact-sum learners' fits --
// ValueLearningBidder (win count, win-rate fit, 'policy' fit) and DoublyRobustBidder (win-rate
// fit, estimated utilities, imitation, DR policy fit) -- as ONE LAUNCH PER EPOCH, the whole
// training state of a learner (FitSt) in HBM between launches. Launch k, every workgroup of
// every learner:
//   1. steps the learner's state with the summed partials of launch k - 1 (summed over this
//      rank's workgroups by launch k - 1's tree root, then over the ranks by the caller's
//      all-reduce of those int64 words): loss, Adam, scheduler, early stop and the move to the
//      next fit, exactly as the persistent fits do it -- every workgroup computes the same
//      step from the same integers;
//   2. adds its records' exact fixed-point terms of the next epoch at the new state;
//   3. sums them up the agent's combining tree without waiting (agent_reduce_nowait): the
//      root stores the rank's totals for launch k + 1 (or the caller's all-reduce).
// No workgroup waits for another: no co-residency, no device-wide barrier. The sums are
// integers, so a rank holding a shard of the records (its records' global indices keep the
// synthetic rsample draws) steps to the model one process fits on all of them, bit for bit --
// and that model is the persistent fits' (k_bidder_train), which the GPU tests check.
// A policy fit that runs out of host-drawn noise epochs (ag_bidder_rp_noise) waits, with its
// state kept, for the next window: the drop-in update draws the reference's torch noise
// window by window and never re-runs a fit.
struct FitSt {
  int32_t fit, epoch, status, have_tot, need_noise, pad0;
  int32_t ep[3], pad1;
  double lr;
  Plateau pl;
  Stopper sp;
  float wr[4], pol[12];
  AdamState adam;
};

// the learner's state on entering `fit` (the persistent fits' initialisations)
__device__ __forceinline__ void fit_enter(FitSt &st, int fit, int bk) {
  st.fit = fit;
  st.epoch = 0;
  for (int j = 0; j < 16; ++j) st.adam.ea[j] = st.adam.es[j] = st.adam.mx[j] = 0.0f;
  if (fit != kFitWr && fit != kFitInit && fit != kFitPol) return;
  const FitHyper H = fit_hyper(fit, bk);
  st.lr = H.lr;
  if (fit != kFitInit) st.pl = plateau_of(H);  // (the imitation has no scheduler)
  st.sp = stopper_of(H);
}

// the fit after `st.fit` ended (the reference's order, src/Bidder.py:229-325, :500-615)
__device__ __forceinline__ void fit_after(FitSt &st, int bk, int mode, int init) {
  int nxt = kFitDone;
  switch (st.fit) {
    case kFitWins: nxt = kFitWr; break;
    case kFitWr: nxt = bk == AG_BIDDER_DOUBLY_ROBUST ? kFitEu : (mode == AG_VL_POLICY ? kFitPol : kFitDone); break;
    case kFitEu: nxt = init ? kFitPol : kFitInit; break;
    case kFitInit: nxt = kFitPol; break;
    default: nxt = kFitDone;
  }
  fit_enter(st, nxt, bk);
}

__device__ __forceinline__ int fit_max_epochs(int fit, int bk) { return fit_hyper(fit, bk).max_epochs; }

// step 1 (thread 0 with threads 0..15 for Adam): the learner's state after the epoch whose
// summed partials are tot (hi, lo pairs); n: the learner's records over all ranks
__device__ __forceinline__ void fit_step(FitSt &st, const int64_t *tot, double n, int bk, int mode, int init, const double *adam_tab,
                         float *s_grad, float *s_loss, int *s_np, float *tr, const double *bcp = nullptr) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    *s_np = 0;
    if (st.fit == kFitWins) {
      if (tot[0] == 0 && tot[1] == 0) {  // no wins: revert to Gaussian shading (src/Bidder.py:206-211)
        st.status = 1;
        fit_enter(st, kFitDone, bk);
      } else {
        fit_after(st, bk, mode, init);
      }
    } else if (st.fit == kFitWr) {
      const double M = 2.0 * n;
      *s_loss = (float)(fxv(tot[0], tot[1]) / M);
      for (int j = 0; j < 4; ++j) s_grad[j] = (float)(fxv(tot[2 + 2 * j], tot[3 + 2 * j]) / M);
      *s_np = 4;
    } else {  // imitation / policy fits: 12 parameters
      *s_loss = st.fit == kFitInit ? (float)(fxv(tot[24], tot[25]) / n + fxv(tot[26], tot[27]) / n)
                                   : (float)(fxv(tot[24], tot[25]) / n);
      for (int j = 0; j < 12; ++j) s_grad[j] = (float)(fxv(tot[2 * j], tot[2 * j + 1]) / n);
      *s_np = 12;
    }
  }
  __syncthreads();
  const int np = *s_np;
  if (np == 0) return;
  // Adam: thread j steps parameter j (adam_step_block's arithmetic)
  const int e = st.epoch;
  const float wd = fit_hyper(st.fit, bk).wd;
  double bc1;
  float bc2f;
  if (bcp) {  // adam_tab[e], adam_tab[kDrEpochs + e] fetched by the caller
    bc1 = bcp[0];
    bc2f = (float)bcp[1];
  } else {
    bias_corrections(e, adam_tab, bc2f, bc1);
  }
  const float neg_step = (float)(-(st.lr / bc1));
  float *par = st.fit == kFitWr ? st.wr : st.pol;
  __syncthreads();
  if (tid < np) {
    float p = par[tid];
    adam_param(p, s_grad[tid], tid, st.adam, neg_step, bc2f, wd);
    par[tid] = p;
  }
  __syncthreads();
  if (tid == 0) {
    const float loss = *s_loss;
    if (tr) tr[e] = loss;
    if (st.fit != kFitInit) plateau_step(st.pl, loss, st.lr);
    const bool stop = stop_step(st.sp, e, loss);
    const bool nan = loss != loss && st.fit == kFitPol && bk == AG_BIDDER_DOUBLY_ROBUST;
    st.epoch = e + 1;
    if (stop || nan || st.epoch >= fit_max_epochs(st.fit, bk)) {
      st.ep[fit_slot(st.fit)] = st.epoch;
      if (nan) {
        st.status = -2;  // the reference exits (src/Bidder.py:592-600)
        fit_enter(st, kFitDone, bk);
      } else {
        fit_after(st, bk, mode, init);
      }
    }
  }
  __syncthreads();
}

// step 2: this workgroup's exact terms of the learner's current epoch (st.fit at st.epoch,
// the models in st) over its nb records V -> S.tot; returns the words to sum (fit_words). PH:
// the fits of phase 0 (win count, win-rate) or 1 (imitation, the DR / DM policy fit). i0: the
// rsample index of local record 0 -- its global index over all ranks, so a rank holding a
// shard keeps the draws of the one-process fit. A view with cap = 0 reads every record from
// the store. (k_bidder_epoch and k_bidder_pipe; the persistent fits loop over the same terms.)
template <int PH>
__device__ __forceinline__ int epoch_partial(const FitSt &st, const RecView &V, int64_t nb, int bk, const FitNoise &F,
                                             int64_t i0, TrainLds &S) {
  const int tid = threadIdx.x;
  const int64_t nrec = nb > tid ? (nb - tid + kDrThreads - 1) / kDrThreads : 0;
  if constexpr (PH == 0) {
    if (st.fit == kFitWins) {
      int64_t acc[1] = {0};
      each_record(V, nb, [&](int64_t j, auto L) { acc[0] += V.template won_<decltype(L)::value>(j) != 0.0 ? 1 : 0; });
      block_sums<1>(acc, S.w, S.tot);
      return fit_words(kFitWins);
    }
    int64_t acc[5] = {0, 0, 0, 0, 0};
    const double w0 = (double)st.wr[0], w1 = (double)st.wr[1], w2 = (double)st.wr[2], w3 = (double)st.wr[3];
    each_record(V, nb, [&](int64_t j, auto L) {
      constexpr bool l = decltype(L)::value;
      const double c = V.template ctr_<l>(j), v = V.template val_<l>(j);
      wr_pair(acc, c, v, V.template gam_<l>(j), V.template won_<l>(j), w0, w1, w2, w3, S.tab);
    });
    wr_unbias(acc, nrec);
    block_sums<5>(acc, S.w, S.tot);
    return fit_words(kFitWr);
  } else {
    int64_t acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
    const int e = st.epoch;
    if (st.fit == kFitInit) {
      each_record(V, nb, [&](int64_t j, auto L) {
        constexpr bool l = decltype(L)::value;
        imit_rec(acc, st.pol, V.template ctr_<l>(j), V.template val_<l>(j), V.template gam_<l>(j), S.tab);
      });
#pragma unroll
      for (int q = 0; q < 14; ++q) fx_unbias(acc[q], nrec);
    } else if (bk == AG_BIDDER_DOUBLY_ROBUST) {
      each_record(V, nb, [&](int64_t j, auto L) {
        constexpr bool l = decltype(L)::value;
        dr_rec(acc, st.pol, st.wr, V.template ctr_<l>(j), V.template val_<l>(j), V.template gam_<l>(j),
               V.template prop_<l>(j), V.template util_<l>(j) - V.template eut_<l>(j), fit_eps(F, e, i0 + j), S.tab);
      });
#pragma unroll
      for (int q = 0; q < 13; ++q) fx_unbias(acc[q], nrec);
    } else {
      each_record(V, nb, [&](int64_t j, auto L) {
        constexpr bool l = decltype(L)::value;
        dm_rec(acc, st.pol, st.wr, V.template ctr_<l>(j), V.template val_<l>(j), fit_eps(F, e, i0 + j), S.tab);
      });
#pragma unroll
      for (int q = 0; q < 13; ++q) fx_unbias(acc[q], nrec);
    }
    block_sums<16>(acc, S.w, S.tot);
    return fit_words(kFitPol);
  }
}

__global__ __launch_bounds__(kDrThreads) void k_bidder_epoch(
    const int32_t *__restrict__ bkind, const int32_t *__restrict__ bmode, const int32_t *__restrict__ initialised,
    const int32_t *__restrict__ blk_agent, const int32_t *__restrict__ blk_rank,
    const int32_t *__restrict__ agent_nblk, const int64_t *__restrict__ offsets, const int64_t *__restrict__ n_total,
    const int64_t *__restrict__ g_base, DrRecords R0, double *__restrict__ eu_ws, const FitSt *__restrict__ st_in,
    FitSt *__restrict__ st_out, const int64_t *__restrict__ tot_in, int64_t *__restrict__ tot_out,
    int64_t *__restrict__ acc_rows, unsigned *__restrict__ bars, const int32_t *__restrict__ bar_off,
    const float *__restrict__ noise, int64_t noise_n, int32_t noise_e0, int32_t noise_epochs, uint64_t noise_seed,
    const double *__restrict__ adam_tab, float *__restrict__ traces) {
  const int a = blk_agent[blockIdx.x], rank = blk_rank[blockIdx.x], nblk = agent_nblk[a];
  const int tid = threadIdx.x;
  const int bk = bkind[a], mode = bmode[a], init = initialised[a];
  __shared__ TrainLds S;
  __shared__ FitSt st;
  __shared__ float s_grad[16], s_loss;
  __shared__ int s_np;
  for (int i = tid; i < 256; i += kDrThreads) S.tab[i] = ag_exp_tab[i];
  if (tid == 0) st = st_in[a];
  __syncthreads();
  const double n = (double)n_total[a];
  if (st.fit != kFitDone && st.have_tot) {
    float *tr =
        (traces && g_base[a] == 0 && rank == 0 && st.fit >= kFitWr) ? trace_row(traces, a, st.fit) : nullptr;
    fit_step(st, tot_in + (size_t)a * 32, n, bk, mode, init, adam_tab, s_grad, &s_loss, &s_np, tr);
  }
  const int64_t s0 = offsets[a];
  const Chunk K = wg_slice(offsets[a + 1] - s0, nblk, rank);
  // this workgroup's records (a slice of the agent's) as local records 0 .. nb - 1
  const int64_t r0 = s0 + K.c0;
  const DrRecords R{R0.ctr + r0, R0.value + r0, R0.gamma + r0, R0.prop + r0, R0.util + r0, R0.won + r0};
  if (st.fit == kFitEu) {
    estimated_utilities(R, 0, K.nb, st.wr, eu_ws + r0, S.tab);
    __syncthreads();
    if (tid == 0) fit_after(st, bk, mode, init);
    __syncthreads();
  }
  const bool noisy = st.fit == kFitPol;  // the DR / DM policy fits draw an rsample per record per epoch
  if (tid == 0)
    st.need_noise = noisy && noise && (st.epoch < noise_e0 || st.epoch >= noise_e0 + noise_epochs) ? 1 : 0;
  __syncthreads();
  const bool active = st.fit != kFitDone && !st.need_noise;
  if (active) {
    const FitNoise F{noise ? noise - (int64_t)noise_e0 * noise_n : nullptr, noise_n, noise_seed, (uint32_t)a,
                     1 << 30};
    const RecView V{R, eu_ws + r0, 0, nullptr, nullptr, 0};  // no record cache: every field from the store
    const int64_t i0 = g_base[a] + K.c0;  // the global index, over all ranks, of this slice's record 0
    const int W = st.fit == kFitWins || st.fit == kFitWr ? epoch_partial<0>(st, V, K.nb, bk, F, i0, S)
                                                         : epoch_partial<1>(st, V, K.nb, bk, F, i0, S);
    // the agent's region: accumulator rows [bar_lines(nblk)][32], barrier lines
    agcoop::agent_reduce_nowait(bars + (size_t)bar_off[a] * agcoop::kBarLineWords,
                                acc_rows + (size_t)bar_off[a] * 32, 32, rank, nblk, S.tot, W,
                                tot_out + (size_t)a * 32, &S.flag);
  }
  if (rank == 0 && tid == 0) {
    st.have_tot = active ? 1 : 0;
    st_out[a] = st;
  }
}

// ---------------------------------------------------------------------------------------
// Pipelined persistent training (ag_bidder_rp_run; ag_bidder_update's exact-sum learners):
// the FitSt state machine of k_bidder_epoch inside ONE cooperative launch per phase, every
// workgroup holding a contiguous slice of EVERY learner's records (slot i: learner
// agents[i]). A round visits the learners in turn: finish learner i's last epoch sum (its
// combining tree, agent_allreduce_finish), step its state (fit_step: loss, Adam, scheduler,
// early stop, next fit -- every workgroup the same integers, so the same step), add this
// workgroup's exact terms of its next epoch and start that sum up the tree
// (agent_allreduce_start) -- then the next learner. A learner's sum climbs the tree while the
// workgroups compute the OTHER learners' epochs, so the cross-workgroup latency that one
// learner per launch (k_bidder_train) or per epoch (k_bidder_epoch) waits out is hidden
// behind useful work. Integer sums: the same models, epochs and status bit for bit as both.
//   PH = 0: the win count and the win-rate fit (4 workgroups per CU, <= 128 VGPRs);
//   PH = 1: estimated utilities, imitation, the policy fits (3 per CU).
// A policy fit whose host-drawn noise window ends waits with its state kept (need_noise);
// the launch ends when no learner has an epoch left in its phase.
constexpr int kPipeMaxAgents = 16;
constexpr int kPipeFanIn = 32;  // the trees' fan-in: 2 levels up to 1024 workgroups
struct PipeArgs {
  int NA;                       // learners in the launch (<= kPipeMaxAgents)
  const int32_t *agents;        // [NA] their agent indices
  const int32_t *bkind, *bmode, *initialised;
  const int64_t *offsets;       // [N + 1] sorted records
  const int64_t *n_total;       // [N] the learners' record counts (fit_step's n)
  DrRecords R0;
  double *eu_ws;
  FitSt *st;                    // [N] in / out
  const int64_t *tot_in;        // [N][32] totals pending from ag_bidder_rp_epoch (have_tot)
  int64_t *acc;                 // [NA][lines][32] combining-tree rows
  unsigned *bars;               // [NA][lines][kBarLineWords]
  int lines;
  const int32_t *lds_off;       // [NA] record-cache byte offsets (dynamic LDS, after the FitSt copies)
  const int32_t *lds_cap;       // [NA] records cached per workgroup
  const float *noise;           // host-drawn draws or NULL (synthetic)
  const int64_t *noise_off;     // [N] per-learner offsets (NULL: 0)
  int64_t noise_stride;         // floats per epoch (0: the learner's record count)
  int32_t noise_e0, noise_epochs;
  uint64_t noise_seed;
  const double *adam_tab;
  float *traces;                // [N][3][kDrEpochs] or NULL
  long long *prof;              // diagnostics (AG_PIPE_PROF): [G][8] wall-clock ticks per part, or NULL
};

template <int PH>
__device__ __forceinline__ bool pipe_in_phase(int fit) {
  return PH == 0 ? (fit == kFitWins || fit == kFitWr) : (fit == kFitEu || fit == kFitInit || fit == kFitPol);
}

// a slot's constants, read once into LDS (the rounds read nothing from global memory but the
// records beyond the cache and the Adam table)
struct PipeSlot {
  int64_t s0, c0, nb, cap;  // the learner's first sorted record; this workgroup's slice; cached records
  double n;                 // records (fit_step's n)
  uint32_t off;             // record cache: byte offset in the dynamic LDS (not a pointer: kept
                            // an LDS address, ds_read, not a flat load through a generic pointer)
  int a, bk, mode, init, nf;
};

template <int PH>
__global__ __launch_bounds__(kDrThreads, PH == 0 ? 4 : AG_DR_PH1_MIN_WAVES) void k_bidder_pipe(PipeArgs A) {
  __shared__ TrainLds S;
  __shared__ float s_grad[16], s_loss;
  __shared__ int s_np;
  __shared__ unsigned s_gen[kPipeMaxAgents];
  __shared__ PipeSlot s_slot[kPipeMaxAgents];
  __shared__ double s_bc[kPipeMaxAgents][2];  // the Adam bias corrections of each slot's epoch in flight
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  FitSt *fst = reinterpret_cast<FitSt *>(s_dyn);
  const int tid = threadIdx.x, G = gridDim.x, rank = blockIdx.x, NA = A.NA;
  for (int i = tid; i < 256; i += kDrThreads) S.tab[i] = ag_exp_tab[i];
  for (int i = tid; i < NA; i += kDrThreads) {
    const int a = A.agents[i], bk = A.bkind[a];
    fst[i] = A.st[a];
    PipeSlot &P = s_slot[i];
    P.a = a;
    P.bk = bk;
    P.mode = A.bmode[a];
    P.init = A.initialised[a];
    P.n = (double)A.n_total[a];
    P.s0 = A.offsets[a];
    const Chunk K = wg_slice(A.offsets[a + 1] - P.s0, G, rank);
    P.c0 = K.c0;
    P.nb = K.nb;
    P.cap = A.lds_cap[i];
    P.off = (uint32_t)A.lds_off[i];
    P.nf = PH == 0 ? 3 : (bk == AG_BIDDER_DOUBLY_ROBUST ? 6 : 2);
  }
  __syncthreads();
  // stage every slot's cached records (this phase's fields)
  for (int i = 0; i < NA; ++i) {
    const PipeSlot &P = s_slot[i];
    const int64_t cap = P.cap, ns = P.nb < cap ? P.nb : cap;
    float *lf = reinterpret_cast<float *>(s_dyn + P.off);
    const bool dr = P.bk == AG_BIDDER_DOUBLY_ROBUST;
    uint8_t *lw = reinterpret_cast<uint8_t *>(lf + (size_t)P.nf * cap);
    const bool eu_ready = dr && fst[i].fit > kFitEu && fst[i].fit != kFitDone;
    for (int64_t j = tid; j < ns; j += kDrThreads) {
      const int64_t r = P.s0 + P.c0 + j;
      lf[kFCtr * cap + j] = (float)A.R0.ctr[r];
      lf[kFVal * cap + j] = (float)A.R0.value[r];
      if (PH == 0 || dr) lf[kFGam * cap + j] = (float)A.R0.gamma[r];
      if (PH == 0) lw[j] = A.R0.won[r];
      if (PH == 1 && dr) {
        lf[kFProp * cap + j] = (float)A.R0.prop[r];
        lf[kFUtil * cap + j] = (float)A.R0.util[r];
        if (eu_ready) lf[kFEu * cap + j] = (float)A.eu_ws[r];
      }
    }
  }
  __syncthreads();
  // AG_PIPE_PROF: finish, step, partial, start, total, finishes (thread 0's; LDS, not registers)
  __shared__ long long pr[8];
  if (tid < 8) pr[tid] = 0;
  auto view = [&](const PipeSlot &P) -> RecView {
    const int64_t s0 = P.s0;
    const DrRecords R{A.R0.ctr + s0, A.R0.value + s0, A.R0.gamma + s0, A.R0.prop + s0, A.R0.util + s0, A.R0.won + s0};
    const float *lf = reinterpret_cast<const float *>(s_dyn + P.off);
    return RecView{R, A.eu_ws + s0, P.c0, lf, reinterpret_cast<const uint8_t *>(lf + (size_t)P.nf * P.cap), P.cap};
  };
  auto tr_of = [&](int a, const FitSt &st) -> float * {
    return (A.traces && rank == 0 && st.fit >= kFitWr) ? trace_row(A.traces, a, st.fit) : nullptr;
  };
  auto step = [&](int i, const int64_t *tot, bool prefetched) {
    const PipeSlot &P = s_slot[i];
    fit_step(fst[i], tot, P.n, P.bk, P.mode, P.init, A.adam_tab, s_grad, &s_loss, &s_np, tr_of(P.a, fst[i]),
             prefetched ? s_bc[i] : nullptr);
  };
  // the next epoch of slot i: estimated utilities when its fit reaches them, then its partial
  // sums started up its tree; false when it has no epoch left in this phase (or waits for noise)
  auto begin = [&](int i, bool &root) -> bool {
    FitSt &st = fst[i];
    const PipeSlot &P = s_slot[i];
    const int a = P.a, bk = P.bk;
    const int64_t nb = P.nb;
    const RecView V = view(P);
    if (PH == 1 && st.fit == kFitEu) {
      float *lfe = reinterpret_cast<float *>(s_dyn + P.off) + (size_t)kFEu * V.cap;
      estimated_utilities(V.R, V.c0, nb, st.wr, A.eu_ws + P.s0, S.tab, lfe, V.cap);
      __syncthreads();
      if (tid == 0) fit_after(st, bk, P.mode, P.init);
      __syncthreads();
    }
    if (!pipe_in_phase<PH>(st.fit) || st.fit == kFitEu) return false;
    const bool wait = PH == 1 && st.fit == kFitPol && A.noise &&
                      (st.epoch < A.noise_e0 || st.epoch >= A.noise_e0 + A.noise_epochs);
    __syncthreads();
    if (tid == 0) st.need_noise = wait ? 1 : 0;
    __syncthreads();
    if (wait) return false;
    // this epoch's Adam bias corrections, loaded now and stored after the partial sums (the
    // load's latency hidden behind them); fit_step reads them from LDS
    const int e = st.epoch;
    double b1 = 0.0, b2 = 0.0;
    if (tid == 0 && st.fit != kFitWins) {
      b1 = A.adam_tab[e];
      b2 = A.adam_tab[kDrEpochs + e];
    }
    const int64_t stride = A.noise_stride ? A.noise_stride : (int64_t)P.n;
    const FitNoise F{A.noise ? A.noise + (A.noise_off ? A.noise_off[a] : 0) - (int64_t)A.noise_e0 * stride : nullptr,
                     stride, A.noise_seed, (uint32_t)a, 1 << 30};
    long long tp = A.prof && tid == 0 ? wall_clock64() : 0;
    const int W = epoch_partial<PH>(st, V, nb, bk, F, V.c0, S);
    if (tid == 0) {
      s_bc[i][0] = b1;
      s_bc[i][1] = b2;
    }
    if (A.prof) {
      __syncthreads();
      if (tid == 0) {
        const long long tq = wall_clock64();
        pr[2] += tq - tp;
        tp = tq;
      }
    }
    root = agcoop::agent_allreduce_start<kPipeFanIn>(A.bars + (size_t)i * A.lines * kBarLineWords, A.acc + (size_t)i * A.lines * 32,
                                         32, rank, G, S.tot, W, &s_gen[i], &S.flag);
    if (A.prof && tid == 0) pr[3] += wall_clock64() - tp;
    return true;
  };
  // totals left by ag_bidder_rp_epoch launches
  for (int i = 0; i < NA; ++i)
    if (fst[i].have_tot && fst[i].fit != kFitDone) step(i, A.tot_in + (size_t)s_slot[i].a * 32, false);
  uint32_t pend = 0, roots = 0;
  const long long t_start = A.prof ? wall_clock64() : 0;
  for (int i = 0; i < NA; ++i) {
    bool root = false;
    if (begin(i, root)) pend |= 1u << i;
    if (root) roots |= 1u << i;
  }
  while (pend) {
    for (int i = 0; i < NA; ++i) {
      if (!(pend >> i & 1)) continue;
      const int W = fit_words(fst[i].fit);
      long long tf = A.prof && tid == 0 ? wall_clock64() : 0;
      agcoop::agent_allreduce_finish(A.bars + (size_t)i * A.lines * kBarLineWords, A.acc + (size_t)i * A.lines * 32, G,
                                     roots >> i & 1, &s_gen[i], W, S.tot);
      if (A.prof && tid == 0) {
        const long long tg = wall_clock64();
        pr[0] += tg - tf;
        tf = tg;
        pr[5] += 1;
      }
      step(i, S.tot, true);
      if (A.prof) {
        __syncthreads();
        if (tid == 0) pr[1] += wall_clock64() - tf;
      }
      bool root = false;
      pend &= ~(1u << i);
      roots &= ~(1u << i);
      if (begin(i, root)) pend |= 1u << i;
      if (root) roots |= 1u << i;
    }
  }
  __syncthreads();
  if (A.prof && tid == 0) {
    pr[4] = wall_clock64() - t_start;
    for (int k = 0; k < 8; ++k) A.prof[(size_t)rank * 8 + k] = pr[k];
  }
  if (rank == 0)
    for (int i = tid; i < NA; i += kDrThreads) {
      FitSt f = fst[i];
      f.have_tot = 0;
      A.st[s_slot[i].a] = f;
    }
}

// the learners' FitSt at the start of a resumable update (state16: win-rate model, policy)
__global__ void k_rp_init(int N, const int32_t *__restrict__ bkind, const int32_t *__restrict__ bmode,
                          const int32_t *__restrict__ mask, const float *__restrict__ state, FitSt *__restrict__ st,
                          int parities) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  FitSt f;
  memset(&f, 0, sizeof f);
  for (int j = 0; j < 4; ++j) f.wr[j] = state[(size_t)a * 16 + j];
  for (int j = 0; j < 12; ++j) f.pol[j] = state[(size_t)a * 16 + 4 + j];
  const int bk = bkind[a];
  fit_enter(f, !mask[a] ? kFitDone : (bk == AG_BIDDER_DOUBLY_ROBUST ? kFitWr : kFitWins), bk);
  st[a] = f;
  if (parities == 2) st[N + a] = f;  // [2][N] states: parity 1 too -- the epoch launches never
                                     // write unmasked agents' rows
}

__global__ __launch_bounds__(kDrThreads) void k_sh_hist(const int32_t *__restrict__ agent, int64_t n, int N,
                                                        int64_t *__restrict__ counts) {
  extern __shared__ unsigned int s_hist[];
  for (int a = threadIdx.x; a < N; a += kDrThreads) s_hist[a] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDrThreads)
    atomicAdd(&s_hist[agent[i]], 1u);
  __syncthreads();
  for (int a = threadIdx.x; a < N; a += kDrThreads)
    if (s_hist[a]) atomicAdd((unsigned long long *)&counts[a], (unsigned long long)s_hist[a]);
}

// records in (agent, log order): two stable radix sorts, by the whole 64-bit order, then by
// agent; then every field gathered
__global__ __launch_bounds__(kDrThreads) void k_sh_keys(ag_shading_samples s, int64_t n, uint64_t *__restrict__ key,
                                                        uint32_t *__restrict__ idx) {
  for (int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDrThreads) {
    key[i] = s.order[i];
    idx[i] = (uint32_t)i;
  }
}

// the agents of the records idx (in log order): the second sort's keys
__global__ __launch_bounds__(kDrThreads) void k_sh_agent_keys(const int32_t *__restrict__ agent, int64_t n,
                                                              const uint32_t *__restrict__ idx,
                                                              uint32_t *__restrict__ key) {
  for (int64_t j = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kDrThreads)
    key[j] = (uint32_t)agent[idx[j]];
}

__global__ __launch_bounds__(kDrThreads) void k_sh_gather(ag_shading_samples s, int64_t n,
                                                          const uint32_t *__restrict__ idx,
                                                          double *__restrict__ o_ctr, double *__restrict__ o_val,
                                                          double *__restrict__ o_gam, double *__restrict__ o_prop,
                                                          double *__restrict__ o_util, uint8_t *__restrict__ o_won) {
  for (int64_t j = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kDrThreads) {
    const uint32_t i = idx[j];
    o_ctr[j] = s.ctr[i];
    o_val[j] = s.value[i];
    o_gam[j] = s.gamma[i];
    o_prop[j] = s.propensity[i];
    o_util[j] = s.utility[i];
    o_won[j] = s.won[i];
  }
}

int grid_over(int64_t n) { return agtrain::grid_over(n, kDrThreads); }

DrRecords records_of(const agtrain::SortedRecs &S) { return DrRecords{S.ctr, S.val, S.gam, S.prop, S.util, S.won}; }

}  // namespace

using agtrain::BlockTables;
using agtrain::Carve;
using agtrain::SortedRecs;

void ag_dr_release(ag_ctx *c) {
  ag_dr_ws &w = c->dr;
  (void)hipFree(w.buf);
  (void)hipFree(w.counts);
  (void)hipFree(w.adam_tab);
  (void)hipFree(w.state);
  (void)hipFree(w.init);
  (void)hipFree(w.mode);
  (void)hipFree(w.scratch);
  (void)hipFree(w.coop);
  (void)hipFree(w.rp.st);
  (void)hipFree(w.rp.acc);
  (void)hipFree(w.rp.tables);
  (void)hipFree(w.rp.pipe);
  (void)hipFree(w.rp.pipe_st);
  w = ag_dr_ws();
}

// k_bidder_pipe's record-cache budgets (dynamic LDS per workgroup: 4 / 3 per CU) and the
// records per workgroup it aims at (AG_PIPE_RECS overrides, for tuning): fewer workgroups for
// small learners -- a shorter tree to climb each epoch -- and the whole resident grid for
// large ones
constexpr size_t kPipeLds[2] = {32 * 1024, 44 * 1024};
constexpr int64_t kPipeRecs = 512;

struct PipeNoise {
  const float *noise = nullptr;
  const int64_t *noise_off = nullptr;
  int64_t stride = 0;
  int32_t e0 = 0, epochs = 0;
};

// Runs the learners `slots` (agent indices; FitSt in d_st) through k_bidder_pipe's phases
// `phases` (bit p: phase p), one cooperative launch each.
static int pipe_run(ag_ctx *c, const std::vector<int32_t> &slots, const std::vector<int64_t> &cnt, const DrRecords &R,
                    double *eu, const int64_t *d_off, const int64_t *d_ntot, FitSt *d_st, const int64_t *tot_in,
                    const PipeNoise &nz, float *traces, int phases, hipStream_t st) {
  ag_dr_ws &w = c->dr;
  ag_dr_rp &rp = w.rp;
  const int NA = (int)slots.size();
  if (NA == 0) return AG_OK;
  if (NA > kPipeMaxAgents) return ag_set_error(AG_ERR_UNSUPPORTED, "k_bidder_pipe: > %d learners", kPipeMaxAgents);
  int64_t recs = 0;
  for (int a : slots) recs += cnt[a];
  int64_t want_recs = kPipeRecs;
  if (const char *e = getenv("AG_PIPE_RECS")) want_recs = std::max<int64_t>(1, atoll(e));
  for (int ph = 0; ph < 2; ++ph)
    if (!rp.pipe_blocks[ph]) {
      const void *fn = ph == 0 ? (const void *)k_bidder_pipe<0> : (const void *)k_bidder_pipe<1>;
      AG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPipeLds[ph]));
      AG_HIP(agtrain::resident_blocks(fn, kDrThreads, kPipeLds[ph], c->device, &rp.pipe_blocks[ph]));
    }
  // device tables, sized once for the largest grid (every slot's rows [lines][32]), 64 bytes
  // between the phases'
  const size_t lines_max = (size_t)std::max(1, bar_lines(std::max(rp.pipe_blocks[0], rp.pipe_blocks[1]), kPipeFanIn));
  const size_t per_ph = agtrain::layout_bytes(agtrain::pipe_layout, kPipeMaxAgents, kPipeMaxAgents * lines_max * 32) + 64;
  AG_HIP(agtrain::dev_reserve(&rp.pipe, &rp.pipe_bytes, 2 * per_ph));
  for (int ph = 0; ph < 2; ++ph) {
    if (!(phases >> ph & 1)) continue;
    const auto fn = ph == 0 ? k_bidder_pipe<0> : k_bidder_pipe<1>;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(rp.pipe_blocks[ph], (recs + want_recs - 1) / want_recs));
    const int lines = std::max(1, bar_lines(G, kPipeFanIn));
    // record caches after the FitSt copies: slot i caches min(chunk, share) records
    const size_t fst_bytes = ((size_t)NA * sizeof(FitSt) + 15) / 16 * 16;
    const size_t budget = kPipeLds[ph] - fst_bytes;
    std::vector<int64_t> chunk(NA), bytes(NA);
    double total = 0.0;
    for (int i = 0; i < NA; ++i) {
      const int bk = c->h_bkind[slots[i]];
      chunk[i] = (cnt[slots[i]] + G - 1) / G;
      bytes[i] = ph == 0 ? 13 : (bk == AG_BIDDER_DOUBLY_ROBUST ? 24 : 8);
      total += (double)(chunk[i] * bytes[i] + 16);
    }
    const double f = total > (double)budget ? (double)budget / total : 1.0;
    std::vector<int32_t> tab(3 * kPipeMaxAgents, 0);
    size_t off = fst_bytes;
    for (int i = 0; i < NA; ++i) {
      const int64_t cap = std::min<int64_t>(chunk[i], (int64_t)((double)chunk[i] * f));
      tab[i] = slots[i];
      tab[kPipeMaxAgents + i] = (int32_t)off;
      tab[2 * kPipeMaxAgents + i] = (int32_t)cap;
      off += ((size_t)cap * bytes[i] + 15) / 16 * 16;
    }
    if (off > kPipeLds[ph])
      return ag_set_error(AG_ERR_UNSUPPORTED, "k_bidder_pipe: record cache plan %zu > %zu", off, kPipeLds[ph]);
    const size_t rows = (size_t)NA * lines * 32;
    Carve carve((char *)rp.pipe + ph * per_ph);
    const agtrain::PipeTables D = agtrain::pipe_layout(carve, kPipeMaxAgents, rows);
    AG_HIP(hipMemcpyAsync(D.tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, st));
    AG_HIP(hipMemsetAsync(D.acc, 0, rows * (sizeof(int64_t) + sizeof(unsigned)), st));
    PipeArgs A;
    A.NA = NA;
    A.agents = D.tab;
    A.bkind = c->d_bkind;
    A.bmode = w.mode;
    A.initialised = w.init;
    A.offsets = d_off;
    A.n_total = d_ntot;
    A.R0 = R;
    A.eu_ws = eu;
    A.st = d_st;
    A.tot_in = tot_in;
    A.acc = D.acc;
    A.bars = D.bar;
    A.lines = lines;
    A.lds_off = D.tab + kPipeMaxAgents;
    A.lds_cap = D.tab + 2 * kPipeMaxAgents;
    A.noise = nz.noise;
    A.noise_off = nz.noise_off;
    A.noise_stride = nz.stride;
    A.noise_e0 = nz.e0;
    A.noise_epochs = nz.epochs;
    A.noise_seed = c->fit_noise_seed;
    A.adam_tab = w.adam_tab;
    A.traces = traces;
    A.prof = nullptr;
    const bool prof = getenv("AG_PIPE_PROF") != nullptr;
    if (prof) AG_HIP(hipMalloc(&A.prof, sizeof(long long) * 8 * G));
    AG_HIP(agtrain::launch_group(fn, true, G, kDrThreads, kPipeLds[ph], st, A));
    if (prof) {  // diagnostics: mean over workgroups of each part, microseconds (100 MHz clock)
      std::vector<long long> h(8 * (size_t)G);
      AG_HIP(hipMemcpy(h.data(), A.prof, sizeof(long long) * 8 * G, hipMemcpyDeviceToHost));
      (void)hipFree(A.prof);
      double m[8] = {0};
      for (int b = 0; b < G; ++b)
        for (int k = 0; k < 8; ++k) m[k] += (double)h[8 * (size_t)b + k] / G;
      fprintf(stderr, "k_bidder_pipe<%d> G=%d NA=%d: finish-wait %.0f us, step %.0f us, partial %.0f us, start %.0f "
              "us, total %.0f us, finishes %.0f\n", ph, G, NA, m[0] / 100, m[1] / 100, m[2] / 100, m[3] / 100,
              m[4] / 100, m[5]);
    }
  }
  return AG_OK;
}

// FitSt [N] then a mask [N] for ag_bidder_update's pipe run (its own buffer: pipe_run may
// reallocate the tables)
static FitSt *pipe_fitst(ag_ctx *c) {
  ag_dr_rp &rp = c->dr.rp;
  const size_t N = (size_t)c->shape.num_agents;
  if (!rp.pipe_st && hipMalloc(&rp.pipe_st, (sizeof(FitSt) + sizeof(int32_t)) * N) != hipSuccess) return nullptr;
  return (FitSt *)rp.pipe_st;
}

// which agents bid from a fitted policy / a win-rate search (ag_simulate checks its inputs)
static void learner_flags(ag_ctx *c, const int32_t *init) {
  c->dr_any_init = c->vl_any_search = false;
  for (int a = 0; a < c->shape.num_agents; ++a) {
    const int bk = c->h_bkind ? c->h_bkind[a] : -1;
    const bool learner = bk == AG_BIDDER_VALUE_LEARNING || bk == AG_BIDDER_POLICY_LEARNING || bk == AG_BIDDER_DOUBLY_ROBUST;
    if (learner && init[a] == AG_LEARNER_POLICY) c->dr_any_init = true;
    if (bk == AG_BIDDER_VALUE_LEARNING && init[a] == AG_LEARNER_SEARCH) c->vl_any_search = true;
  }
}

// The host's end of learner a's fit. f: its FitSt (k_bidder_pipe, the per-epoch launches), whose
// epochs and status go out and whose models go into the agent's `state` row unless the
// ValueLearningBidder's no-win fallback trained nothing (status 1, src/Bidder.py:206-211); null
// after k_bidder_train, which wrote all three itself. A fit that waits for noise epochs past the
// caller's (status -3) is not applied. Otherwise the agent bids from what it fitted from now on
// (src/Bidder.py:321, :430, :612-613): the policy, the win-rate search (ValueLearningBidder
// 'search'), or the Gaussian again after the fallback. Returns rc or, the first time, the
// reference's error for an update without logs (-1) or a NaN loss (-2).
static int apply_fit(const ag_ctx *c, int a, const FitSt *f, int mode, float *state, int32_t *init, int32_t *ep,
                     int32_t *status, int rc) {
  static const char *names[] = {"", "", "ValueLearningBidder", "PolicyLearningBidder", "DoublyRobustBidder"};
  const int bk = c->h_bkind[a];
  if (f) {
    for (int j = 0; j < 3; ++j) ep[j] = f->ep[j];
    *status = f->status;
    if (f->fit != kFitDone) {
      *status = -3;
      ep[2] = f->epoch;
    } else if (f->status != 1) {
      for (int j = 0; j < 4; ++j) state[j] = f->wr[j];
      for (int j = 0; j < 12; ++j) state[4 + j] = f->pol[j];
    }
  }
  if (*status == -3) return rc;
  if (*status == -1 && rc == AG_OK)
    rc = ag_set_error(AG_ERR_INVALID, "agent %d: %s.update without logs", a, names[bk]);
  if (*status == -2 && rc == AG_OK)
    rc = ag_set_error(AG_ERR_INVALID, "agent %d: %s: NAN DETECTED! in losses (src/Bidder.py:%d)", a, names[bk],
                      bk == AG_BIDDER_DOUBLY_ROBUST ? 592 : 409);
  if (bk == AG_BIDDER_VALUE_LEARNING)
    *init = *status == 1 ? AG_LEARNER_UNINITIALISED : (mode == AG_VL_POLICY ? AG_LEARNER_POLICY : AG_LEARNER_SEARCH);
  else
    *init = AG_LEARNER_POLICY;
  return rc;
}

// workspace: counts / offsets / cursors, the Adam bias-correction table, the learner state
static int dr_ws_ready(ag_ctx *c) {
  ag_dr_ws &w = c->dr;
  if (w.adam_tab) return AG_OK;
  const int N = c->shape.num_agents;
  const std::vector<double> tab = agtrain::adam_bias_table(kDrEpochs);
  hipError_t e = hipMalloc(&w.adam_tab, sizeof(double) * tab.size());
  if (e == hipSuccess) e = hipMemcpy(w.adam_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&w.counts, sizeof(int64_t) * (3 * (size_t)N + 1));
  if (e == hipSuccess) e = hipMalloc(&w.state, sizeof(float) * 16 * (size_t)N);
  if (e == hipSuccess) e = hipMemset(w.state, 0, sizeof(float) * 16 * (size_t)N);
  if (e == hipSuccess) e = hipMalloc(&w.init, sizeof(int32_t) * (size_t)N);
  if (e == hipSuccess) e = hipMemset(w.init, 0, sizeof(int32_t) * (size_t)N);
  if (e == hipSuccess) e = hipMalloc(&w.mode, sizeof(int32_t) * (size_t)N);
  if (e == hipSuccess) {  // defaults: ValueLearningBidder 'search', PolicyLearningBidder 'PPO'
    std::vector<int32_t> m(N, AG_VL_SEARCH);
    for (int a = 0; a < N; ++a)
      if (c->h_bkind && c->h_bkind[a] == AG_BIDDER_POLICY_LEARNING) m[a] = AG_PL_LOSS_PPO;
    e = hipMemcpy(w.mode, m.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc(&w.scratch, sizeof(int64_t) * (size_t)N + sizeof(int32_t) * 5 * (size_t)N);
  if (e != hipSuccess) {
    ag_dr_release(c);
    return ag_set_error(AG_ERR_HIP, "DR workspace: %s", hipGetErrorString(e));
  }
  return AG_OK;
}

// The learning bidders' records of a store sorted into (agent, log order) in the workspace
// (stable radix sorts on the 64-bit order, then on agent; every field gathered): cnt / off host
// [N] / [N + 1]; out: device arrays [n] and d_off [N + 1].
static int sort_records(ag_ctx *c, const ag_shading_samples *s, std::vector<int64_t> &cnt, std::vector<int64_t> &off,
                        SortedRecs &out, hipStream_t st) {
  const int N = c->shape.num_agents;
  if (int rc = ag_shading_counts(c, s, cnt.data(), st)) return rc;
  int64_t n = 0;
  for (int a = 0; a < N; ++a) n += cnt[a];
  ag_dr_ws &w = c->dr;
  off.assign((size_t)N + 1, 0);
  for (int a = 0; a < N; ++a) off[a + 1] = off[a] + cnt[a];
  int64_t *d_off = w.counts + N;  // [N + 1] offsets
  AG_HIP(hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * ((size_t)N + 1), hipMemcpyHostToDevice, st));
  if (n >= ((int64_t)1 << 32)) return ag_set_error(AG_ERR_UNSUPPORTED, "learning bidders' update: >= 2^32 records");
  // radix-sort workspace: keys in/out (8 B), indices in/out (4 B), then hipcub's temp (the
  // larger of the two sorts')
  size_t sort_tmp = 0, agent_tmp = 0;
  AG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (uint64_t *)nullptr, (uint64_t *)nullptr,
                                            (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(n > 0 ? n : 1), 0, 64,
                                            st));
  AG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, agent_tmp, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                            (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(n > 0 ? n : 1), 0, 32,
                                            st));
  if (agent_tmp > sort_tmp) sort_tmp = agent_tmp;
  const size_t cap = (size_t)(n > 0 ? n : 1);
  const size_t need = agtrain::layout_bytes(agtrain::sorted_layout, cap, sort_tmp);
  AG_HIP(agtrain::dev_reserve(&w.buf, &w.buf_bytes, need, need + (need >> 2)));
  Carve carve(w.buf);
  out = agtrain::sorted_layout(carve, cap, sort_tmp);
  out.d_off = d_off;
  out.n = n;
  uint64_t *k_in = out.k_in, *k_out = out.k_out;
  uint32_t *i_in = out.i_in, *i_out = out.i_out;
  void *tmp = out.tmp;
  if (n > 0) {
    if (!s->order) return ag_set_error(AG_ERR_INVALID, "learning bidders' update: the store needs order");
    hipLaunchKernelGGL(k_sh_keys, dim3(grid_over(n)), dim3(kDrThreads), 0, st, *s, n, k_in, i_in);
    AG_HIP(hipGetLastError());
    AG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, sort_tmp, k_in, k_out, i_in, i_out, (int)n, 0, 64, st));
    // i_out: the records by order. Stably by agent (the order keys' space now holds the agent keys)
    uint32_t *a_in = (uint32_t *)k_in, *a_out = a_in + cap;
    hipLaunchKernelGGL(k_sh_agent_keys, dim3(grid_over(n)), dim3(kDrThreads), 0, st, s->agent, n, i_out, a_in);
    AG_HIP(hipGetLastError());
    int agent_bits = 1;
    while ((1ll << agent_bits) < N) ++agent_bits;
    AG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, agent_tmp, a_in, a_out, i_out, i_in, (int)n, 0, agent_bits, st));
    hipLaunchKernelGGL(k_sh_gather, dim3(grid_over(n)), dim3(kDrThreads), 0, st, *s, n, i_in, out.ctr, out.val,
                       out.gam, out.prop, out.util, out.won);
    AG_HIP(hipGetLastError());
  }
  return AG_OK;
}

// One phase's launch of k_bidder_train (ag_bidder_update) for the learners `trained`: the
// workgroups per learner and the record cache. Workgroups per learning bidder, co-resident (cooperative launch) when an agent has
// several; capped to the resident grid (occupancy with the phase's largest record cache).
// With AG_OPT_BIDDER_BLOCK_SAMPLES set: one per that many records. By default the
// exact-sum learners (ValueLearning, DoublyRobust: results independent of the split)
// share the resident grid in proportion to their records, >= kMinChunk records per
// workgroup; a PolicyLearningBidder (fixed-order float sums: its result follows the split)
// keeps one workgroup per kBidderChunk records. Both phases use the same rule with their
// own grid.
struct TrainPlan {
  decltype(&k_bidder_train<0>) fn = nullptr;
  BlockTables T;
  int nf = 0;
  int64_t rcap = 0;
  size_t dyn = 0;
};
static int train_plan(ag_ctx *c, int ph, const std::vector<int64_t> &cnt, const std::vector<char> &trained,
                      TrainPlan &P) {
  ag_dr_ws &w = c->dr;
  const int N = c->shape.num_agents;
  P.fn = ph == 0 ? k_bidder_train<0> : k_bidder_train<1>;
  const size_t lds_budget = ph == 0 ? kRecLdsBytes0 : kRecLdsBytes;
  int &coop_blocks = ph == 0 ? w.coop_blocks0 : w.coop_blocks;
  AG_HIP(agtrain::resident_blocks((const void *)P.fn, kDrThreads, lds_budget, c->device, &coop_blocks));
  std::vector<int32_t> &nblk = P.T.nblk;
  nblk.assign(N, 0);
  int64_t exact_recs = 0, fixed_blocks = 0;
  int nf = 0;  // float fields of the record cache: 3 (win-rate, ValueLearning), 5 (PolicyLearning), 6 (DR)
  for (int a = 0; a < N; ++a) {
    const int bk = c->h_bkind[a];
    if (!trained[a] || (ph == 0 && bk == AG_BIDDER_POLICY_LEARNING)) continue;
    nf = std::max(nf, ph == 0 ? 3 : (bk == AG_BIDDER_DOUBLY_ROBUST ? 6 : (bk == AG_BIDDER_POLICY_LEARNING ? 5 : 3)));
    if (c->bidder_chunk > 0 || bk == AG_BIDDER_POLICY_LEARNING) {
      const int64_t chunk = c->bidder_chunk > 0 ? c->bidder_chunk : kBidderChunk;
      nblk[a] = cnt[a] > 0 ? (int32_t)((cnt[a] + chunk - 1) / chunk) : 1;
      fixed_blocks += nblk[a];
    } else {
      exact_recs += cnt[a];
      nblk[a] = -1;
    }
  }
  for (int a = 0; a < N; ++a)
    if (nblk[a] < 0) {
      const int64_t avail = std::max<int64_t>(1, coop_blocks - fixed_blocks);
      const int64_t share = exact_recs > 0 ? (int64_t)((double)avail * (double)cnt[a] / (double)exact_recs) : 1;
      nblk[a] = (int32_t)std::max<int64_t>(1, std::min<int64_t>((cnt[a] + kMinChunk - 1) / kMinChunk, share));
    }
  agtrain::share_out(nblk, coop_blocks);
  agtrain::block_tables(P.T, [](int nb) { return bar_lines(nb); });
  int64_t most = 0;  // records of the largest workgroup chunk
  for (int a = 0; a < N; ++a)
    if (nblk[a]) most = std::max<int64_t>(most, (cnt[a] + nblk[a] - 1) / nblk[a]);
  // record cache: [nf][cap] floats + [cap] bytes, cap a multiple of the block size
  const int64_t rcap_fit = nf ? (int64_t)lds_budget / (4 * nf + 1) / kDrThreads * kDrThreads : 0;
  P.rcap = std::min<int64_t>(rcap_fit, (most + kDrThreads - 1) / kDrThreads * kDrThreads);
  if (c->bidder_cache >= 0) P.rcap = std::min<int64_t>(P.rcap, c->bidder_cache / kDrThreads * kDrThreads);
  P.nf = nf;
  P.dyn = ((size_t)P.rcap * (4 * nf + 1) + 15) / 16 * 16;
  return AG_OK;
}

// One launch of a plan: its tables into D (ag_bidder_update's, shared by the two launches)
static int train_launch(ag_ctx *c, const TrainPlan &P, const agtrain::TrainTables &D, const SortedRecs &SR,
                        const float *noise, const int64_t *d_noff, int32_t noise_epochs, int32_t *d_epochs,
                        int32_t *d_stat, float *traces, hipStream_t st) {
  const int G = P.T.G(), N = c->shape.num_agents;
  if (G == 0) return AG_OK;
  ag_dr_ws &w = c->dr;
  AG_HIP(hipMemcpyAsync(D.bagent, P.T.blk_agent.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(D.brank, P.T.blk_rank.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(D.nblk, P.T.nblk.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(D.baroff, P.T.bar_off.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  if (P.T.lines) AG_HIP(hipMemsetAsync(D.bar, 0, sizeof(unsigned) * kBarLineWords * P.T.lines, st));
  if (P.T.multi()) AG_HIP(hipMemsetAsync(D.part, 0, sizeof(int64_t) * 96 * (size_t)G, st));  // accumulators
  AG_HIP(agtrain::launch_group(P.fn, P.T.multi(), G, kDrThreads, P.dyn, st, c->d_bkind, w.mode, D.bagent, D.brank,
                               D.nblk, SR.d_off, records_of(SR), SR.eu, w.state, D.wr, w.init, noise, d_noff,
                               noise_epochs, c->fit_noise_seed, w.adam_tab, d_epochs, d_stat, traces, D.part, D.bar,
                               D.baroff, P.nf, P.rcap));
  return AG_OK;
}

extern "C" {

int ag_set_dr_state(ag_ctx *c, const float *state, const int32_t *initialised) {
  if (!c || !state || !initialised) return ag_set_error(AG_ERR_INVALID, "ag_set_dr_state: null argument");
  AgDeviceGuard g(c->device);
  if (int rc = dr_ws_ready(c)) return rc;
  const int N = c->shape.num_agents;
  AG_HIP(hipMemcpy(c->dr.state, state, sizeof(float) * 16 * N, hipMemcpyHostToDevice));
  AG_HIP(hipMemcpy(c->dr.init, initialised, sizeof(int32_t) * N, hipMemcpyHostToDevice));
  c->dr_loaded = true;
  learner_flags(c, initialised);
  return AG_OK;
}

int ag_get_dr_state(ag_ctx *c, float *state, int32_t *initialised) {
  if (!c) return ag_set_error(AG_ERR_INVALID, "ag_get_dr_state: null ctx");
  AgDeviceGuard g(c->device);
  if (int rc = dr_ws_ready(c)) return rc;
  const int N = c->shape.num_agents;
  AG_HIP(hipDeviceSynchronize());
  if (state) AG_HIP(hipMemcpy(state, c->dr.state, sizeof(float) * 16 * N, hipMemcpyDeviceToHost));
  if (initialised) AG_HIP(hipMemcpy(initialised, c->dr.init, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  return AG_OK;
}

int ag_shading_counts(ag_ctx *c, const ag_shading_samples *s, int64_t *counts, void *stream) {
  if (!c || !s || !counts) return ag_set_error(AG_ERR_INVALID, "ag_shading_counts: null argument");
  AG_CHECK_STRUCT(s, "ag_shading_counts", "ag_shading_samples");
  AgDeviceGuard g(c->device);
  if (int rc = dr_ws_ready(c)) return rc;
  const int N = c->shape.num_agents;
  hipStream_t st = (hipStream_t)stream;
  uint64_t n = 0;
  if (int rc = agtrain::read_store_count(s->count, s->capacity, "ag_shading_counts", "records", st, &n)) return rc;
  int64_t *d_counts = c->dr.counts;
  AG_HIP(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * N, st));
  if (n > 0) {
    if ((size_t)N * 4 > 64 * 1024) return ag_set_error(AG_ERR_UNSUPPORTED, "ag_shading_counts: N > 16384");
    hipLaunchKernelGGL(k_sh_hist, dim3(grid_over((int64_t)n)), dim3(kDrThreads), (size_t)N * 4, st, s->agent,
                       (int64_t)n, N, d_counts);
    AG_HIP(hipGetLastError());
  }
  AG_HIP(hipMemcpyAsync(counts, d_counts, sizeof(int64_t) * N, hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  return AG_OK;
}

int ag_bidder_update(ag_ctx *c, const ag_shading_samples *s, const int32_t *agents, const float *noise,
                     const int64_t *noise_offsets, int32_t noise_epochs, int32_t *epochs, int32_t *status,
                     float *traces, void *stream) {
  if (!c || !s || !noise_offsets) return ag_set_error(AG_ERR_INVALID, "ag_bidder_update: null argument");
  AG_CHECK_STRUCT(s, "ag_bidder_update", "ag_shading_samples");
  if (!s->ctr || !s->value || !s->propensity || !s->won || !s->order)
    return ag_set_error(AG_ERR_INVALID, "ag_bidder_update: the store needs ctr, value, propensity, won, order");
  if (!c->dr_loaded) return ag_set_error(AG_ERR_STATE, "ag_bidder_update: ag_set_dr_state not called");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents;
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> cnt(N), off;
  SortedRecs SR;
  if (int rc = sort_records(c, s, cnt, off, SR, st)) return rc;
  ag_dr_ws &w = c->dr;
  int64_t *d_noff = w.scratch;                       // [N] noise offsets
  int32_t *d_epochs = (int32_t *)(w.scratch + N);     // [N][3] epochs, then [N] status
  int32_t *d_stat = d_epochs + 3 * (size_t)N;
  AG_HIP(hipMemcpyAsync(d_noff, noise_offsets, sizeof(int64_t) * N, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemsetAsync(d_epochs, 0, sizeof(int32_t) * 4 * N, st));
  // k_bidder_train, one group of workgroups per learner, by default: measured on the bench's
  // populations (profiles/r04j_*), the pipelined launches (k_bidder_pipe, every learner in
  // every workgroup) lose -- each round pays one epoch's serial step and tree climb per
  // learner on 1/A of the work, 1.4-3.4x the time. AG_BIDDER_PIPE=1 takes the pipe for the
  // exact-sum learners (A/B); ag_bidder_rp_run (one learner of the drop-in update at a time,
  // where the alternative is a launch per epoch) always does.
  std::vector<int32_t> pipe_slots, pipe_mask(N, 0);
  {
    const char *e = getenv("AG_BIDDER_PIPE");
    const bool off = !(e && e[0] == '1') || c->bidder_chunk > 0;
    for (int a = 0; a < N && !off; ++a) {
      const int bk = c->h_bkind[a];
      // (a learner without logs takes k_bidder_train's no-logs path: fallback or error)
      if ((bk == AG_BIDDER_VALUE_LEARNING || bk == AG_BIDDER_DOUBLY_ROBUST) && !(agents && !agents[a]) && cnt[a] > 0)
        pipe_slots.push_back(a);
    }
    if ((int)pipe_slots.size() > kPipeMaxAgents) pipe_slots.clear();
    for (int a : pipe_slots) pipe_mask[a] = 1;
  }
  std::vector<char> trained(N, 0);  // k_bidder_train's learners: every learner in `agents` the pipe does not take
  for (int a = 0; a < N; ++a) {
    const int bk = c->h_bkind[a];
    trained[a] = (bk == AG_BIDDER_VALUE_LEARNING || bk == AG_BIDDER_POLICY_LEARNING || bk == AG_BIDDER_DOUBLY_ROBUST) &&
                 !(agents && !agents[a]) && !pipe_mask[a];
  }
  TrainPlan P0, P1;
  if (int rc = train_plan(c, 0, cnt, trained, P0)) return rc;
  if (int rc = train_plan(c, 1, cnt, trained, P1)) return rc;
  const size_t gmax = (size_t)std::max(P0.T.G(), P1.T.G()), lmax = (size_t)std::max(P0.T.lines, P1.T.lines);
  AG_HIP(agtrain::dev_reserve(&w.coop, &w.coop_bytes, agtrain::layout_bytes(agtrain::train_layout, N, gmax, lmax) + 64));
  Carve carve(w.coop);
  const agtrain::TrainTables D = agtrain::train_layout(carve, N, gmax, lmax);
  FitSt *pst = nullptr;
  if (!pipe_slots.empty()) {
    pst = pipe_fitst(c);
    if (!pst) return ag_set_error(AG_ERR_HIP, "ag_bidder_update: FitSt allocation failed");
    int32_t *d_pmask = (int32_t *)(pst + N);
    AG_HIP(hipMemcpyAsync(d_pmask, pipe_mask.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rp_init, dim3((N + 255) / 256), dim3(256), 0, st, N, c->d_bkind, w.mode, d_pmask, w.state,
                       pst, 1);
    AG_HIP(hipGetLastError());
    // n_total = the counts (w.counts [N]); noise: agent a's draws of epoch e at noise_offsets[a] + e n_a
    PipeNoise nz;
    nz.noise = noise;
    nz.noise_off = d_noff;
    nz.stride = 0;
    nz.e0 = 0;
    nz.epochs = noise_epochs;
    if (int rc = pipe_run(c, pipe_slots, cnt, records_of(SR), SR.eu, SR.d_off, w.counts, pst, nullptr, nz, traces, 3, st))
      return rc;
  }
  for (const TrainPlan *P : {&P0, &P1})
    if (int rc = train_launch(c, *P, D, SR, noise, d_noff, noise_epochs, d_epochs, d_stat, traces, st)) return rc;
  std::vector<int32_t> h(4 * (size_t)N);
  AG_HIP(hipMemcpyAsync(h.data(), d_epochs, sizeof(int32_t) * 4 * N, hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  // k_bidder_train wrote its learners' epochs, status and models; the pipe's are in their FitSt
  std::vector<FitSt> fs(pst ? N : 0);
  std::vector<float> state(16 * (size_t)N);
  std::vector<int32_t> init(N), mode(N);
  if (pst) {
    AG_HIP(hipMemcpy(fs.data(), pst, sizeof(FitSt) * N, hipMemcpyDeviceToHost));
    AG_HIP(hipMemcpy(state.data(), w.state, sizeof(float) * 16 * N, hipMemcpyDeviceToHost));
  }
  AG_HIP(hipMemcpy(init.data(), w.init, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  AG_HIP(hipMemcpy(mode.data(), w.mode, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  int rc = AG_OK;
  for (int a = 0; a < N; ++a)
    if (trained[a] || pipe_mask[a])
      rc = apply_fit(c, a, pipe_mask[a] ? &fs[a] : nullptr, mode[a], &state[16 * (size_t)a], &init[a], &h[3 * (size_t)a],
                     &h[3 * (size_t)N + a], rc);
  if (pst) AG_HIP(hipMemcpy(w.state, state.data(), sizeof(float) * 16 * N, hipMemcpyHostToDevice));
  if (epochs) memcpy(epochs, h.data(), sizeof(int32_t) * 3 * N);
  if (status) memcpy(status, h.data() + 3 * (size_t)N, sizeof(int32_t) * N);
  if (rc) return rc;  // (the learner flags stay as they were)
  AG_HIP(hipMemcpy(w.init, init.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
  learner_flags(c, init.data());
  return AG_OK;
}

int ag_dr_update(ag_ctx *c, const ag_shading_samples *s, const float *noise, const int64_t *noise_offsets,
                 int32_t noise_epochs, int32_t *epochs, float *traces, void *stream) {
  std::vector<int32_t> stat(c->shape.num_agents);
  if (int rc = ag_bidder_update(c, s, nullptr, noise, noise_offsets, noise_epochs, epochs, stat.data(), traces, stream))
    return rc;
  for (int a = 0; a < c->shape.num_agents; ++a)
    if (stat[a] == -3)
      return ag_set_error(AG_ERR_INVALID, "agent %d: the DR fit needs more than %d noise epochs", a, noise_epochs);
  return AG_OK;
}

// ---- resumable / record-parallel training (k_bidder_epoch) ----
int ag_bidder_rp_begin(ag_ctx *c, const ag_shading_samples *s, const int32_t *agents, const int64_t *records_total,
                       const int64_t *records_base, int64_t *totals, void *stream) {
  if (!c || !s || !totals) return ag_set_error(AG_ERR_INVALID, "ag_bidder_rp_begin: null argument");
  AG_CHECK_STRUCT(s, "ag_bidder_rp_begin", "ag_shading_samples");
  if (!s->ctr || !s->value || !s->propensity || !s->won || !s->order)
    return ag_set_error(AG_ERR_INVALID, "ag_bidder_rp_begin: the store needs ctr, value, propensity, won, order");
  if (!c->dr_loaded) return ag_set_error(AG_ERR_STATE, "ag_bidder_rp_begin: ag_set_dr_state not called");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents;
  hipStream_t st = (hipStream_t)stream;
  ag_dr_ws &w = c->dr;
  ag_dr_rp &rp = w.rp;
  std::vector<int32_t> mask(N, 0);
  for (int a = 0; a < N; ++a) {
    const int bk = c->h_bkind ? c->h_bkind[a] : -1;
    if (agents && !agents[a]) continue;
    if (bk == AG_BIDDER_DOUBLY_ROBUST || bk == AG_BIDDER_VALUE_LEARNING) mask[a] = 1;
    else if (bk == AG_BIDDER_POLICY_LEARNING && agents)
      return ag_set_error(AG_ERR_UNSUPPORTED, "ag_bidder_rp_begin: agent %d: PolicyLearningBidder fits use "
                          "fixed-order float sums (their result follows the record split): ag_bidder_update", a);
  }
  std::vector<int64_t> cnt(N), off;
  SortedRecs SR;
  if (int rc = sort_records(c, s, cnt, off, SR, st)) return rc;
  // workgroups: one per kRpChunk of an agent's records on this rank, at least one per trained
  // agent (a rank without records of it still steps its state and adds zeros)
  constexpr int64_t kRpChunk = 2048;
  BlockTables T;
  T.nblk.assign(N, 0);
  for (int a = 0; a < N; ++a)
    if (mask[a]) T.nblk[a] = (int32_t)std::max<int64_t>(1, (cnt[a] + kRpChunk - 1) / kRpChunk);
  agtrain::block_tables(T, [](int nb) { return std::max(1, agcoop::bar_lines(nb)); });
  const int lines = T.lines, G = T.G();
  // (room for 64 more workgroups and 16 more lines before the buffers grow again)
  AG_HIP(agtrain::dev_reserve(&rp.st, &rp.st_bytes, sizeof(FitSt) * 2 * (size_t)N));
  AG_HIP(agtrain::dev_reserve(&rp.acc, &rp.acc_bytes, agtrain::layout_bytes(agtrain::rp_acc_layout, lines, 32),
                              agtrain::layout_bytes(agtrain::rp_acc_layout, lines + 16, 32)));
  AG_HIP(agtrain::dev_reserve(&rp.tables, &rp.tables_bytes, agtrain::layout_bytes(agtrain::rp_tables_layout, N, G, 2 * N),
                              agtrain::layout_bytes(agtrain::rp_tables_layout, N, G + 64, 2 * N)));
  Carve carve_acc(rp.acc), carve_tables(rp.tables);
  rp.A = agtrain::rp_acc_layout(carve_acc, lines, 32);
  rp.T = agtrain::rp_tables_layout(carve_tables, N, G, 2 * N);
  AG_HIP(hipMemcpyAsync(rp.T.bagent, T.blk_agent.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(rp.T.brank, T.blk_rank.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(rp.T.nblk, T.nblk.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(rp.T.baroff, T.bar_off.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  AG_HIP(hipMemcpyAsync(rp.T.mask, mask.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
  std::vector<int64_t> nt(2 * (size_t)N);
  for (int a = 0; a < N; ++a) {
    nt[a] = records_total ? records_total[a] : cnt[a];
    nt[N + a] = records_base ? records_base[a] : 0;
    if (mask[a] && nt[a] < 1)
      return ag_set_error(AG_ERR_INVALID, "agent %d: %s.update without logs", a,
                          c->h_bkind[a] == AG_BIDDER_DOUBLY_ROBUST ? "DoublyRobustBidder" : "ValueLearningBidder");
    if (nt[N + a] < 0 || nt[N + a] + cnt[a] > nt[a])
      return ag_set_error(AG_ERR_INVALID, "ag_bidder_rp_begin: agent %d: records_base %lld + %lld local records "
                          "> records_total %lld", a, (long long)nt[N + a], (long long)cnt[a], (long long)nt[a]);
  }
  AG_HIP(hipMemcpyAsync(rp.T.ntot, nt.data(), sizeof(int64_t) * 2 * N, hipMemcpyHostToDevice, st));
  if (lines) AG_HIP(hipMemsetAsync(rp.acc, 0, carve_acc.bytes(), st));
  AG_HIP(hipMemsetAsync(totals, 0, sizeof(int64_t) * 2 * 32 * (size_t)N, st));
  hipLaunchKernelGGL(k_rp_init, dim3((N + 255) / 256), dim3(256), 0, st, N, c->d_bkind, w.mode, rp.T.mask, w.state,
                     (FitSt *)rp.st, 2);
  AG_HIP(hipGetLastError());
  if (int rc = dr_ws_ready(c)) return rc;  // the Adam table
  rp.G = G;
  rp.lines = lines;
  rp.k = 0;
  rp.totals = totals;
  rp.noise = nullptr;
  rp.noise_n = 0;
  rp.noise_e0 = rp.noise_epochs = 0;
  rp.recs = SR;
  rp.single = true;
  for (int a = 0; a < N; ++a)
    if (mask[a] && (nt[a] != cnt[a] || nt[N + a] != 0)) rp.single = false;
  rp.active = true;
  return AG_OK;
}

// The rest of a one-rank resumable update in persistent launches (k_bidder_pipe): every
// learner under training runs until it is done or waits for the next noise window
// (ag_bidder_rp_noise) -- ag_bidder_rp_poll tells which; ag_bidder_rp_end applies the result.
// The launches read and write the same FitSt as ag_bidder_rp_epoch (which it may follow or
// precede), so the two mix freely.
int ag_bidder_rp_run(ag_ctx *c, float *traces, void *stream) {
  if (!c || !c->dr.rp.active) return ag_set_error(AG_ERR_STATE, "ag_bidder_rp_run: no ag_bidder_rp_begin");
  ag_dr_ws &w = c->dr;
  ag_dr_rp &rp = w.rp;
  if (!rp.single)
    return ag_set_error(AG_ERR_UNSUPPORTED, "ag_bidder_rp_run: this rank holds part of the learners' records "
                        "(records_total / records_base): the ranks' sums meet per epoch, ag_bidder_rp_epoch");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents;
  hipStream_t st = (hipStream_t)stream;
  std::vector<int32_t> mask(N);
  std::vector<int64_t> cnt(N + 1);
  std::vector<FitSt> h(N);
  FitSt *S = (FitSt *)rp.st + (size_t)(rp.k & 1) * N;
  AG_HIP(hipMemcpyAsync(mask.data(), rp.T.mask, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
  AG_HIP(hipMemcpyAsync(cnt.data(), w.counts + N, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, st));
  AG_HIP(hipMemcpyAsync(h.data(), S, sizeof(FitSt) * N, hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  std::vector<int32_t> slots;
  std::vector<int64_t> n(N, 0);
  bool ph0 = false;
  for (int a = 0; a < N; ++a) {
    n[a] = cnt[a + 1] - cnt[a];
    if (mask[a] && h[a].fit != kFitDone) {
      slots.push_back(a);
      ph0 |= h[a].fit == kFitWins || h[a].fit == kFitWr;
    }
  }
  if (slots.empty()) return AG_OK;
  if ((int)slots.size() > kPipeMaxAgents) {  // per-epoch launches, polled, until done or waiting
    std::vector<int32_t> fit(N), ep(N), need(N);
    for (;;) {
      if (int rc = ag_bidder_rp_epoch(c, 64, nullptr, traces, stream)) return rc;
      if (int rc = ag_bidder_rp_poll(c, fit.data(), ep.data(), need.data(), stream)) return rc;
      bool busy = false;
      for (int a = 0; a < N; ++a) busy |= mask[a] && fit[a] >= 0 && need[a] < 0;
      if (!busy) return AG_OK;
    }
  }
  PipeNoise nz;
  nz.noise = rp.noise;
  nz.stride = rp.noise_n;
  nz.e0 = rp.noise_e0;
  nz.epochs = rp.noise_epochs;
  return pipe_run(c, slots, n, records_of(rp.recs), rp.recs.eu, rp.recs.d_off, rp.T.ntot, S, rp.totals + (size_t)((rp.k + 1) & 1) * 32 * N, nz,
                  traces, ph0 ? 3 : 2, st);
}

int ag_bidder_rp_noise(ag_ctx *c, const float *noise, int64_t noise_n, int32_t first_epoch, int32_t epochs) {
  if (!c || !c->dr.rp.active) return ag_set_error(AG_ERR_STATE, "ag_bidder_rp_noise: no ag_bidder_rp_begin");
  if (noise && (noise_n < 1 || first_epoch < 0 || epochs < 0))
    return ag_set_error(AG_ERR_INVALID, "ag_bidder_rp_noise: bad window");
  ag_dr_rp &rp = c->dr.rp;
  rp.noise = noise;
  rp.noise_n = noise_n;
  rp.noise_e0 = first_epoch;
  rp.noise_epochs = epochs;
  return AG_OK;
}

int ag_bidder_rp_epoch(ag_ctx *c, int32_t launches, int64_t *launch_index, float *traces, void *stream) {
  if (!c || !c->dr.rp.active) return ag_set_error(AG_ERR_STATE, "ag_bidder_rp_epoch: no ag_bidder_rp_begin");
  if (launches < 0) return ag_set_error(AG_ERR_INVALID, "ag_bidder_rp_epoch: launches < 0");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents;
  hipStream_t st = (hipStream_t)stream;
  ag_dr_ws &w = c->dr;
  ag_dr_rp &rp = w.rp;
  const DrRecords R = records_of(rp.recs);
  FitSt *S = (FitSt *)rp.st;
  for (int32_t l = 0; l < launches; ++l) {
    const int64_t k = rp.k;
    if (rp.G > 0)
      hipLaunchKernelGGL(k_bidder_epoch, dim3(rp.G), dim3(kDrThreads), 0, st, c->d_bkind, w.mode, w.init, rp.T.bagent,
                         rp.T.brank, rp.T.nblk, rp.recs.d_off, rp.T.ntot, rp.T.ntot + N, R, rp.recs.eu, S + (size_t)(k & 1) * N,
                         S + (size_t)((k + 1) & 1) * N, rp.totals + (size_t)((k + 1) & 1) * 32 * N,
                         rp.totals + (size_t)(k & 1) * 32 * N, rp.A.acc, rp.A.bar, rp.T.baroff, rp.noise, rp.noise_n,
                         rp.noise_e0, rp.noise_epochs, c->fit_noise_seed, w.adam_tab, traces);
    AG_HIP(hipGetLastError());
    rp.k = k + 1;
  }
  if (launch_index) *launch_index = rp.k - 1;  // the last launch: its totals are at totals + 32 N (index & 1)
  return AG_OK;
}

int ag_bidder_rp_poll(ag_ctx *c, int32_t *fit, int32_t *epoch, int32_t *need_noise, void *stream) {
  if (!c || !c->dr.rp.active) return ag_set_error(AG_ERR_STATE, "ag_bidder_rp_poll: no ag_bidder_rp_begin");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents;
  ag_dr_rp &rp = c->dr.rp;
  std::vector<FitSt> h(N);
  hipStream_t st = (hipStream_t)stream;
  AG_HIP(hipMemcpyAsync(h.data(), (FitSt *)rp.st + (size_t)(rp.k & 1) * N, sizeof(FitSt) * N, hipMemcpyDeviceToHost,
                        st));
  AG_HIP(hipStreamSynchronize(st));
  for (int a = 0; a < N; ++a) {
    if (fit) fit[a] = h[a].fit == kFitDone ? -1 : h[a].fit;
    if (epoch) epoch[a] = h[a].epoch;
    if (need_noise) need_noise[a] = h[a].need_noise ? h[a].epoch : -1;
  }
  return AG_OK;
}

int ag_bidder_rp_end(ag_ctx *c, int32_t *epochs, int32_t *status, void *stream) {
  if (!c || !c->dr.rp.active) return ag_set_error(AG_ERR_STATE, "ag_bidder_rp_end: no ag_bidder_rp_begin");
  AgDeviceGuard g(c->device);
  const int N = c->shape.num_agents;
  ag_dr_ws &w = c->dr;
  ag_dr_rp &rp = w.rp;
  hipStream_t st = (hipStream_t)stream;
  std::vector<FitSt> h(N);
  std::vector<int32_t> mask(N), init(N), mode(N);
  std::vector<float> state(16 * (size_t)N);
  AG_HIP(hipMemcpyAsync(h.data(), (FitSt *)rp.st + (size_t)(rp.k & 1) * N, sizeof(FitSt) * N, hipMemcpyDeviceToHost,
                        st));
  AG_HIP(hipMemcpyAsync(mask.data(), rp.T.mask, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  rp.active = false;
  for (int a = 0; a < N; ++a)
    if (mask[a] && h[a].fit != kFitDone)
      return ag_set_error(AG_ERR_STATE, "ag_bidder_rp_end: agent %d is still training (fit %d, epoch %d)", a,
                          h[a].fit, h[a].epoch);
  AG_HIP(hipMemcpy(state.data(), w.state, sizeof(float) * 16 * N, hipMemcpyDeviceToHost));
  AG_HIP(hipMemcpy(init.data(), w.init, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  AG_HIP(hipMemcpy(mode.data(), w.mode, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  int rc = AG_OK;
  for (int a = 0; a < N; ++a) {
    int32_t ep[3] = {0, 0, 0}, stat = 0;
    if (mask[a]) rc = apply_fit(c, a, &h[a], mode[a], &state[16 * (size_t)a], &init[a], ep, &stat, rc);
    if (epochs) memcpy(epochs + 3 * a, ep, sizeof ep);
    if (status) status[a] = stat;
  }
  AG_HIP(hipMemcpy(w.state, state.data(), sizeof(float) * 16 * N, hipMemcpyHostToDevice));
  AG_HIP(hipMemcpy(w.init, init.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
  learner_flags(c, init.data());
  return rc;
}

int ag_set_bidder_modes(ag_ctx *c, const int32_t *modes) {
  if (!c || !modes) return ag_set_error(AG_ERR_INVALID, "ag_set_bidder_modes: null argument");
  AgDeviceGuard g(c->device);
  if (int rc = dr_ws_ready(c)) return rc;
  const int N = c->shape.num_agents;
  for (int a = 0; a < N; ++a) {
    const int bk = c->h_bkind ? c->h_bkind[a] : -1;
    if (bk == AG_BIDDER_VALUE_LEARNING && modes[a] != AG_VL_SEARCH && modes[a] != AG_VL_POLICY)
      return ag_set_error(AG_ERR_INVALID, "agent %d: ValueLearningBidder inference must be 'search' or 'policy'", a);
    if (bk == AG_BIDDER_POLICY_LEARNING && (modes[a] < AG_PL_LOSS_REINFORCE || modes[a] > AG_PL_LOSS_PPO))
      return ag_set_error(AG_ERR_UNSUPPORTED,
                          "agent %d: PolicyLearningBidder loss %d (REINFORCE, REINFORCE_offpolicy, TRPO, PPO are built)",
                          a, modes[a]);
  }
  AG_HIP(hipMemcpy(c->dr.mode, modes, sizeof(int32_t) * N, hipMemcpyHostToDevice));
  return AG_OK;
}

}  // extern "C"
