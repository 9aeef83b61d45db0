// ag_selftest.hip -- stress test of the learners' cross-workgroup exact sums (ag_coop.h), the
// hand-off every trainer relies on (k_lrts_train, k_bidder_train, the pipe, the per-epoch
// kernels): many cooperative workgroups -- spread over every XCD -- run generation after
// generation of interleaved combining-tree all-reduces of int64 words whose totals each
// workgroup also knows in closed form, and count every total that differs. A stale read (a
// node row or total seen before another XCD's addition, or a counter / generation observed
// out of order) shows up as a wrong total or a hang, so tests/test_gpu_coop.py runs it under a
// time limit on the built form (AG_COOP_FENCED 0 by default; the fenced form is the A/B build
// `make variant NAME=fenced VFLAGS=-DAG_COOP_FENCED=1`).
// Also ag_div_selftest (ag_div.h's split division against `a / b`) and ag_math_kat: the small
// functions every parity claim rests on, evaluated on caller-chosen inputs by the device build
// or by the host build of the same source.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ag_coop.h"
#include "ag_div.h"
#include "ag_host.h"
#include "ag_sim.h"
#include "ag_train_math.h"

namespace {

constexpr int kStThreads = 256;
constexpr int kStWords = 32;     // words per all-reduce (the pipe's row width)
constexpr int kStMaxRegions = 4;

// the word a workgroup contributes: any function of (generation, region, rank, word) that
// changes every generation
__device__ __forceinline__ int64_t st_val(uint32_t gen, int region, int rank, int j) {
  uint64_t x = ((uint64_t)gen << 40) ^ ((uint64_t)region << 32) ^ ((uint64_t)rank << 8) ^ (uint64_t)j;
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return (int64_t)x;
}

// Every workgroup is a member of every region (as in k_bidder_pipe, where each workgroup takes
// part in every learner's sum): generation g starts the regions' sums one after the other and
// then finishes them in the same order, so up to `regions` sums climb the trees at once.
__global__ __launch_bounds__(kStThreads) void k_coop_stress(unsigned *bars, int64_t *acc, int lines, int regions,
                                                            int gens, unsigned long long *bad) {
  __shared__ int64_t s_vals[kStMaxRegions][kStWords], s_tot[kStMaxRegions][kStWords], s_want[kStWords];
  __shared__ unsigned s_gen[kStMaxRegions];
  __shared__ int s_flag;
  __shared__ bool s_root[kStMaxRegions];
  const int t = threadIdx.x, rank = blockIdx.x, nblk = gridDim.x;
  unsigned long long nbad = 0;
  for (int g = 0; g < gens; ++g) {
    for (int r = 0; r < regions; ++r) {
      if (t < kStWords) s_vals[r][t] = st_val((uint32_t)g, r, rank, t);
      // (agent_allreduce_start's leading workgroup barrier publishes s_vals)
      const bool root = agcoop::agent_allreduce_start(bars + (size_t)r * lines * agcoop::kBarLineWords,
                                                      acc + (size_t)r * lines * kStWords, kStWords, rank, nblk,
                                                      s_vals[r], kStWords, &s_gen[r], &s_flag);
      if (t == 0) s_root[r] = root;
    }
    for (int r = 0; r < regions; ++r) {
      __syncthreads();
      agcoop::agent_allreduce_finish(bars + (size_t)r * lines * agcoop::kBarLineWords,
                                     acc + (size_t)r * lines * kStWords, nblk, s_root[r], &s_gen[r], kStWords,
                                     s_tot[r]);
      // the closed form: every rank's word summed mod 2^64 (the threads split the ranks)
      if (t < kStWords) s_want[t] = 0;
      __syncthreads();
      for (int j = 0; j < kStWords; ++j) {
        uint64_t part = 0;
        for (int q = t; q < nblk; q += kStThreads) part += (uint64_t)st_val((uint32_t)g, r, q, j);
        for (int o = 32; o > 0; o >>= 1) part += (uint64_t)__shfl_xor((long long)part, o, 64);
        if ((t & 63) == 0) atomicAdd((unsigned long long *)&s_want[j], (unsigned long long)part);
      }
      __syncthreads();
      if (t < kStWords && s_tot[r][t] != s_want[t]) ++nbad;
    }
  }
  if (nbad) atomicAdd(bad, nbad);
}

// ag_div.h's split division against the compiler's `a / b`, bit for bit, over operands in
// div_safe's range: per thread `iters` pairs of three kinds -- anywhere in the range; the BCE
// row's (1 or e) / (1 + e) and log1p's c / (1 + e) with e down to 2^-740; log1p's f / (2 + f)
__device__ __forceinline__ uint64_t st_mix(uint64_t x) {
  x ^= x >> 31;
  x *= 0x7fb5d329728ea185ull;
  x ^= x >> 27;
  x *= 0x81dadef4bc2dd44dull;
  x ^= x >> 33;
  return x;
}
__device__ __forceinline__ double st_num(uint64_t h, int lo, int hi) {  // +-(1 + m) 2^k, k in [lo, hi)
  const int k = lo + (int)((h >> 52) % (uint64_t)(hi - lo));
  const double m = __builtin_bit_cast(double, 0x3ff0000000000000ull | (h & 0x000fffffffffffffull));
  return __builtin_ldexp((h >> 63) ? -m : m, k);
}
__global__ __launch_bounds__(256) void k_div_stress(uint64_t seed, int iters, unsigned long long *bad,
                                                    unsigned long long *tested) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long nbad = 0, n = 0;
  for (int i = 0; i < iters; ++i) {
    const uint64_t h1 = st_mix(seed ^ (t * 0x9e3779b97f4a7c15ull) ^ ((uint64_t)i << 40) ^ 1),
                   h2 = st_mix(h1 ^ 0x2545f4914f6cdd1dull), h3 = st_mix(h2 + 7);
    double a, b;
    switch (i % 3) {
      case 0:
        a = st_num(h1, -900, 600);
        b = st_num(h2, -60, 60);
        break;
      case 1: {
        const double e = __builtin_fabs(st_num(h1, -740, 0));
        b = 1.0 + e;
        const int w = (int)(h3 % 3);
        a = w == 0 ? 1.0 : (w == 1 ? e : (e - (b - 1.0)));  // the last: log1p's c (may be +0)
        break;
      }
      default: {
        const double f = (double)(int64_t)(h1 >> 11) * 0x1p-53 * 0.71 - 0.29;  // [-0.29, 0.42)
        a = f;
        b = 2.0 + f;
        break;
      }
    }
    if (!agdiv::div_safe(a, b)) continue;
    ++n;
    const double want = a / b, got = agdiv::div_core(a, b, agdiv::recip(b));
    if (__builtin_bit_cast(uint64_t, want) != __builtin_bit_cast(uint64_t, got)) ++nbad;
  }
  if (nbad) atomicAdd(bad, nbad);
  atomicAdd(tested, n);
}

// ---------------------------------------------------------------------------------------
// ag_math_kat: function `fn` of include/auctiongym.h's table on element i. One source for the
// device kernel and the host loop; every function called is the kernels' own (ag_exp.h,
// ag_log1p.h, ag_div.h, ag_sim.h, ag_train_math.h). `tab`: the kExpTabLds-entry table.
// ---------------------------------------------------------------------------------------
struct KatIo {
  int in_bytes, out_bytes;
};
__host__ __device__ __forceinline__ KatIo kat_io(int fn) {
  switch (fn) {
    case AG_KAT_EXP: case AG_KAT_EXP_FAST: case AG_KAT_SIGMOID: case AG_KAT_SIGMOID_FAST: case AG_KAT_LOG1P:
    case AG_KAT_FXB: case AG_KAT_FXB_FAST: case AG_KAT_FXB_X: case AG_KAT_FX_ROUND_GRAD: case AG_KAT_FX_ROUND_LOSS:
    case AG_KAT_LR_BCE:
      return {8, 8};
    case AG_KAT_EXP_MAIN: case AG_KAT_LOG1P_MAIN: case AG_KAT_LOG1P_SHARED: case AG_KAT_SOFTPLUS_FAST:
    case AG_KAT_WR_ROW:
      return {8, 16};
    case AG_KAT_EXPF_GLIBC: case AG_KAT_TORCH_EXPF:
      return {4, 4};
    case AG_KAT_TS_CTR_OF:
      return {12, 4};
    case AG_KAT_DIV:
      return {16, 16};
    case AG_KAT_POLAR:
      return {16, 8};
    default:
      return {0, 0};
  }
}
// SharedDiv with the operands of its two divisions tested against div_safe on the way
struct KatSharedDiv {
  agtm::SharedDiv d;
  bool *safe_cu, *safe_fs;
  __host__ __device__ double cu(double c, double u) const {
    *safe_cu = agdiv::div_safe(c, u);
    return d.cu(c, u);
  }
  __host__ __device__ double fs(double f, double dd) const {
    *safe_fs = agdiv::div_safe(f, dd);
    return d.fs(f, dd);
  }
};
__host__ __device__ __forceinline__ void kat_eval(int fn, const void *in, void *out, int64_t i, const uint64_t *tab) {
  using agexp::asu64;
  const double *xd = (const double *)in;
  const float *xf = (const float *)in;
  uint64_t *od = (uint64_t *)out;
  uint32_t *of = (uint32_t *)out;
  switch (fn) {
    case AG_KAT_EXP: od[i] = asu64(agexp::exp(xd[i], tab)); break;
    case AG_KAT_EXP_FAST: od[i] = asu64(agexp::exp_fast(xd[i], tab)); break;
    case AG_KAT_SIGMOID: od[i] = asu64(agexp::sigmoid(xd[i], tab)); break;
    case AG_KAT_SIGMOID_FAST: od[i] = asu64(agexp::sigmoid_fast(xd[i], tab)); break;
    case AG_KAT_EXP_MAIN:
      od[2 * i] = asu64(agexp::exp_main(xd[i], tab));
      od[2 * i + 1] = agexp::exp_in_main(xd[i]);
      break;
    case AG_KAT_EXPF_GLIBC: of[i] = __builtin_bit_cast(uint32_t, agexp::expf_glibc(xf[i], tab + 256)); break;
    case AG_KAT_TORCH_EXPF: of[i] = __builtin_bit_cast(uint32_t, ag::torch_expf(xf[i])); break;
    case AG_KAT_TS_CTR_OF: {
      const int32_t *q = (const int32_t *)in + 3 * i;
      of[i] = __builtin_bit_cast(uint32_t, ag::ts_ctr_of(xf[3 * i], q[1], q[2], tab));
      break;
    }
    case AG_KAT_LOG1P: od[i] = asu64(aglog1p::log1p(xd[i])); break;
    case AG_KAT_LOG1P_MAIN: {
      bool ok;
      od[2 * i] = asu64(aglog1p::log1p_main(xd[i], ok));
      od[2 * i + 1] = ok;
      break;
    }
    case AG_KAT_LOG1P_SHARED: {
      bool ok, s1 = false, s2 = false;
      const double r = agdiv::recip(1.0 + xd[i]);
      od[2 * i] = asu64(aglog1p::log1p_main_t(xd[i], ok, KatSharedDiv{agtm::SharedDiv{r}, &s1, &s2}));
      od[2 * i + 1] = (uint64_t)ok | ((uint64_t)s1 << 1) | ((uint64_t)s2 << 2);
      break;
    }
    case AG_KAT_DIV: {
      const double a = xd[2 * i], b = xd[2 * i + 1];
      od[2 * i] = asu64(agdiv::div_core(a, b, agdiv::recip(b)));
      od[2 * i + 1] = agdiv::div_safe(a, b);
      break;
    }
    case AG_KAT_FXB: od[i] = (uint64_t)agtm::fxb(xd[i]); break;
    case AG_KAT_FXB_FAST: od[i] = (uint64_t)agtm::fxb_fast(xd[i]); break;
    case AG_KAT_FXB_X: od[i] = (uint64_t)agtm::fxb_x(xd[i]); break;
    case AG_KAT_FX_ROUND_GRAD: od[i] = (uint64_t)agtm::fx_round(xd[i], agtm::kGradScale); break;
    case AG_KAT_FX_ROUND_LOSS: od[i] = (uint64_t)agtm::fx_round(xd[i], agtm::kLossScale); break;
    case AG_KAT_POLAR: od[i] = asu64(agtm::polar_transform(xd[2 * i], xd[2 * i + 1])); break;
    case AG_KAT_LR_BCE: {
      const int32_t y = ((const int32_t *)in)[2 * i + 1];
      od[i] = (uint64_t)agtm::fx_round(agtm::lr_bce_term(xf[2 * i], y), agtm::kLossScale);
      break;
    }
    case AG_KAT_SOFTPLUS_FAST: {
      double e;
      od[2 * i] = asu64(agtm::softplus_fast(xd[i], e, tab));
      od[2 * i + 1] = asu64(e);
      break;
    }
    case AG_KAT_WR_ROW: {  // a y = 0 row whose logit is the input: z = 0 0 + 0 0 + 0 0 + x
      agtm::WrMain m = agtm::wr_main(0.0, 0.0, 0.0, 0.0, false, 0.0, 0.0, 0.0, xd[i], tab);
      if (!m.main) agtm::wr_patch(m, 0.0, tab);
      od[2 * i] = asu64(m.pw);
      od[2 * i + 1] = asu64(m.Lz);
      break;
    }
    default: break;
  }
}
__global__ __launch_bounds__(256) void k_math_kat(int fn, const void *in, void *out, int64_t n) {
  __shared__ uint64_t s_tab[agexp::kExpTabLds];
  for (int i = threadIdx.x; i < 256; i += 256) s_tab[i] = ag_exp_tab[i];
  if (threadIdx.x < 32) s_tab[256 + threadIdx.x] = agexp::expf_tab_entry(ag_exp_tab, threadIdx.x);
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    kat_eval(fn, in, out, i, s_tab);
}

}  // namespace

extern "C" int ag_math_kat(int32_t device, int32_t fn, const void *in, int64_t n, void *out) {
  const KatIo io = kat_io(fn);
  if (io.in_bytes == 0) return ag_set_error(AG_ERR_INVALID, "ag_math_kat: fn %d outside [0, %d)", fn, AG_KAT_COUNT);
  if (n < 0 || device < -1 || ((!in || !out) && n > 0))
    return ag_set_error(AG_ERR_INVALID, "ag_math_kat: device >= -1, n >= 0, non-null in / out");
  if (n == 0) return AG_OK;
  if (device < 0) {  // the host build of the same source
    uint64_t tab[agexp::kExpTabLds];
    for (int i = 0; i < 256; ++i) tab[i] = ag_exp_tab[i];
    for (int j = 0; j < 32; ++j) tab[256 + j] = agexp::expf_tab_entry(ag_exp_tab, j);
    for (int64_t i = 0; i < n; ++i) kat_eval(fn, in, out, i, tab);
    return AG_OK;
  }
  AgDeviceGuard dg(device);
  void *d_in = nullptr, *d_out = nullptr;
  const size_t nin = (size_t)n * io.in_bytes, nout = (size_t)n * io.out_bytes;
  hipError_t e = hipMalloc(&d_in, nin);
  if (e == hipSuccess) e = hipMalloc(&d_out, nout);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_math_kat, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, nullptr, fn,
                       (const void *)d_in, d_out, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  if (e != hipSuccess) return ag_set_error(AG_ERR_HIP, "ag_math_kat: %s", hipGetErrorString(e));
  return AG_OK;
}

extern "C" int ag_div_selftest(int32_t device, int64_t pairs, uint64_t seed, int64_t *tested, int64_t *mismatches) {
  if (!mismatches || !tested || pairs < 0)
    return ag_set_error(AG_ERR_INVALID, "ag_div_selftest: pairs >= 0, non-null tested / mismatches");
  AgDeviceGuard dg(device);
  constexpr int kBlocks = 4096, kIters = 48;
  const int64_t per_launch = (int64_t)kBlocks * 256 * kIters;
  unsigned long long *cnt = nullptr;
  hipError_t e = hipMalloc(&cnt, 2 * sizeof(*cnt));
  if (e == hipSuccess) e = hipMemset(cnt, 0, 2 * sizeof(*cnt));
  for (int64_t done = 0, l = 0; e == hipSuccess && done < pairs; done += per_launch, ++l) {
    hipLaunchKernelGGL(k_div_stress, dim3(kBlocks), dim3(256), 0, nullptr, seed + (uint64_t)l * 0x100000001b3ull,
                       kIters, cnt, cnt + 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned long long h[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpy(h, cnt, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(cnt);
  if (e != hipSuccess) return ag_set_error(AG_ERR_HIP, "ag_div_selftest: %s", hipGetErrorString(e));
  *mismatches = (int64_t)h[0];
  *tested = (int64_t)h[1];
  return AG_OK;
}

extern "C" int ag_coop_selftest(int32_t device, int32_t workgroups, int32_t generations, int32_t regions,
                                int64_t *mismatches) {
  if (!mismatches) return ag_set_error(AG_ERR_INVALID, "ag_coop_selftest: null mismatches");
  if (generations < 0 || regions < 1 || regions > kStMaxRegions)
    return ag_set_error(AG_ERR_INVALID, "ag_coop_selftest: generations >= 0, regions in [1, %d]", kStMaxRegions);
  AgDeviceGuard dg(device);
  int cus = 0, per_cu = 0;
  AG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  AG_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_coop_stress, kStThreads, 0));
  const int cap = per_cu * cus;
  int G = workgroups > 0 ? workgroups : 4 * cus;
  if (G > cap)
    return ag_set_error(AG_ERR_UNSUPPORTED, "ag_coop_selftest: %d workgroups > %d co-resident", G, cap);
  int lines = agcoop::bar_lines(G);
  if (lines < 1) lines = 1;
  // bars: [regions][lines][32] u32; acc: [regions][lines][32] int64 (zero on entry, zero again
  // after every sum but row 0); bad: one u64
  unsigned *bars = nullptr;
  int64_t *acc = nullptr;
  unsigned long long *bad = nullptr;
  const size_t nb = (size_t)regions * lines * agcoop::kBarLineWords * sizeof(unsigned);
  const size_t na = (size_t)regions * lines * kStWords * sizeof(int64_t);
  hipError_t e = hipMalloc(&bars, nb);
  if (e == hipSuccess) e = hipMalloc(&acc, na);
  if (e == hipSuccess) e = hipMalloc(&bad, sizeof(*bad));
  if (e == hipSuccess) e = hipMemset(bars, 0, nb);
  if (e == hipSuccess) e = hipMemset(acc, 0, na);
  if (e == hipSuccess) e = hipMemset(bad, 0, sizeof(*bad));
  void *args[] = {&bars, &acc, &lines, &regions, &generations, &bad};
  if (e == hipSuccess)
    e = hipLaunchCooperativeKernel((const void *)k_coop_stress, dim3(G), dim3(kStThreads), args, 0, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned long long h = 0;
  if (e == hipSuccess) e = hipMemcpy(&h, bad, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(bars);
  (void)hipFree(acc);
  (void)hipFree(bad);
  if (e != hipSuccess) return ag_set_error(AG_ERR_HIP, "ag_coop_selftest: %s", hipGetErrorString(e));
  *mismatches = (int64_t)h;
  return AG_OK;
}
