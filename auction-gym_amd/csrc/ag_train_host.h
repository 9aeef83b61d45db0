// ag_train_host.h -- the host side the trainers share (ag_dr.hip: ag_bidder_update, ag_bidder_rp_*;
// ag_lrts.hip: ag_lrts_update, ag_lrts_rp_*), each piece once: the workgroup tables of a launch,
// the share-out of the resident grid, the Adam bias-correction table, the layouts of the device
// buffers that grow on demand and, for hipcc, how those grow, the typed launch and the store's
// count. Everything down to "HIP wrappers" is plain C++17 (tests/host/train_host_check.cpp
// compiles it with g++ and checks it without a GPU).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>
#include <vector>

namespace agtrain {

// The block tables of a launch, from the workgroups per agent (nblk; 0: the agent is not in the
// launch): workgroup b works on agent blk_agent[b] as its workgroup blk_rank[b] (an agent's
// workgroups have consecutive indices); agent a's barrier lines (and accumulator rows) start
// at line bar_off[a], lines_of(nblk[a]) of them, `lines` in all.
struct BlockTables {
  std::vector<int32_t> nblk, blk_agent, blk_rank, bar_off;
  int lines = 0;
  int G() const { return (int)blk_agent.size(); }
  bool multi() const {  // some agent's workgroups wait for each other: they must all be resident
    for (int32_t nb : nblk)
      if (nb > 1) return true;
    return false;
  }
};
template <class LinesOf>
inline void block_tables(BlockTables &T, LinesOf lines_of) {
  const int N = (int)T.nblk.size();
  T.bar_off.assign(N, 0);
  T.blk_agent.clear();
  T.blk_rank.clear();
  T.lines = 0;
  for (int a = 0; a < N; ++a) {
    if (!T.nblk[a]) continue;
    T.bar_off[a] = T.lines;
    T.lines += lines_of(T.nblk[a]);
    for (int r = 0; r < T.nblk[a]; ++r) {
      T.blk_agent.push_back(a);
      T.blk_rank.push_back(r);
    }
  }
}

// More workgroups wanted than the `resident` grid holds: every agent's count scaled by
// resident / wanted, at least one. The floor stops at 1, so many agents of one workgroup can keep
// the total above the resident grid: then every agent trains on one workgroup (a plain launch
// of any size; the trainers' record loops take any n). So afterwards the launch fits the
// resident grid or needs no cooperative launch: the planners have no refusal.
inline void share_out(std::vector<int32_t> &nblk, int resident) {
  int64_t want = 0;
  for (int32_t nb : nblk) want += nb;
  if (want <= resident) return;
  const double f = (double)resident / (double)want;
  want = 0;
  for (int32_t &nb : nblk)
    if (nb > 0) want += nb = (int32_t)(nb * f) > 1 ? (int32_t)(nb * f) : 1;
  if (want > resident)
    for (int32_t &nb : nblk)
      if (nb > 1) nb = 1;
}

// torch.optim.Adam's bias corrections of steps 1 .. epochs, [2][epochs]: 1 - 0.9^t, then
// (1 - 0.999^t)^0.5 (Python floats, libm pow: the values are part of parity)
inline std::vector<double> adam_bias_table(int epochs) {
  std::vector<double> tab(2 * (size_t)epochs);
  for (int t = 0; t < epochs; ++t) {
    tab[t] = 1.0 - pow(0.9, (double)(t + 1));
    tab[epochs + t] = pow(1.0 - pow(0.999, (double)(t + 1)), 0.5);
  }
  return tab;
}

inline int grid_over(int64_t n, int threads) {
  int64_t g = (n + threads - 1) / threads;
  if (g > 4096) g = 4096;
  return (int)(g < 1 ? 1 : g);
}

// A cursor that carves one buffer into arrays. Every layout below is one function over it, run
// with a null base for the buffer's size (bytes()) and with the buffer for the pointers, so the
// two cannot disagree. Alignments are of the offset: the bases (hipMalloc's, or a 64-byte
// multiple past one) are aligned further than any array asks.
struct Carve {
  char *base;
  size_t off = 0;
  explicit Carve(void *b = nullptr) : base((char *)b) {}
  template <class T>
  T *take(size_t n, size_t align = alignof(T)) {
    off = (off + align - 1) / align * align;
    T *p = base ? (T *)(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  size_t bytes() const { return off; }
};

// The learning bidders' records sorted into (agent, log order), the sorts' keys / indices and
// hipcub's temp (ag_dr_ws::buf); d_off [N + 1] (ag_dr_ws::counts) and n ride along.
struct SortedRecs {
  double *ctr, *val, *gam, *prop, *util, *eu;  // eu: the estimated-utility workspace
  uint64_t *k_in, *k_out;
  uint32_t *i_in, *i_out;
  uint8_t *won;
  void *tmp;
  int64_t *d_off;
  int64_t n;
};
inline SortedRecs sorted_layout(Carve &c, size_t cap, size_t sort_tmp) {
  SortedRecs S{};
  S.ctr = c.take<double>(cap), S.val = c.take<double>(cap), S.gam = c.take<double>(cap);
  S.prop = c.take<double>(cap), S.util = c.take<double>(cap), S.eu = c.take<double>(cap);
  S.k_in = c.take<uint64_t>(cap), S.k_out = c.take<uint64_t>(cap);
  S.i_in = c.take<uint32_t>(cap), S.i_out = c.take<uint32_t>(cap);
  S.won = c.take<uint8_t>(cap);
  S.tmp = c.take<char>(sort_tmp, 256);
  return S;
}

// ag_bidder_update's device tables (ag_dr_ws::coop, shared by its two launches and rewritten in
// stream order): exchange partials [G][96] i64; barrier lines [lines][32] u32; the block tables;
// the win-rate models [N][4] f32 (phase 0 -> phase 1)
struct TrainTables {
  int64_t *part;
  unsigned *bar;
  int32_t *bagent, *brank, *nblk, *baroff;
  float *wr;
};
inline TrainTables train_layout(Carve &c, size_t N, size_t G, size_t lines) {
  TrainTables D;
  D.part = c.take<int64_t>(96 * G);
  D.bar = c.take<unsigned>(32 * lines);
  D.bagent = c.take<int32_t>(G), D.brank = c.take<int32_t>(G);
  D.nblk = c.take<int32_t>(N), D.baroff = c.take<int32_t>(N);
  D.wr = c.take<float>(4 * N);
  return D;
}

// The per-epoch launches' tables (ag_bidder_rp_*, ag_lrts_rp_*): the block tables and the mask of
// the agents under training, then (learning bidders: n_ntot = 2 N) [N] records over all ranks and
// [N] the global index of this rank's first; their combining-tree accumulator rows
// [lines][acc_stride] i64 and barrier lines [lines][32] u32.
struct RpTables {
  int32_t *bagent, *brank, *nblk, *baroff, *mask;
  int64_t *ntot;
};
inline RpTables rp_tables_layout(Carve &c, size_t N, size_t G, size_t n_ntot) {
  RpTables D;
  D.bagent = c.take<int32_t>(G), D.brank = c.take<int32_t>(G);
  D.nblk = c.take<int32_t>(N), D.baroff = c.take<int32_t>(N), D.mask = c.take<int32_t>(N);
  D.ntot = c.take<int64_t>(n_ntot, 16);
  return D;
}
struct RpAcc {
  int64_t *acc;
  unsigned *bar;
};
inline RpAcc rp_acc_layout(Carve &c, size_t lines, size_t acc_stride) {
  RpAcc D;
  D.acc = c.take<int64_t>(acc_stride * lines);
  D.bar = c.take<unsigned>(32 * lines);
  return D;
}

// One phase of k_bidder_pipe's tables (ag_dr_rp::pipe holds two: the launches of a run never
// share a word): slot agents / LDS offsets / LDS capacities [3][max_agents] i32, then the slots'
// accumulator rows [rows] i64 and barrier lines [rows] u32
struct PipeTables {
  int32_t *tab;
  int64_t *acc;
  unsigned *bar;
};
inline PipeTables pipe_layout(Carve &c, size_t max_agents, size_t rows) {
  PipeTables D;
  D.tab = c.take<int32_t>(3 * max_agents);
  D.acc = c.take<int64_t>(rows, 16);
  D.bar = c.take<unsigned>(rows);
  return D;
}

// ag_lrts_update's tables (ag_lrts_ws::tables): the block tables (agent_nblk with N words to
// spare), agent_pbase [N] i64 = bar_off * the accumulator row, bar_off, barrier lines [lines][32]
struct LrtsTables {
  int32_t *bagent, *brank, *nblk, *baroff;
  int64_t *pbase;
  unsigned *bar;
};
inline LrtsTables lrts_layout(Carve &c, size_t N, size_t G, size_t lines) {
  LrtsTables D;
  D.bagent = c.take<int32_t>(G), D.brank = c.take<int32_t>(G);
  D.nblk = c.take<int32_t>(2 * N);
  D.pbase = c.take<int64_t>(N);
  D.baroff = c.take<int32_t>(N);
  D.bar = c.take<unsigned>(32 * lines);
  return D;
}

template <class Layout, class... A>
inline size_t layout_bytes(Layout layout, A... a) {
  Carve c;
  layout(c, a...);
  return c.bytes();
}

}  // namespace agtrain

// ---- HIP wrappers ----
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "ag_host.h"

namespace agtrain {

// A device buffer that grows on demand: holds `need` bytes afterwards (`want` >= need allocated
// where the caller leaves room to grow). It frees, nulls and zeroes the capacity before it
// allocates: a failed allocation leaves the buffer empty, and the next call allocates it again.
// hipFree, not an async free: it synchronises, so no launch of an earlier call uses the old
// buffer any more.
template <class T>
inline hipError_t dev_reserve(T **ptr, size_t *have, size_t need, size_t want = 0) {
  if (*ptr && need <= *have) return hipSuccess;
  (void)hipFree(*ptr);
  *ptr = nullptr;
  *have = 0;
  if (want < need) want = need;
  const hipError_t e = hipMalloc((void **)ptr, want);
  if (e == hipSuccess) *have = want;
  return e;
}

// Co-resident workgroups of `fn` at `threads` and `lds` dynamic bytes on the whole device,
// at least one; queried once (*cached)
inline hipError_t resident_blocks(const void *fn, int threads, size_t lds, int device, int *cached) {
  if (*cached) return hipSuccess;
  int per_cu = 0, cus = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) *cached = per_cu * cus > 0 ? per_cu * cus : 1;
  return e;
}

// One launch of a trainer: cooperative where workgroups of one agent wait for each other. The
// arguments convert to the kernel's own parameter types here (a wrong count or an unrelated
// pointer does not compile) and the void *[] is built from those.
template <class... P>
inline hipError_t launch_group(void (*kernel)(P...), bool cooperative, int grid, int block, size_t lds,
                               hipStream_t st, std::enable_if_t<true, P>... a) {
  void *args[] = {(void *)&a...};
  if (cooperative) return hipLaunchCooperativeKernel((const void *)kernel, dim3(grid), dim3(block), args, lds, st);
  return hipLaunchKernel((const void *)kernel, dim3(grid), dim3(block), args, lds, st);
}

// The store's count on the host (synchronises `st`); an overflowed store is refused
inline int read_store_count(const void *count, int64_t capacity, const char *who, const char *what, hipStream_t st,
                            uint64_t *n) {
  *n = 0;
  AG_HIP(hipMemcpyAsync(n, count, sizeof *n, hipMemcpyDeviceToHost, st));
  AG_HIP(hipStreamSynchronize(st));
  if ((int64_t)*n > capacity)
    return ag_set_error(AG_ERR_INVALID, "%s: %llu %s overflowed the store (capacity %lld)", who,
                        (unsigned long long)*n, what, (long long)capacity);
  return AG_OK;
}

}  // namespace agtrain
#endif
