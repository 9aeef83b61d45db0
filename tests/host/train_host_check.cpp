// The trainers' host planner (auction-gym_amd/csrc/ag_train_host.h, its part without HIP) checked
// on the CPU: g++ -std=c++17 -fsanitize=address,undefined -I auction-gym_amd/csrc, run as a program
// (tests/test_host.py does). Every layout's arrays are written end to end inside a buffer of exactly
// the size pass's bytes, so an array that passes its layout's end is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#include "ag_train_host.h"

using namespace agtrain;

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static int two_per(int nb) { return nb > 1 ? 2 + nb / 3 : 0; }  // some lines_of with a zero

static void check_block_tables() {
  BlockTables T;
  T.nblk = {3, 0, 1, 0, 0, 7, 2, 0};
  block_tables(T, two_per);
  int b = 0, lines = 0;
  for (size_t a = 0; a < T.nblk.size(); ++a) {
    if (!T.nblk[a]) {
      CHECK(T.bar_off[a] == 0);  // contributes nothing: no workgroup, no line
      continue;
    }
    CHECK(T.bar_off[a] == lines);  // the running sum of lines_of
    lines += two_per(T.nblk[a]);
    for (int r = 0; r < T.nblk[a]; ++r, ++b) CHECK(T.blk_agent[b] == (int)a && T.blk_rank[b] == r);
  }
  CHECK(b == T.G() && b == 13 && T.lines == lines && T.multi());
  T.nblk = {0, 1, 1};
  block_tables(T, two_per);  // (tables of an earlier launch are replaced)
  CHECK(T.G() == 2 && T.lines == 0 && !T.multi() && T.blk_agent[1] == 2 && T.blk_rank[1] == 0);
  T.nblk = {0, 0};
  block_tables(T, two_per);
  CHECK(T.G() == 0 && T.lines == 0 && !T.multi());
}

// share_out against its statement: max(1, int(n * (resident / sum))) per agent where that fits the
// resident grid, else one workgroup per agent; agents out of the launch stay out
static void check_share(std::vector<int32_t> nblk, int resident) {
  const std::vector<int32_t> in = nblk;
  share_out(nblk, resident);
  const int64_t sum = std::accumulate(in.begin(), in.end(), (int64_t)0);
  std::vector<int32_t> want = in;
  if (sum > resident) {
    int64_t scaled = 0;
    for (int32_t &n : want)
      if (n) scaled += n = std::max(1, (int)(n * ((double)resident / (double)sum)));
    if (scaled > resident)
      for (int32_t &n : want) n = n ? 1 : 0;
  }
  CHECK(nblk == want);
  const int64_t got = std::accumulate(nblk.begin(), nblk.end(), (int64_t)0);
  CHECK(got <= resident || *std::max_element(nblk.begin(), nblk.end()) == 1);
}

static void check_share_out() {
  for (int cus : {1, 8, 256, 304})
    for (int per_cu = 1; per_cu <= 8; ++per_cu) {
      const int resident = per_cu * cus, total = 8 * cus + 248, big = total * 45 / 100;
      // the grid-shared-out tests (tests/test_gpu_lrts_edges.py, test_gpu_trainer_plan.py), one
      // sample / record per workgroup: 45 % / 45 % / 10 % and an agent of two / of one
      for (int last : {2, 1}) {
        std::vector<int32_t> sizes = {big, big, total - 2 * big, last};
        check_share(sizes, resident);
        sizes.insert(sizes.begin() + 1, 0);  // an agent that does not train in between
        check_share(sizes, resident);
        if (cus >= 256) {  // (what those tests assert on a real device: shared out, never the fall-back)
          share_out(sizes, resident);
          CHECK(std::accumulate(sizes.begin(), sizes.end(), 0) <= resident && sizes[0] > 16);
        }
      }
      // the fall-back tests: 8 * CUs + 1 agents of one workgroup beside one that wants 100
      std::vector<int32_t> many(8 * cus + 2, 1);
      many.back() = 100;
      check_share(many, resident);
      share_out(many, resident);
      CHECK(*std::max_element(many.begin(), many.end()) == 1 && *std::min_element(many.begin(), many.end()) == 1);
      check_share({5, 3}, resident);  // fits, or not
    }
  std::vector<int32_t> fits = {4, 0, 2};
  share_out(fits, 6);
  CHECK((fits == std::vector<int32_t>{4, 0, 2}));
}

// One layout at one size: the buffer holds exactly the size pass's bytes; `arrays` lists (pointer,
// bytes, alignment, the parent commit's byte offset) in layout order and `end` the parent's end.
struct Arr {
  const void *p;
  size_t bytes, align, offset;
};
template <class Layout, class List>
static void check_layout(const char *name, Layout layout, List arrays, size_t end) {
  Carve size;
  layout(size);
  CHECK(size.bytes() == end);
  char *buf = (char *)aligned_alloc(256, (size.bytes() + 255) / 256 * 256 + 256);
  Carve c(buf);
  auto D = layout(c);
  CHECK(c.bytes() == size.bytes());  // the size pass ends where the pointer pass ends
  size_t prev = 0;
  for (const Arr &a : arrays(D)) {
    const size_t off = (size_t)((const char *)a.p - buf);
    if (off != a.offset || off % a.align || off < prev || off + a.bytes > size.bytes()) {
      printf("%s: array at %zu (+%zu, align %zu), the parent's at %zu, layout ends at %zu\n", name, off, a.bytes,
             a.align, a.offset, size.bytes());
      ++failures;
    }
    prev = off + a.bytes;
  }
  free(buf);
  // and inside a buffer of exactly that size, written end to end
  char *exact = (char *)malloc(size.bytes() ? size.bytes() : 1);
  Carve w(exact);
  auto E = layout(w);
  for (const Arr &a : arrays(E)) memset((void *)a.p, 0x5a, a.bytes);
  free(exact);
}

static size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }

static void check_layouts() {
  for (size_t N : {1, 3, 32})
    for (size_t G : {1, 517}) {
      const size_t L = G == 1 ? 0 : 83, cap = 37 * G, tmp = 1000 + G, M = 64, rows = 32 * L + 32;
      // sort_records' buffer: the parent asked for cap * 73 + tmp + 256 and aligned tmp by hand
      check_layout("sorted", [&](Carve &c) { return sorted_layout(c, cap, tmp); },
                   [&](const SortedRecs &S) {
                     return std::vector<Arr>{{S.ctr, 8 * cap, 8, 0},          {S.val, 8 * cap, 8, 8 * cap},
                                             {S.gam, 8 * cap, 8, 16 * cap},   {S.prop, 8 * cap, 8, 24 * cap},
                                             {S.util, 8 * cap, 8, 32 * cap},  {S.eu, 8 * cap, 8, 40 * cap},
                                             {S.k_in, 8 * cap, 8, 48 * cap},  {S.k_out, 8 * cap, 8, 56 * cap},
                                             {S.i_in, 4 * cap, 4, 64 * cap},  {S.i_out, 4 * cap, 4, 68 * cap},
                                             {S.won, cap, 1, 72 * cap},       {S.tmp, tmp, 256, up(73 * cap, 256)}};
                   },
                   up(73 * cap, 256) + tmp);
      CHECK(up(73 * cap, 256) + tmp <= cap * 73 + tmp + 256);
      // ag_bidder_update's tables: the parent's need_coop less its 64 spare bytes
      check_layout("train", [&](Carve &c) { return train_layout(c, N, G, L); },
                   [&](const TrainTables &D) {
                     const size_t t = 768 * G + 128 * L;
                     return std::vector<Arr>{{D.part, 768 * G, 8, 0},          {D.bar, 128 * L, 4, 768 * G},
                                             {D.bagent, 4 * G, 4, t},          {D.brank, 4 * G, 4, t + 4 * G},
                                             {D.nblk, 4 * N, 4, t + 8 * G},    {D.baroff, 4 * N, 4, t + 8 * G + 4 * N},
                                             {D.wr, 16 * N, 4, t + 8 * G + 8 * N}};
                   },
                   8 * 96 * G + 4 * 32 * L + 4 * (2 * G + 2 * N) + 4 * 4 * N);
      // the per-epoch launches' tables: the bidders' (2 N int64 behind, 16-byte aligned) and LR-TS's
      for (size_t nt : {2 * N, (size_t)0})
        check_layout("rp_tables", [&](Carve &c) { return rp_tables_layout(c, N, G, nt); },
                     [&](const RpTables &D) {
                       return std::vector<Arr>{{D.bagent, 4 * G, 4, 0},
                                               {D.brank, 4 * G, 4, 4 * G},
                                               {D.nblk, 4 * N, 4, 8 * G},
                                               {D.baroff, 4 * N, 4, 8 * G + 4 * N},
                                               {D.mask, 4 * N, 4, 8 * G + 8 * N},
                                               {D.ntot, 8 * nt, 16, up(8 * G + 12 * N, 16)}};
                     },
                     up(4 * (2 * G + 3 * N), 16) + 8 * nt);
      CHECK(up(4 * (2 * G + 3 * N), 16) + 16 * N <= 4 * (2 * G + 3 * N) + 8 * 2 * N + 16);
      for (size_t stride : {32, 144})
        check_layout("rp_acc", [&](Carve &c) { return rp_acc_layout(c, L, stride); },
                     [&](const RpAcc &D) {
                       return std::vector<Arr>{{D.acc, 8 * stride * L, 8, 0}, {D.bar, 128 * L, 4, 8 * stride * L}};
                     },
                     8 * stride * L + 4 * 32 * L);
      // one phase of k_bidder_pipe's tables: the parent's per_ph less its 64 spare bytes
      check_layout("pipe", [&](Carve &c) { return pipe_layout(c, M, rows); },
                   [&](const PipeTables &D) {
                     return std::vector<Arr>{{D.tab, 12 * M, 4, 0},
                                             {D.acc, 8 * rows, 16, up(12 * M, 16)},
                                             {D.bar, 4 * rows, 4, up(12 * M, 16) + 8 * rows}};
                   },
                   3 * M * 4 + rows * (8 + 4));
      // ag_lrts_update's tables: the parent's malloc size
      check_layout("lrts", [&](Carve &c) { return lrts_layout(c, N, G, L); },
                   [&](const LrtsTables &D) {
                     return std::vector<Arr>{{D.bagent, 4 * G, 4, 0},
                                             {D.brank, 4 * G, 4, 4 * G},
                                             {D.nblk, 4 * N, 4, 8 * G},
                                             {D.pbase, 8 * N, 8, 8 * G + 8 * N},
                                             {D.baroff, 4 * N, 4, 8 * G + 16 * N},
                                             {D.bar, 128 * L, 4, 8 * G + 20 * N}};
                   },
                   8 * (G + 2 * N) + 4 * N + 4 * 32 * L);
      CHECK(layout_bytes(lrts_layout, N, G, L) == 8 * (G + 2 * N) + 4 * N + 128 * L);
    }
}

int main() {
  check_block_tables();
  check_share_out();
  check_layouts();
  const std::vector<double> tab = adam_bias_table(3);
  CHECK(tab.size() == 6 && tab[0] == 1.0 - 0.9 && tab[3] == pow(1.0 - 0.999, 0.5) && tab[2] == 1.0 - pow(0.9, 3.0));
  CHECK(grid_over(0, 256) == 1 && grid_over(257, 256) == 2 && grid_over((int64_t)1 << 40, 256) == 4096);
  printf(failures ? "train_host_check: %d FAILED\n" : "train_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
