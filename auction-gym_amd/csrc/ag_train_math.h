// ag_train_math.h -- the trainers' scalar arithmetic, host and device from one source: the
// fixed-point roundings of the exact sums, softplus and the win-rate BCE row through the
// branch-free main paths (ag_dr.hip), the polar draw's transform, and the LR-TS trainer's
// rounding and BCE term (ag_lrts.hip). The trainers include it for their kernels;
// ag_selftest.hip's ag_math_kat evaluates every function here on either side, so the tests
// compare the device build with the host build of the very same lines (tests/
// test_gpu_math_kat.py) and the host build with libm / numpy (tests/test_math_kat_host.py).
//
// Compile with -ffp-contract=off, as everything that includes ag_exp.h / ag_log1p.h: their sums
// of products must not fuse (and the device maths library's log of the BCE term is compiled in
// the caller's unit). The magic-number roundings below would survive a fusion -- their scale is a
// power of two, so the product is exact -- but nothing else here would (PARITY.md).
#pragma once
#include <math.h>
#include <stdint.h>

#include "ag_div.h"
#include "ag_exp.h"
#include "ag_log1p.h"

#if defined(__HIPCC__)
#define AG_TM_HD __host__ __device__ __forceinline__
#define AG_TM_MEMBER __host__ __device__
#else
#define AG_TM_HD static inline
#define AG_TM_MEMBER
#endif

namespace agtm {

// ---------------------------------------------------------------------------------------
// ag_dr.hip
// ---------------------------------------------------------------------------------------
constexpr double kGrid = 0x1p40, kInv = 0x1p-40;

// Fixed-point terms (int64)rint(v * 2^40). For |v * 2^40| < 2^51 (every term in practice)
// adding 1.5 * 2^52 rounds to the integer (nearest, ties to even, as rint) and leaves it in
// the low mantissa bits.
// The accumulators hold them biased: fxb(v) = (int64)rint(v * 2^40) + kFxMagic (mod 2^64),
// kFxMagic = the bits of 1.5 * 2^52 -- for |v * 2^40| < 2^51 simply the bits of v * 2^40 +
// 1.5 * 2^52, so a term costs one add and the 64-bit accumulate (no subtract); a lane that
// added n terms to an accumulator takes n * kFxMagic off once (fx_unbias) before the exact
// sums. Integer arithmetic mod 2^64: the same totals, bit for bit.
constexpr uint64_t kFxMagic = 0x4338000000000000ull;  // asu64(0x1.8p52)
AG_TM_HD int64_t fxb_fast(double v) {  // |v| <= 2^10 guaranteed by the caller
  return (int64_t)agexp::asu64(v * kGrid + 0x1.8p52);
}
AG_TM_HD int64_t fxb(double v) {
  const double x = v * kGrid;
  if (__builtin_expect(__builtin_fabs(x) < 0x1p51, 1)) return (int64_t)agexp::asu64(x + 0x1.8p52);
  return (int64_t)((uint64_t)(int64_t)__builtin_rint(x) + kFxMagic);
}
// fxb's fast path on x = v * 2^40 already formed, and its range test (callers test a
// record's terms together and take fxb for all of them when one is out of range)
AG_TM_HD int64_t fxb_x(double x) { return (int64_t)agexp::asu64(x + 0x1.8p52); }
AG_TM_HD bool fx_in(double x) { return __builtin_fabs(x) < 0x1p51; }

// log1p_main's divisions for a caller that holds r = the reciprocal of its 1 + x (ag_div.h)
struct SharedDiv {
  double r;
  AG_TM_MEMBER double cu(double c, double u) const { return agdiv::div_core(c, u, r); }
  AG_TM_MEMBER double fs(double f, double d) const { return agdiv::div_core(f, d, agdiv::recip(d)); }
};

// exp(x) and softplus from the branch-free main paths (the same bits), the rare inputs
// outside them patched with the full functions
// e = exp(u); returns softplus(u)
AG_TM_HD double softplus_fast(double u, double &e, const uint64_t *tab) {
  e = agexp::exp_main(u, tab);
  bool lok;
  double l = aglog1p::log1p_main(e, lok);
  if (__builtin_expect(!(agexp::exp_in_main(u) && (lok || u > 20.0)), 0)) {
    e = agexp::exp(u, tab);
    l = aglog1p::log1p(e);
  }
  return u > 20.0 ? u : l;
}

// the polar (Marsaglia) draw's transform of an accepted (u, s = u^2 + v^2 in (0, 1)): the
// standard normal, rounded to float32 as the reference's rsample noise is
AG_TM_HD double polar_transform(double u, double s) {
  return (double)(float)(u * __builtin_sqrt(-2.0 * aglog1p::log1p(s - 1.0) / s));
}

// One BCE row of the win-rate fit (its loss and gradient terms, biased: see fxb) at the model
// (w0, w1, w2, w3). One exp per row (oracle/ag_oracle_dr.c fit_winrate): e = exp(-|z|), L =
// log1p(e); p = (z >= 0 ? 1 : e) / (1 + e); -log(p) = softplus(-z) for a win, -log(1 - p) =
// softplus(z) otherwise, softplus(u) = L for u <= 0, |z| + L for u > 0 (u past 20: u).
// Branch-free main paths of exp and log1p (the same bits), the rare inputs outside them
// patched with the full functions afterwards. aug: the gamma = 0, y = 0 augmentation row.
// The row in two parts so that a record's two rows (and a lane's records) can be computed
// in one basic block before either takes its rare branch: wr_main is branch-free, wr_patch
// recomputes (rarely) what the main paths could not give.
struct WrMain {
  double z, a, e, Lz, pw, u, t, gz, x2, x3;
  bool main;  // exp and log1p on their main paths
  bool ok;    // main, and the checked terms in fxb's fast range
};
AG_TM_HD WrMain wr_main(double c, double v, double g, double y, bool aug, double w0, double w1, double w2,
                        double w3, const uint64_t *tab) {
  WrMain m;
  m.z = c * w0 + v * w1 + g * w2 + w3;
  m.a = __builtin_fabs(m.z);
  m.e = agexp::exp_main(-m.a, tab);
  bool lok;
  // p's division and log1p's c / u both divide by 1 + e: one reciprocal (ag_div.h; on the main
  // paths e >= exp(-512), c is 0 or >= 2^-81 in magnitude, |f| >= 2^-53: div_safe's range)
  const double d1 = 1.0 + m.e, r1 = agdiv::recip(d1);
  m.Lz = aglog1p::log1p_main_t(m.e, lok, SharedDiv{r1});
  m.pw = agdiv::div_core(m.z >= 0.0 ? 1.0 : m.e, d1, r1);
  m.u = y > 0.0 ? -m.z : m.z;
  m.t = fmin(m.u > 20.0 ? m.u : (m.u > 0.0 ? m.a + m.Lz : m.Lz), 100.0);
  m.gz = m.pw - y;
  // |t| <= 100, |pw - y| <= 1, ctr in [0, 1]: those terms are far inside fxb's fast range;
  // gz * value and gz * gamma are checked. ONE rare branch per row (the exp / log1p patch and
  // an out-of-range term together) instead of one per patch: the common path stays straight.
  // (the augmentation row's x3 is gz * 0: always in range, and its term is never added)
  m.x2 = (m.gz * v) * kGrid;
  m.x3 = (m.gz * g) * kGrid;
  m.main = (int)agexp::exp_in_main(m.a) & (int)lok;
  m.ok = (int)m.main & (int)fx_in(m.x2) & ((int)aug | (int)fx_in(m.x3));
  return m;
}
// a row whose exp or log1p left its main path: the full functions and the plain division
AG_TM_HD void wr_patch(WrMain &m, double y, const uint64_t *tab) {
  m.e = agexp::exp(-m.a, tab);
  m.Lz = aglog1p::log1p(m.e);
  m.pw = (m.z >= 0.0 ? 1.0 : m.e) / (1.0 + m.e);
  m.t = fmin(m.u > 20.0 ? m.u : (m.u > 0.0 ? m.a + m.Lz : m.Lz), 100.0);
  m.gz = m.pw - y;
}

// ---------------------------------------------------------------------------------------
// ag_lrts.hip
// ---------------------------------------------------------------------------------------
constexpr double kGradScale = 0x1p40, kLossScale = 0x1p32;

AG_TM_HD int64_t fx_round(double v, double scale) { return (int64_t)__builtin_rint(v * scale); }

// torch's binary_cross_entropy term of one sample at the float32 prediction p, label y: the
// logs clamped at -100 (oracle/ag_oracle.c lrts_loss_grad)
AG_TM_HD double lr_bce_term(float p, int y) {
  return y ? -fmax(log((double)p), -100.0) : -fmax(log1p(-(double)p), -100.0);
}

}  // namespace agtm
