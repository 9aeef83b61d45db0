"""ag_math_kat's HOST side (device = -1: the kernels' own source, compiled for the CPU) against
definitions from outside the project: libm through a few lines of C built here, numpy's IEEE
division, sqrt and rint, and the oracle's restatements that tests/test_oracle_golden.py pins to
torch. tests/test_gpu_math_kat.py then compares the device build with this host side bit for bit, on
the same inputs (tests/math_kat_cases.py) -- a comparison with the truth, not with a twin. No GPU."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import math_kat_cases as C

REF_SRC = r'''
#include <math.h>
#include <stdint.h>
void ref_exp(long n, const double *x, double *y) { for (long i = 0; i < n; ++i) y[i] = exp(x[i]); }
void ref_sigmoid(long n, const double *x, double *y) { for (long i = 0; i < n; ++i) y[i] = 1.0 / (1.0 + exp(-x[i])); }
void ref_expf(long n, const float *x, float *y) { for (long i = 0; i < n; ++i) y[i] = expf(x[i]); }
void ref_log1p(long n, const double *x, double *y) { for (long i = 0; i < n; ++i) y[i] = log1p(x[i]); }
void ref_log(long n, const double *x, double *y) { for (long i = 0; i < n; ++i) y[i] = log(x[i]); }
/* oracle/ag_oracle.c lrts_loss_grad's BCE term, fx_round = nearbyint */
void ref_bce(long n, const float *p, const int32_t *lab, int64_t *out) {
  for (long i = 0; i < n; ++i) {
    double t = lab[i] ? -fmax(log((double)p[i]), -100.0) : -fmax(log1p(-(double)p[i]), -100.0);
    out[i] = (int64_t)nearbyint(t * 0x1p32);
  }
}
/* any scalar function of the oracle's over an array */
void map_f32(float (*f)(float), long n, const float *x, float *y) { for (long i = 0; i < n; ++i) y[i] = f(x[i]); }
void map_f64(double (*f)(double), long n, const double *x, double *y) { for (long i = 0; i < n; ++i) y[i] = f(x[i]); }
'''


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("kat_ref")
    (d / "ref.c").write_text(REF_SRC)
    so = d / "libkatref.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(d / "ref.c"), "-o",
                    str(so), "-lm"], check=True)
    return ctypes.CDLL(str(so))


def _apply(fn, x, out_dtype, *more):
    x = np.ascontiguousarray(x)
    y = np.empty(x.shape[0], out_dtype)
    fn.restype = None
    fn(*more, ctypes.c_long(x.shape[0]), ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data))
    return y


def _kat(name, x=None):
    from auctiongym_amd import _lib
    return _lib.math_kat(name, C.cases(name) if x is None else x, device=-1)


def _same(got_bits, want, what):
    """Bit equality, NaNs compared as NaN."""
    want = np.ascontiguousarray(want)
    got = got_bits.view(want.dtype)
    both_nan = np.isnan(got) & np.isnan(want) if want.dtype.kind == "f" else np.zeros(got.shape, bool)
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    bad = np.flatnonzero((got.view(u) != want.view(u)) & ~both_nan)
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name", ["exp", "exp_fast"])
def test_exp_equals_libm(ref, name):
    x = C.cases(name)
    _same(_kat(name), _apply(ref.ref_exp, x, np.float64), name)


@pytest.mark.parametrize("name", ["sigmoid", "sigmoid_fast"])
def test_sigmoid_equals_libm(ref, name):
    x = C.cases(name)
    _same(_kat(name), _apply(ref.ref_sigmoid, x, np.float64), name)


def test_exp_main_equals_exp_where_valid(ref):
    x = C.cases("exp_main")
    r = _kat("exp_main")
    ok = r["ok"] != 0
    ax = np.abs(x)
    assert np.array_equal(ok, (ax >= 2.0 ** -54) & (ax < 512.0))  # exp_in_main's documented range (nan: outside)
    assert ok.sum() > (1 << 19)
    _same(r["v"][ok], _apply(ref.ref_exp, x, np.float64)[ok], "exp_main")


def test_expf_glibc_equals_libm(ref):
    x = C.cases("expf_glibc")
    _same(_kat("expf_glibc"), _apply(ref.ref_expf, x, np.float32), "expf_glibc")


def test_torch_expf_equals_oracle_sigmoid(ref, oracle):
    """torch_expf through 1 / (1 + e) against ora_torch_sigmoidf(-x) = 1 / (1 + torch_expf(x)), the
    restatement test_oracle_golden.py pins to torch.sigmoid's vectorised path."""
    x = C.cases("torch_expf")
    f = ctypes.cast(oracle.lib().ora_torch_sigmoidf, ctypes.c_void_p)
    want = _apply(ref.map_f32, -x, np.float32, f)
    with np.errstate(over="ignore", invalid="ignore"):
        got = np.float32(1.0) / (np.float32(1.0) + _kat("torch_expf").view(np.float32))
    _same(got.view(np.uint32), want, "torch_expf")


def test_ts_ctr_of_splits_at_whole_chunks(ref, oracle):
    """ts_ctr_of: items below K & ~31 through torch_expf, the rest through glibc's expf."""
    r = C.cases("ts_ctr_of")
    z = np.ascontiguousarray(r["z"])
    vec = _apply(ref.map_f32, z, np.float32, ctypes.cast(oracle.lib().ora_torch_sigmoidf, ctypes.c_void_p))
    with np.errstate(over="ignore"):
        sca = np.float32(1.0) / (np.float32(1.0) + _apply(ref.ref_expf, -z, np.float32))
    chunk = r["k"] < (r["K"] & ~31)
    assert chunk.any() and (~chunk).any() and (vec.view(np.uint32) != sca.view(np.uint32)).any()
    _same(_kat("ts_ctr_of"), np.where(chunk, vec, sca), "ts_ctr_of")


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_log1p_equals_oracle_restatement(ref, oracle):
    x = C.cases("log1p")
    _same(_kat("log1p"), _apply(ref.map_f64, x, np.float64, ctypes.cast(oracle.lib().ora_log1p_restated, ctypes.c_void_p)),
          "log1p vs ora_log1p_restated")


def _log1p_against_libm(ref):
    x = C.cases("log1p")
    g = _kat("log1p").view(np.float64)
    want = _apply(ref.ref_log1p, x, np.float64)  # libm's log1p: Python's math.log1p
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(g[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert np.array_equal(np.signbit(g[fin]), np.signbit(want[fin]))
    some = np.flatnonzero(fin)[:: max(1, int(fin.sum()) // 2000)]
    assert all(math.log1p(float(x[i])) == float(want[i]) for i in some)
    d = np.zeros(x.shape[0], np.int64)
    d[fin] = _ulps(g[fin], want[fin])
    return x, g, want, d


def test_log1p_within_an_ulp_of_libm(ref):
    """Within 1 ulp of libm's log1p on every input of the case set (on glibc 2.35: 0 inputs differ by
    more, a few hundred of the 1.05e6 by one ulp). With the later BSD copies' branch constant
    0xbfd2bec4 in place of fdlibm's 0xbfd2bec3 this failed at x = -0x1.2bec400000001p-2: the k = 0
    path gave -0x1.62e4420e1ff12p-2 where libm, on the other path, gives -0x1.62e4420e1ff10p-2."""
    x, g, want, d = _log1p_against_libm(ref)
    bad = np.flatnonzero(d > 1)
    print("log1p vs libm: %d of %d differ by one ulp, %d by more" % ((d == 1).sum(), x.shape[0], bad.size))
    for i in bad[:10]:
        print("  x=%s restated=%s libm=%s" % (float(x[i]).hex(), float(g[i]).hex(), float(want[i]).hex()))
    assert bad.size == 0, (bad.size, [float(v).hex() for v in x[bad[:5]]])


def test_log1p_within_an_ulp_of_the_exact_value(ref):
    """Wherever the restated log1p and libm's disagree, the restated result is within 1 ulp of the
    exact value (60-digit decimal arithmetic): the one-ulp disagreements are not the restatement
    drifting. (Where the two agree they share fdlibm's error, which can pass an ulp: 1.83 at x =
    -0x1.2bec400000001p-2.)"""
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    x, g, want, d = _log1p_against_libm(ref)
    for i in np.flatnonzero(d >= 1):
        exact = (Decimal(1) + Decimal(float(x[i]))).ln()
        ulp = Decimal(math.ulp(float(g[i])))
        assert abs(Decimal(float(g[i])) - exact) < ulp, (float(x[i]).hex(), float(g[i]).hex())


def _log1p_main_valid(x):
    """log1p_main's documented range: 2^-29 <= x < 2^53 and not log1p's hu == 0 case (1 + x on a
    power-of-two boundary: the 20 high mantissa bits of 1 + x zero below the 0x6a09e split, or within
    3 of 2^20 above it), which only x >= sqrt(2) - 1 (high word 0x3FDA827A) can reach."""
    hx = (x.view(np.int64) >> 32).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        hu = ((1.0 + x).view(np.int64) >> 32) & 0xfffff
    special = (hx >= 0x3FDA827A) & ((hu == 0) | (hu > 0xffffc))
    return (hx >= 0x3e200000) & (hx < 0x43400000) & ~special


@pytest.mark.parametrize("name", ["log1p_main", "log1p_shared"])
def test_log1p_main_paths_equal_log1p_where_valid(name):
    x = C.cases(name)
    r = _kat(name)
    flags = r["ok"] if name == "log1p_main" else r["flags"]
    ok = (flags & 1) != 0
    assert np.array_equal(ok, _log1p_main_valid(x))
    assert ok.sum() > (1 << 18) and (~ok & (x > 0.42) & (x < 2.0 ** 53)).sum() >= 100  # the hu == 0 cases are there
    _same(r["v"][ok], _kat("log1p").view(np.float64)[ok], name)
    if name == "log1p_shared":  # on the main path both divisions are in the split division's range
        assert ((flags[ok] >> 1) == 3).all()


def test_division_equals_numpy():
    r = C.cases("div")
    got = _kat("div")
    with np.errstate(all="ignore"):
        _same(got["v"], r["a"] / r["b"], "div")
    a, b = np.abs(r["a"]), np.abs(r["b"])
    safe = (((a >= 2.0 ** -900) & (a <= 2.0 ** 600)) | ((r["a"] == 0) & ~np.signbit(r["a"]))) & (b >= 2.0 ** -60) & (b <= 2.0 ** 60)
    assert np.array_equal(got["safe"] != 0, safe) and safe.sum() > (1 << 19) and (~safe).sum() > 1000


@pytest.mark.parametrize("name,scale,biased", [("fxb", 40, True), ("fxb_fast", 40, True), ("fxb_x", 0, True),
                                               ("fx_round_grad", 40, False), ("fx_round_loss", 32, False)])
def test_fixed_point_roundings_equal_rint(name, scale, biased):
    v = C.cases(name)
    want = np.rint(v * 2.0 ** scale).astype(np.int64)
    if biased:
        want = (want.view(np.uint64) + np.uint64(C.K_FX_MAGIC)).view(np.int64)
    got = _kat(name)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad.size, v[bad[:5]], got[bad[:5]], want[bad[:5]])
    x = v * 2.0 ** scale
    ties = (np.abs(x) < 2.0 ** 51) & (x - np.floor(x) == 0.5)
    assert ties.sum() > 100000  # the round-to-even cases are there, even and odd
    assert (np.floor(x[ties]) % 2 == 0).any() and (np.floor(x[ties]) % 2 == 1).any()


def test_polar_transform_equals_numpy(ref, oracle):
    r = C.cases("polar")
    l1p = _apply(ref.map_f64, r["s"] - 1.0, np.float64, ctypes.cast(oracle.lib().ora_log1p_restated, ctypes.c_void_p))
    with np.errstate(all="ignore"):
        want = (r["u"] * np.sqrt(-2.0 * l1p / r["s"])).astype(np.float32).astype(np.float64)
    _same(_kat("polar"), want, "polar")


def test_lr_bce_term_equals_libm(ref):
    r = C.cases("lr_bce")
    want = np.empty(r.shape[0], np.int64)
    p, y = np.ascontiguousarray(r["p"]), np.ascontiguousarray(r["y"])
    ref.ref_bce.restype = None
    ref.ref_bce(ctypes.c_long(r.shape[0]), ctypes.c_void_p(p.ctypes.data), ctypes.c_void_p(y.ctypes.data),
                ctypes.c_void_p(want.ctypes.data))
    got = _kat("lr_bce")
    assert (want == 100 << 32).sum() >= 2  # the clamp acts: p = 0 with y = 1, p = 1 with y = 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, r[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_softplus_fast_and_winrate_row(ref, oracle):
    """softplus_fast(u) = (u > 20 ? u : log1p(exp(u)), exp(u)); the win-rate row at logit z: e =
    exp(-|z|), p = (z >= 0 ? 1 : e) / (1 + e), Lz = log1p(e) -- with libm's exp and the restated log1p."""
    l1p = ctypes.cast(oracle.lib().ora_log1p_restated, ctypes.c_void_p)
    u = C.cases("softplus_fast")
    e = _apply(ref.ref_exp, u, np.float64)
    r = _kat("softplus_fast")
    _same(r["e"], e, "softplus_fast e")
    _same(r["v"], np.where(u > 20.0, u, _apply(ref.map_f64, e, np.float64, l1p)), "softplus_fast")
    z = C.cases("wr_row")
    e = _apply(ref.ref_exp, -np.abs(z), np.float64)
    r = _kat("wr_row")
    _same(r["Lz"], _apply(ref.map_f64, e, np.float64, l1p), "wr_row Lz")
    _same(r["p"], np.where(z >= 0.0, 1.0, e) / (1.0 + e), "wr_row p")


def test_math_kat_refuses_bad_arguments():
    from auctiongym_amd import _lib
    L = _lib.load()
    x = np.zeros(4)
    o = np.zeros(8)
    for fn in (-1, len(_lib.KAT), 1000):
        assert L.ag_math_kat(-1, fn, x.ctypes.data, 4, o.ctypes.data) == _lib.AG_ERR_INVALID
        assert b"fn" in L.ag_last_error()
    assert L.ag_math_kat(-1, 0, None, 4, o.ctypes.data) == _lib.AG_ERR_INVALID
    assert L.ag_math_kat(-1, 0, x.ctypes.data, 4, None) == _lib.AG_ERR_INVALID
    assert L.ag_math_kat(-1, 0, x.ctypes.data, -1, o.ctypes.data) == _lib.AG_ERR_INVALID
    assert L.ag_math_kat(-2, 0, x.ctypes.data, 4, o.ctypes.data) == _lib.AG_ERR_INVALID
    assert L.ag_math_kat(-1, 0, None, 0, None) == _lib.AG_OK
    with pytest.raises(ValueError, match="ag_math_kat"):
        _lib.check(L.ag_math_kat(-1, 0, x.ctypes.data, -1, o.ctypes.data), "ag_math_kat", L)
