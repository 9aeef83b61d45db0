"""The device builds of the small functions every parity claim rests on (ag_math_kat: csrc/ag_exp.h,
ag_log1p.h, ag_div.h, ag_train_math.h, the simulate kernels' torch_expf / ts_ctr_of) against the host
build of the same source, bit for bit, on the inputs of tests/math_kat_cases.py: a dense part over
each function's use range and its edges with their +-4 ulp neighbours (thresholds, branch constants,
round-to-even ties, the table index's half-way points). tests/test_math_kat_host.py pins the host
side to libm, numpy and the oracle, so equality here is equality with those. Needs an MI355X."""
import numpy as np
import pytest

import math_kat_cases as C

pytestmark = pytest.mark.gpu

PLAIN = ["exp", "exp_fast", "sigmoid", "sigmoid_fast", "exp_main", "expf_glibc", "torch_expf", "ts_ctr_of", "log1p",
         "log1p_main", "fxb", "fxb_fast", "fxb_x", "fx_round_grad", "fx_round_loss", "polar", "lr_bce", "softplus_fast",
         "wr_row"]
FLOAT_FIELDS = {"exp": "f8", "exp_fast": "f8", "sigmoid": "f8", "sigmoid_fast": "f8", "expf_glibc": "f4", "torch_expf": "f4",
                "ts_ctr_of": "f4", "log1p": "f8", "polar": "f8"}


def _both(name):
    from auctiongym_amd import _lib
    x = C.cases(name)
    return x, _lib.math_kat(name, x, device=0), _lib.math_kat(name, x, device=-1)


def _differ(dev, host, as_float):
    """Indices whose bits differ, NaNs compared as NaN."""
    ne = dev != host
    if as_float:
        ne &= ~(np.isnan(dev.view(as_float)) & np.isnan(host.view(as_float)))
    return np.flatnonzero(ne)


def test_every_function_is_covered():
    from auctiongym_amd import _lib
    assert set(PLAIN) | {"log1p_shared", "div"} == set(_lib.KAT)
    assert all(C.cases(n).shape[0] >= 1 << 20 for n in _lib.KAT)


@pytest.mark.parametrize("name", PLAIN)
def test_device_equals_host(gpu, name):
    x, dev, host = _both(name)
    if dev.dtype.names:  # a value and its flag, or two values: every field
        for f in dev.dtype.names:
            flag = f in ("ok",)
            bad = _differ(dev[f], host[f], None if flag else "f8")
            assert bad.size == 0, (name, f, bad.size, x[bad[:5]], dev[f][bad[:5]], host[f][bad[:5]])
    else:
        bad = _differ(dev, host, FLOAT_FIELDS.get(name))
        assert bad.size == 0, (name, bad.size, x[bad[:5]], dev[bad[:5]], host[bad[:5]])


def test_split_division_equals_host_division_where_safe(gpu):
    """agdiv::div_core(a, b, recip(b)) on the device against the host's a / b: equal wherever div_safe
    holds -- its boundary exponents, extreme mantissas, a = +0 and the BCE rows' shapes included --
    and div_safe itself equal everywhere."""
    x, dev, host = _both("div")
    assert np.array_equal(dev["safe"], host["safe"])
    safe = host["safe"] != 0
    assert safe.sum() > 1 << 19
    bad = np.flatnonzero(safe & (dev["v"] != host["v"]))
    assert bad.size == 0, (bad.size, x[bad[:5]], dev["v"][bad[:5]], host["v"][bad[:5]])


def test_shared_reciprocal_log1p_equals_host_where_safe(gpu):
    """log1p_main_t<SharedDiv> with r = recip(1 + x): ok and the div_safe flags of its two divisions
    equal the host's; the value equal wherever both divisions are in the split form's range."""
    x, dev, host = _both("log1p_shared")
    assert np.array_equal(dev["flags"], host["flags"])
    safe = (host["flags"] >> 1) == 3
    assert ((host["flags"] & 1) != 0).sum() > 1 << 18 and safe.sum() > 1 << 19
    bad = safe & (dev["v"] != host["v"]) & ~(np.isnan(dev["v"].view("f8")) & np.isnan(host["v"].view("f8")))
    bad = np.flatnonzero(bad)
    assert bad.size == 0, (bad.size, x[bad[:5]], dev["v"][bad[:5]], host["v"][bad[:5]])


def test_math_kat_refuses_bad_arguments_on_the_device(gpu):
    from auctiongym_amd import _lib
    L = _lib.load()
    x, o = np.zeros(4), np.zeros(8)
    assert L.ag_math_kat(0, len(_lib.KAT), x.ctypes.data, 4, o.ctypes.data) == _lib.AG_ERR_INVALID
    assert L.ag_math_kat(0, 0, None, 4, o.ctypes.data) == _lib.AG_ERR_INVALID
    assert L.ag_math_kat(0, 0, x.ctypes.data, -1, o.ctypes.data) == _lib.AG_ERR_INVALID
    assert L.ag_math_kat(0, 0, None, 0, None) == _lib.AG_OK
