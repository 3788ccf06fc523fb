"""GPU: the range-stated float operations of fealess_amd/csrc/fl_ranged_math.h against the compiler's own sqrtf(x), 1.0f / x and
n / d -- the correctly rounded operations the quantisers used before -- over EVERY argument of each stated domain
(fl_dev_ranged_math: both sides are compiled in one kernel of fl_frontend.hip, with the library's flags).  Any result that
differs in any bit is a mismatch; none is expected."""
import ctypes as C

import pytest

from fealess_amd import _lib as L

pytestmark = pytest.mark.gpu

SQRT, RCP, DIV = 0, 1, 2
PIECE = 1 << 29                    # arguments per launch: a fraction of a second each


def _bits(exponent):
    """bit pattern of the float 2^exponent"""
    return (127 + exponent) << 23


def _sweep(ctx, which, first, last):
    fn = L.dev(ctx.lib, "fl_dev_ranged_math")
    total, first_bad, walked = 0, None, 0
    a = first
    while a <= last:
        b = min(a + PIECE - 1, last)
        n, bad = C.c_ulonglong(0), C.c_uint32(0)
        ctx.check(fn(ctx.h, which, a, b, C.byref(n), C.byref(bad)))
        total += n.value
        walked += b - a + 1
        if n.value and first_bad is None:
            first_bad = bad.value
        else:
            assert n.value or bad.value == 0xFFFFFFFF
        a = b + 1
    print(f"which {which}: {walked} arguments, {total} mismatches, first at {first_bad if first_bad is None else hex(first_bad)}")
    return walked, total, first_bad


def test_sqrt_rn_every_float_of_its_domain(ctx):
    """sqrt_rn on [2^-96, FLT_MAX]: 0x70000000 floats."""
    walked, bad, where = _sweep(ctx, SQRT, _bits(-96), 0x7F7FFFFF)
    assert walked == 0x70000000
    assert bad == 0, (bad, hex(where))


def test_rcp_rn_every_float_of_its_domain(ctx):
    """rcp_rn on [1, 2^64]: 0x20000001 floats."""
    walked, bad, where = _sweep(ctx, RCP, _bits(0), _bits(64))
    assert walked == 0x20000001
    assert bad == 0, (bad, hex(where))


def test_div_rn_every_pair_of_sobel_sums(ctx):
    """div_rn on every pair the colour quantiser's arctangent can form: |dx|, |dy| in 0 .. 1020, the smaller over the larger
    plus the epsilon, as fast_atan2_deg forms them (argument a = |dy| * 1021 + |dx|)."""
    walked, bad, where = _sweep(ctx, DIV, 0, 1021 * 1021 - 1)
    assert walked == 1021 * 1021
    assert bad == 0, (bad, where)


def test_ranged_math_refuses_what_it_cannot_walk(ctx):
    fn = L.dev(ctx.lib, "fl_dev_ranged_math")
    n, bad = C.c_ulonglong(0), C.c_uint32(0)
    assert fn(ctx.h, 3, 0, 1, C.byref(n), C.byref(bad)) == L.FL_ERR_INVALID
    assert fn(ctx.h, SQRT, 2, 1, C.byref(n), C.byref(bad)) == L.FL_ERR_INVALID
    assert fn(ctx.h, DIV, 0, 1021 * 1021, C.byref(n), C.byref(bad)) == L.FL_ERR_INVALID
