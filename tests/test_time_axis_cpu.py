"""The time axis without a GPU: the C oracle against the big-integer reference (tests/time_axis_ref.py) over the whole
matrix of slice sizes, time bases and offsets, and Phase P's 32-bit slice division restated for the host with the
constants jm::fast_slice_make builds for the engine (flink_amd/csrc/java_math.h)."""
import ctypes
import os
import random
import subprocess

import pytest

import time_axis_ref as R
from flink_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4000                           # records per case: the Python side dominates the time

PROBE = r'''
#include <stdint.h>
#include "java_math.h"
extern "C" {
int t_fast_make(int64_t g, int64_t table, uint64_t* m, int32_t* sh, uint64_t* lim) {
    const jm::FastSlice f = jm::fast_slice_make(g, table);
    *m = f.m; *sh = f.sh; *lim = f.lim;
    return f.m != 0;
}
// partition3_kernel's line: rel = (dd * fast_m) >> fast_sh, in uint64_t
void t_fast_apply(int64_t g, int64_t table, const uint64_t* dd, int64_t n, uint64_t* out) {
    const jm::FastSlice f = jm::fast_slice_make(g, table);
    for (int64_t i = 0; i < n; ++i) out[i] = (dd[i] * f.m) >> f.sh;
}
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("time_axis")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    so = d / "probe.so"
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "flink_amd", "csrc"),
                           str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    L.t_fast_make.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64),
                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
    L.t_fast_make.restype = ctypes.c_int
    L.t_fast_apply.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.t_fast_apply.restype = None
    return L


def oracle_rows(cfg, k, ts, v):
    from oracle.oracle import Oracle
    o = Oracle(cfg)
    try:
        assert o.push(k, ts, [v]) == 0
        return o.advance_watermark(A.LONG_MAX)
    finally:
        o.close()


def case_seed(*parts):
    return random.Random(repr(parts)).randrange(1 << 32)


@pytest.mark.parametrize("size", R.SIZES)
def test_oracle_tumble_equals_big_integers(size):
    for base in R.BASES:
        for off in sorted(set(R.offsets(size))):
            k, ts, v = R.build_stream(base, off, size, N, case_seed("tumble", size, base, off))
            cfg = A.make_config(window_kind="TUMBLE", size_ms=size, offset_ms=off, aggs=[("COUNT", 0), ("SUM_I64", 0)])
            got = R.rows_as_dict(oracle_rows(cfg, k, ts, v), size)
            want = R.tumble_rows(k.tolist(), ts.tolist(), v.tolist(), off, size)
            assert len(want) > 1000
            assert len({s for _, s in want}) == 7, "the stream misses a slice"
            assert got == want, (size, base, off)


@pytest.mark.parametrize("size,slide", R.SLIDES)
def test_oracle_slide_equals_big_integers(size, slide):
    g = R.slide_slice(size, slide)
    for base in R.BASES:
        for off in sorted({0, -(g // 3), g - 1, slide - 1}):
            k, ts, v = R.build_stream(base, off, g, N, case_seed("slide", size, slide, base, off))
            cfg = A.make_config(window_kind="SLIDE", size_ms=size, slide_ms=slide, offset_ms=off,
                                aggs=[("COUNT", 0), ("SUM_I64", 0)])
            got = R.rows_as_dict(oracle_rows(cfg, k, ts, v), size)
            want = R.slide_rows(k.tolist(), ts.tolist(), v.tolist(), off, size, slide)
            assert len(want) > 1000
            assert got == want, (size, slide, base, off)


def test_reference_floor_division_on_negatives():
    """The reference itself, at the points the device copies get wrong when their fix-up is off by one."""
    assert R.slice_number(-1, 0, 7) == -1 and R.slice_number(-7, 0, 7) == -1 and R.slice_number(-8, 0, 7) == -2
    assert R.slice_number(0, 0, 7) == 0 and R.slice_number(6, 0, 7) == 0 and R.slice_number(-14, 0, 7) == -2
    assert R.window_start(-1, 0, 7) == -7 and R.window_start(-7, 0, 7) == -7 and R.window_start(-8, 0, 7) == -14
    assert R.window_start(5, -2, 7) == 5 and R.window_start(4, -2, 7) == -2 and R.window_start(-3, -2, 7) == -9
    assert R.wrap64((1 << 63) + 5) == -(1 << 63) + 5 and R.wrap64(-(1 << 63) - 1) == (1 << 63) - 1
    assert R.fast_form_expected(1_048_575, (1 << 40) - 1, False)
    assert not R.fast_form_expected(1_048_575, 1 << 40, False) and not R.fast_form_expected(1_048_575, -(1 << 40), False)
    assert not R.fast_form_expected(1_048_576, 0, False) and not R.fast_form_expected(1000, 0, True)


def fast_sizes():
    rng = random.Random(11)
    listed = [g for g in R.SIZES if g * R.REL_CAP < 1 << 32]
    assert listed == [1, 3, 7, 700, 1000, 60_000, 524_288, 524_289, 600_000, 900_000, 1_048_575]
    return listed + [786_433, 999_983] + [rng.randrange(1, 1 << 20) for _ in range(300)]


def test_fast_form_is_exact_at_every_slice_border(probe):
    """(dd * m) >> sh == dd // g on both sides of every border of the relative table, for every dd the kernel's guard
    dd < g * 4096 lets through, and the 64-bit product never wraps."""
    import numpy as np
    m, sh, lim = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_uint64()
    for g in fast_sizes():
        assert probe.t_fast_make(g, R.REL_CAP, ctypes.byref(m), ctypes.byref(sh), ctypes.byref(lim)) == 1, g
        assert lim.value == g * R.REL_CAP and m.value > 0
        L = (g - 1).bit_length()                                  # ceil(log2 g)
        assert sh.value == 32 + L and m.value == -(-(1 << sh.value) // g), g
        dds = sorted({dd for k in range(1, R.REL_CAP + 1) for dd in (k * g - g, k * g - 1, k * g) if dd < lim.value})
        assert dds[-1] == lim.value - 1
        assert max(dds) * m.value < 1 << 64, g                    # the full product, in Python integers
        a = np.array(dds, dtype=np.uint64)
        out = np.empty_like(a)
        probe.t_fast_apply(g, R.REL_CAP, a.ctypes.data, len(a), out.ctypes.data)
        assert out.tolist() == [dd // g for dd in dds], g


def test_fast_form_not_armed_from_2_to_the_20(probe):
    m, sh, lim = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_uint64()
    for g in (1_048_576, 1_048_577, 3_600_000, 86_400_000, 604_800_000, 1 << 62, 0, -5):
        assert probe.t_fast_make(g, R.REL_CAP, ctypes.byref(m), ctypes.byref(sh), ctypes.byref(lim)) == 0, g
        assert m.value == 0 and lim.value == 0
    assert probe.t_fast_make(1_048_575, R.REL_CAP, ctypes.byref(m), ctypes.byref(sh), ctypes.byref(lim)) == 1
