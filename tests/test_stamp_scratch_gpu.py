"""The chaining DP's "visited in this iteration" stamps (lchain.c's t[]) live in one int32
scratch per context (hymet_ctx::stamp): zero whenever no chaining kernel of the context runs,
zero-filled only when it grows, released by hymet_scratch_trim.  hymet_mm_chain_dp takes its
stamps from there like the mapper, so the tests go through it, f and p against the oracle's
mg_lchain_rmq, with hymet_mm_stamp_scratch reporting no non-zero word after every call.

Inputs are one group of anchors dense enough that the inner walk's stamps decide the result:
tp = sort(integers(0, S, n)), qp = integers(0, S, n), default_rng(3).
  LIST      n = 2000, S = 20000: ~100 anchors per 1,000-bp inner window, the in-LDS list walk;
  OVERFLOW  n = 1500, S = 2250:  ~670, above the 256-entry list, the overflow walk.
Each at max_chn_skip 0, 1, 25 and 1 << 30 for both passes (bw 1,000 and 100,000).  On the
oracle, against the unlimited skip, f differs in 995 / 223 anchors of LIST at skip 0 / 1 and
in 1129 / 952 of OVERFLOW, and in 4 anchors of OVERFLOW at skip 25 (first pass): a build that
ignores the stamps cannot pass, and the tests assert that skip 1 and skip 1 << 30 disagree.
"""
import ctypes

import numpy as np
import pytest

from tests._anchors import PEN_GAP, assemble, pack

pytestmark = pytest.mark.gpu

HYMET_E_ARG = -2
U = np.uint64
PASSES = {"first": (10000, 1000, 1000), "long": (10000, 1000, 100000)}
SKIPS = (0, 1, 25, 1 << 30)
SHAPES = {"list": (2000, 20000), "overflow": (1500, 2250)}


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def one_group(n, S):
    rng = np.random.default_rng(3)
    tp = np.sort(rng.integers(0, S, n))
    qp = rng.integers(0, S, n)
    return assemble([pack(tp, qp)])


@pytest.fixture(scope="module")
def ref():
    """{shape: (x, y, {(pass, skip): (f, p)})} from the CPU oracle, computed once."""
    from oracle import oracle_lib
    out = {}
    for name, (n, S) in SHAPES.items():
        x, y = one_group(n, S)
        a = np.stack([x, y], axis=1)
        res = {(ps, sk): oracle_lib.mm_debug_chain(a, md, inner, bw, sk, 100000, float(PEN_GAP), 0.0)
               for ps, (md, inner, bw) in PASSES.items() for sk in SKIPS}
        out[name] = (x, y, res)
    return out


def chain_dp(g, x, y, ps, skip):
    md, inner, bw = PASSES[ps]
    n = len(x)
    f, p = np.zeros(n, np.int32), np.zeros(n, np.int64)
    rc = g.lib.hymet_mm_chain_dp(g.ctx, vp(x), vp(y), n, md, inner, bw, skip, 100000, ctypes.c_float(PEN_GAP),
                                 ctypes.c_float(0.0), vp(f), vp(p))
    return rc, f, p


def scratch(g):
    cap, nz = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = g.lib.hymet_mm_stamp_scratch(g.ctx, ctypes.byref(cap), ctypes.byref(nz))
    assert rc == 0, g.lib.hymet_last_error()
    return cap.value, nz.value


def check_shape(g, ref, name):
    """Every (pass, skip) of one shape: f and p equal to the oracle's, the scratch left zeroed
    and large enough, after every call."""
    x, y, res = ref[name]
    for (ps, sk), (fo, po) in res.items():
        rc, f, p = chain_dp(g, x, y, ps, sk)
        assert rc == 0, g.lib.hymet_last_error()
        cap, nz = scratch(g)
        print(f"{name} {ps} skip {sk}: f mismatches {int((f != fo).sum())}, p mismatches {int((p != po).sum())}, "
              f"capacity {cap}, nonzero {nz}")
        np.testing.assert_array_equal(f, fo, err_msg=f"{name} {ps} skip {sk}")
        np.testing.assert_array_equal(p, po, err_msg=f"{name} {ps} skip {sk}")
        assert nz == 0 and cap >= len(x)
    return scratch(g)[0]


def test_oracle_stamps_decide(ref):
    """The reference side: the stamps change f on both shapes, so ignoring them cannot pass."""
    for name, (x, y, res) in ref.items():
        for ps in PASSES:
            d = {sk: int((res[(ps, sk)][0] != res[(ps, 1 << 30)][0]).sum()) for sk in SKIPS}
            print(name, ps, d)
            assert d[1] > 0 and d[0] > 0, (name, ps, d)
    x, y, res = ref["overflow"]
    assert (res[("first", 25)][0] != res[("first", 1 << 30)][0]).any()


def test_stamp_scratch_lifecycle(ref):
    from hymet_amd._lib import Gpu
    a, b = Gpu(0), Gpu(0)
    try:
        for g in (a, b):
            assert scratch(g) == (0, 0)                    # before first use
        # smaller set first, then the scratch grows, then the smaller set at the older capacity
        c1 = check_shape(a, ref, "overflow")
        assert scratch(b) == (0, 0)                        # the scratch is the context's own
        c2 = check_shape(a, ref, "list")
        assert c2 >= 2000 and c2 >= c1
        assert check_shape(a, ref, "overflow") == c2       # never shrinks, never refilled
        # a rejected call (y of two spans) launches nothing and leaves the scratch as it was
        x, y, res = ref["list"]
        y2 = y.copy()
        y2[len(y) // 2] = U(19) << U(32) | (y2[len(y) // 2] & U(0xffffffff))
        rc, f, p = chain_dp(a, x, y2, "first", 25)
        assert rc == HYMET_E_ARG and b"span" in a.lib.hymet_last_error()
        assert not f.any() and not p.any()
        assert scratch(a) == (c2, 0)
        rc, f, p = chain_dp(a, x, y, "first", 25)
        assert rc == 0, a.lib.hymet_last_error()
        np.testing.assert_array_equal(f, res[("first", 25)][0])
        np.testing.assert_array_equal(p, res[("first", 25)][1])
        assert scratch(a) == (c2, 0)
        # a second context beside the first, calls interleaved: each keeps its own scratch
        for name in ("overflow", "list", "overflow"):
            xs, ys, rs = ref[name]
            for g in (b, a):
                for ps, sk in (("first", 1), ("long", 0)):
                    rc, f, p = chain_dp(g, xs, ys, ps, sk)
                    assert rc == 0, g.lib.hymet_last_error()
                    np.testing.assert_array_equal(f, rs[(ps, sk)][0], err_msg=f"{name} {ps} {sk}")
                    np.testing.assert_array_equal(p, rs[(ps, sk)][1], err_msg=f"{name} {ps} {sk}")
                    cap, nz = scratch(g)
                    assert nz == 0 and cap >= len(xs)
        rc, f, p = chain_dp(b, x, y2, "long", 1)
        assert rc == HYMET_E_ARG
        rc, f, p = chain_dp(b, x, y, "long", 1)
        assert rc == 0, b.lib.hymet_last_error()
        np.testing.assert_array_equal(f, res[("long", 1)][0])
        np.testing.assert_array_equal(p, res[("long", 1)][1])
        assert scratch(b)[1] == 0
        # trim releases the context's scratch; the next call grows and zero-fills it again
        a.trim()
        assert scratch(a) == (0, 0)
        assert scratch(b)[0] > 0                           # b's stays: trim released a's alone
        xs, ys, rs = ref["overflow"]
        rc, f, p = chain_dp(a, xs, ys, "first", 1)
        assert rc == 0, a.lib.hymet_last_error()
        np.testing.assert_array_equal(f, rs[("first", 1)][0])
        np.testing.assert_array_equal(p, rs[("first", 1)][1])
        cap, nz = scratch(a)
        assert cap >= len(xs) and nz == 0
        check_shape(b, ref, "overflow")                    # after the device-wide trim, b still right
    finally:
        a.close()
        b.close()
