"""rsp_convert_scaled and rsp_refine_update, the element-wise kernels of the
iterative refinement, bit for bit against numpy: np.ldexp is exact short of
fp64's range and astype rounds once to nearest even, which is the contract.

Sizes walk the kernels' paths: below and around a wave (63, 64, 65) and a
workgroup's first pass (255, 256, 257), around one chunk (C - 1, C, C + 1: one
and two workgroups, a 1-element tail), 3 C + 5 (four workgroups, a tail shorter
than a group of four) and (G - 1) C + 777 (the full grid but one, a tail with
whole and partial groups). Every size runs with 16-byte aligned pointers (the
vector path) and with base + 1 element on either side (the element path).

Data: seeded values over 40 binades with a crafted block in front: +-0, +-inf,
NaN, exact fp32 ties (to even, both ways), values that narrow to fp32 denormals
(the largest, the smallest, the tie under it, the tie that rounds up to
FLT_MIN), values that overflow to inf (the tie above FLT_MAX included). NaNs
must stay NaNs; every other element is compared as bits.

Under Handle(ftz=True) the expectation follows the oracle's flush-to-zero
convention (the x86 FTZ + DAZ modes of oracle/rsp_oracle.c): an fp32 denormal
read counts as a zero of its sign, an fp32 result that is denormal after
rounding becomes one; fp64 never flushes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from respasol_amd import _lib
from respasol_amd.sparse import Handle, convert_scaled, refine_update

pytestmark = pytest.mark.gpu

CH, G = _lib.KRY_CHUNK, _lib.KRY_MAX_GRID
SIZES = [1, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 3 * CH + 5, (G - 1) * CH + 777]
EXPS = [0, -40, 37]
NPT = {"f64": np.float64, "f32": np.float32}
TT = {"f64": torch.float64, "f32": torch.float32}
FLT_MIN = np.float32(2.0 ** -126)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def handles():
    hs = {False: Handle(), True: Handle(ftz=True)}
    yield hs
    torch.cuda.synchronize()
    for h in hs.values():
        h.close()


def crafted_targets():
    """fp64 values whose rounding to fp32 is a case of its own."""
    t = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0,
         1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, -(1.0 + 2.0 ** -24),  # ties, and past one
         2.0 ** -126, 2.0 ** -126 - 2.0 ** -150, 2.0 ** -126 - 2.0 ** -151, 2.0 ** -126 - 2.0 ** -149,
         2.0 ** -130, 1.5 * 2.0 ** -140, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -30), 2.0 ** -151,
         -(2.0 ** -126 - 2.0 ** -150), -1.25 * 2.0 ** -133, -(2.0 ** -150), -(2.0 ** -149),
         3.5e38, -3.5e38, 2.0 ** 128 - 2.0 ** 103, 2.0 ** 128 - 2.0 ** 103 - 2.0 ** 80, 2.0 ** 128 - 2.0 ** 104,
         1e300, -1e300, 1e-300]
    return np.array(t, np.float64)


def source(n, src, exp2, seed):
    """n source values: the crafted block, placed so that the scaled value is
    the crafted target (fp64) or the crafted fp32 value itself, then seeded data."""
    rng = np.random.default_rng(seed)
    body = rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-20, 21, n))
    t = crafted_targets()
    if src == "f64":
        with np.errstate(over="ignore", under="ignore"):
            head = np.ldexp(t, -exp2)
    else:
        with np.errstate(over="ignore", under="ignore"):
            head = np.concatenate([t.astype(np.float32).astype(np.float64),
                                   np.ldexp(t, -exp2).astype(np.float32).astype(np.float64)])
    return np.concatenate([head, body])[:n].astype(NPT[src])


def daz(a):
    if a.dtype != np.float32:
        return a
    return np.where(np.abs(a) < FLT_MIN, np.copysign(np.float32(0), a), a)


def expected_convert(src, exp2, dst, ftz):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = daz(src) if ftz else src
        out = np.ldexp(s.astype(np.float64), exp2).astype(NPT[dst])
        return daz(out) if ftz else out


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_same_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero(bits(got)[~nan] != bits(want)[~nan])
    assert bad.size == 0, (what, int(bad[0]), got[~nan][bad[0]], want[~nan][bad[0]])


def placed(values, shift):
    """values in a sentinel-filled buffer, at the (16-byte aligned) base + 4
    elements, or one element further: (buffer, view, offset)."""
    t = torch.from_numpy(values).cuda()
    off = 4 + (1 if shift else 0)
    buf = torch.full((t.numel() + 12,), SENTINEL, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t)
    assert (view.data_ptr() % 16 == 0) == (not shift)
    return buf, view, off


def untouched_around(buf, off, n):
    return bool(torch.all(buf[:off] == SENTINEL)) and bool(torch.all(buf[off + n:] == SENTINEL))


@pytest.mark.parametrize("ftz", [False, True], ids=["ieee", "ftz"])
@pytest.mark.parametrize("exp2", EXPS)
@pytest.mark.parametrize("src,dst", [("f64", "f32"), ("f32", "f64"), ("f64", "f64"), ("f32", "f32")])
def test_convert_scaled_is_ldexp_then_one_rounding(handles, src, dst, exp2, ftz):
    h = handles[ftz]
    counts = {"denormal": 0, "inf": 0, "nan": 0}
    for n in SIZES:
        a = source(n, src, exp2, seed=n)
        want = expected_convert(a, exp2, dst, ftz)
        if dst == "f32" and not ftz:
            counts["denormal"] += int(np.sum((want != 0) & (np.abs(want) < FLT_MIN)))
        counts["inf"] += int(np.sum(np.isinf(want)))
        counts["nan"] += int(np.sum(np.isnan(want)))
        # the large sizes: aligned and both shifted; the small ones: every combination
        shifts = ((0, 0), (1, 1), (1, 0), (0, 1)) if n <= 3 * CH + 5 else ((0, 0), (1, 1))
        for ss, ds in shifts:
            _, sv, _ = placed(a, ss)
            dbuf, dv, off = placed(np.full(n, 3.5, NPT[dst]), ds)
            convert_scaled(h, sv, dv, exp2)
            torch.cuda.synchronize()
            assert untouched_around(dbuf, off, n), (n, ss, ds)
            assert_same_bits(dv.cpu().numpy(), want, (src, dst, exp2, n, ss, ds))
        if src == dst:  # in place
            _, sv, _ = placed(a, 0)
            convert_scaled(h, sv, sv, exp2)
            assert_same_bits(sv.cpu().numpy(), want, ("in place", src, exp2, n))
    # the crafted block did what it is there for
    assert counts["nan"] >= len(SIZES) - 1
    if dst == "f32":
        assert counts["inf"] > 0
        if not ftz and src == "f64":
            assert counts["denormal"] > 0


def test_ftz_flushes_what_ieee_keeps(handles):
    """The two modes differ exactly on fp32 denormals: the crafted block under
    both handles, and the expectation's own two conventions differ there."""
    a = source(64, "f64", 0, seed=1)
    ieee = expected_convert(a, 0, "f32", False)
    flushed = expected_convert(a, 0, "f32", True)
    den = (ieee != 0) & (np.abs(ieee) < FLT_MIN)
    # the crafted block's seven: 2^-126 - 2^-149, 2^-130, 1.5 * 2^-140, 2^-149, 2^-150 (1 + 2^-30), -1.25 * 2^-133, -2^-149
    assert den.sum() >= 7 and np.all(flushed[den] == 0)
    assert np.array_equal(np.signbit(flushed[den]), np.signbit(ieee[den]))
    assert_same_bits(flushed[~den], ieee[~den], "outside the denormals")
    # 2^-126 - 2^-150 rounds up to FLT_MIN before the flush looks: it is kept
    k = int(np.flatnonzero(a == 2.0 ** -126 - 2.0 ** -150)[0])
    assert flushed[k] == FLT_MIN
    src = torch.from_numpy(a).cuda()
    for ftz, want in ((False, ieee), (True, flushed)):
        got = convert_scaled(handles[ftz], src, exp2=0, dtype=torch.float32)
        assert_same_bits(got.cpu().numpy(), want, ("ftz", ftz))


@pytest.mark.parametrize("ftz", [False, True], ids=["ieee", "ftz"])
@pytest.mark.parametrize("exp2", EXPS)
def test_refine_update_adds_once_and_saves_x(handles, exp2, ftz):
    h = handles[ftz]
    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        d = source(n, "f32", 0, seed=n + 7)
        x = rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-10, 11, n) + exp2)
        x[::17] = 0.0
        with np.errstate(over="ignore", invalid="ignore"):
            want = x + np.ldexp((daz(d) if ftz else d).astype(np.float64), exp2)
        shifts = ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)) if n <= 3 * CH + 5 else ((0, 0, 0), (1, 1, 1))
        for sd, sx, so in shifts:
            _, dv, _ = placed(d, sd)
            xbuf, xv, xoff = placed(x, sx)
            obuf, ov, ooff = placed(np.full(n, 9.0), so)
            refine_update(h, dv, xv, exp2, x_old=ov)
            torch.cuda.synchronize()
            assert untouched_around(xbuf, xoff, n) and untouched_around(obuf, ooff, n), (n, sd, sx, so)
            assert_same_bits(xv.cpu().numpy(), want, ("x", exp2, n, sd, sx, so))
            assert np.array_equal(bits(ov.cpu().numpy()), bits(x)), ("x_old", exp2, n, sd, sx, so)
        # x_old = NULL: the same x, nothing saved
        for sd, sx in ((0, 0), (1, 1)):
            _, dv, _ = placed(d, sd)
            _, xv, _ = placed(x, sx)
            refine_update(h, dv, xv, exp2)
            assert_same_bits(xv.cpu().numpy(), want, ("no x_old", exp2, n, sd, sx))


def test_argument_checks_write_nothing(handles):
    h = handles[False]
    n = 300
    src = torch.full((n,), 2.0, dtype=torch.float64, device="cuda")
    dst = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    d32 = torch.full((n,), 1.0, dtype=torch.float32, device="cuda")
    x = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    xo = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    cs, up = _lib.rsp.rsp_convert_scaled, _lib.rsp.rsp_refine_update
    bad_convert = [
        (h.ptr, -1, _lib.R_64F, p(src), 0, _lib.R_32F, p(dst)),
        (h.ptr, n, 2, p(src), 0, _lib.R_32F, p(dst)),
        (h.ptr, n, _lib.R_64F, p(src), 0, -1, p(dst)),
        (h.ptr, n, _lib.R_64F, p(src), 1023, _lib.R_32F, p(dst)),
        (h.ptr, n, _lib.R_64F, p(src), -1023, _lib.R_32F, p(dst)),
        (h.ptr, n, _lib.R_64F, None, 0, _lib.R_32F, p(dst)),
        (h.ptr, n, _lib.R_64F, p(src), 0, _lib.R_32F, None),
        (h.ptr, n, _lib.R_32F, p(dst), 0, _lib.R_64F, p(dst)),  # in place with two types
    ]
    for args in bad_convert:
        assert cs(*args) == _lib.STATUS_INVALID_VALUE, args[1:]
    assert cs(None, n, _lib.R_64F, p(src), 0, _lib.R_32F, p(dst)) == _lib.STATUS_NOT_INITIALIZED
    bad_update = [
        (h.ptr, -1, p(d32), 0, p(x), p(xo)),
        (h.ptr, n, p(d32), 1023, p(x), p(xo)),
        (h.ptr, n, p(d32), -1023, p(x), p(xo)),
        (h.ptr, n, None, 0, p(x), p(xo)),
        (h.ptr, n, p(d32), 0, None, p(xo)),
        (h.ptr, n, p(d32), 0, p(x), p(x)),
    ]
    for args in bad_update:
        assert up(*args) == _lib.STATUS_INVALID_VALUE, args[1:]
    assert up(None, n, p(d32), 0, p(x), p(xo)) == _lib.STATUS_NOT_INITIALIZED
    # n = 0 does nothing, with or without pointers
    assert cs(h.ptr, 0, _lib.R_64F, None, 0, _lib.R_32F, None) == _lib.STATUS_SUCCESS
    assert cs(h.ptr, 0, _lib.R_64F, p(src), 5, _lib.R_32F, p(dst)) == _lib.STATUS_SUCCESS
    assert up(h.ptr, 0, None, 0, None, None) == _lib.STATUS_SUCCESS
    torch.cuda.synchronize()
    for t in (dst, x, xo):
        assert bool(torch.all(t == SENTINEL))
    assert bool(torch.all(src == 2.0)) and bool(torch.all(d32 == 1.0))
