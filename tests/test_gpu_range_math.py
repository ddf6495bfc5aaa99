"""GPU (-m gpu): the range-proved fp64 square root and division of the lean resident loops (cice_amd/csrc/evp_range_math.h:
sqrt_core, div_core -- the compiler's expansions without their range handling) against the compiler's sqrt and / on the same
device, bit for bit wherever the window test the kernels use says "inside", over a sweep built to sit on the window's edges; and
the window test itself against its definition restated in numpy: zero, -0, denormals, inf, NaN, negative radicands and every
magnitude outside [2^-250, 2^250) must read "outside".

The sweep (build_sweep, 4 234 127 elements; tests/test_range_math_sweep_cpu.py checks its make-up without a GPU):
  A  every exponent from the lower edge - 4 to the upper edge + 4, 2048 mantissas each (the first two all zeros and all ones, the
     rest random); the division's operands at the same index: numerator of that exponent, denominator of a random one, random signs
  B  division on a grid of exponent pairs: the nine exponents around each edge and every tenth in between, all pairs (so the four
     corners and the four edges of the window are there), 640 mantissa pairs each, the first four the all-zeros / all-ones pairs
  C  exact results: x = g^2 and n = q * d with 26-bit g, q, d
  D  quotients as close to half-way as fp64 operands allow (a quotient of two fp64 numbers is never exactly half-way between two
     fp64 numbers): 53-bit integers n, d with n * 2^53 = d * Y +- 1, Y odd -- n / d lies 2^-105 (relative) off a midpoint
  E  special operands: +-0, denormals, inf, NaN, negative values, values next to the window's edges
Share of the sweep inside the window: square root 91.4 %, division 83.1 % (asserted >= 50 % below, printed by the test)."""
import functools

import numpy as np
import pytest

from cice_amd import evp

WIN = 250                         # the window: 2^-WIN <= |x| < 2^WIN  (evp_range_math.h: WIN_EXP)
LO, HI = np.ldexp(1.0, -WIN), np.ldexp(1.0, WIN)
ONES = (1 << 52) - 1


def _mk(sign, exp, mant):
    """fp64 from sign (0 / 1), unbiased exponent and 52-bit mantissa arrays."""
    bits = (np.asarray(sign, np.uint64) << np.uint64(63)) | ((np.asarray(exp, np.int64) + 1023).astype(np.uint64) << np.uint64(52)) | np.asarray(mant, np.uint64)
    return bits.view(np.float64)


def inside(a):
    """The window by its definition (magnitude; NaN, inf, 0 and denormals fall outside by comparison)."""
    m = np.abs(a)
    with np.errstate(invalid="ignore"):
        return (m >= LO) & (m < HI)


@functools.lru_cache(maxsize=None)
def build_sweep():
    rng = np.random.default_rng(20261019)
    X, N, D = [], [], []
    # A
    exps = np.arange(-WIN - 4, WIN + 4)
    k = 2048
    e = np.repeat(exps, k)
    mant = rng.integers(0, 1 << 52, size=e.size, dtype=np.uint64)
    mant[0::k] = 0
    mant[1::k] = ONES
    x = _mk(0, e, mant)
    X.append(x)
    N.append(_mk(rng.integers(0, 2, e.size), e, mant))
    D.append(_mk(rng.integers(0, 2, e.size), rng.choice(exps, e.size), rng.integers(0, 1 << 52, size=e.size, dtype=np.uint64)))
    # B
    grid = np.array(sorted(set(range(-WIN - 4, -WIN + 5)) | set(range(-WIN, WIN, 10)) | set(range(WIN - 5, WIN + 4))))
    en, ed = (g.ravel() for g in np.meshgrid(grid, grid, indexing="ij"))
    k = 640
    en, ed = np.repeat(en, k), np.repeat(ed, k)
    mn = rng.integers(0, 1 << 52, size=en.size, dtype=np.uint64)
    md = rng.integers(0, 1 << 52, size=en.size, dtype=np.uint64)
    for j, (a, b) in enumerate(((0, 0), (0, ONES), (ONES, 0), (ONES, ONES))):
        mn[j::k] = a
        md[j::k] = b
    N.append(_mk(rng.integers(0, 2, en.size), en, mn))
    D.append(_mk(rng.integers(0, 2, en.size), ed, md))
    X.append(_mk(0, en, mn))
    # C
    n = 1 << 18
    small = lambda: (rng.integers(1 << 25, 1 << 26, size=n).astype(np.float64) * np.ldexp(1.0, -25))      # [1, 2), 26 bits
    g, q, d = small(), small(), small()
    eg = rng.integers(-(WIN + 4) // 2, (WIN + 4) // 2, size=n)
    eq, edd = rng.integers(-120, 120, size=n), rng.integers(-WIN - 4, WIN + 4, size=n)
    g = np.ldexp(g, eg)
    X.append(g * g)
    dd = np.ldexp(d, edd) * rng.choice([-1.0, 1.0], n)
    qq = np.ldexp(q, eq) * rng.choice([-1.0, 1.0], n)
    N.append(qq * dd)               # exact: 26 x 26 bits
    D.append(dd)
    # D
    n = 1 << 15
    nn, dn = [], []
    ds = rng.integers(1 << 52, 1 << 53, size=4 * n) | 1
    for r in (1, -1):
        got = 0
        for dv in ds[(0 if r == 1 else 2 * n):]:
            dv = int(dv)
            y = ((-r * pow(dv, -1, 1 << 53)) % (1 << 53)) + (1 << 53)
            num = (dv * y + r) >> 53
            if (1 << 52) <= num < (1 << 53):
                assert num << 53 == dv * y + r
                nn.append(num); dn.append(dv); got += 1
                if got == n:
                    break
    nn, dn = np.array(nn, dtype=np.float64), np.array(dn, dtype=np.float64)
    sh_n, sh_d = rng.integers(-WIN - 56, WIN - 48, size=nn.size), rng.integers(-WIN - 56, WIN - 48, size=nn.size)
    N.append(np.ldexp(nn, sh_n) * rng.choice([-1.0, 1.0], nn.size))
    D.append(np.ldexp(dn, sh_d))
    X.append(np.ldexp(nn, 2 * (sh_n // 2)))
    # E
    den_min, den_max = np.float64(5e-324), _mk(0, -1023, ONES)      # smallest / largest denormal
    below, above = np.nextafter(LO, 0.0), np.nextafter(HI, 0.0)
    sp = np.array([0.0, -0.0, den_min, -den_min, den_max, -den_max, np.inf, -np.inf, np.nan, -1.0, -LO, LO, below, -below, HI, -HI, above, -above,
                   1.0, np.finfo(np.float64).tiny, np.finfo(np.float64).max, 2.0 ** -767, 2.0 ** -768, 2.0 ** 600, -2.0 ** -600])
    a, b = (g.ravel() for g in np.meshgrid(sp, sp, indexing="ij"))
    X.append(a); N.append(a); D.append(b)
    x, num, den = (np.concatenate(v) for v in (X, N, D))
    for v in (x, num, den):
        v.setflags(write=False)
    return x, num, den


@functools.lru_cache(maxsize=None)
def _results():
    return evp.range_math(*build_sweep())


pytestmark = pytest.mark.gpu


def test_window_verdicts_match_the_definition():
    x, num, den = build_sweep()
    r = _results()
    want_x = inside(x) & (x > 0)
    want_q = inside(num) & inside(den)
    assert np.array_equal(r["x_inside"], want_x), np.flatnonzero(r["x_inside"] != want_x)[:8]
    assert np.array_equal(r["q_inside"], want_q), np.flatnonzero(r["q_inside"] != want_q)[:8]
    # every special value reads "outside", wherever it sits in the sweep
    with np.errstate(invalid="ignore"):
        odd_x = ~np.isfinite(x) | (x <= 0) | (np.abs(x) < np.finfo(np.float64).tiny)
        odd_q = ~np.isfinite(num) | ~np.isfinite(den) | (np.abs(num) < np.finfo(np.float64).tiny) | (np.abs(den) < np.finfo(np.float64).tiny)
    assert odd_x.sum() > 20 and odd_q.sum() > 200
    assert not r["x_inside"][odd_x].any() and not r["q_inside"][odd_q].any()


def test_cores_equal_the_compilers_forms_inside_the_window():
    x, num, den = build_sweep()
    r = _results()
    xi, qi = r["x_inside"], r["q_inside"]
    share_x, share_q = xi.mean(), qi.mean()
    print(f"inside the window: square root {100 * share_x:.1f} % of {x.size}, division {100 * share_q:.1f} %")
    assert share_x >= 0.5 and share_q >= 0.5          # the comparison cannot pass by excluding everything
    bits = lambda a: a.view(np.uint64)
    bad = np.flatnonzero(xi & (bits(r["sqrt_core"]) != bits(r["sqrt_lib"])))
    assert bad.size == 0, (bad.size, [(float.hex(float(x[j])), float.hex(float(r["sqrt_core"][j])), float.hex(float(r["sqrt_lib"][j]))) for j in bad[:4]])
    bad = np.flatnonzero(qi & (bits(r["div_core"]) != bits(r["div_lib"])))
    assert bad.size == 0, (bad.size, [(float.hex(float(num[j])), float.hex(float(den[j])), float.hex(float(r["div_core"][j])), float.hex(float(r["div_lib"][j])))
                                      for j in bad[:4]])
    # ... and both are the correctly rounded results (numpy's, on the CPU)
    assert np.array_equal(bits(r["sqrt_lib"][xi]), bits(np.sqrt(x[xi])))
    assert np.array_equal(bits(r["div_lib"][qi]), bits(num[qi] / den[qi]))
