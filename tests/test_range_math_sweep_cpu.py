"""CPU: the make-up of the sweep tests/test_gpu_range_math.py runs on the GPU -- at least half of it inside the window (so the
bit comparison there cannot pass by excluding everything), the window's edges, corners and special operands present."""
import numpy as np

from test_gpu_range_math import HI, LO, WIN, build_sweep, inside


def test_sweep_makeup():
    x, num, den = build_sweep()
    assert x.size == num.size == den.size and abs(x.size - (1 << 22)) < (1 << 17)
    xi = inside(x) & (x > 0)
    qi = inside(num) & inside(den)
    assert xi.mean() >= 0.5 and qi.mean() >= 0.5, (xi.mean(), qi.mean())
    assert abs(xi.mean() - 0.914) < 0.002 and abs(qi.mean() - 0.831) < 0.002, (xi.mean(), qi.mean())      # the docstring's figures
    ex = np.frexp(np.abs(x[np.isfinite(x) & (x != 0)]))[1] - 1
    assert set(range(-WIN - 4, WIN + 4)) <= set(ex.tolist())
    # the four corners of the division's window, and a pair just outside each
    en, ed = np.frexp(np.abs(num))[1] - 1, np.frexp(np.abs(den))[1] - 1
    fin = np.isfinite(num) & np.isfinite(den) & (num != 0) & (den != 0)
    for a in (-WIN, WIN - 1):
        for b in (-WIN, WIN - 1):
            assert (fin & (en == a) & (ed == b) & qi).any(), (a, b)
    for a, b in ((-WIN - 1, -WIN), (WIN, WIN - 1), (-WIN, WIN), (WIN - 1, -WIN - 1)):
        assert (fin & (en == a) & (ed == b) & ~qi).any(), (a, b)
    for v in (0.0, np.inf, LO, HI):
        assert (x == v).any() and (num == v).any() and (den == v).any()
    assert np.isnan(x).any() and np.signbit(x[x == 0]).any()
    # exact quotients and the near-half-way ones are inside the window for the most part
    assert (num[qi] / den[qi] * den[qi] == num[qi]).sum() > (1 << 17)
