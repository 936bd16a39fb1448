"""The tolerances of test_gpu_cg_trajectory.py and the proof that they separate
a CG solver that misses one workgroup's partial from one that does not (CPU
only; the restatement is cg_ref.py, the method test_krylov_trajectory.py's).

The GPU test runs rsp_cg_solve for exactly K iterations (rtol = 0) from a
seeded b and a non-zero x0 on the symmetric 5-point grid ((cx, cy) = (0, 0))
and compares every history entry and x with the same iterations restated in
numpy with np.longdouble dots. What separates the two is the order in which a
dot is summed, so the tolerance is 100 x the spread of the restatement under
three fp64 summation orders (forward, reverse, 2048-element blocks in block
order), per case; a spread under one fp64 ulp counts as one ulp. Nothing here
comes from a GPU run.

Measured spreads (s_hist, s_x), and in brackets the smallest displacement
max(dh / tol_hist, dx / tol_x) of a walked single-dot mutation, in tolerances
(at the point the run was ended):

    K = 6   fp64 ILU(0)                fp32 ILU(0)                 none
      S   7.1e-16, 5.3e-16 [5.1e7]   8.5e-16, 7.4e-16 [4.2e7]   4.3e-16, 4.8e-16 [3.0e9]
      L   3.4e-15, 7.1e-16 [1.4e9]   1.4e-11, 1.1e-8  [3.3e5]   2.4e-15, 7.6e-16 [2.7e9]
      S, all fp32   1.3e-16, 0 [1.6e8]
    K = 4
      T   1.6e-15, 3.7e-16 [3.7e4]
    K = 3
      X                                                         8.1e-16, 7.5e-16 [1.1e10]

(In L under the fp32 preconditioner single fp32 roundings of the
preconditioner's input flip with the summation order: the effect
test_krylov_trajectory.py describes for GMRES.)

Mutation walk: every dot of iterations 1-3 ((r,z) with a preconditioner,
(p,q), (r,r)) ignores, in turn, each range of krylov_ref.dropped_ranges(n),
and the longdouble trajectory must leave the reference by at least 10
tolerances in history or x. Every case meets it at the K above; none had to be
changed.
"""
import numpy as np
import pytest

import cg_ref as cr

IDS = [cr.case_id(c) for c in cr.CASES]


def loop_grid(nx, ny, cx, cy):
    """The symmetric grid, entry by entry."""
    rp, ci, va = [0], [], []
    for j in range(ny):
        for i in range(nx):
            k = j * nx + i
            if j > 0:
                ci.append(k - nx), va.append(-1.0 - cy)
            if i > 0:
                ci.append(k - 1), va.append(-1.0 - cx)
            ci.append(k), va.append(4.0 + 2.0 * cx + 2.0 * cy)
            if i < nx - 1:
                ci.append(k + 1), va.append(-1.0 - cx)
            if j < ny - 1:
                ci.append(k + nx), va.append(-1.0 - cy)
            rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64)


@pytest.mark.parametrize("shape,c", [((1, 1), (0.0, 0.0)), ((1, 5), (8.0, 0.5)), ((6, 1), (0.0, 0.0)),
                                     ((7, 5), (8.0, 0.5)), ((37, 29), (0.0, 0.0))])
def test_grid_is_the_loop_grid_and_positive_definite(shape, c):
    g = cr.SymGrid(*shape, *c)
    rp, ci, va = loop_grid(*shape, *c)
    assert g.n == shape[0] * shape[1]
    assert np.array_equal(g.rowptr, rp) and np.array_equal(g.colidx, ci) and np.array_equal(g.values, va)
    a = g.dense()
    assert np.array_equal(a, a.T)
    assert np.linalg.eigvalsh(a)[0] > 0.0


def test_cases_are_the_ones_listed():
    assert [c[:3] for c in cr.CASES] == [("S", "fp64", "f64"), ("S", "fp32", "f64"), ("S", "none", "f64"),
                                         ("S", "fp32", "f32"), ("T", "fp64", "f64"), ("L", "fp64", "f64"),
                                         ("L", "fp32", "f64"), ("L", "none", "f64"), ("X", "none", "f64")]
    assert set(cr.SPREAD) == set(cr.CASES)
    n = {k: cr.grid(k).n for k in cr.SIZES}
    assert n == {"S": 3 * 2048 + 5, "T": 2049, "L": 525312, "X": 2101248}


def test_restatement_dot_order_and_a_solve():
    """Dots per iteration (3 with M, 2 without), and the restatement solves:
    42 iterations to 1e-10 on the 40 x 40 grid under fp64 ILU(0), b = 1, x0 = 0
    (the count test_gpu_cg.py pins for its own reference)."""
    g = cr.SymGrid(40, 40)
    b, x0 = np.ones(g.n), np.zeros(g.n)
    dot = cr.Dot("forward")
    x, hist = cr.cg_trajectory(g, np.float64, np.float64, 42, b, x0, dot)
    assert dot.calls == {0: 2, **{it: 3 for it in range(1, 43)}}
    assert hist[40] > 1e-10 >= hist[41]
    assert np.linalg.norm(b - g.matvec(x)) <= 2e-10 * np.linalg.norm(b)
    dot = cr.Dot("forward")
    cr.cg_trajectory(g, None, np.float64, 3, b, x0, dot)
    assert dot.calls == {0: 2, 1: 2, 2: 2, 3: 2}


@pytest.mark.parametrize("case", cr.CASES, ids=IDS)
def test_spread_stays_under_the_constants(case):
    x_ref, h_ref, _ = cr.reference(case)
    K = case[3]
    assert len(h_ref) == K and np.all(np.isfinite(h_ref)) and np.all(h_ref > 0.0)
    s_hist = s_x = 0.0
    for kind in cr.FP64_ORDERS:
        x, hist, _ = cr.run_case(case, kind)
        dh, dx = cr.deviation(x, hist, x_ref, h_ref)
        s_hist, s_x = max(s_hist, dh), max(s_x, dx)
    c_hist, c_x = cr.SPREAD[case]
    tol = cr.tolerance(case)
    print(f"{cr.case_id(case)}: s_hist {s_hist:.2e} (<= {c_hist:.2e}), s_x {s_x:.2e} (<= {c_x:.2e}); "
          f"GPU tolerance {tol[0]:.2e}, {tol[1]:.2e}")
    assert s_hist <= c_hist and s_x <= c_x
    assert tol == (cr.MARGIN * max(c_hist, cr.EPS), cr.MARGIN * max(c_x, cr.EPS))


@pytest.mark.parametrize("case", cr.CASES, ids=IDS)
def test_a_missed_partial_leaves_the_tolerance(case):
    """Every dot of iterations 1-3, every dropped range: the mutated
    longdouble trajectory is at least SEPARATION tolerances from the reference.
    A run ends at the first history entry that is (the common case)."""
    x_ref, h_ref, calls = cr.reference(case)
    tol_hist, tol_x = cr.tolerance(case)
    ranges = cr.dropped_ranges(cr.grid(case[0]).n)
    dots = cr.walked_dots(calls)
    assert ranges and len(dots) == 3 * (2 if case[1] == "none" else 3)

    def moved(hist):
        i = len(hist) - 1
        return abs(hist[i] - h_ref[i]) >= cr.SEPARATION * tol_hist * h_ref[i]

    smallest = np.inf
    for it, k in dots:
        for name, rng in ranges.items():
            x, hist, dot = cr.run_case(case, "longdouble", (it, k, rng), watch=moved)
            assert dot.hit
            n = len(hist)
            shift = float(np.max(np.abs(hist - h_ref[:n]) / h_ref[:n])) / tol_hist
            if x is not None:
                shift = max(shift, cr.deviation(x, hist, x_ref, h_ref)[1] / tol_x)
            smallest = min(smallest, shift)
            assert shift >= cr.SEPARATION, (it, k, name, shift)
    print(f"{cr.case_id(case)}: {len(dots) * len(ranges)} mutations, the smallest moves the trajectory by "
          f"{smallest:.3g} tolerances (at the point the run was ended)")
