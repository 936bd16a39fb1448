"""The tolerances of test_gpu_krylov_trajectory.py and the proof that they
separate a solver that misses one workgroup's partial from one that does not
(CPU only; the restatements are krylov_ref.py).

The GPU test runs each solver for exactly K iterations (rtol = 0) from a seeded
b and a non-zero x0 and compares every history entry and x with the same
iterations restated in numpy with np.longdouble dots. What separates the two is
the order in which a dot is summed, so the tolerance comes from running the
restatement with three fp64 summation orders (forward, reverse, 2048-element
blocks in block order):

    s_hist  the largest relative deviation of a history entry from the
            longdouble trajectory over the three orders
    s_x     max|x - x_ld| / max|x_ld| over the same runs

and is 100 x the largest spread over the cases of the same solver, size and
preconditioner class (the device's order is a fourth one, and three samples
under-estimate a spread). A spread under one fp64 ulp counts as one ulp.
Nothing here comes from a GPU run.

Sizes (5-point grid, (cx, cy) = (2, 1)): S 143 x 43 (n = 6149 = 3 * 2048 + 5),
T 683 x 3 (2049), L 1024 x 513 (525 312: 257 workgroups), X 2048 x 1026
(2 101 248: 513 workgroups of 4096). BiCGStab K = 4; GMRES restart 3 / K = 5
and restart 30 / K = 10. Preconditioner: fp64 ILU(0), fp32 ILU(0) or none under
an fp64 iteration, and the all-fp32 iteration on S.

Measured spreads (s_hist, s_x), and in brackets the smallest displacement
max(dh / tol_hist, dx / tol_x) of a walked single-dot mutation, in tolerances:

    BiCGStab, K = 4    fp64                       fp32 preconditioner        none
      S   4.6e-14, 1.4e-14 [1.8e6]   7.4e-14, 2.3e-14 [1.2e6]   1.8e-16, 8.7e-16 [1.1e7]
      T   8.1e-13, 5.3e-16 [20]
      L   5.9e-16, 1.3e-15 [1.6e8]   2.6e-14, 9.6e-15 [2.0e7]   5.1e-16, 7.0e-16 [6.4e8]
      X                                                         8.2e-16, 7.8e-16 [1.4e9]
      S, all fp32   1.6e-16, 0 [8.7e8]
    GMRES, restart 3, K = 5
      S   3.1e-16, 3.6e-16 [2.4e7]   3.3e-16, 3.6e-16 [3.7e7]   1.2e-16, 2.7e-16 [5.3e6]
      T   1.2e-14, 2.4e-16 [381]
      L   6.7e-16, 6.3e-16 [5.5e6]   7.4e-16, 4.7e-16 [3198]    7.1e-16, 4.9e-16 [2.0e7]
      X                                                         7.1e-16, 6.1e-16 [6.4e5]
      S, all fp32   2.5e-16, 0 [5.1e7]
    GMRES, restart 30, K = 10
      S   1.2e-15, 7.1e-16 [1.8e7]   8.3e-16, 7.1e-16 [2.7e7]   2.3e-16, 8.6e-16 [1.5e7]
      T   6.9e-11, 2.4e-16 [37]
      L   6.7e-16, 9.5e-16 [5.5e6]   1.9e-12, 3.2e-9 [3198]     1.0e-15, 1.4e-15 [4.7e7]
      X                                                         7.5e-16, 1.5e-15 [2.3e6]
      S, all fp32   7.5e-16, 0 [3.1e7]

(T is nearly tridiagonal, so ILU(0) is nearly exact and the residual falls by
five per iteration: its late history entries are small numbers with a large
relative spread. An fp32 preconditioner rounds its input to fp32, and an input
that moved by an fp64 ulp now and then rounds the other way: the 3.2e-9.)

Resulting GPU tolerances (tol_hist, tol_x) = 100 x krylov_ref.SPREAD:

    BiCGStab   S fp64/none 4.7e-12, 1.5e-12   S fp32 7.4e-12, 2.4e-12   S all fp32 2.2e-14, 2.2e-14
               T fp64 8.2e-11, 5.4e-14        L fp64/none 6.0e-14, 1.4e-13
               L fp32 2.7e-12, 9.7e-13        X none 8.3e-14, 7.9e-14
    GMRES      S fp64/none 1.3e-13, 8.7e-14   S fp32 8.4e-14, 7.2e-14   S all fp32 7.5e-14, 2.2e-14
               T fp64 7.0e-9, 2.4e-14         L fp64/none 1.1e-13, 1.5e-13
               L fp32 1.9e-10, 3.3e-7         X none 7.6e-14, 1.5e-13

Mutation walk: every dot of iterations 1-3 ignores, in turn, workgroup 1's
range, the last partly filled workgroup's and workgroup 256's (those that
exist at the size), and the longdouble trajectory must leave the reference by
at least 10 tolerances in history or x. Every case meets it; none had to be
dropped or shortened. One group of dots is outside the walk: GMRES's first
Gram-Schmidt pass. Its coefficients are corrected by the second pass (h = h +
h', w is orthogonalised again), so dropping a range from one of them moves the
trajectory by rounding only (measured: no more than the case's own spread, or
single fp32 roundings in the all-fp32 iteration) and no trajectory test can
see it. The second pass's dots, the norm and the residual's are walked.

The first pass is proved on its own instead (krylov_ref.ortho_*): the same
three kernels through rsp_orthogonalize on V = 2 Q, where V^T V = 4 I keeps the
second pass from repairing the first, so a first-pass coefficient short by
delta shifts the returned h + h' by -3 delta. Tolerance and separation are
computed the same way (100 x the spread of the three orders; every first-pass
dot, every dropped range, >= 10 tolerances): measured tolerance 3.3e-14 (n =
6149, 3 columns, fp64), 4.1e-14 (10 columns), 2.2e-14 (fp32: one ulp, no
rounding flipped), 6.2e-14 (n = 525 312); the smallest mutation is 2.7e9
tolerances away.
"""
import numpy as np
import pytest

import krylov_ref as kr

IDS = [kr.case_id(c) for c in kr.CASES]


def loop_grid(nx, ny, cx, cy):
    """The grid as test_gpu_solver.py builds it."""
    rp, ci, va = [0], [], []
    for j in range(ny):
        for i in range(nx):
            k = j * nx + i
            if j > 0:
                ci.append(k - nx), va.append(-1.0 - cy)
            if i > 0:
                ci.append(k - 1), va.append(-1.0 - cx)
            ci.append(k), va.append(4.0 + cx + cy)
            if i < nx - 1:
                ci.append(k + 1), va.append(-1.0)
            if j < ny - 1:
                ci.append(k + nx), va.append(-1.0)
            rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64)


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (6, 1), (7, 5), (37, 29)])
def test_vectorised_grid_is_the_loop_grid(shape):
    g = kr.Grid(*shape, 2.0, 1.0)
    rp, ci, va = loop_grid(*shape, 2.0, 1.0)
    assert g.n == shape[0] * shape[1]
    assert np.array_equal(g.rowptr, rp) and np.array_equal(g.colidx, ci) and np.array_equal(g.values, va)


def test_sizes_reach_what_they_are_for():
    n = {k: kr.grid(k).n for k in kr.SIZES}
    assert n == {"S": 3 * 2048 + 5, "T": 2049, "L": 525312, "X": 2101248}
    assert kr.kry_chunk(n["L"]) == 2048 and -(-n["L"] // 2048) == 257
    assert kr.kry_chunk(n["X"]) == 4096 and n["X"] // 4096 == 513
    assert kr.dropped_ranges(n["S"]) == {"wg1": (2048, 4096), "tail": (6144, 6149)}
    assert kr.dropped_ranges(n["T"]) == {"wg1": (2048, 2049)}  # (the tail is the same element)
    assert kr.dropped_ranges(n["L"]) == {"wg1": (2048, 4096), "tail": (524288, 525312)}  # (workgroup 256 is the tail)
    assert kr.dropped_ranges(n["X"]) == {"wg1": (4096, 8192), "wg256": (256 * 4096, 257 * 4096)}


def test_dots_and_the_mutation_hook():
    rng = np.random.default_rng(3)
    a, c = rng.standard_normal(5000), rng.standard_normal(5000)
    exact = float(np.dot(a.astype(np.longdouble), c.astype(np.longdouble)))
    scale = float(np.dot(np.abs(a), np.abs(c)))
    for kind in kr.DOTS:
        assert abs(kr.Dot(kind)(a, c) - exact) <= 5000 * 2.0 ** -53 * scale
    assert kr.Dot("longdouble")(a.astype(np.float32), c.astype(np.float32)) == float(
        np.dot(a.astype(np.float32).astype(np.longdouble), c.astype(np.float32).astype(np.longdouble)))
    d = kr.Dot("longdouble", mutate=(2, 1, (2048, 4096)))
    d.at(2)
    assert d(a, c) == exact and not d.hit
    keep = np.r_[0:2048, 4096:5000]
    rest = float(np.dot(a[keep].astype(np.longdouble), c[keep].astype(np.longdouble)))
    assert d(a, c) == rest and d.hit
    assert d(a, c) == exact
    assert d.calls == {2: 3}


def test_restatements_reach_the_pinned_counts():
    """b = 1, x0 = 0 on the 40 x 40 grid: the counts test_gpu_solver.py and
    test_gpu_gmres.py pin (16 and 25 iterations to 1e-10 with fp64 ILU(0))."""
    g = kr.Grid(40, 40, 2.0, 1.0)
    b, x0 = np.ones(g.n), np.zeros(g.n)
    _, hist = kr.bicgstab_trajectory(g, np.float64, np.float64, 16, b, x0, kr.Dot("forward"))
    assert hist[14] > 1e-10 >= hist[15]
    x, hist = kr.fgmres_trajectory(g, np.float64, np.float64, 30, 25, b, x0, kr.Dot("forward"))
    assert len(hist) == 25 and hist[23] > 1e-10 >= hist[24]
    assert np.linalg.norm(b - g.matvec(x)) <= 1e-10 * np.linalg.norm(b)
    # restart 5, 12 iterations: cycle ends at 5, 10 and the last iteration
    _, hist = kr.fgmres_trajectory(g, np.float64, np.float64, 5, 12, b, x0, kr.Dot("forward"))
    assert len(hist) == 12


@pytest.mark.parametrize("case", kr.CASES, ids=IDS)
def test_spread_stays_under_the_constants(case):
    x_ref, h_ref, _ = kr.reference(case)
    K = case[2]
    assert len(h_ref) == K and np.all(np.isfinite(h_ref)) and np.all(h_ref > 0.0)
    s_hist = s_x = 0.0
    for kind in kr.FP64_ORDERS:
        x, hist, _ = kr.run_case(case, kind)
        dh, dx = kr.deviation(x, hist, x_ref, h_ref)
        s_hist, s_x = max(s_hist, dh), max(s_x, dx)
    c_hist, c_x = kr.SPREAD[kr.spread_key(case)]
    tol = kr.tolerance(case)
    print(f"{kr.case_id(case)}: s_hist {s_hist:.2e} (<= {c_hist:.2e}), s_x {s_x:.2e} (<= {c_x:.2e}); "
          f"GPU tolerance {tol[0]:.2e}, {tol[1]:.2e}")
    assert s_hist <= c_hist and s_x <= c_x
    assert tol == (kr.MARGIN * max(c_hist, kr.EPS), kr.MARGIN * max(c_x, kr.EPS))


@pytest.mark.parametrize("case", kr.CASES, ids=IDS)
def test_a_missed_partial_leaves_the_tolerance(case):
    """Every walked dot of iterations 1-3, every dropped range: the mutated
    longdouble trajectory is at least SEPARATION tolerances from the reference.
    A run ends at the first history entry that is (the common case)."""
    x_ref, h_ref, calls = kr.reference(case)
    tol_hist, tol_x = kr.tolerance(case)
    ranges = kr.dropped_ranges(kr.grid(case[3]).n)
    dots = kr.walked_dots(case, calls)
    assert dots and ranges

    def moved(hist):
        i = len(hist) - 1
        return abs(hist[i] - h_ref[i]) >= kr.SEPARATION * tol_hist * h_ref[i]

    smallest = np.inf
    for it, k in dots:
        for name, rng in ranges.items():
            x, hist, dot = kr.run_case(case, "longdouble", (it, k, rng), watch=moved)
            assert dot.hit
            n = len(hist)
            shift = float(np.max(np.abs(hist - h_ref[:n]) / h_ref[:n])) / tol_hist
            if x is not None:
                shift = max(shift, kr.deviation(x, hist, x_ref, h_ref)[1] / tol_x)
            smallest = min(smallest, shift)
            assert shift >= kr.SEPARATION, (it, k, name, shift)
    print(f"{kr.case_id(case)}: {len(dots) * len(ranges)} mutations, the smallest moves the trajectory by "
          f"{smallest:.3g} tolerances (at the point the run was ended)")


# (n, columns, type): several workgroups with a tail; more columns than one batch of 8; fp32; 257 workgroups
ORTHO_CASES = [(6149, 3, np.float64), (6149, 10, np.float64), (6149, 3, np.float32), (525312, 3, np.float64)]


@pytest.mark.parametrize("n,k,dtype", ORTHO_CASES)
def test_a_missed_first_pass_partial_shows_in_h(n, k, dtype):
    V, w = kr.ortho_problem(n, k, dtype)
    gram = V.astype(np.float64) @ V.astype(np.float64).T
    assert np.max(np.abs(gram - 4.0 * np.eye(k))) < 0.2  # far from orthonormal, by design
    ref = kr.ortho_run(V, w)
    tol = kr.ortho_tolerance(V, w, ref)
    smallest = np.inf
    for i in range(k):  # the first pass's dots
        for name, rng in kr.dropped_ranges(n).items():
            shift = kr.ortho_deviation(kr.ortho_run(V, w, "longdouble", (1, i, rng)), ref) / tol
            smallest = min(smallest, shift)
            assert shift >= kr.SEPARATION, (i, name, shift)
    print(f"n = {n}, k = {k}, {dtype.__name__}: tolerance {tol:.2e}, the smallest first-pass mutation is "
          f"{smallest:.3g} tolerances away")
