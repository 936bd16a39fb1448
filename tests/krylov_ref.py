"""Trajectory restatements of the two Krylov solvers (CPU only; test
infrastructure for test_krylov_trajectory.py and test_gpu_krylov_trajectory.py).

bicgstab_trajectory / fgmres_trajectory restate rsp_bicgstab_solve and
rsp_gmres_solve (include/rsp.h) at rtol = 0, max_iters = K, check_every = 1:
exactly K iterations, returning x and the history with the library's meaning.
Every element-wise step is written as krylov.hip writes it (the same
parenthesisation, scalars rounded to the iteration type first, no fused
multiply-add: the library is built with -ffp-contract=off), the SpMV goes
through the oracle in the kernels' canonical order and ILU(0) and the
triangular solves through the oracle, so what separates a restatement from the
device is the order in which a dot product is summed, and nothing else.

The dot is pluggable (DOTS): numpy fp64 forward (np.sum of the products), the
same reversed, fp64 in
2048-element blocks added in block order (the device's shape: one partial per
workgroup), and np.longdouble, which is the reference trajectory. Every dot
returns an fp64 value, as the device's dots do; the scalar arithmetic after it
is fp64.

Mutation hook: Dot(kind, mutate=(iteration, k, (lo, hi))) makes the k-th dot
of that iteration ignore the elements [lo, hi) — a workgroup's partial that was
never added. Iteration 0 is the set-up ((b,b) and the first (r,r)).
"""
import functools
import math

import numpy as np

import oracle_bind as ob

CHUNK = 2048      # rsp::kKryChunk
MAX_GRID = 1024   # rsp::kKryMaxGrid

# label -> (nx, ny): the smallest grids at which each mechanism of krylov.hip exists
SIZES = {"S": (143, 43), "T": (683, 3), "L": (1024, 513), "X": (2048, 1026)}


def kry_chunk(n):
    """Elements per workgroup (rsp::kry_grid)."""
    span = CHUNK * MAX_GRID
    return CHUNK * ((n + span - 1) // span if n > span else 1)


def dropped_ranges(n):
    """The element ranges a mutation drops, those that exist at n: workgroup
    1's, the last (partly filled) workgroup's, workgroup 256's."""
    c = kry_chunk(n)
    out = {}
    if n > c:
        out["wg1"] = (c, min(2 * c, n))
    if n % c:
        out["tail"] = (n - n % c, n)
    if n > 256 * c:
        out["wg256"] = (256 * c, min(257 * c, n))
    seen, uniq = set(), {}
    for k, r in out.items():
        if r not in seen:
            seen.add(r)
            uniq[k] = r
    return uniq


class Csr:
    """A square CSR matrix with what the restatements need of it: the SpMV in
    the kernels' canonical order, ILU(0) and M^-1 = U^-1 L^-1 by the oracle."""

    def __init__(self, rowptr, colidx, values):
        self.n = len(rowptr) - 1
        self.rowptr = np.ascontiguousarray(rowptr, np.int32)
        self.colidx = np.ascontiguousarray(colidx, np.int32)
        self.values = np.ascontiguousarray(values, np.float64)
        self._cast = {}

    def vals(self, dtype):
        if dtype not in self._cast:
            self._cast[dtype] = self.values.astype(dtype)
        return self._cast[dtype]

    def matvec(self, x, dtype=np.float64):
        return ob.spmv(self.rowptr, self.colidx, self.vals(dtype), x.astype(dtype), order="canon")

    def rhs_and_start(self, dtype=np.float64, seed=20240607):
        """b and a non-zero x0 from a seeded generator, rounded to dtype."""
        rng = np.random.default_rng(seed)
        b = rng.uniform(-1.0, 1.0, self.n).astype(dtype)
        x0 = rng.uniform(-0.5, 0.5, self.n).astype(dtype)
        return b, x0

    @functools.lru_cache(maxsize=None)
    def factor(self, precond, ftz=False):
        fac, sz, zp = ob.ilu0(self.rowptr, self.colidx, self.vals(precond), ftz=ftz)
        assert sz == -1 and zp == -1
        return fac

    def apply(self, precond, ftz=False):
        """z = M^-1 y in the preconditioner's precision (None: M = I)."""
        if precond is None:
            return lambda y: y
        fac = self.factor(precond, ftz)

        def apply(y):
            z = ob.trsv("lower_n", self.rowptr, self.colidx, fac, y.astype(precond), ftz=ftz)
            return ob.trsv("upper", self.rowptr, self.colidx, fac, z, ftz=ftz).astype(y.dtype)
        return apply


class Grid(Csr):
    """The 5-point convection-diffusion grid of test_gpu_solver.py (diagonal
    4 + cx + cy, west -1 - cx, east -1, south -1 - cy, north -1, Dirichlet
    boundaries, rows sorted), built without a Python loop."""

    def __init__(self, nx, ny, cx=2.0, cy=1.0):
        n = nx * ny
        k = np.arange(n, dtype=np.int64)
        i, j = k % nx, k // nx
        cols = np.stack([k - nx, k - 1, k, k + 1, k + nx], axis=1)
        vals = np.broadcast_to(np.array([-1.0 - cy, -1.0 - cx, 4.0 + cx + cy, -1.0, -1.0]), (n, 5))
        keep = np.stack([j > 0, i > 0, np.ones(n, bool), i < nx - 1, j < ny - 1], axis=1)
        rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
        super().__init__(rowptr, cols[keep], vals[keep])


def skew_blocks(n):
    """[[0, 1], [-1, 0]] repeated along the diagonal (n even): (y, A y) = 0 for every y."""
    k = np.arange(n)
    return Csr(np.arange(n + 1), k ^ 1, np.where(k % 2 == 0, 1.0, -1.0))


@functools.lru_cache(maxsize=None)
def grid(label):
    return Grid(*SIZES[label])


def _f8(a):
    return a if a.dtype == np.float64 else a.astype(np.float64)


def _dot_forward(a, c):
    return float(np.sum(a * c))  # numpy's own pairwise sum: no BLAS, the same on every host


def _dot_reverse(a, c):
    return float(np.sum((a * c)[::-1]))


def _dot_blocks(a, c):
    p = a * c
    pad = -len(p) % CHUNK
    if pad:
        p = np.concatenate([p, np.zeros(pad)])
    total = 0.0
    for s in p.reshape(-1, CHUNK).sum(axis=1):  # one partial per workgroup-sized block, in block order
        total += float(s)
    return total


def _dot_longdouble(a, c):
    return float(np.dot(a.astype(np.longdouble), c.astype(np.longdouble)))


DOTS = {"forward": _dot_forward, "reverse": _dot_reverse, "blocks": _dot_blocks, "longdouble": _dot_longdouble}
FP64_ORDERS = ("forward", "reverse", "blocks")


class Dot:
    """A dot of the chosen kind that counts its calls per iteration and, with
    mutate = (iteration, k, (lo, hi)), drops [lo, hi) from that one call."""

    def __init__(self, kind="longdouble", mutate=None):
        self.fn = DOTS[kind]
        self.mutate = mutate
        self.it, self.k = 0, 0
        self.calls = {}
        self.hit = False

    def at(self, it):
        self.it, self.k = it, 0

    def __call__(self, a, c):
        a, c = _f8(a), _f8(c)
        if self.mutate is not None and self.mutate[0] == self.it and self.mutate[1] == self.k:
            lo, hi = self.mutate[2]
            a = a.copy()
            a[lo:hi] = 0.0
            self.hit = True
        self.k += 1
        self.calls[self.it] = self.k
        return self.fn(a, c)


def bicgstab_trajectory(g, precond, dtype, K, b, x0, dot, watch=None):
    """K iterations of rsp_bicgstab_solve: (x, history), history[i] = ||r|| /
    ||b|| of the recurrence residual after iteration i + 1. The dots of an
    iteration, in call order: (rhat,r), (rhat,v), (t,s), (t,t), (r,r).
    watch(history), called after each entry, ends the run early by returning
    True; x is then None."""
    M = g.apply(precond)
    A = lambda y: g.matvec(y, dtype)
    dot.at(0)
    x = x0.astype(dtype)
    r = b - A(x)
    rh = r.copy()
    bn = math.sqrt(dot(b, b))
    dot(r, r)
    rho = alpha = omega = 1.0
    p = v = None
    hist = []
    for it in range(1, K + 1):
        dot.at(it)
        rho_new = dot(rh, r)
        if it == 1:
            p = r.copy()
        else:
            beta = (rho_new / rho) * (alpha / omega)
            p = r + dtype(beta) * (p - dtype(omega) * v)
        rho = rho_new
        ph = M(p)
        v = A(ph)
        alpha = rho / dot(rh, v)
        s = r - dtype(alpha) * v
        sh = M(s)
        t = A(sh)
        ts = dot(t, s)
        tt = dot(t, t)
        omega = ts / tt if tt != 0.0 else 0.0
        x = (x + dtype(alpha) * ph) + dtype(omega) * sh
        r = s - dtype(omega) * t
        hist.append(math.sqrt(dot(r, r)) / bn)
        if watch is not None and watch(hist):
            return None, hist
    return x, hist


def rotate_column(col, j, cs, sn, gv):
    """rsp::gmres_lsq's column step; False: the rotated diagonal is 0."""
    for i in range(j):
        a, b = col[i], col[i + 1]
        col[i], col[i + 1] = cs[i] * a + sn[i] * b, cs[i] * b - sn[i] * a
    a, b = col[j], col[j + 1]
    s = max(abs(a), abs(b))
    if s == 0.0 or not math.isfinite(s):
        return False
    r = s * math.sqrt((a / s) ** 2 + (b / s) ** 2)
    cs[j], sn[j] = a / r, b / r
    col[j], col[j + 1] = r, 0.0
    gv[j], gv[j + 1] = cs[j] * gv[j], -(sn[j] * gv[j])
    return True


def cgs2(V, w, dot, dtype):
    """Classical Gram-Schmidt twice as gm_multidot, gm_update<0> and
    gm_update<1> do it: every coefficient of a pass from the same w, the update
    accumulated in fp64 in column order and rounded once to the type. Returns
    (h + h', ||w||, w). Dots in call order: (v_i, w) for each i, the same after
    the first update, (w, w)."""
    h = np.zeros(len(V))
    for _ in range(2):
        hp = [dot(v, w) for v in V]
        d = _f8(w).copy()
        for i, v in enumerate(V):
            d -= hp[i] * _f8(v)
        w = d.astype(dtype)
        h += hp
    return h, math.sqrt(dot(w, w)), w


def fgmres_trajectory(g, precond, dtype, restart, K, b, x0, dot, watch=None):
    """K iterations of rsp_gmres_solve: (x, history); a history entry is est
    after a column, or the recomputed ||b - A x|| / ||b|| at a cycle end and
    after the last iteration. The dots of iteration total + j + 1 (column j),
    in call order: (v_i, w) i <= j, the same after the first update, (w, w),
    and at a cycle's last column the (r, r) of the recomputed residual.
    h_{j+1,j} = 0 is the exact solve: it ends the cycle (rsp.h). watch: as
    bicgstab_trajectory."""
    M = g.apply(precond)
    A = lambda y: g.matvec(y, dtype)
    m = restart
    dot.at(0)
    x = x0.astype(dtype)
    w = b - A(x)
    bn = math.sqrt(dot(b, b))
    rr = dot(w, w)
    total, hist = 0, []
    while total < K:
        beta = math.sqrt(rr)
        V = [(_f8(w) / beta).astype(dtype)]
        Z, R = [], np.zeros((m + 1, m))
        cs, sn, gv = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        gv[0] = beta
        cols = 0
        while cols < m and total + cols < K:
            j = cols
            dot.at(total + j + 1)
            Z.append(M(V[j]))
            w = A(Z[j])
            h, hn, w = cgs2(V, w, dot, dtype)
            col = np.append(h, hn)
            assert rotate_column(col, j, cs, sn, gv)
            R[:j + 2, j] = col
            cols += 1
            if hn == 0.0 or cols == m or total + cols == K:
                break
            V.append((_f8(w) / hn).astype(dtype))
            hist.append(abs(gv[j + 1]) / bn)
            if watch is not None and watch(hist):
                return None, hist
        y = np.zeros(cols)
        for i in range(cols - 1, -1, -1):
            v = gv[i]
            for l in range(i + 1, cols):
                v -= R[i, l] * y[l]
            y[i] = v / R[i, i]
        d = _f8(x).copy()
        for i in range(cols):
            d += y[i] * _f8(Z[i])
        x = d.astype(dtype)
        w = b - A(x)
        rr = dot(w, w)
        total += cols
        hist.append(math.sqrt(rr) / bn)
        if watch is not None and watch(hist):
            return None, hist
        if rr == 0.0:
            break
    return x, hist


# ------------------------------------------------------------------ the cases

NP = {"fp64": np.float64, "fp32": np.float32, "none": None}
# (size, preconditioner, iteration type); "allfp32": fp32 iteration under the fp32 preconditioner
PRECOND_CASES = [("S", "fp64", "f64"), ("S", "fp32", "f64"), ("S", "none", "f64"), ("S", "fp32", "f32"),
                 ("T", "fp64", "f64"),
                 ("L", "fp64", "f64"), ("L", "fp32", "f64"), ("L", "none", "f64"),
                 ("X", "none", "f64")]
# solver variants: (name, restart, K)
VARIANTS = [("bicgstab", 0, 4), ("gmres", 3, 5), ("gmres", 30, 10)]
CASES = [(sv, r, K, size, pc, it) for (sv, r, K) in VARIANTS for (size, pc, it) in PRECOND_CASES]


def case_id(case):
    sv, r, K, size, pc, it = case
    return f"{sv}{'' if sv == 'bicgstab' else '-m%d' % r}-K{K}-{size}-{pc}-{it}"


def precond_class(pc, it):
    return "allfp32" if it == "f32" else ("fp32" if pc == "fp32" else "fp64")


def run_case(case, kind="longdouble", mutate=None, watch=None):
    """(x as fp64, history, the Dot) of one case's restatement."""
    sv, restart, K, size, pc, it = case
    g = grid(size)
    dtype = np.float32 if it == "f32" else np.float64
    b, x0 = g.rhs_and_start(dtype)
    dot = Dot(kind, mutate)
    if sv == "bicgstab":
        x, hist = bicgstab_trajectory(g, NP[pc], dtype, K, b, x0, dot, watch)
    else:
        x, hist = fgmres_trajectory(g, NP[pc], dtype, restart, K, b, x0, dot, watch)
    return None if x is None else x.astype(np.float64), np.array(hist), dot


@functools.lru_cache(maxsize=None)
def reference(case):
    """The longdouble trajectory of a case: (x, history, dots per iteration)."""
    x, hist, dot = run_case(case)
    x.setflags(write=False)
    hist.setflags(write=False)
    return x, hist, dict(dot.calls)


def deviation(x, hist, x_ref, hist_ref):
    """(largest relative deviation of a history entry, max|x - x_ref| / max|x_ref|)."""
    assert len(hist) == len(hist_ref)
    dh = float(np.max(np.abs(np.asarray(hist) - hist_ref) / np.abs(hist_ref)))
    dx = float(np.max(np.abs(np.asarray(x, np.float64) - x_ref)) / np.max(np.abs(x_ref)))
    return dh, dx


# ------------------------------------------------------------- the tolerances
#
# SPREAD[(solver, size, class)] = (s_hist, s_x): the largest deviation of the
# three fp64 dot orders from the longdouble trajectory over the cases of that
# solver, size and preconditioner class (fp64 and no preconditioner are one
# class; GMRES: both restart lengths), measured on the CPU and rounded up to
# two digits; test_krylov_trajectory.py recomputes them and holds the table.
# A spread below one fp64 ulp (the all-fp32 x: no rounding of the fp32 solve
# flipped in any order) counts as one ulp, the resolution of the comparison.
EPS = 2.0 ** -52
SPREAD = {
    ("bicgstab", "S", "fp64"): (4.7e-14, 1.5e-14),
    ("bicgstab", "S", "fp32"): (7.4e-14, 2.4e-14),
    ("bicgstab", "S", "allfp32"): (EPS, EPS),
    ("bicgstab", "T", "fp64"): (8.2e-13, 5.4e-16),
    ("bicgstab", "L", "fp64"): (6.0e-16, 1.4e-15),
    ("bicgstab", "L", "fp32"): (2.7e-14, 9.7e-15),
    ("bicgstab", "X", "fp64"): (8.3e-16, 7.9e-16),
    ("gmres", "S", "fp64"): (1.3e-15, 8.7e-16),
    ("gmres", "S", "fp32"): (8.4e-16, 7.2e-16),
    ("gmres", "S", "allfp32"): (7.5e-16, EPS),
    ("gmres", "T", "fp64"): (7.0e-11, 2.4e-16),
    ("gmres", "L", "fp64"): (1.1e-15, 1.5e-15),
    ("gmres", "L", "fp32"): (1.9e-12, 3.3e-9),
    ("gmres", "X", "fp64"): (7.6e-16, 1.5e-15),
}
MARGIN = 100.0      # the device's order is a fourth one, and three samples under-estimate a spread
SEPARATION = 10.0   # a single-dot mutation must leave the reference by this many tolerances


def spread_key(case):
    sv, _, _, size, pc, it = case
    return sv, size, precond_class(pc, it)


def tolerance(case):
    """(tol_hist, tol_x) of the GPU comparison: MARGIN x the class's spread."""
    s_hist, s_x = SPREAD[spread_key(case)]
    return MARGIN * max(s_hist, EPS), MARGIN * max(s_x, EPS)


def walked_dots(case, calls):
    """(iteration, k) of every dot of iterations 1-3 that the mutation walk
    covers. GMRES: without the first Gram-Schmidt pass's dots (k <= column): a
    coefficient the first pass gets wrong is what the second pass removes again
    (h = h + h'), so no trajectory can show it."""
    sv, restart = case[0], case[1]
    out = []
    for it in (1, 2, 3):
        first_pass = ((it - 1) % restart) + 1 if sv == "gmres" else 0
        out += [(it, k) for k in range(first_pass, calls[it])]
    return out


# -------------------------------------------- the first Gram-Schmidt pass alone
#
# With an orthonormal V the second pass hides what the first got wrong. With
# V = 2 Q it cannot: V^T V = 4 I, so a first-pass coefficient that is short by
# delta comes out of h + h' as a shift of -3 delta, and rsp_orthogonalize
# returns h + h'.

def ortho_problem(n, k, dtype, seed=11):
    """(V, w): k seeded columns of length 2 (nearly orthogonal, far from
    orthonormal), w = uniform(-1, 1) + 3 v_0, in dtype."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((k, n))
    V *= 2.0 / np.linalg.norm(V, axis=1, keepdims=True)
    w = rng.uniform(-1.0, 1.0, n) + 3.0 * V[0]
    return V.astype(dtype), w.astype(dtype)


def ortho_run(V, w, kind="longdouble", mutate=None):
    """cgs2 as one 'iteration 1': (h + h', ||w||, w as fp64)."""
    dot = Dot(kind, mutate)
    dot.at(1)
    h, hn, w = cgs2(list(V), w, dot, w.dtype.type)
    assert mutate is None or dot.hit
    return h, hn, w.astype(np.float64)


def ortho_deviation(run, ref):
    """The largest of: max|h - h_ref| / max|h_ref|, the relative deviation of
    ||w||, max|w - w_ref| / max|w_ref|."""
    (h, hn, w), (h_r, hn_r, w_r) = run, ref
    return max(float(np.max(np.abs(h - h_r)) / np.max(np.abs(h_r))), abs(hn - hn_r) / hn_r,
               float(np.max(np.abs(w - w_r)) / np.max(np.abs(w_r))))


def ortho_tolerance(V, w, ref):
    """MARGIN x the spread of the three fp64 orders (at least one ulp)."""
    return MARGIN * max(EPS, max(ortho_deviation(ortho_run(V, w, kind), ref) for kind in FP64_ORDERS))
