"""Marginal and joint covariances Sigma = (JtJ + P)^-1 in 50-digit arithmetic, on the small structures of tests/solve_reference.py (a test
helper, not a test).

Input: the whitened records of a linearisation (J per factor; b plays no part) and the dense prior's P, as in solve_reference.

reference_columns(): the 3 or 6 columns of Sigma that belong to a variable are the solutions of H x = e_j.  They come from
solve_reference.reference_solve with lambda = 0, every b set to zero and eta = e_j: fp64 Cholesky corrections, residuals e_j - Jt (J x)
- P x in 50 digits factor by factor (H is never formed in high precision), stop at a correction below 1e-25 |x|_inf, every step must
contract (both asserted there).  That stop leaves an error of 1e-25 x the contraction of one step (about 1e-12: 1e-37), so one more
correction is added behind it (asserted to contract as well): the columns then agree with mpmath's inverse of the exactly formed H
to 1e-40 (tests/test_marginal_reference.py).  Columns are cached per graph object and record set (compared with np.array_equal), one variable at a
time, so the queries of one structure share them.  Every block - the diagonal block of a variable, the joint matrix of a key list with
its cross blocks - is read off those columns.

Measure.  Three classes of variables: pose-like ("pose", 6 x 6), points kept in the reduced system by a dense prior ("kept", 3 x 3) and
Schur-eliminated points ("schur", 3 x 3).  A diagonal block: max |a - ref| / max |ref block|; a class: the largest over its queried
variables.  A cross block (i, j), i != j: max |a - ref| / sqrt(max |Sigma_ii| max |Sigma_jj|), the Cauchy-Schwarz scale of
tests/test_gpu_joint_marginals.py (the cross block of two nearly independent variables is tiny and carries the rounding of its row and
column); "cross": the largest over the pairs of a key list.

Tolerance (cpu_reference()): per structure, key list and class, from the CPU alone.  The structure is linearised by the oracle, and on
those records three fp64 computations of the same blocks are measured against the 50-digit columns:
    inv       np.linalg.inv(H)
    cholesky  numpy's Cholesky factor and two triangular solves of the identity
    selinv    takahashi(): the recurrence the device uses restated in numpy - the points eliminated first
              (C C' = Hpp^-1, W = Hcp C), the reduced system factorised in 32 x 32 tiles with explicit inverses T_K^-1 and panel
              products M(I,K) = A(I,K) T_K^-1, Z(I,K) = - sum_J Zsym(I,J) M(J,K), Z(K,K) = T_K^-1 - sum_J M(J,K)' Z(J,K) symmetrised,
              Sigma_pp = C (I + W' Z W) C'.  Its elimination order: points, then the pose-like variables in key order, kept points last.
The tolerance is 16 x the largest of the three measures, floored at 64 eps: the rule of solve_reference.tolerance (16 covers the device's
other order of summation, its other elimination order and its MFMA contractions).  The third computation makes the tolerance reflect
the algorithm and not only LAPACK's.  The factor changes only together with a CPU computation that justifies it.  The device test
applies these numbers to the device's blocks, whose error it measures against the 50-digit columns of the DEVICE's records; nothing
comes from the device's output.  Every tolerance must be <= 1e-9 (solve_reference.MAX_TOL; asserted by the tests).

takahashi(plant=...) also computes what a kernel with one of five mistakes would (tests/test_marginal_reference.py shows that the measure
sees each of them).

query_vars(): which variables a structure is asked for.  Up to 130 scalars: every variable that is not a point of a point chain (those
are not implemented; a chain's first point kept by a dense prior is).  Above: at most 12 (5 on the 120-pose trees, whose columns cost
0.3 s each: under 10 s per record set), by rule - the first and the last pose-like variable in (frame, key) order, which the layouts of csrc/pose_layout.h are
built from and whose ends are the leaves of their arms; the sixth variable of the longest chain of keys (segments start on a tile
boundary and give each variable 6 rows: the sixth has rows 30 .. 35 of its segment and straddles two tiles); the kept points; one Schur
point per distinct edge count, those with >= 49 edge pairs first (k_point_cov strides a point's e^2 pairs over 64 lanes); then the
sixth, the last, the first and the middle variable of every chain and evenly spaced variables.

`python tests/marginal_reference.py` prints the CPU measures and tolerances of every structure the device test uses (no GPU).
"""
import copy
import functools
import os
import sys

import mpmath as mp
import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests import solve_reference as SR
else:
    from . import solve_reference as SR

from dynosam_amd import graph as G  # noqa: E402

TILE = 32
CLASSES = ("pose", "kept", "schur")
MEASURES = CLASSES + ("cross",)
SMALL = 130                      # scalars up to which every variable is queried
PLANTS = ("source", "transpose", "identity", "triangle", "panel")


# ---------------------------------------------------------------------------------------------- variables, classes, edges
def var_classes(g):
    """per variable: "pose", "kept" (a point of the dense prior), "schur", or "chain" (a point of a point chain: not implemented)"""
    d, off = SR.dims(g)
    chained = SR.chained_mask(g)
    kept = set() if g.prior is None else {g.key_index(int(k)) for k in g.prior.keys}
    out = []
    for i in range(g.n_vars):
        if g.var_type[i] != G.VAR_POINT3:
            out.append("pose")
        elif i in kept:
            out.append("kept")
        else:
            out.append("chain" if chained[off[i]] else "schur")
    return out


def edge_counts(g):
    """point variable -> number of (factor, pose-like slot) incidences: the edges k_point_cov pairs up"""
    ne = {}
    for blk in g.blocks:
        widths = G.SLOT_WIDTHS[blk.type & 15]
        pts = [s for s, w in enumerate(widths) if w == 3]
        poses = sum(1 for w in widths if w == 6)
        for row in blk.var_idx:
            for s in pts:
                ne[int(row[s])] = ne.get(int(row[s]), 0) + poses
    return ne


def query_vars(name, cap=12):
    g = SR.graph(name)
    d, off = SR.dims(g)
    cls = var_classes(g)
    if off[-1] <= SMALL:
        return tuple(i for i in range(g.n_vars) if cls[i] != "chain")
    if off[-1] > 600:
        cap = min(cap, 5)
    frame = lambda i: (int(g.var_keys[i]) & 0xFFFFFFFFFFFF, int(g.var_keys[i]))      # noqa: E731
    poses = sorted((i for i in range(g.n_vars) if cls[i] == "pose"), key=frame)
    chains = {}
    for i in poses:
        chains.setdefault(int(g.var_keys[i]) >> 48, []).append(i)
    chains = [chains[k] for k in sorted(chains)]
    ne = edge_counts(g)
    points = [i for i in range(g.n_vars) if cls[i] == "kept"]
    by_count = {}
    for i in range(g.n_vars):
        if cls[i] == "schur":
            by_count.setdefault(ne[i], i)                                             # the first point of every edge count
    points += [by_count[e] for e in sorted(by_count, key=lambda e: (e * e < 49, e))]
    ranked = [poses[0], poses[-1]] + [c[5] for c in sorted(chains, key=len, reverse=True)[:1] if len(c) >= 6]
    n_first = len(ranked)
    ranked += [c[5] for c in chains if len(c) >= 6]
    ranked += [c[-1] for c in chains] + [c[0] for c in chains] + [c[len(c) // 2] for c in chains]
    ranked += [poses[int(round(x))] for x in np.linspace(0, len(poses) - 1, cap)]
    picks = []
    for i in ranked[:n_first] + points + ranked[n_first:]:
        if i not in picks and len(picks) < cap:
            picks.append(i)
    return tuple(picks)


# ---------------------------------------------------------------------------------------------- the 50-digit columns
_columns = {}


def _same_records(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _column(hit, j):
    """column j of H^-1: the refinement of solve_reference with zero b and eta = e_j"""
    s = copy.copy(hit["system"])
    P = hit["P"]
    s.pidx = sorted(set(s.pidx) | {j})
    s.P = [[mp.mpf(float(P[a, b])) for b in s.pidx] for a in s.pidx]
    s.eta = [mp.mpf(int(a == j)) for a in s.pidx]
    x, steps = SR.reference_solve(s, hit["J"], P, 0.0, False)
    hit["steps"] = max(hit["steps"], len(steps))
    with mp.workdps(SR.DPS):                   # one correction behind the stop (see the docstring)
        r = np.array([float(v) for v in s.residual(x, [mp.mpf(0)] * s.n)])
        dx = np.linalg.solve(hit["L"].T, np.linalg.solve(hit["L"], r))
        assert np.abs(dx).max() <= 0.5 * steps[-1], ("the correction behind the stop does not contract", steps, np.abs(dx).max())
        return [xi + mp.mpf(float(di)) for xi, di in zip(x, dx)]


def reference_columns(g, recs, vars):
    """{variable: its 3 or 6 columns of (JtJ + P)^-1, each a list of n mpmath numbers}"""
    d, off = SR.dims(g)
    sets = _columns.setdefault(id(g), [])          # (the oracle's records and the device's: two sets per structure)
    hit = next((h for h in sets if _same_records(h["recs"], recs)), None)
    if hit is None:
        n = int(off[-1])
        P, _eta = SR.prior_system(g)
        zero = [(cols, Jf, np.zeros_like(bf)) for cols, Jf, bf in recs]
        J = SR.dense(zero, n)[0]
        hit = dict(g=g, recs=recs, P=P, J=J, L=np.linalg.cholesky(J.T @ J + P), system=SR.System(zero, n, P, np.zeros(n)), cols={}, steps=0)
        sets.append(hit)
    for v in vars:
        if v not in hit["cols"]:
            hit["cols"][v] = [_column(hit, int(off[v]) + k) for k in range(d[v])]
    return {v: hit["cols"][v] for v in vars}


def refinement_steps(g):
    """the most steps any column of the graph took to the stop"""
    return max(h["steps"] for h in _columns[id(g)])


def block(g, cols, i, j):
    """rows of variable i, columns of variable j (mpmath, d_i x d_j)"""
    d, off = SR.dims(g)
    return [[cols[j][c][int(off[i]) + r] for c in range(d[j])] for r in range(d[i])]


def joint_matrix(g, cols, vars):
    """the joint covariance of `vars` in caller order (mpmath, D x D)"""
    rows = []
    for i in vars:
        parts = [block(g, cols, i, j) for j in vars]
        rows += [sum((p[r] for p in parts), []) for r in range(len(parts[0]))]
    return rows


# ---------------------------------------------------------------------------------------------- measures
def _err(a, ref):
    return max(abs(mp.mpf(float(a[r][c])) - ref[r][c]) for r in range(len(ref)) for c in range(len(ref[0])))


def _max(ref):
    return max(abs(v) for row in ref for v in row)


def measure_blocks(g, cols, vars, blocks):
    """blocks[n]: the (>= d x d) array of variable vars[n] -> {class: the largest diagonal-block measure, 0.0 for a class not queried}"""
    d, _ = SR.dims(g)
    cls = var_classes(g)
    out = dict.fromkeys(CLASSES, 0.0)
    with mp.workdps(SR.DPS):
        for n, i in enumerate(vars):
            ref = block(g, cols, i, i)
            out[cls[i]] = max(out[cls[i]], float(_err(np.asarray(blocks[n])[:d[i], :d[i]], ref) / _max(ref)))
    return out


def measure_joint(g, cols, vars, M):
    """M: the D x D joint matrix of `vars` in caller order -> the class measures of its diagonal blocks and "cross" """
    d, _ = SR.dims(g)
    st = np.concatenate([[0], np.cumsum([d[i] for i in vars])])
    M = np.asarray(M)
    out = measure_blocks(g, cols, vars, [M[st[n]:st[n + 1], st[n]:st[n + 1]] for n in range(len(vars))])
    out["cross"] = 0.0
    with mp.workdps(SR.DPS):
        scale = [_max(block(g, cols, i, i)) for i in vars]
        for x, i in enumerate(vars):
            for y, j in enumerate(vars):
                if x != y:
                    e = _err(M[st[x]:st[x + 1], st[y]:st[y + 1]], block(g, cols, i, j))
                    out["cross"] = max(out["cross"], float(e / mp.sqrt(scale[x] * scale[y])))
    return out


def rows_of(g, vars):
    d, off = SR.dims(g)
    return np.concatenate([off[i] + np.arange(d[i]) for i in vars])


def measure_dense(g, cols, vars, Sig):
    """a dense n x n covariance in the compact columns, measured on the blocks of `vars`"""
    r = rows_of(g, vars)
    return measure_joint(g, cols, vars, Sig[np.ix_(r, r)])


# ---------------------------------------------------------------------------------------------- three fp64 computations
def hessian(g, recs):
    n = int(SR.dims(g)[1][-1])
    J, _b = SR.dense(recs, n)
    return J.T @ J + SR.prior_system(g)[0]


def cholesky_inverse(H):
    L = np.linalg.cholesky(H)
    return np.linalg.solve(L.T, np.linalg.solve(L, np.eye(len(H))))


def elimination_order(g):
    """(scalars of the eliminated points, scalars of the reduced system: pose-like variables in key order, kept points last)"""
    cls = var_classes(g)
    pts = [i for i in range(g.n_vars) if cls[i] in ("schur", "chain")]
    red = [i for i in range(g.n_vars) if cls[i] == "pose"] + [i for i in range(g.n_vars) if cls[i] == "kept"]
    return (rows_of(g, pts) if pts else np.zeros(0, int)), rows_of(g, red)


def takahashi(g, H, plant=None, at=(), ts=TILE):
    """Sigma (dense, compact columns) by the device's recurrence.  plant (tests): "source" every off-diagonal target loses its last
    source term, "transpose" M where M' belongs in the diagonal targets, "identity" the I of a point block left out, "triangle" a
    diagonal tile used as a source before its upper triangle is mirrored, "panel" one entry of one panel tile off by 1e-8 of itself:
    the largest one in the columns of the compact scalars `at` (of a pose-like variable below the root tile)"""
    p, c = elimination_order(g)
    npt, nc = len(p), len(c)
    C = np.linalg.inv(np.linalg.cholesky(H[np.ix_(p, p)])).T if npt else np.zeros((0, 0))       # C C' = Hpp^-1
    W = H[np.ix_(c, p)] @ C                                                                      # the Z_e of every edge, stacked
    nt = (nc + ts - 1) // ts
    A = np.eye(nt * ts)                                                                          # identity padding of the last tile
    A[:nc, :nc] = H[np.ix_(c, c)] - W @ W.T
    s = [slice(k * ts, (k + 1) * ts) for k in range(nt)]
    M, Tinv = {}, []
    for K in range(nt):
        Tinv.append(np.linalg.inv(A[s[K], s[K]]))
        for I in range(K + 1, nt):
            M[I, K] = A[s[I], s[K]] @ Tinv[K]
        for I in range(K + 1, nt):
            for J in range(K + 1, I + 1):
                A[s[I], s[J]] -= M[I, K] @ A[s[J], s[K]].T
    if plant == "panel":                                                                         # the largest entry under the scalars `at`
        place = {int(v): k for k, v in enumerate(c)}
        qs = [place[int(v)] for v in at if place[int(v)] // ts < nt - 1]
        K = qs[0] // ts
        qs = [q - K * ts for q in qs if q // ts == K]
        _m, J, r, q = max((abs(M[J, K][r, q]), J, r, q) for J in range(K + 1, nt) for r in range(ts) for q in qs)
        M[J, K][r, q] *= 1.0 + 1e-8
    Z = np.zeros((nt * ts, nt * ts))                                                             # lower tiles; diagonal tiles full
    for K in reversed(range(nt)):
        for I in range(K + 1, nt):
            acc = np.zeros((ts, ts))
            for J in range(K + 1, nt - 1 if plant == "source" else nt):
                Zs = Z[s[I], s[J]] if I >= J else Z[s[J], s[I]].T
                acc += (np.tril(Zs) if plant == "triangle" and I == J else Zs) @ M[J, K]
            Z[s[I], s[K]] = -acc
        acc = np.zeros((ts, ts))
        for J in range(K + 1, nt):
            acc += (M[J, K] if plant == "transpose" else M[J, K].T) @ Z[s[J], s[K]]
        D = Tinv[K] - acc
        Z[s[K], s[K]] = 0.5 * (D + D.T)
    Z = (np.tril(Z) + np.tril(Z, -1).T)[:nc, :nc]
    Sig = np.zeros_like(H)
    Sig[np.ix_(c, c)] = Z
    if npt:
        B = W.T @ Z @ W + (0.0 if plant == "identity" else np.eye(npt))
        Sig[np.ix_(p, p)] = C @ B @ C.T
        Sig[np.ix_(p, c)] = -C @ (W.T @ Z)
        Sig[np.ix_(c, p)] = Sig[np.ix_(p, c)].T
    return Sig


class CpuReference:
    """the records of one CPU linearisation and a key list: the three fp64 computations' measures and the tolerances made of them"""

    def __init__(self, g, recs, vars):
        self.g, self.vars = g, tuple(vars)
        self.columns = reference_columns(g, recs, self.vars)
        self.steps = refinement_steps(g)
        H = hessian(g, recs)
        self.cond = float(np.linalg.cond(H))
        self.cpu = {"inv": measure_dense(g, self.columns, self.vars, np.linalg.inv(H)),
                    "cholesky": measure_dense(g, self.columns, self.vars, cholesky_inverse(H)),
                    "selinv": measure_dense(g, self.columns, self.vars, takahashi(g, H))}
        self.tol = {k: SR.tolerance([m[k] for m in self.cpu.values()]) for k in MEASURES}
        cls = var_classes(g)
        self.present = tuple(k for k in CLASSES if any(cls[i] == k for i in self.vars)) + (("cross",) if len(self.vars) > 1 else ())


def oracle_records_of(g):
    """the records of the oracle's linearisation of a graph at its values"""
    from oracle import oracle_py as O
    Jr, br, _ = O.OracleGraph(g).linearize()
    return SR.records(g, Jr, br)


@functools.lru_cache(maxsize=None)
def cpu_reference(name, vars=None):
    """the structure linearised by the oracle, and the blocks of `vars` (default: query_vars(name)) computed on the CPU alone: its .tol
    are the tolerances of the case, on the CPU and on the device"""
    return CpuReference(SR.graph(name), SR.oracle_records(name), query_vars(name) if vars is None else vars)


def report(name, ref, got=None, what=""):
    """one line per class queried: CPU measures (oracle records), tolerance and - with the device's measures `got` - device error and ratio"""
    lines = []
    for k in (k for k in ref.present if got is None or k in got):
        cpu = " ".join(f"{who} {m[k]:.1e}" for who, m in ref.cpu.items())
        dev = "" if got is None else f"  device {got[k]:.2e}  ratio {got[k] / ref.tol[k]:.3f}"
        lines.append(f"{name:12s} {what:14s} {k:5s} {cpu}  tol {ref.tol[k]:.2e}{dev}")
    return "\n".join(lines)


# the structures of the device test (tests/test_gpu_marginal_reference.py)
PLAIN = ("degree", "degree_wide", "pairs_1", "pairs_16", "pairs_65", "kept_hybrid", "kept_chain", "clip", "chain_wcpe") + tuple(f"poses_{N}" for N in SR.POSE_COUNTS)
TREES = ("tree_band", "tree_loops", "tree_star")


if __name__ == "__main__":
    for name in (sys.argv[1:] or PLAIN + TREES):
        ref = cpu_reference(name)
        n = int(SR.dims(SR.graph(name))[1][-1])
        print(report(name, ref), f"\n{'':12s} n = {n}, {len(ref.vars)} keys, refinement steps {ref.steps}, cond(H) {ref.cond:.1e}")
