"""What a device step of the GKR sum-check publishes, in plain Python over the
oracle's field (test helper, not a test module): the grid-point product sums of
a one- or two-round step and the 27 moment sums of a three-round step. Shared
by tests/test_dist_cpu.py (the multi-rank schedule over gloo) and
tests/test_gkr_rounds_cpu.py (the library's round formulas on the CPU)."""
from __future__ import annotations


def _corner(tab, idx_bits, nb, q):
    """Element of a table at corner idx_bits (nb leading variables) of block q."""
    L = len(tab)
    return tab[idx_bits * (L >> nb) + q]


def _grid(p, tab, nb, q, pt):
    """The table's multilinear extension in its nb leading variables at grid
    point pt (coordinates in {0, 1, 2}), block q."""
    vals = {}
    for c in range(1 << nb):
        vals[c] = _corner(tab, c, nb, q)
    # extend one axis at a time: X(2) = 2 X(1) - X(0)
    for axis in range(nb):
        sh = nb - 1 - axis
        t = pt[axis]
        nxt = {}
        for c, v in vals.items():
            if (c >> sh) & 1:
                continue
            x0, x1 = v, vals[c | (1 << sh)]
            nxt[c] = x0 if t == 0 else x1 if t == 1 else (2 * x1 - x0) % p
        vals = nxt
    return vals[0]


def _step_sums(p, tabs, nb, first):
    """What one device step publishes, as field values (mod p)."""
    A, S, M, P = tabs
    nq = len(A) >> nb
    if nb == 1:
        pts = [(0,), (1,), (2,)] if first else [(0,), (2,)]
    elif nb == 2:
        # categories (kernels.hpp): 0 V00, 1 V22, 2 V01, 3 V02, 4 V10, 5 V20, 6 V21, 7 V12 (+ 8 V11 first)
        pts = [(0, 0), (2, 2), (0, 1), (0, 2), (1, 0), (2, 0), (2, 1), (1, 2)] + ([(1, 1)] if first else [])
    else:
        pts = None
    if pts is not None:
        out = []
        for pt in pts:
            acc = 0
            for q in range(nq):
                acc += _grid(p, A, nb, q, pt) * _grid(p, S, nb, q, pt) + _grid(p, M, nb, q, pt) * _grid(p, P, nb, q, pt)
            out.append(acc % p)
        return out
    # three rounds: 27 moment tiles, id 9 alpha + 3 beta + gamma; per axis
    # moment 0 = X0 Y0, 1 = X1 Y1, 2 = X0 Y1 + X1 Y0 over the octant's corners
    sel = {0: [(0, 0)], 1: [(1, 1)], 2: [(0, 1), (1, 0)]}
    T = [0] * 27
    for q in range(nq):
        cx = [[_corner(X, c, 3, q) for c in range(8)] for X in (A, M)]
        cy = [[_corner(Y, c, 3, q) for c in range(8)] for Y in (S, P)]
        for a in range(3):
            for b in range(3):
                for g in range(3):
                    acc = 0
                    for ua, va in sel[a]:
                        for ub, vb in sel[b]:
                            for ug, vg in sel[g]:
                                u, v = 4 * ua + 2 * ub + ug, 4 * va + 2 * vb + vg
                                acc += cx[0][u] * cy[0][v] + cx[1][u] * cy[1][v]
                    T[9 * a + 3 * b + g] += acc
    return [t % p for t in T]
