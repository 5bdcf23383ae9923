"""The index arithmetic of the interpolation kernels (csrc/poly.hpp) restated in
Python, one statement per statement of the kernel: which global elements a
block of k_poly_tree_level stages, into which LDS slots, which slots a lane
reads for each product, the implicit leading 1 of every M, the pass-through
of a node without a sibling, and the deal of a large level's steps over
blockIdx.y with the kernel that adds the partial sums; likewise the j tiling of k_poly_weights and the
chunked Horner of k_poly_eval with its combining kernel. Every global index is
checked against the table length and every LDS slot against the array it
belongs to, every output must be written exactly once, and the results are
returned for comparison with tests/poly_oracle.py. Arithmetic is plain ints
mod p; nothing of the GPU is needed."""
from __future__ import annotations

BLOCK = 256
EVAL_TILE = 512
TREE_TILE = 128
TREE_SPLIT = 8
FILL = 4


class _Table:
    """A global table whose every access is bounds-checked."""

    def __init__(self, n, values=None):
        self.v = list(values) if values is not None else [None] * n

    def ld(self, i):
        assert 0 <= i < len(self.v), ("global load out of range", i, len(self.v))
        assert self.v[i] is not None, ("global load of an unwritten element", i)
        return self.v[i]

    def st(self, i, x):
        assert 0 <= i < len(self.v), ("global store out of range", i, len(self.v))
        assert self.v[i] is None, ("an output written twice", i)
        self.v[i] = x


class _Lds:
    def __init__(self, n):
        self.v = [None] * n

    def get(self, e):
        assert 0 <= e < len(self.v), ("LDS read out of range", e, len(self.v))
        assert self.v[e] is not None, ("LDS read of an unwritten slot", e)
        return self.v[e]

    def put(self, e, x):
        assert 0 <= e < len(self.v), ("LDS write out of range", e, len(self.v))
        self.v[e] = x


def ceil_div(a, b):
    return (a + b - 1) // b


# --- poly_plan.hpp --------------------------------------------------------------------
def eval_plan(m, d, num_cus):
    tiles = ceil_div(m, BLOCK) if m else 1
    want = FILL * (num_cus or 1)
    if tiles >= want or d <= EVAL_TILE:
        return 1, d
    chunks = min(ceil_div(want, tiles), ceil_div(d, EVAL_TILE))
    length = ceil_div(ceil_div(d, chunks), EVAL_TILE) * EVAL_TILE
    return ceil_div(d, length), length


def weights_plan(n, num_cus):
    tiles = ceil_div(n, BLOCK) if n else 1
    want = FILL * (num_cus or 1)
    parts = 1 if tiles >= want else ceil_div(want, tiles)
    parts = min(parts, tiles)
    length = ceil_div(tiles, parts) * BLOCK
    return (ceil_div(n, length) if n else 1), length


def tree_plan(n):
    """[(log_len, in_nodes, last_in_len, out_nodes, last_out_len, pass_through)]"""
    pl, l = [], 0
    while n > (1 << l):
        i_n, o_n = ceil_div(n, 1 << l), ceil_div(n, 2 << l)
        pl.append((l, i_n, n - ((i_n - 1) << l), o_n, n - ((o_n - 1) << (l + 1)), bool(i_n & 1)))
        l += 1
    return pl


def tree_split(log_len, split=TREE_SPLIT):
    """poly_tree_split with kPolyTreeSplit = `split` (the build's: the default)."""
    length = 1 << log_len
    if 2 * length <= BLOCK:
        return 1
    return max(1, min(split, length // TREE_TILE))


def tree_steps(n, log_len):
    """The steps of its left operand each multiplying block of a level with
    2 len > BLOCK takes before they are dealt over blockIdx.y (the trips of
    k_poly_tree_level's i0 loop), one entry per tile; no such block: []."""
    length = 1 << log_len
    if 2 * length <= BLOCK:
        return []
    steps = []
    for g0 in range(0, n, BLOCK):
        off = (g0 >> (log_len + 1)) << (log_len + 1)
        rem = n - off
        if rem <= length:
            continue
        a, b = length, min(rem - length, length)
        k0 = g0 - off
        i_min = k0 - b + 1 if k0 >= b else 0
        steps.append(ceil_div(min(k0 + BLOCK, a) - i_min, TREE_TILE))
    return steps


def tree_most_steps(n):
    """(steps, log_len, parts): the most steps one block of the tree over n
    points takes, at the highest level where it does, and that level's parts."""
    best = (0, 0, 1)
    for (log_len, *_rest) in tree_plan(n):
        most = max(tree_steps(n, log_len), default=0)
        if most >= best[0] and most > 0:
            best = (most, log_len, tree_split(log_len))
    return best


# --- k_poly_eval / k_poly_eval_combine -----------------------------------------------
def evaluate(p, coeffs, xs, num_cus, grid_x=None):
    d, m = len(coeffs), len(xs)
    if m == 0:
        return []
    chunks, chunk_len = eval_plan(m, d, num_cus)
    C, X = _Table(d, coeffs), _Table(m, xs)
    cells = _Table(chunks * m)
    tiles = ceil_div(m, BLOCK)
    gx = min(grid_x or tiles, tiles)
    for by in range(chunks):
        lo = by * chunk_len
        assert lo <= d
        hi = d if d - lo < chunk_len else lo + chunk_len
        for bx in range(gx):
            for tl in range(bx, tiles, gx):
                cf = _Lds(EVAL_TILE)
                acc = [0] * BLOCK
                top = hi
                while top > lo:
                    base = top - EVAL_TILE if top - lo > EVAL_TILE else lo
                    cnt = top - base
                    for e in range(cnt):
                        cf.put(e, C.ld(base + e))
                    for t in range(BLOCK):
                        i = tl * BLOCK + t
                        x = X.ld(i) if i < m else 0
                        for k in range(cnt - 1, -1, -1):
                            acc[t] = (acc[t] * x + cf.get(k)) % p
                    top = base
                for t in range(BLOCK):
                    i = tl * BLOCK + t
                    if i < m:
                        cells.st(by * m + i, acc[t])
    if chunks == 1:
        return cells.v
    out = _Table(m)
    for i in range(m):
        x = X.ld(i)
        xl = 1
        for b in range((chunk_len | 1).bit_length() - 1, -1, -1):
            xl = xl * xl % p
            if (chunk_len >> b) & 1:
                xl = xl * x % p
        acc = cells.ld((chunks - 1) * m + i)
        for c in range(chunks - 2, -1, -1):
            acc = (acc * xl + cells.ld(c * m + i)) % p
        out.st(i, acc)
    return out.v


# --- k_poly_weights / k_poly_leaves ---------------------------------------------------
def leaves(p, xs, ys, num_cus, grid_x=None):
    """(M, N, dup): level 0 of the tree and the duplicate flag."""
    n = len(xs)
    parts_n, part_len = weights_plan(n, num_cus)
    X, Y = _Table(n, xs), _Table(n, ys)
    parts = _Table(parts_n * n)
    tiles = ceil_div(n, BLOCK)
    gx = min(grid_x or tiles, tiles)
    for by in range(parts_n):
        j_lo = by * part_len
        assert j_lo <= n
        j_hi = n if n - j_lo < part_len else j_lo + part_len
        for bx in range(gx):
            for tl in range(bx, tiles, gx):
                acc = [1] * BLOCK
                for j0 in range(j_lo, j_hi, BLOCK):
                    xj = _Lds(BLOCK)
                    cnt = min(BLOCK, j_hi - j0)
                    for t in range(cnt):
                        xj.put(t, X.ld(j0 + t))
                    for t in range(BLOCK):
                        i = tl * BLOCK + t
                        xi = X.ld(i) if i < n else 0
                        for jj in range(cnt):
                            df = (xi - xj.get(jj)) % p
                            if j0 + jj == i:
                                df = 1
                            acc[t] = acc[t] * df % p
                for t in range(BLOCK):
                    i = tl * BLOCK + t
                    if i < n:
                        parts.st(by * n + i, acc[t])
    M, N, dup = _Table(n), _Table(n), 0
    for i in range(n):
        dd = parts.ld(i)
        for q in range(1, parts_n):
            dd = dd * parts.ld(q * n + i) % p
        if dd == 0:
            dup = 1
        N.st(i, Y.ld(i) * pow(dd, p - 2, p) % p)
        M.st(i, (0 - X.ld(i)) % p)
    return M.v, N.v, dup


# --- k_poly_tree_level ----------------------------------------------------------------
def tree_level(p, Min, Nin, n, log_len, grid_x=None, split=TREE_SPLIT):
    T, W = TREE_TILE, TREE_TILE + BLOCK
    Mi, Ni = _Table(n, Min), _Table(n, Nin)
    Mo, No = _Table(n), _Table(n)
    length = 1 << log_len
    S = tree_split(log_len, split)  # gridDim.y
    Mp, Np = _Table(S * n), _Table(S * n)
    tiles = ceil_div(n, BLOCK)
    gx = min(grid_x or tiles, tiles)
    for bx in range(gx):
        for tl in range(bx, tiles, gx):
            g0 = tl * BLOCK
            if 2 * length <= BLOCK:
                mr, nr = _Lds(W), _Lds(W)
                for t in range(BLOCK):
                    if g0 + t < n:
                        mr.put(t, Mi.ld(g0 + t))
                        nr.put(t, Ni.ld(g0 + t))
                for t in range(BLOCK):
                    g = g0 + t
                    if g >= n:
                        continue
                    off = (g >> (log_len + 1)) << (log_len + 1)
                    assert off >= g0
                    rem = n - off
                    if rem <= length:
                        m_out, n_out = mr.get(t), nr.get(t)
                    else:
                        a, b = length, min(rem - length, length)
                        k, lb = g - off, off - g0
                        rb = lb + a
                        assert k < a + b
                        wm = wn = 0
                        i_lo = k - b + 1 if k >= b else 0
                        i_hi = k + 1 if k < a else a
                        for i in range(i_lo, i_hi):
                            l_m, l_n = mr.get(lb + i), nr.get(lb + i)
                            r_m, r_n = mr.get(rb + k - i), nr.get(rb + k - i)
                            wm += l_m * r_m
                            wn += l_n * r_m + r_n * l_m
                        m_out, n_out = wm % p, wn % p
                        if k >= a:
                            m_out = (m_out + mr.get(rb + k - a)) % p
                            n_out = (n_out + nr.get(rb + k - a)) % p
                        if k >= b and k - b < a:
                            m_out = (m_out + mr.get(lb + k - b)) % p
                            n_out = (n_out + nr.get(lb + k - b)) % p
                    Mo.st(g, m_out)
                    No.st(g, n_out)
            else:
                off = (g0 >> (log_len + 1)) << (log_len + 1)
                rem = n - off
                if rem <= length:
                    for t in range(BLOCK):  # (blockIdx.y == 0 only)
                        if g0 + t < n:
                            Mo.st(g0 + t, Mi.ld(g0 + t))
                            No.st(g0 + t, Ni.ld(g0 + t))
                    continue
                a, b = length, min(rem - length, length)
                k0 = g0 - off
                assert k0 + BLOCK <= 2 * length  # the tile lies in one pair
                i_min = k0 - b + 1 if k0 >= b else 0
                i_end = min(k0 + BLOCK, a)
                for y in range(S):  # blockIdx.y
                    wm, wn = [0] * BLOCK, [0] * BLOCK
                    for q, i0 in enumerate(range(i_min, i_end, T)):
                        if q % S != y:
                            continue
                        ml, nl, mr, nr = _Lds(T), _Lds(T), _Lds(W), _Lds(W)
                        jbase = k0 - i0 - (T - 1)
                        for t in range(T):
                            i = i0 + t
                            ml.put(t, Mi.ld(off + i) if i < a else 0)
                            nl.put(t, Ni.ld(off + i) if i < a else 0)
                        for w in range(W):
                            j = jbase + w
                            inside = 0 <= j < b
                            mr.put(w, Mi.ld(off + a + j) if inside else 0)
                            nr.put(w, Ni.ld(off + a + j) if inside else 0)
                        for t in range(BLOCK):
                            for e in range(T):
                                l_m, l_n = ml.get(e), nl.get(e)
                                r_m, r_n = mr.get(t + T - 1 - e), nr.get(t + T - 1 - e)
                                wm[t] += l_m * r_m
                                wn[t] += l_n * r_m + r_n * l_m
                    if S > 1:
                        for t in range(BLOCK):
                            if k0 + t < a + b:
                                Mp.st(y * n + g0 + t, wm[t] % p)
                                Np.st(y * n + g0 + t, wn[t] % p)
                        continue
                    for t in range(BLOCK):
                        k = k0 + t
                        if k < a + b:
                            g = g0 + t
                            assert g < n
                            m_out, n_out = wm[t] % p, wn[t] % p
                            if k >= a:
                                m_out = (m_out + Mi.ld(off + a + (k - a))) % p
                                n_out = (n_out + Ni.ld(off + a + (k - a))) % p
                            if k >= b and k - b < a:
                                m_out = (m_out + Mi.ld(off + (k - b))) % p
                                n_out = (n_out + Ni.ld(off + (k - b))) % p
                            Mo.st(g, m_out)
                            No.st(g, n_out)
                        else:
                            assert g0 + t >= n
    if S > 1:  # k_poly_tree_combine
        for g in range(n):
            off = (g >> (log_len + 1)) << (log_len + 1)
            rem = n - off
            if rem <= length:
                continue
            a, b, k = length, min(rem - length, length), g - off
            m_out, n_out = Mp.ld(g), Np.ld(g)
            for y in range(1, S):
                m_out = (m_out + Mp.ld(y * n + g)) % p
                n_out = (n_out + Np.ld(y * n + g)) % p
            if k >= a:
                m_out = (m_out + Mi.ld(off + a + (k - a))) % p
                n_out = (n_out + Ni.ld(off + a + (k - a))) % p
            if k >= b and k - b < a:
                m_out = (m_out + Mi.ld(off + (k - b))) % p
                n_out = (n_out + Ni.ld(off + (k - b))) % p
            Mo.st(g, m_out)
            No.st(g, n_out)
    assert None not in Mo.v and None not in No.v
    return Mo.v, No.v


def interpolate(p, points, num_cus=256, grid_x=None, split=TREE_SPLIT):
    """The device path end to end: weights, leaves, the levels of tree_plan,
    trim. Raises ZeroDivisionError where the library returns ZK_EINVAL. `split`
    stands in for kPolyTreeSplit (a smaller one wraps the deal at smaller n)."""
    n = len(points)
    if n == 0:
        return []
    M, N, dup = leaves(p, [x % p for x, _ in points], [y % p for _, y in points], num_cus, grid_x)
    if dup:
        raise ZeroDivisionError("two points with the same x")
    for (log_len, *_rest) in tree_plan(n):
        M, N = tree_level(p, M, N, n, log_len, grid_x, split)
    while N and N[-1] == 0:
        N.pop()
    return N
