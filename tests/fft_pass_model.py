"""The index arithmetic of k_fft_pass (csrc/fft.hpp) restated in Python, one
statement per statement of the kernel: which global element a tile slot
loads, its inter-pass twiddle exponent and the Hi/Lo split, the in-place
decimation-in-frequency stages and their stage-root index, and where the store
phase fetches from (the bit-reversed row) and writes to. It runs a whole
transform from a plan [(a, log_ns, log_c), ...] as csrc/fft_plan.hpp gives it,
asserts that every index is in range and every output written exactly once, and
returns the result for comparison with tests/fft_oracle.py. Arithmetic is plain
ints mod p; nothing of the GPU is needed."""
from __future__ import annotations

TILE_ELEMS_LOG_MAX = 12  # sanity only: the plan's a + log_c is what sizes a tile


def _brev(k: int, bits: int) -> int:
    return int(format(k, "0%db" % bits)[::-1], 2) if bits else 0


def transform(x, m: int, plan, w: int, p: int, scale: int = 1) -> list[int]:
    """The passes of `plan` over x (2^m values) with root w (w^-1 for the inverse);
    `scale` (n^-1 for the inverse) rides where the host puts it: on the last pass's
    Lo table, or on the way in when there is one pass."""
    n = 1 << m
    assert len(x) == n and sum(a for a, _, _ in plan) == m
    if m == 0:
        return list(x)
    h = (m + 1) // 2
    passes = len(plan)
    log_w = max(a for a, _, _ in plan)
    stage_roots = [pow(w, t * (n >> log_w), p) for t in range(1 << (log_w - 1))]
    lo = [pow(w, i, p) for i in range(1 << h)] if passes > 1 else []
    hi = [pow(w, i << h, p) for i in range(1 << (m - h))] if passes > 1 else []
    cur = list(x)
    for pi, (a, log_ns, log_c) in enumerate(plan):
        last = pi == passes - 1
        R, C, E = 1 << a, 1 << log_c, 1 << (a + log_c)
        assert a + log_c <= TILE_ELEMS_LOG_MAX and n % E == 0
        ns_mask = (1 << log_ns) - 1
        log_l = min(log_c, log_ns)
        out = [None] * n
        for tl in range(n >> (a + log_c)):
            j0 = tl << log_c
            tile = [None] * E
            for e in range(E):  # load (+ twiddle)
                jj, r = e & (C - 1), e >> log_c
                src = j0 + jj + r * (n >> a)
                assert src < n
                v = cur[src]
                if log_ns > 0:
                    ex = (r * ((j0 + jj) & ns_mask)) << (m - log_ns - a)
                    assert ex < n and (ex >> h) < len(hi) and (ex & ((1 << h) - 1)) < len(lo)
                    tw = hi[ex >> h] * lo[ex & ((1 << h) - 1)] % p
                    v = v * tw % p * (scale if last else 1) % p
                elif passes == 1:
                    v = v * scale % p
                tile[e] = v
            for s in range(a - 1, -1, -1):  # stages
                half = 1 << s
                for b in range(E // 2):
                    jj, rr = b & (C - 1), b >> log_c
                    i = rr & (half - 1)
                    r = ((rr >> s) << (s + 1)) | i
                    e0 = (r << log_c) | jj
                    e1 = e0 + (half << log_c)
                    assert e1 < E
                    u, v = tile[e0], tile[e1]
                    tile[e0] = (u + v) % p
                    d = (u - v) % p
                    if s > 0:
                        ri = i << (log_w - s - 1)
                        assert ri < len(stage_roots)
                        d = d * stage_roots[ri] % p
                    tile[e1] = d
            for o in range(E):  # store
                jlo = o & ((1 << log_l) - 1)
                k = (o >> log_l) & (R - 1)
                jhi = o >> (log_l + a)
                jj = (jhi << log_l) | jlo
                assert jj < C
                j = j0 + jj
                dst = ((j >> log_ns) << (log_ns + a)) + (j & ns_mask) + (k << log_ns)
                assert dst < n and out[dst] is None
                out[dst] = tile[(_brev(k, a) << log_c) | jj]
        assert None not in out
        cur = out
    return cur
