"""Boundary cases for the KZG path's kernel code — csrc/ec.hpp (BLS12-381 Fq and
G1), csrc/msm.hpp (signed-digit Pippenger) — with their expected values from
Python integers (test helper, not a test module).

Everything is exact: a case is a few raw Montgomery words (R = 2^384, 12 x u32
per Fq element, what the kernels hold in registers and memory), the expected
value an integer or a group element. tests/native/ec_probe.hip (built into
zk_amd/_lib/libzkecprobe.so) applies one ec.hpp function per element to such
words, on the host (device = 0) or on the GPU (device = 1):
tests/test_ec_cases_cpu.py and tests/test_gpu_ec_probe.py run the same cases
through the two legs.

Group elements are compared as group elements: an output is normalised here
(None for infinity, else the canonical affine pair), so a Jacobian or XYZZ
result may use any Z. Every output word must be below p, and an XYZZ output
must keep ZZ^3 = ZZZ^2.

kzg_oracle.mul reduces its scalar mod r; the point T = (0, 2) (order 3) and the
palette points are not in the r-torsion in general, so `mul_int` does not
reduce, and `msm_expected` folds scalars mod r only over bases k G, mod 3 over
T, and as plain integers over the palette points.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

import kzg_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zk-research-implementations_amd")
PROBE_PATH = os.path.join(PKG, "zk_amd", "_lib", "libzkecprobe.so")
PROBE_SRC = os.path.join(ROOT, "tests", "native", "ec_probe.hip")

P = ko.Q  # the base field's modulus
R = ko.R  # the group order (the scalar field's modulus)
RM = 1 << 384  # the Montgomery radix of ec.hpp
RINV = pow(RM, -1, P)
G = ko.G1
T = (0, 2)  # on y^2 = x^3 + 4, order 3; only (0, 0) stands for infinity


def mont(x: int) -> int:
    return x * RM % P


def canon(w: int) -> int:
    return w * RINV % P


# ---- the 381-bit palette --------------------------------------------------------------
def palette() -> list[int]:
    """extreme_tables.palette's recipe for R = 2^384: the ends and the middle of
    [0, p), R mod p with its neighbours and R^2 mod p, both sides of every
    32-bit limb boundary k = 1..11 from below and from above, and eleven
    all-ones low limbs under the largest top limb that stays below p. 56 words."""
    r = RM % P
    words = {0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, r, r - 1, r + 1, r * r % P}
    for k in range(1, 12):
        words |= {w for w in (1 << 32 * k, (1 << 32 * k) - 1, P - (1 << 32 * k), P - (1 << 32 * k) + 1) if 0 <= w < P}
    words.add((((P >> 352) - 1) << 352) | ((1 << 352) - 1))
    assert all(0 <= w < P for w in words)
    return sorted(words)


PALETTE = palette()
NOT_CANONICAL = [P, P + 1, 2 * P - 1, RM - 1, P + (1 << 352), (P & ((1 << 352) - 1)) | (0xFFFFFFFF << 352)]
BELOW_2P = [P, P + 1, 2 * P - 1]  # fq_reduce_once's domain above p


def words_array(words) -> np.ndarray:
    """integers below 2^384 -> uint32[n, 12], little-endian limbs"""
    buf = b"".join(int(w).to_bytes(48, "little") for w in words)
    return np.frombuffer(bytearray(buf), dtype="<u4").reshape(-1, 12)


def array_words(a: np.ndarray) -> list[int]:
    b = np.ascontiguousarray(a, dtype="<u4").tobytes()
    return [int.from_bytes(b[i: i + 48], "little") for i in range(0, len(b), 48)]


# ---- Fq cases -------------------------------------------------------------------------
FQ_OPS = ("add", "sub", "neg", "dbl", "mul", "sqr", "to_mont", "from_mont", "inv", "reduce_once", "is_canonical")
FQ_BINARY = ("add", "sub", "mul")


def fq_cases(op: str):
    """-> (a words, b words or None, expected words)"""
    pal = PALETTE
    if op in FQ_BINARY:
        a = [x for x in pal for _ in pal]
        b = [y for _ in pal for y in pal]
        f = {"add": lambda x, y: (x + y) % P, "sub": lambda x, y: (x - y) % P, "mul": lambda x, y: x * y * RINV % P}[op]
        return a, b, [f(x, y) for x, y in zip(a, b)]
    if op == "reduce_once":
        a = pal + BELOW_2P
        return a, None, [x % P for x in a]
    if op == "is_canonical":
        a = pal + NOT_CANONICAL
        return a, None, [int(x < P) for x in a]
    f = {"neg": lambda x: -x % P, "dbl": lambda x: 2 * x % P, "sqr": lambda x: x * x * RINV % P,
         "to_mont": lambda x: x * RM % P, "from_mont": lambda x: x * RINV % P,
         "inv": lambda x: pow(x * RINV, P - 2, P) * RM % P}[op]  # (0 maps to 0)
    return pal, None, [f(x) for x in pal]


# ---- curve points ---------------------------------------------------------------------
def mul_int(k: int, pt):
    """k * pt for a non-negative integer k, NOT reduced mod r (pt need not have order r)"""
    acc = None
    while k:
        if k & 1:
            acc = ko.add(acc, pt)
        pt = ko.add(pt, pt)
        k >>= 1
    return acc


def palette_points() -> list:
    """The curve points whose MONTGOMERY x-coordinate is a palette word."""
    out = []
    for w in PALETTE:
        x = canon(w)
        rhs = (x * x * x + 4) % P
        y = pow(rhs, (P + 1) // 4, P)  # p = 3 mod 4
        if y * y % P == rhs:
            out.append((x, y))
    return out


PALETTE_POINTS = palette_points()
POINTS = [G, ko.add(G, G), ko.neg(G), T] + PALETTE_POINTS
_NONZERO_WORDS = [w for w in PALETTE if w]
GARBAGE = (PALETTE[-1], (P - 1) // 2, RM % P)  # non-zero words under an infinity's Z = 0


class Opd(NamedTuple):
    """One operand: a point (None: infinity) scaled by lam (Z = lam canonical);
    an infinity is g1_inf() / g1x_inf(), or Z = 0 over non-zero garbage."""
    pt: tuple | None
    lam: int = 1
    garbage: bool = False


def enc_affine(o: Opd) -> list[int]:
    return [0, 0] if o.pt is None else [mont(o.pt[0]), mont(o.pt[1])]


def enc_jac(o: Opd) -> list[int]:
    if o.pt is None:
        return [GARBAGE[0], GARBAGE[1], 0] if o.garbage else [0, RM % P, 0]
    x, y = o.pt
    l2 = o.lam * o.lam % P
    return [mont(x * l2), mont(y * l2 * o.lam), mont(o.lam)]


def enc_xyzz(o: Opd) -> list[int]:
    if o.pt is None:
        return [GARBAGE[0], GARBAGE[1], 0, GARBAGE[2]] if o.garbage else [0, 0, 0, 0]
    x, y = o.pt
    l2 = o.lam * o.lam % P
    l3 = l2 * o.lam % P
    return [mont(x * l2), mont(y * l3), mont(l2), mont(l3)]


def _below_p(words):
    assert all(w < P for w in words), "an output word is not below p"


def dec_affine(words):
    _below_p(words)
    x, y = (canon(w) for w in words)
    return None if x == 0 and y == 0 else (x, y)


def dec_jac(words):
    _below_p(words)
    X, Y, Z = (canon(w) for w in words)
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def dec_xyzz(words):
    _below_p(words)
    X, Y, ZZ, ZZZ = (canon(w) for w in words)
    if ZZ == 0:
        return None
    assert pow(ZZ, 3, P) == ZZZ * ZZZ % P, "XYZZ output with ZZ^3 != ZZZ^2"
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def lams(i: int) -> tuple[int, int]:
    """Two different scalings for point i: one of 2, p - 1, 1 (canonical), and
    the value whose Montgomery word is a non-zero palette word."""
    a = (2, P - 1, 1)[i % 3]
    b = canon(_NONZERO_WORDS[(7 * i + 3) % len(_NONZERO_WORDS)])
    if b in (a, 1):
        b = canon(_NONZERO_WORDS[(7 * i + 4) % len(_NONZERO_WORDS)])
    return a, b


INF, GINF = Opd(None), Opd(None, garbage=True)


def pair_cases() -> list:
    """-> [(label, Opd a, Opd b, expected a + b)] for every two-operand op"""
    out = [("inf+inf", INF, INF), ("inf+ginf", INF, GINF), ("ginf+inf", GINF, INF), ("ginf+ginf", GINF, GINF)]
    for i, pt in enumerate(POINTS):
        la, lb = lams(i)
        q = POINTS[(i + 1) % len(POINTS)]
        d = ko.add(pt, pt)
        n = ko.neg(pt)
        out += [
            (f"P{i}+P same Z", Opd(pt, la), Opd(pt, la)),
            (f"P{i}+P Z=1", Opd(pt), Opd(pt)),
            (f"P{i}+P other Z", Opd(pt, la), Opd(pt, lb)),
            (f"P{i}+P other Z'", Opd(pt, lb), Opd(pt, 1)),
            (f"P{i}-P same Z", Opd(pt, la), Opd(n, la)),
            (f"P{i}-P other Z", Opd(pt, la), Opd(n, lb)),
            (f"P{i}-P other Z'", Opd(pt, lb), Opd(n, 1)),
            (f"P{i}+Q", Opd(pt, la), Opd(q, lb)),
            (f"P{i}+Q Z=1", Opd(pt), Opd(q)),
            (f"P{i}+2P", Opd(pt, la), Opd(d, lb)),
            (f"2P{i}+P", Opd(d, lb), Opd(pt)),
            (f"inf+P{i}", INF, Opd(pt, lb)),
            (f"P{i}+inf", Opd(pt, lb), INF),
            (f"ginf+P{i}", GINF, Opd(pt, la)),
            (f"P{i}+ginf", Opd(pt, la), GINF),
        ]
    out += [("T+T", Opd(T, lams(3)[1]), Opd(T)), ("T+2T", Opd(T, 2), Opd(ko.neg(T), P - 1))]
    return [(label, a, b, ko.add(a.pt, b.pt)) for label, a, b in out]


def unary_operands() -> list[Opd]:
    out = [INF, GINF]
    for i, pt in enumerate(POINTS):
        la, lb = lams(i)
        out += [Opd(pt), Opd(pt, la), Opd(pt, lb)]
    return out


MUL_SMALL_KS = (0, 1, 2, 3, 1 << 31, (1 << 32) - 1)


def mul_small_cases() -> list:
    """-> [(Opd, k, expected)]: G, T and infinity in several representations"""
    ops = [Opd(G), Opd(G, lams(0)[1]), Opd(T), Opd(T, lams(3)[1]), Opd(T, P - 1), INF, GINF]
    return [(o, k, mul_int(k, o.pt)) for o in ops for k in MUL_SMALL_KS]


# ---- the probe ------------------------------------------------------------------------
G1_OPS = ("g1_dbl", "g1_add", "g1_add_mixed", "g1x_dbl", "g1x_add", "g1x_add_mixed", "g1x_to_jac", "g1_to_affine",
          "g1_to_affine_zi", "g1_mul_small", "g1_from_affine")
# words per element of (a, b, out), as ec_probe.hip's zk_ecprobe_g1_shape reports them
G1_SHAPES = {"g1_dbl": (36, 0, 36), "g1_add": (36, 36, 36), "g1_add_mixed": (36, 24, 36), "g1x_dbl": (48, 0, 48),
             "g1x_add": (48, 48, 48), "g1x_add_mixed": (48, 24, 48), "g1x_to_jac": (48, 0, 36),
             "g1_to_affine": (36, 0, 24), "g1_to_affine_zi": (36, 12, 24), "g1_mul_small": (36, 1, 36),
             "g1_from_affine": (24, 0, 36)}
_ENC = {24: enc_affine, 36: enc_jac, 48: enc_xyzz}
_DEC = {24: dec_affine, 36: dec_jac, 48: dec_xyzz}


class Probe:
    def __init__(self, path: str = PROBE_PATH):
        self.lib = C.CDLL(path)
        u32p = C.POINTER(C.c_uint32)
        for name in ("zk_ecprobe_fq", "zk_ecprobe_g1"):
            fn = getattr(self.lib, name)
            fn.argtypes = [C.c_int, C.c_int, u32p, u32p, C.c_uint64, u32p]
            fn.restype = C.c_int
        self.lib.zk_ecprobe_g1_shape.argtypes = [C.c_int, u32p]
        self.lib.zk_ecprobe_g1_shape.restype = C.c_int

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))

    def fq(self, op: str, device: int, a, b=None) -> list[int]:
        """op over lists of words -> list of output words; RuntimeError on a nonzero return code"""
        wa = np.ascontiguousarray(words_array(a))
        wb = None if b is None else np.ascontiguousarray(words_array(b))
        out = np.zeros_like(wa)
        rc = self.lib.zk_ecprobe_fq(FQ_OPS.index(op), device, self._p(wa), self._p(wb), len(a), self._p(out))
        if rc:
            raise RuntimeError(f"zk_ecprobe_fq({op}, device={device}) returned {rc}")
        return array_words(out)

    def g1_shape(self, op: str) -> tuple:
        s = (C.c_uint32 * 3)()
        assert self.lib.zk_ecprobe_g1_shape(G1_OPS.index(op), s) == 0
        return tuple(s)

    def g1(self, op: str, device: int, a_rows: list, b_rows: list | None = None) -> list:
        """op over rows of words (b rows: words, or one u32 for g1_mul_small) -> rows of output words"""
        sa, sb, so = G1_SHAPES[op]
        n = len(a_rows)
        wa = np.ascontiguousarray(words_array([w for row in a_rows for w in row]).reshape(n, sa))
        wb = None
        if sb == 1:
            wb = np.array(b_rows, dtype="<u4").reshape(n, 1)
        elif sb:
            wb = np.ascontiguousarray(words_array([w for row in b_rows for w in row]).reshape(n, sb))
        out = np.zeros((n, so), dtype="<u4")
        rc = self.lib.zk_ecprobe_g1(G1_OPS.index(op), device, self._p(wa), self._p(wb), n, self._p(out))
        if rc:
            raise RuntimeError(f"zk_ecprobe_g1({op}, device={device}) returned {rc}")
        flat = array_words(out.reshape(-1, 12))
        k = so // 12
        return [flat[i * k: (i + 1) * k] for i in range(n)]


def fq_failures(probe: Probe, op: str, device: int) -> list:
    a, b, want = fq_cases(op)
    got = probe.fq(op, device, a, b)
    return [(op, hex(x), hex(b[i]) if b else None, hex(w), hex(g))
            for i, (x, w, g) in enumerate(zip(a, want, got)) if w != g]


def g1_cases(op: str):
    """-> (labels, a rows, b rows or None, expected group elements)"""
    sa, sb, _ = G1_SHAPES[op]
    if op in ("g1_add", "g1_add_mixed", "g1x_add", "g1x_add_mixed"):
        cs = pair_cases()
        if sb == 24:  # the affine operand has one representation: (0, 0) for either infinity
            cs = [c for c in cs if not c[2].garbage]
        return ([c[0] for c in cs], [_ENC[sa](c[1]) for c in cs], [_ENC[sb](c[2]) for c in cs], [c[3] for c in cs])
    if op == "g1_mul_small":
        cs = mul_small_cases()
        return ([f"{k} * {o}" for o, k, _ in cs], [enc_jac(o) for o, _, _ in cs], [k for _, k, _ in cs],
                [w for _, _, w in cs])
    if op == "g1_from_affine":
        ops = [INF] + [Opd(pt) for pt in POINTS]
        return [str(o) for o in ops], [enc_affine(o) for o in ops], None, [o.pt for o in ops]
    ops = unary_operands()
    labels = [str(o) for o in ops]
    if op in ("g1_dbl", "g1x_dbl"):
        return labels, [_ENC[sa](o) for o in ops], None, [ko.add(o.pt, o.pt) for o in ops]
    if op == "g1_to_affine_zi":  # b: Z^-1 (ignored for an infinity: any word)
        zi = [[mont(pow(o.lam, -1, P)) if o.pt is not None else GARBAGE[2]] for o in ops]
        return labels, [enc_jac(o) for o in ops], zi, [o.pt for o in ops]
    return labels, [_ENC[sa](o) for o in ops], None, [o.pt for o in ops]  # g1x_to_jac, g1_to_affine


def g1_failures(probe: Probe, op: str, device: int) -> list:
    labels, a, b, want = g1_cases(op)
    got = probe.g1(op, device, a, b)
    dec = _DEC[G1_SHAPES[op][2]]
    bad = []
    for label, w, g in zip(labels, want, got):
        try:
            pt = dec(g)
        except AssertionError as e:
            bad.append((op, label, str(e)))
            continue
        if pt != w:
            bad.append((op, label, w, pt))
    return bad


# ---- signed digits and window widths (csrc/msm.hpp, csrc/kzg.hip restated) ------------------
MSM_WIDTHS = (6, 8, 10, 13, 16, 20)  # msm_window_bits' candidates
BUCKET_COST = 5.0
SORT_BINS_MAX = 16896


def window_shape(c0: int) -> tuple[int, int]:
    """(W, cb) for a requested width c0: W = ceil(256 / c0) windows of cb = ceil(256 / W) bits"""
    W = -(-256 // c0)
    return W, -(-256 // W)


def sort_bins(c0: int, levels: int = 0) -> int:
    """the bucket sort's coarse bins (msm.hpp k_sort_hist): Wt << C"""
    W, cb = window_shape(c0)
    bb = cb - 1
    return (levels * W if levels else W) << (bb - bb // 2)


def msm_window_bits(n: int, levels: int = 0, forced: int | None = None) -> int:
    """kzg.hip msm_window_bits: forced is ZK_MSM_C"""
    if forced is not None and 6 <= forced <= 20:
        return forced
    lg = n.bit_length() - 1
    if lg < 12 and levels == 0:
        return min(20, max(6, lg - 3 if lg > 9 else 6))
    best, best_cost = 0, float("inf")
    for cc in MSM_WIDTHS:
        W, cb = window_shape(cc)
        bb = cb - 1
        Wt = levels * W if levels else W
        if Wt << (bb - bb // 2) > SORT_BINS_MAX or (levels == 0 and cc == 6):
            continue
        cost = float(n) * W + BUCKET_COST * Wt * float(1 << bb)
        if cost < best_cost:
            best, best_cost = cc, cost
    assert best
    return best


def signed_digits(s: int, c: int, W: int):
    """msm.hpp signed_digits: -> ([(w, raw, magnitude, negative)] for every window, final carry).
    A window with magnitude 0 is skipped by the kernels; magnitude 2^(c-1) goes to bucket 0."""
    half, carry, out = 1 << (c - 1), 0, []
    for w in range(W):
        raw = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        neg = int(raw > half)
        carry = neg
        out.append((w, raw, (1 << c) - raw if neg else raw, neg))
    return out, carry


def half_all(c: int) -> int:
    """H(c): every window that fits below 2^254 at exactly 2^(c-1)"""
    return sum(1 << (c * w + c - 1) for w in range(256) if c * w + c - 1 <= 253)


def scalar_family(c: int) -> list[int]:
    """The scalars that reach signed_digits' edges at width c; all canonical."""
    h = half_all(c)
    alt = [sum(((1 << c) - 1) << (c * w) for w in range(ph, 256, 2) if c * (w + 1) <= 254) for ph in (0, 1)]
    fam = [h, h + 1, h - 1, (1 << 254) - 1, R - 1, R - 2, 0, 1, 1 << (c - 1), (1 << c) - 1, 1 << c] + alt
    assert all(0 <= s < R for s in fam)
    return fam


def byte_family() -> list[int]:
    """Scalars at the byte boundaries of k_fixed_base8's 32 unsigned 8-bit windows:
    runs of 0xff, single bytes, and r - 1."""
    fam = [0, 1, 0xFF, 0x100, 0xFFFF, 0xFF00, (1 << 248) - 1, 0xFF << 240, 1 << 248, 0x73 << 248, R - 1, R - 2,
           int.from_bytes(b"\xff\x00" * 15 + b"\xff\x00", "little"), int.from_bytes(b"\x00\xff" * 15 + b"\x00\x00", "little")]
    fam += [0xFF << (8 * k) for k in (1, 7, 8, 15, 16, 30)] + [1 << (8 * k) for k in (1, 4, 8, 31)]
    assert all(0 <= s < R for s in fam)
    return fam


# ---- MSM oracle over mixed bases --------------------------------------------------------
class Base(NamedTuple):
    kind: str  # "g": k * G; "t": T; "p": a palette point; "inf"
    k: int
    pt: tuple | None


def base_g(k: int) -> Base:
    return Base("g", k, ko.mul(k, G))


BASE_T = Base("t", 0, T)
BASE_INF = Base("inf", 0, None)


def base_palette(i: int) -> Base:
    return Base("p", i, PALETTE_POINTS[i])


def msm_expected(bases: list[Base], scalars: list[int]):
    """sum_i scalars[i] * bases[i] without a group operation per term: scalars fold
    mod r over the bases k G, mod 3 over T, and as integers over each palette point."""
    g, t, pal = 0, 0, {}
    for b, s in zip(bases, scalars):
        if b.kind == "g":
            g += s * b.k
        elif b.kind == "t":
            t += s
        elif b.kind == "p":
            pal[b.k] = pal.get(b.k, 0) + s
    acc = ko.add(ko.mul(g % R, G), mul_int(t % 3, T))
    for i, s in sorted(pal.items()):
        acc = ko.add(acc, mul_int(s, PALETTE_POINTS[i]))
    return acc
