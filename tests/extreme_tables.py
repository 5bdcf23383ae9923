"""Saturating and boundary-value tables for the GKR round kernels (test helper,
not a test module).

The matrix-core kernels (csrc/mfma.hpp) take the signed 8-bit digits of the
256-bit word a device table holds IN MEMORY, which is the Montgomery form. So
every pattern here is defined on that word; the canonical value the oracle
needs is word * R^-1 mod p (R = 2^256). A table is built from a small palette
of words and an index array, so 2^20-element tables cost no Python loop.

Special words per field (all below p, tests/test_extreme_tables_cpu.py):
  0, 1, p - 1
  sat-  ((p >> 248) - 1) << 248 | 0x7F..7F80: digits [-128] * 31 + [p >> 248];
        its encoding carries out of the low 128 bits and ripples through every
        high word (0x7F7F7F7F + 0x80808080 = 0xFFFFFFFF) into the top byte
  sat+  ((p >> 248) - 1) << 248 | 0x7F..7F7F: digits [127] * 31 + [(p >> 248) - 1], no carry
  half  = sat- (low 128 bits 0x7F..7F80, high words 0x7F7F7F7F) and
  below = sat+ (one less in the low half, no carry): kept under both names.

Variable 0 is the top index bit (tests/gkr_step_sums.py _corner).
"""
from __future__ import annotations

import numpy as np

import pyoracle as po

R = 1 << 256
K = int.from_bytes(b"\x80" * 32, "little")  # 0x8080...80, the digit offset of mfma.hpp to_digits
FIELDS = (0, 1, 2)


def modulus(field: int) -> int:
    return po.MODULI[field]


def specials(field: int) -> dict[str, int]:
    p = modulus(field)
    top = ((p >> 248) - 1) << 248
    body = int.from_bytes(b"\x7f" * 31, "little")  # bytes 0..30 = 0x7F
    sat_pos = top | body
    sat_neg = top | (body + 1)  # byte 0 = 0x80
    return {"zero": 0, "one": 1, "pm1": p - 1, "sat+": sat_pos, "sat-": sat_neg, "half": sat_neg, "below": sat_pos}


def special_list(field: int) -> list[int]:
    """The seven special words in the order `sprinkled` cycles through."""
    s = specials(field)
    return [s[k] for k in ("zero", "one", "pm1", "sat+", "sat-", "half", "below")]


def canonical(field: int, word: int) -> int:
    """The field element a device table holding `word` stands for."""
    p = modulus(field)
    return word * pow(R, -1, p) % p


def montgomery(field: int, value: int) -> int:
    return value * R % modulus(field)


def limbs(values) -> np.ndarray:
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(bytearray(buf), dtype="<u8").reshape(-1, 4)


class Table:
    """One table: the in-memory (Montgomery) words and the canonical values, uint64[N, 4] each."""

    def __init__(self, field: int, palette: list[int], index: np.ndarray | None = None):
        p = modulus(field)
        rinv = pow(R, -1, p)
        w, c = limbs(palette), limbs([x * rinv % p for x in palette])
        self.palette = list(palette)
        self.words = w if index is None else np.ascontiguousarray(w[index])
        self.canon = c if index is None else np.ascontiguousarray(c[index])

    def word_ints(self) -> list[int]:
        return ints(self.words)

    def canon_ints(self) -> list[int]:
        return ints(self.canon)


def ints(a: np.ndarray) -> list[int]:
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i: i + 32], "little") for i in range(0, len(b), 32)]


def _parity(x: np.ndarray) -> np.ndarray:
    x = x.copy()
    for s in (16, 8, 4, 2, 1):
        x ^= x >> s
    return (x & 1).astype(np.intp)


def _const(field: int, n: int, word: int) -> Table:
    return Table(field, [word], np.zeros(1 << n, np.intp))


def top3_mask(n: int) -> int:
    return 7 << (n - 3)


def const_neg_neg(field: int, n: int) -> list[Table]:
    s = specials(field)
    return [_const(field, n, s["sat-"]) for _ in range(4)]


def const_pos_neg(field: int, n: int) -> list[Table]:
    s = specials(field)
    return [_const(field, n, s["sat+" if t in (0, 2) else "sat-"]) for t in range(4)]


def const_pm1(field: int, n: int) -> list[Table]:
    return [_const(field, n, modulus(field) - 1) for _ in range(4)]


def checker_pm1(field: int, n: int) -> list[Table]:
    """A, M: p - 1 where the parity of the top three index bits is odd, else 0; S, P: the complement."""
    par = _parity((np.arange(1 << n, dtype=np.int64) & top3_mask(n)))
    pm1 = modulus(field) - 1
    return [Table(field, [0, pm1], par if t in (0, 2) else 1 - par) for t in range(4)]


def checker_sat(field: int, n: int, mask: int) -> list[Table]:
    """A, M: sat- / sat+ by the parity of i & mask (even: sat-); S, P: all sat-."""
    s = specials(field)
    par = _parity(np.arange(1 << n, dtype=np.int64) & mask)
    return [Table(field, [s["sat-"], s["sat+"]], par) if t in (0, 2) else _const(field, n, s["sat-"]) for t in range(4)]


def sprinkled(field: int, n: int, seed: int = 29) -> list[Table]:
    """synth tables with element i replaced by special[(i // stride) % 7] when
    i % stride == 0: stride 37 for A and M, 41 for S and P."""
    import coracle as co

    sp = special_list(field)
    out = []
    for t in range(4):
        stride = 37 if t in (0, 2) else 41
        words = [montgomery(field, v) for v in ints(co.synth(field, seed, t, 0, 1 << n))]
        for i in range(0, 1 << n, stride):
            words[i] = sp[(i // stride) % 7]
        out.append(Table(field, words))
    return out


FAMILIES = {
    "const_neg_neg": const_neg_neg,
    "const_pos_neg": const_pos_neg,
    "const_pm1": const_pm1,
    "checker_pm1": checker_pm1,
    "checker_sat_top3": lambda field, n: checker_sat(field, n, top3_mask(n)),
    "checker_sat_lane": lambda field, n: checker_sat(field, n, 1),
    "checker_sat_group": lambda field, n: checker_sat(field, n, 1 << 5),
    "sprinkled": sprinkled,
}


def family(name: str, field: int, n: int) -> list[Table]:
    """The four tables (A, S, M, P) of family `name` over 2^n elements, n >= 3."""
    assert n >= 3
    return FAMILIES[name](field, n)


# ---------------------------------------------------------------------------
# The boundary palette and the table families of the composed sum-check
# ---------------------------------------------------------------------------
def palette(field: int) -> list[int]:
    """The boundary words a table can hold in memory, all below p, sorted: the
    ends and the middle of [0, p); R mod p (the image of 1) with its
    neighbours and R^2 mod p; around every 32-bit limb boundary from below
    (2^(32k), 2^(32k) - 1) and from above (p - 2^(32k), p - 2^(32k) + 1), whose
    sums and differences carry or borrow through k limbs; the word whose low
    seven limbs are all ones under the largest top limb that keeps it below p;
    sat+ and sat-. 42 words in each of the three fields."""
    p = modulus(field)
    r = R % p
    words = {0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, r, r - 1, r + 1, r * r % p}
    for k in range(1, 8):
        words |= {w for w in (1 << 32 * k, (1 << 32 * k) - 1, p - (1 << 32 * k), p - (1 << 32 * k) + 1) if 0 <= w < p}
    words.add((((p >> 224) - 1) << 224) | ((1 << 224) - 1))
    s = specials(field)
    words |= {s["sat+"], s["sat-"]}
    assert all(0 <= w < p for w in words)
    return sorted(words)


SPRINKLE_POOL = 211  # synth words a `sprinkled` composed table draws from (a prime, so no stride lines up with it)


def _all_bits_parity(nvars: int) -> np.ndarray:
    x = np.arange(1 << nvars, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        x ^= x >> s
    return (x & 1).astype(np.intp)


def _composed_table(name: str, field: int, t: int, nvars: int, seed: int) -> Table:
    p, n = modulus(field), 1 << nvars
    if name == "const_pm1":
        return Table(field, [p - 1], np.zeros(n, np.intp))
    if name == "const_sat":
        return Table(field, [specials(field)["sat-"]], np.zeros(n, np.intp))
    if name == "checker_pm1":
        par = _all_bits_parity(nvars)
        return Table(field, [0, p - 1], par if t % 2 == 0 else 1 - par)
    pal = palette(field)
    i = np.arange(n, dtype=np.int64)
    if name == "palette_cycle":
        return Table(field, pal, ((i * (2 * t + 1)) % len(pal)).astype(np.intp))
    assert name == "sprinkled"
    import coracle as co

    pool = ints(co.synth(field, seed, t, 0, SPRINKLE_POOL))  # (below p: valid words as they are)
    index = np.random.default_rng(1000 * seed + t).integers(0, SPRINKLE_POOL, n).astype(np.intp)
    stride = 37 if t % 2 == 0 else 41
    at = np.arange(0, n, stride)
    index[at] = SPRINKLE_POOL + (at // stride) % len(pal)
    return Table(field, pool + pal, index)


COMPOSED_FAMILIES = ("const_pm1", "const_sat", "checker_pm1", "sprinkled", "palette_cycle")


def composed_family(name: str, field: int, ntables: int, nvars: int, seed: int = 29) -> list[Table]:
    """`ntables` tables of 2^nvars words for the composed sum-check, each a
    palette plus an index array (no per-element Python work at size):
      const_pm1      every word p - 1
      const_sat      every word sat-
      checker_pm1    0 or p - 1 by the parity of ALL index bits, even-numbered
                     tables the complement of odd-numbered ones: both hi - lo
                     and lo - hi occur in every pair, and the pattern survives
                     every fold (a top-bit checker is gone after one round)
      sprinkled      synth words (SPRINKLE_POOL of them per table, drawn by a
                     seeded index) with a palette word at every 37th index
                     (41st in odd-numbered tables)
      palette_cycle  element i of table t is palette word (i (2t + 1)) mod 42
    """
    assert name in COMPOSED_FAMILIES
    return [_composed_table(name, field, t, nvars, seed) for t in range(ntables)]
