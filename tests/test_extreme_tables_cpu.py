"""Paper audit, in exact Python integers, of the range claims the matrix-core
GKR kernels rest on (csrc/mfma.hpp: comments and static_asserts), and of the
table families of tests/extreme_tables.py that drive the kernels to those
ranges on the GPU (tests/test_gpu_extreme_tables.py).

* Digit model: to_digits and to_digits_halves, on the special words and the
  edges of the lazy ranges; kLazyDigits as mfma.hpp evaluates it.
* Tile bounds: the k*ChunksMax constants are read from mfma.hpp, so the audit
  follows the code: int32 tile slots, the flush of a block's waves, the
  anti-diagonal sums T_d, the word sums S_w, G and G + M in 17 words.
* Fold bounds: position sums, the word_of assembly, |Y|, and the range
  dm_finish's two conditional subtractions must cover; dm_finish itself as a
  Python model against (x00 + Y 2^-64) mod p at the extremes.
* Families: every word is below p; the canonical tables are word R^-1 mod p.
"""
from __future__ import annotations

import os
import random
import re

import pytest

import extreme_tables as xt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFMA = os.path.join(ROOT, "zk-research-implementations_amd", "csrc", "mfma.hpp")
FIELDS = xt.FIELDS
M256 = (1 << 256) - 1


# ---------------------------------------------------------------------------
# digit models
# ---------------------------------------------------------------------------
def digits(x: int) -> list[int]:
    """mfma.hpp to_digits on the two's-complement 256-bit word of x: byte k of
    ((x + K) mod 2^256) xor K, read as int8."""
    y = (((x & M256) + xt.K) & M256) ^ xt.K
    return [b - 256 if b >= 128 else b for b in y.to_bytes(32, "little")]


def digits_halves(x: int) -> tuple[list[int], int, int]:
    """mfma.hpp to_digits_halves: each 128-bit half adds its half of K, the
    low half's carry enters the high half, then the xor. Also returns that
    carry and the high half before the carry comes in."""
    m128, k128 = (1 << 128) - 1, xt.K & ((1 << 128) - 1)
    lo, hi = (x & M256) & m128, (x & M256) >> 128
    lo += k128
    carry, lo = lo >> 128, lo & m128
    hi_before = (hi + k128) & m128
    hi = (hi_before + carry) & m128
    y = ((hi << 128) | lo) ^ xt.K
    return [b - 256 if b >= 128 else b for b in y.to_bytes(32, "little")], carry, hi_before


def value_of(d: list[int]) -> int:
    return sum(dk << (8 * k) for k, dk in enumerate(d))


def lazy_digits(field: int) -> bool:
    """kLazyDigits<F> exactly as mfma.hpp:60 evaluates it, from F::P[7]."""
    p7 = xt.modulus(field) >> 224
    return p7 * 2 + 2 < 0x7F7F7F7F


@pytest.mark.parametrize("field", FIELDS)
def test_lazy_predicate_is_the_digit_range(field):
    p = xt.modulus(field)
    assert lazy_digits(field) == (2 * p < (1 << 256) - xt.K)
    assert lazy_digits(field) == (field != 2)  # both BN254 fields lazy, BLS12-381 Fr reduced
    assert p < (1 << 256) - xt.K and p <= xt.K  # [0, p) and (-p, 0] always have valid digits


@pytest.mark.parametrize("field", FIELDS)
def test_digit_model_reproduces_the_value(field):
    p = xt.modulus(field)
    vals = xt.special_list(field)
    if lazy_digits(field):
        vals += [2 * p - 2, -(p - 1), -(2 * p - 2)]  # lazy2's (-p, 2p), dm_fold's |d1|, |d2| < p and |d3| < 2p
    else:  # outside the digit range: the reduced branch is needed, not merely chosen
        assert value_of(digits(2 * p - 2)) != 2 * p - 2
    for x in vals:
        d = digits(x)
        assert all(-128 <= k <= 127 for k in d)
        assert value_of(d) == x, hex(x)
    s = xt.specials(field)
    top = p >> 248
    assert digits(s["sat-"]) == [-128] * 31 + [top]  # (the carry of byte 30 lands in the top digit)
    assert digits(s["sat+"]) == [127] * 31 + [top - 1]
    assert s["half"] == s["sat-"] and s["below"] == s["sat+"]


@pytest.mark.parametrize("field", FIELDS)
def test_halves_model_is_the_whole_word_model(field):
    p = xt.modulus(field)
    for x in xt.special_list(field):
        assert digits_halves(x)[0] == digits(x), hex(x)
    rng = random.Random(1000 + field)
    for _ in range(10000):
        x = rng.getrandbits(256)
        assert digits_halves(x)[0] == digits(x), hex(x)
    # sat-: the low half carries out, and the carry ripples through all four
    # high words, each 0x7F7F7F7F + 0x80808080 = 0xFFFFFFFF before it comes in
    s = xt.specials(field)
    _, carry, hi_before = digits_halves(s["sat-"])
    assert carry == 1
    assert [(hi_before >> (32 * j)) & 0xFFFFFFFF for j in range(3)] == [0xFFFFFFFF] * 3
    assert (hi_before >> 96) & 0x00FFFFFF == 0xFFFFFF  # the top word's low three bytes; its top byte is p's
    assert digits_halves(s["sat+"])[1] == 0 and digits_halves(p - 1)[0] == digits(p - 1)


# ---------------------------------------------------------------------------
# tile bounds
# ---------------------------------------------------------------------------
def read_constants(path: str = MFMA) -> dict:
    src = open(path).read()

    def one(pat):
        m = re.findall(pat, src)
        assert len(m) == 1, (pat, m)
        return m[0]

    c = {k: int(one(rf"constexpr uint32_t {k} = (\d+);")) for k in ("kD0MChunksMax", "kDMChunksMax", "kD0TChunksMax")}
    a, b = one(r"constexpr uint32_t kT33ChunksMax = OCT == 64 \? (\d+) : (\d+);")
    c["kT33ChunksMax"] = {64: int(a), 32: int(b)}
    a, b = one(r"constexpr uint32_t kT33SlotMfmas = OCT == 64 \? (\d+) : (\d+);")
    c["kT33SlotMfmas"] = {64: int(a), 32: int(b)}
    return c


def moment_slot_mfmas() -> int:
    """MFMAs that one moment_products call adds into its busiest tile slot:
    16 products (ux, vy) into slot 3 d(ux >> 1, vy >> 1) + d(ux & 1, vy & 1)."""
    md = lambda x, y: x if x == y else 2  # noqa: E731  (moment_digit)
    cnt = [0] * 9
    for ux in range(4):
        for vy in range(4):
            cnt[3 * md(ux >> 1, vy >> 1) + md(ux & 1, vy & 1)] += 1
    assert sum(cnt) == 16
    return max(cnt)


def kernels(c: dict) -> dict:
    """Per matrix-core step kernel: MFMAs into the busiest int32 tile slot per
    chunk, the chunk maximum the host keeps a block (d0m: a wave) to, the
    waves of a block whose tiles flush into ONE category, the products
    (hypercube points) one MFMA sums, and whether the operands include lazy
    extended points (else corners or reduced values only).
      d0m  one MFMA per grid point and chunk of 32 quads (d0m_phase); all four
           waves hold all nine categories (two wave pairs x two products).
      dm   (and dm3) two K = 32 MFMAs per category and chunk of 64 quads
           (dm_products); waves w and w ^ 1 share categories 4 (w >> 1) .. +3.
      d0t  one moment_products call per chunk of 32 octants; the two s waves
           (1 and 2) share nine categories.
      t33  two (32-octant) or four (64-octant: two K halves) calls per chunk,
           both products into the same tiles; the s waves as d0t."""
    per_call = moment_slot_mfmas()
    assert c["kT33SlotMfmas"] == {32: 2 * per_call, 64: 4 * per_call}
    return {
        "d0m": dict(mfmas=1, chunks=c["kD0MChunksMax"], waves=4, lazy=True),
        "dm": dict(mfmas=2, chunks=c["kDMChunksMax"], waves=2, lazy=True),
        "d0t": dict(mfmas=per_call, chunks=c["kD0TChunksMax"], waves=2, lazy=False),
        "t33<32>": dict(mfmas=c["kT33SlotMfmas"][32], chunks=c["kT33ChunksMax"][32], waves=2, lazy=False),
        "t33<64>": dict(mfmas=c["kT33SlotMfmas"][64], chunks=c["kT33ChunksMax"][64], waves=2, lazy=False),
    }


def digit_maxima(field: int, lazy: bool) -> list[int]:
    """Largest |digit k| of an operand: 128 for k < 31 (sat- reaches it); digit
    31 = floor((x + K) / 2^248) - 128 grows with x, so its extremes are at the
    ends of the operand range: [0, p) or, with lazy points, (-p, 2p)."""
    p = xt.modulus(field)
    ends = [-(p - 1), 2 * p - 2] if lazy and lazy_digits(field) else [0, p - 1]
    return [128] * 31 + [max(abs(digits(x)[31]) for x in ends)]


def tile_audit(field: int, k: dict) -> None:
    p = xt.modulus(field)
    # an MFMA sums 32 points: at most 32 * 128 * 128 = 2^19 per slot entry, and
    # sat- * sat- adds exactly that to every entry with k, l < 31
    sat = digits(xt.specials(field)["sat-"])
    assert all(32 * sat[a] * sat[b] == 1 << 19 for a in range(31) for b in range(31))
    slot = k["mfmas"] * k["chunks"] << 19  # the busiest slot entry after the chunk maximum
    assert slot <= 1 << 30, "int32 tile bound"
    # flush_tiles: the block's waves add their slots (int64 atomics) into the
    # anti-diagonal sums T_d, d = k + l; entry (k, l) scales with the operands' digit maxima
    m = digit_maxima(field, k["lazy"])
    per_entry = k["waves"] * k["mfmas"] * k["chunks"] * 32  # products summed into an entry of a category
    T = [sum(per_entry * m[a] * m[d - a] for a in range(32) if 0 <= d - a < 32) for d in range(63)]
    assert max(T) < 1 << 37, "tiles_to_words: |T_d| < 2^37"
    # S_w = sum_{i<4} T[4w+i] 2^(8i), then + offset word (< 2^32) + carry in int64
    S = [sum(T[4 * w + i] << (8 * i) for i in range(4) if 4 * w + i < 63) for w in range(17)]
    assert max(S) < 1 << 62, "tiles_to_words: |S_w| < 2^62"
    G = sum(t << (8 * d) for d, t in enumerate(T))
    assert G == sum(s << (32 * w) for w, s in enumerate(S))
    M = p << 275
    assert G < M, "|G| < M = p 2^275"
    # both signs (const_neg_neg: every entry +, const_pos_neg: every entry -):
    # G + M is non-negative and fits 17 words, and every carry stays in int64
    for sign in (1, -1):
        assert 0 <= sign * G + M < 1 << (32 * 17)
        carry = 0
        words = []
        for w in range(17):
            v = sign * S[w] + ((M >> (32 * w)) & 0xFFFFFFFF) + carry
            assert -(1 << 63) <= v < 1 << 63
            words.append(v & 0xFFFFFFFF)
            carry = v >> 32
        assert carry == 0 and sum(x << (32 * w) for w, x in enumerate(words)) == sign * G + M


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kernel", ["d0m", "dm", "d0t", "t33<32>", "t33<64>"])
def test_tile_bounds_at_the_chunk_maximum(field, kernel):
    tile_audit(field, kernels(read_constants())[kernel])


def test_tile_audit_follows_the_constants(tmp_path):
    """The audit reads mfma.hpp: a copy with one chunk maximum doubled fails it."""
    src = open(MFMA).read()
    c = read_constants()
    t64, t32 = c["kT33ChunksMax"][64], c["kT33ChunksMax"][32]
    edits = [(f"k{n}ChunksMax = {c[f'k{n}ChunksMax']};", f"k{n}ChunksMax = {2 * c[f'k{n}ChunksMax']};", kern)
             for n, kern in (("D0M", "d0m"), ("DM", "dm"), ("D0T", "d0t"))]
    edits += [(f"kT33ChunksMax = OCT == 64 ? {t64} : {t32};", f"kT33ChunksMax = OCT == 64 ? {2 * t64} : {t32};", "t33<64>"),
              (f"kT33ChunksMax = OCT == 64 ? {t64} : {t32};", f"kT33ChunksMax = OCT == 64 ? {t64} : {2 * t32};", "t33<32>")]
    for i, (old, new, kernel) in enumerate(edits):
        assert src.count(old) == 1, old
        bad = tmp_path / f"mfma_{i}.hpp"
        bad.write_text(src.replace(old, new))
        k = kernels(read_constants(str(bad)))[kernel]
        with pytest.raises(AssertionError, match="int32 tile bound"):
            tile_audit(0, k)


# ---------------------------------------------------------------------------
# fold bounds
# ---------------------------------------------------------------------------
def fold_position_max(K: int) -> int:
    """Largest |position sum| of a fold MFMA: K terms (constant digit) x (input digit), |digit| <= 128."""
    return K * 128 * 128


def fold_y_max(K: int) -> int:
    """|Y| <= the position sums at byte offsets 0 .. 31."""
    return sum(fold_position_max(K) << (8 * pos) for pos in range(32))


def test_fold_position_sums_and_word_assembly():
    # k_gkr_dm: three constants x 32 digits, K = 96: the comment's |.| < 2^21
    assert fold_position_max(96) < 1 << 21
    # k_gkr_t33 / k_gkr_dm3 fold by eight eq weights, K = 256: 2^22, NOT below
    # the 2^21 the k_gkr_dm comment states for K = 96. That bound is not the one
    # the code relies on: the sums live in int32 accumulators, word_of assembles
    # four of them into an int64, and dm_finish needs |Y| < 2^271
    assert fold_position_max(256) == 1 << 22
    for K in (96, 256):
        s = fold_position_max(K)
        assert s < 1 << 31
        word = s + (s << 8) + (s << 16) + (s << 24)  # word_of
        assert word < 1 << 62  # + a carry |c| < 2^31 stays inside int64 (dm_finish's first loop)
        assert fold_y_max(K) < 1 << 271


def dm_finish(p: int, W: list[int], x00: int) -> int:
    """mfma.hpp dm_finish in Python integers: Y = sum W[i] 2^(32 i) as a 256-bit
    y plus a signed top, two 32-bit REDC steps, + x00 + p, then at most one
    subtraction of 2p and one of p. Returns s (asserting the claims on the way)."""
    pinv = (-pow(p, -1, 1 << 32)) % (1 << 32)
    Y = sum(w << (32 * i) for i, w in enumerate(W))
    y, top = Y & M256, Y >> 256
    for _ in range(2):
        m = ((y & 0xFFFFFFFF) * pinv) & 0xFFFFFFFF
        t = y + m * p
        assert t & 0xFFFFFFFF == 0
        t = (t >> 32) + (top << 224)  # (Y + m p) / 2^32, exact
        y, top = t & M256, t >> 256
    V = y + (top << 256)
    assert top in (-1, 0)
    s = x00 + V + p
    assert 0 <= s < 1 << 257  # hi is 0 or 1
    if s >= 2 * p:
        s -= 2 * p
    if s >= p:
        s -= p
    return s


@pytest.mark.parametrize("field", FIELDS)
def test_two_conditional_subtractions_reduce_the_fold(field):
    p = xt.modulus(field)
    ymax = fold_y_max(256)  # the larger of the two folds; k_gkr_dm's K = 96 lies inside
    assert fold_y_max(96) < ymax < 1 << 271
    # two REDC steps: V in [(-ymax) / 2^64, (ymax + (2^64 - 1) p) / 2^64], an upper end of
    # about p + p / 2^32; what the subtractions need is 0 <= s < 4p for
    # s = x00 + V + p, x00 in [0, p)
    vmin = -(ymax >> 64) - 1
    vmax = (ymax + ((1 << 64) - 1) * p >> 64) + 1
    assert vmin + p >= 0
    assert (p - 1) + vmax + p < 4 * p
    # and the model of the code agrees with the field at the extremes
    inv64 = pow(1 << 64, -1, p)
    rng = random.Random(2000 + field)
    smax = fold_position_max(256)
    cases = [[smax] * 32, [-smax] * 32, [0] * 32, [smax if i & 1 else -smax for i in range(32)]]
    cases += [[rng.randint(-smax, smax) for _ in range(32)] for _ in range(200)]
    for pos in cases:
        W = [sum(pos[4 * i + j] << (8 * j) for j in range(4)) for i in range(8)]  # word_of
        Y = sum(w << (32 * i) for i, w in enumerate(W))
        assert Y == sum(s << (8 * k) for k, s in enumerate(pos)) and abs(Y) <= ymax
        for x00 in (0, 1, p - 1, rng.randrange(p)):
            assert dm_finish(p, W, x00) == (x00 + Y * inv64) % p


# ---------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [3, 6])
@pytest.mark.parametrize("name", sorted(xt.FAMILIES))
def test_family_words_are_field_elements(field, n, name):
    p = xt.modulus(field)
    tabs = xt.family(name, field, n)
    assert len(tabs) == 4
    for t in tabs:
        words, canon = t.word_ints(), t.canon_ints()
        assert len(words) == len(canon) == 1 << n
        assert all(0 <= w < p for w in words)
        assert all(c < p and c * xt.R % p == w for w, c in zip(words, canon))


@pytest.mark.parametrize("field", FIELDS)
def test_family_patterns(field):
    p, s = xt.modulus(field), xt.specials(field)
    n = 6
    for sp in s.values():
        assert 0 <= sp < p
    A, S, M, P = (t.word_ints() for t in xt.family("checker_pm1", field, n))
    for i in range(1 << n):
        odd = bin(i >> (n - 3)).count("1") & 1
        assert A[i] == M[i] == (p - 1 if odd else 0) and S[i] == P[i] == (0 if odd else p - 1)
    for name, mask in (("checker_sat_top3", 7 << (n - 3)), ("checker_sat_lane", 1), ("checker_sat_group", 1 << 5)):
        A, S, M, P = (t.word_ints() for t in xt.family(name, field, n))
        for i in range(1 << n):
            assert A[i] == M[i] == (s["sat+"] if bin(i & mask).count("1") & 1 else s["sat-"])
            assert S[i] == P[i] == s["sat-"]
    A, S, M, P = (t.word_ints() for t in xt.family("const_pos_neg", field, n))
    assert set(A) == set(M) == {s["sat+"]} and set(S) == set(P) == {s["sat-"]}
    sp = xt.special_list(field)
    A, S, _, _ = (t.word_ints() for t in xt.family("sprinkled", field, 9))
    assert [A[i] for i in range(0, 512, 37)] == [sp[k % 7] for k in range(14)]
    assert [S[i] for i in range(0, 512, 41)] == [sp[k % 7] for k in range(13)]


# ---------------------------------------------------------------------------
# the boundary palette and the composed families
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_palette(field):
    p, s = xt.modulus(field), xt.specials(field)
    pal = xt.palette(field)
    assert len(pal) == len(set(pal)) == 42 and pal == sorted(pal) and all(0 <= w < p for w in pal)
    r = xt.R % p
    must = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, r - 1, r, r + 1, r * r % p, s["sat+"], s["sat-"]]
    for k in range(1, 8):  # (2^224 < p in all three fields: every one of them lies in [0, p))
        must += [1 << 32 * k, (1 << 32 * k) - 1, p - (1 << 32 * k), p - (1 << 32 * k) + 1]
    ones = [w for w in pal if w & ((1 << 224) - 1) == (1 << 224) - 1 and w >> 224]  # (2^224 - 1 is one of `must`)
    assert set(must) < set(pal) and len(set(must)) == 41 and ones == [p - (p & ((1 << 224) - 1)) - 1]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", xt.COMPOSED_FAMILIES)
def test_composed_family_words(field, name):
    p, pal, s = xt.modulus(field), xt.palette(field), xt.specials(field)
    for ntables, nvars in ((1, 1), (5, 7), (16, 3)):
        tabs = xt.composed_family(name, field, ntables, nvars)
        assert len(tabs) == ntables
        for t, tab in enumerate(tabs):
            words, canon = tab.word_ints(), tab.canon_ints()
            assert len(words) == len(canon) == 1 << nvars
            assert all(0 <= w < p and c < p and c * xt.R % p == w for w, c in zip(words, canon))
            if name.startswith("const"):
                assert set(words) == {p - 1 if name == "const_pm1" else s["sat-"]}
            elif name == "checker_pm1":
                assert words == [(p - 1) if (bin(i).count("1") + t) & 1 else 0 for i in range(1 << nvars)]
            elif name == "palette_cycle":
                assert words == [pal[i * (2 * t + 1) % 42] for i in range(1 << nvars)]
            else:
                stride = 41 if t & 1 else 37
                assert [words[i] for i in range(0, 1 << nvars, stride)] == \
                    [pal[k % 42] for k in range(((1 << nvars) + stride - 1) // stride)]
    if name == "sprinkled":  # between the palette words: many distinct synth words, and another table, other words
        a, b = (tab.word_ints() for tab in xt.composed_family(name, field, 2, 9))
        assert len(set(a)) > 150 and len(set(a) & set(b)) <= 42
