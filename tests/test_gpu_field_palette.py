"""csrc/field.hpp as hipcc generates it for gfx950, on the boundary palette
(tests/extreme_tables.py palette: 42 words per field), and the canonical check
every upload runs.

tests/test_field_palette_cpu.py checks the same source, compiled for the host,
on the same pairs; here the kernels that are nothing but one field operation
per element (k_mle_tensor, k_mle_map, k_fold) run them on the device. Tables go
up as Montgomery words and come down as Montgomery words, so what is compared
is the operation's own output, (a + b) mod p, (a - b) mod p and a b R^-1 mod p
on the words, with no conversion in the way.

The canonical check (k_check_canonical) gets every way a 256-bit word can fail
to be below p, alone in an otherwise valid table, at the first index, the last
one (a block of its own) and in between. ZK_GRID_CAP does not cap the grid of
the upload's kernels (host.hpp grid_for), so the in-between case under
ZK_GRID_CAP=1 is one more position, not a later iteration of a thread's loop;
that loop is reached by the 2^20 + 1-element table, whose last element no
resident grid of a 256-CU device covers in its first pass."""
from __future__ import annotations

import numpy as np
import pytest

import coracle as co
import extreme_tables as xt

import zk_amd
from zk_amd._lib import ZK_EINVAL, ZK_OK, check, lib
from zk_amd.api import MLE_ADD, MLE_MUL, MLE_SUB
from zk_amd.context import REPR_CANONICAL, REPR_MONTGOMERY
from zk_amd.elems import as_limbs, ptr, to_ints

pytestmark = pytest.mark.gpu
FIELDS = [0, 1, 2]
R = xt.R


def padded(field: int) -> list[int]:
    """The 42 palette words repeated to 64."""
    pal = xt.palette(field)
    return [pal[i % len(pal)] for i in range(64)]


def expected(field: int, op: int, a: int, b: int) -> int:
    p = xt.modulus(field)
    return (a + b) % p if op == MLE_ADD else (a - b) % p if op == MLE_SUB else a * b * pow(R, -1, p) % p


@pytest.mark.parametrize("field", FIELDS)
def test_tensor_of_the_palette_with_itself(ctx, field):
    """palette (x) palette: all pairs under + and x, 4096 outputs (sixteen blocks)."""
    words = padded(field)
    d = ctx.upload(field, xt.limbs(words), REPR_MONTGOMERY)
    out = ctx.alloc(field, 64 * 64)
    for op in (MLE_ADD, MLE_MUL):
        check(lib().zk_dev_mle_tensor(ctx.h, field, op, d.ptr, 64, d.ptr, 64, out.ptr))
        assert to_ints(out.download(REPR_MONTGOMERY)) == [expected(field, op, a, b) for a in words for b in words], op
    d.free()
    out.free()


@pytest.mark.parametrize("field", FIELDS)
def test_map_of_the_palette_against_its_rotations(ctx, field):
    """The element-wise map MultilinearPoly's + - * go through (zk_mle_binop, which takes a
    representation): the padded palette against each of its 64 rotations, in one table of 4096."""
    words = padded(field)
    a = words * 64
    b = [words[(i + k) % 64] for k in range(64) for i in range(64)]
    la, lb = xt.limbs(a), xt.limbs(b)
    out = np.zeros((4096, 4), np.uint64)
    for op in (MLE_SUB, MLE_ADD, MLE_MUL):
        check(lib().zk_mle_binop(ctx.h, field, REPR_MONTGOMERY, op, ptr(la), 12, ptr(lb), 12, ptr(out)))
        assert to_ints(out) == [expected(field, op, x, y) for x, y in zip(a, b)], op
    pairs = set(zip(a, b))
    assert len(pairs) == 42 * 42  # (every pair of palette words, in both orders)


@pytest.mark.parametrize("field", FIELDS)
def test_scale_by_every_palette_word(ctx, field):
    words = padded(field)
    lw = xt.limbs(words)
    out = np.zeros((64, 4), np.uint64)
    for s in xt.palette(field):
        check(lib().zk_mle_scale(ctx.h, field, REPR_MONTGOMERY, ptr(lw), 6, ptr(xt.limbs([s])), ptr(out)))
        assert to_ints(out) == [expected(field, MLE_MUL, w, s) for w in words], hex(s)


@pytest.mark.parametrize("field", FIELDS)
def test_partial_evaluate_of_a_palette_table(ctx, field):
    """A 7-variable palette_cycle table folded at every bit by r = 0, 1, p - 1, R mod p and sat-, each
    once as the value (canonical) and once as the word the kernel multiplies by (Montgomery)."""
    p, n = xt.modulus(field), 7
    t = xt.composed_family("palette_cycle", field, 2, n)[1]  # (table 1: stride 3 through the palette)
    rs = [0, 1, p - 1, R % p, xt.specials(field)["sat-"]]
    d_in = ctx.upload(field, t.words, REPR_MONTGOMERY)
    d_out = ctx.alloc(field, 1 << (n - 1))
    for repr_ in (REPR_CANONICAL, REPR_MONTGOMERY):
        for r in rs:
            value = r if repr_ == REPR_CANONICAL else xt.canonical(field, r)
            for bit in range(n):
                check(lib().zk_dev_mle_partial_evaluate(ctx.h, field, d_in.ptr, n, bit, repr_, ptr(as_limbs([r])), d_out.ptr))
                assert np.array_equal(d_out.download(), co.partial_evaluate(field, t.canon, bit, value)), (repr_, hex(r), bit)
    assert np.array_equal(d_in.download(REPR_MONTGOMERY), t.words)
    d_in.free()
    d_out.free()


# ---- the canonical check at upload --------------------------------------------------
N = 1025


def not_below_p(field: int) -> list[int]:
    p = xt.modulus(field)
    vals = [p, p + 1, p + (1 << 64), (1 << 256) - 1, p + (1 << 224), p + (1 << 192),
            ((p - 1) & ((1 << 224) - 1)) | (0xFFFFFFFF << 224)]
    assert all(p <= v < 1 << 256 for v in vals)
    return vals


def _valid_table(field: int, count: int) -> np.ndarray:
    """count words below p: the palette, cycled (valid in both representations)."""
    pal = xt.limbs(xt.palette(field))
    return np.ascontiguousarray(pal[np.arange(count) % len(pal)])


def _upload_rc(ctx, field, repr_, table, dev) -> int:
    return lib().zk_dev_upload(ctx.h, field, repr_, ptr(table), table.shape[0], dev.ptr)


def _check_positions(ctx, field, positions):
    p = xt.modulus(field)
    base = _valid_table(field, N)
    dev = ctx.alloc(field, N)
    for repr_ in (REPR_CANONICAL, REPR_MONTGOMERY):
        for at in positions:
            for v in not_below_p(field):
                bad = base.copy()
                bad[at] = xt.limbs([v])[0]
                assert _upload_rc(ctx, field, repr_, bad, dev) == ZK_EINVAL, (repr_, at, hex(v))
            good = base.copy()
            good[at] = xt.limbs([p - 1])[0]
            assert _upload_rc(ctx, field, repr_, good, dev) == ZK_OK, (repr_, at)
            assert np.array_equal(dev.download(repr_), good), (repr_, at)
    dev.free()


@pytest.mark.parametrize("field", FIELDS)
def test_upload_rejects_every_word_not_below_p(ctx, field):
    _check_positions(ctx, field, (0, N - 1))


def test_upload_rejects_in_a_single_capped_grid(monkeypatch):
    monkeypatch.setenv("ZK_GRID_CAP", "1")
    ctx = zk_amd.Context(0)
    try:
        for field in FIELDS:
            _check_positions(ctx, field, (777,))
    finally:
        ctx.close()


@pytest.mark.parametrize("field", FIELDS)
def test_upload_rejects_in_a_later_pass_of_the_grid(ctx, field):
    """2^20 + 1 elements: more than any resident grid has threads (256 CUs x 2048 lanes = 2^19), so
    the last element is read in a thread's second or later iteration."""
    n = (1 << 20) + 1
    p = xt.modulus(field)
    table = _valid_table(field, n)
    dev = ctx.alloc(field, n)
    for repr_ in (REPR_CANONICAL, REPR_MONTGOMERY):
        table[n - 1] = xt.limbs([p])[0]
        assert _upload_rc(ctx, field, repr_, table, dev) == ZK_EINVAL
        table[n - 1] = xt.limbs([p - 1])[0]
        assert _upload_rc(ctx, field, repr_, table, dev) == ZK_OK
    assert np.array_equal(dev.download(REPR_MONTGOMERY), table)
    dev.free()
