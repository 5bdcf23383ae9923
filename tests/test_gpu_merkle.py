"""GPU parity of the Keccak Merkle tree (zk_amd.merkle, csrc/merkle.hpp) with
merkle_tree/src/merkle_tree.rs as restated in tests/merkle_oracle.py: the
reference's own eight tests, whole trees (leaves and every level) on both sides
of the k_merkle_top hand-over, partial inputs, the grid-stride path, a
device-resident input table, batched openings and batched updates."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import coracle as co
import merkle_oracle as mo
import pyoracle as po
from conftest import ROOT

import zk_amd
from zk_amd import _lib, merkle
from zk_amd.elems import as_limbs, ptr
from zk_amd.merkle import LeafSide, MerkleProof, MerkleTree, ProofData

pytestmark = pytest.mark.gpu

FQ = 1  # the reference's tests are over ark_bn254::Fq
FIELDS = [0, 1, 2]


@functools.lru_cache(maxsize=None)
def _inputs(field: int, depth: int, seed: int = 11) -> tuple:
    return tuple(co.from_limbs(co.synth(field, seed, 0, 0, 1 << depth)))


@functools.lru_cache(maxsize=None)
def _checker(field: int, depth: int, n_inputs: int = -1, seed: int = 11) -> mo.Tree:
    """Shared and never modified: tests that update work on a copy (mo.Tree(...) anew)."""
    ins = _inputs(field, depth, seed)
    return mo.Tree(field, depth, ins if n_inputs < 0 else ins[:n_inputs])


def _assert_same_tree(t: MerkleTree, want: mo.Tree) -> None:
    assert t.depth == want.depth
    assert t.leaves() == want.leaves
    for lvl in range(want.depth):
        assert t.level(lvl) == want.tree[lvl], f"level {lvl}"
    assert t.get_root_hash() == want.root()


def _pairs(proof: MerkleProof) -> list:
    return [(p.data_hash, int(p.data_side)) for p in proof.proof]


# --- the reference's tests (:222-367) --------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_create_tree(ctx, field):  # :222-240, :242-251 (test_get_root_hash)
    t = MerkleTree(field, 2, ctx)
    assert len(t.leaves()) == 4 and t.depth == 2
    assert len(t.level(0)) == 2 and len(t.level(1)) == 1
    assert t.leaves() == [0, 0, 0, 0]
    h1 = mo.hash_pair(field, 0, 0)
    h2 = mo.hash_pair(field, h1, h1)
    assert t.get_root_hash() == h2
    assert merkle.hash_pair(merkle.hash_pair(0, 0, field), merkle.hash_pair(0, 0, field), field) == h2


def test_get_root_hash(ctx):  # :242-251
    h1 = mo.hash_pair(FQ, 0, 0)
    assert MerkleTree(FQ, 2, ctx).get_root_hash() == mo.hash_pair(FQ, h1, h1)


@pytest.mark.parametrize("field", FIELDS)
def test_update_leaf(ctx, field):  # :253-273
    t = MerkleTree(field, 2, ctx)
    t.update_leaf(1, 10, False)
    h = mo.compute_hash(field, 10)
    assert t.leaves()[1] == h
    want = mo.hash_pair(field, mo.hash_pair(field, 0, h), mo.hash_pair(field, 0, 0))
    assert t.get_root_hash() == want


@pytest.mark.parametrize("field", FIELDS)
def test_delete_leaf(ctx, field):  # :275-291
    t = MerkleTree(field, 2, ctx)
    t.update_leaf(0, 10, False)
    t.update_leaf(0, 0, True)
    assert t.leaves()[0] == 0
    h1 = mo.hash_pair(field, 0, 0)
    assert t.get_root_hash() == mo.hash_pair(field, h1, h1)


@pytest.mark.parametrize("field", FIELDS)
def test_proof_and_verify(ctx, field):  # :293-305
    t = MerkleTree(field, 3, ctx)
    t.update_leaf(0, 10, False)
    proof = t.create_proof(10, 0)
    assert len(proof.proof) == 3 and all(p.data_side == LeafSide.Right for p in proof.proof)
    assert t.verify(proof) is True


def test_verify_invalid_proof(ctx):  # :307-326
    t = MerkleTree(FQ, 2, ctx)
    assert t.verify(MerkleProof(10, [ProofData(0, LeafSide.Left)] * 2)) is False


def test_create_proof_invalid_data(ctx):  # :328-340
    t = MerkleTree(FQ, 2, ctx)
    t.update_leaf(0, 10, False)
    with pytest.raises(ValueError):
        t.create_proof(20, 0)


@pytest.mark.parametrize("field", FIELDS)
def test_new_with_inputs(ctx, field):  # :342-367
    t = MerkleTree.new_with_inputs(field, 2, [1, 2, 3], ctx)
    leaves = t.leaves()
    assert len(leaves) == 4 and len(t.level(0)) == 2 and len(t.level(1)) == 1
    assert leaves[:3] == [mo.compute_hash(field, v) for v in (1, 2, 3)]
    assert leaves[3] == 0
    with pytest.raises(ValueError):
        MerkleTree.new_with_inputs(field, 2, [1] * 5, ctx)


# --- whole trees ---------------------------------------------------------------------------
@pytest.mark.parametrize("depth", range(1, 13))
def test_whole_tree_matches_checker(ctx, depth):
    """Depth 1-12: trees narrower than, equal to and wider than one block of
    k_merkle_top (1-3 levels of k_merkle_level below it from depth 10 on)."""
    t = MerkleTree.new_with_inputs(FQ, depth, list(_inputs(FQ, depth)), ctx)
    _assert_same_tree(t, _checker(FQ, depth))
    t.close()


@pytest.mark.parametrize("field", FIELDS)
def test_depth10_all_fields_fixture_roots(ctx, field):
    """The fixture's inputs meet every quotient floor(digest / p) (test_merkle_cpu
    asserts the sets are complete): every branch of the device's digest reduction."""
    with open(os.path.join(ROOT, "tests", "golden", "merkle.json")) as fh:
        g = json.load(fh)
    tr = g["trees"][field]
    assert tr["field"] == field
    t = MerkleTree.new_with_inputs(field, 10, list(_inputs(field, 10, g["seed"])), ctx)
    assert t.get_root_hash() == int(tr["root"], 16)
    _assert_same_tree(t, _checker(field, 10, -1, g["seed"]))


@pytest.mark.parametrize("n_inputs", [0, 1, 2, 3, 31, 32])
def test_partial_inputs(ctx, n_inputs):
    t = MerkleTree.new_with_inputs(FQ, 5, list(_inputs(FQ, 5)[:n_inputs]), ctx)
    _assert_same_tree(t, _checker(FQ, 5, n_inputs))
    if n_inputs == 0:
        _assert_same_tree(MerkleTree(FQ, 5, ctx), _checker(FQ, 5, 0))


def test_error_mapping(ctx):
    p = po.MODULI[FQ]
    with pytest.raises(ValueError):
        MerkleTree.new_with_inputs(FQ, 5, [1] * 33, ctx)
    with pytest.raises(ValueError):
        MerkleTree(FQ, 0, ctx)  # get_root_hash would index tree[depth - 1]
    with pytest.raises(ValueError):
        MerkleTree.new_with_inputs(FQ, 3, [1, p, 2], ctx)
    with pytest.raises(ValueError):
        MerkleTree.new_with_inputs(FQ, 3, as_limbs([1, p - 1, p]), ctx, repr=1)
    t = MerkleTree.new_with_inputs(FQ, 3, [1, 2, 3], ctx)
    before = t.leaves()
    for bad in ((8, 1, False), (1 << 40, 1, True), (0, p, False), (0, p, True)):
        with pytest.raises(ValueError):
            t.update_leaf(*bad)
    with pytest.raises(ValueError):
        t.update_leaves([1, 2, 9], [5, 6, 7], [False] * 3)  # one bad id: nothing applied
    with pytest.raises(ValueError):
        t.update_leaves([1, 2], [5, p], [False] * 2)  # one bad value: nothing applied
    assert t.leaves() == before and t.get_root_hash() == mo.Tree(FQ, 3, [1, 2, 3]).root()
    h = C.c_void_p()
    assert _lib.lib().zk_merkle_new(ctx.h, FQ, 3, 0, ptr(as_limbs([1, p])), 2, C.byref(h)) == _lib.ZK_EINVAL
    assert not h.value
    t.close()
    with pytest.raises(ValueError):
        t.get_root_hash()


def test_grid_stride_path(monkeypatch):
    """A context created under ZK_GRID_CAP=3 launches at most 3 blocks: every wide
    level of the depth-12 tree takes several nodes per thread."""
    monkeypatch.setenv("ZK_GRID_CAP", "3")
    capped = zk_amd.Context(0)
    monkeypatch.delenv("ZK_GRID_CAP")
    try:
        t = MerkleTree.new_with_inputs(FQ, 12, list(_inputs(FQ, 12)), capped)
        _assert_same_tree(t, _checker(FQ, 12))
        ids = [0, 4095, 1234, 1235, 77]
        t.update_leaves(ids, [5, 6, 7, 8, 9], [False] * 5)
        want = mo.Tree(FQ, 12, _inputs(FQ, 12))
        for i, v in zip(ids, [5, 6, 7, 8, 9]):
            want.update_leaf(i, v, False)
        _assert_same_tree(t, want)
        t.close()
    finally:
        capped.close()


@pytest.mark.parametrize("field", FIELDS)
def test_device_table_input(ctx, field):
    depth, n = 6, 50
    vals = list(_inputs(field, depth)[:n])
    want = _checker(field, depth, n)
    table = ctx.upload(field, vals)
    _assert_same_tree(MerkleTree.new_with_inputs(field, depth, table, ctx), want)
    _assert_same_tree(MerkleTree.new_with_inputs(field, depth, table), want)  # the table's own context
    _assert_same_tree(MerkleTree.new_with_inputs(field, depth, vals, ctx), want)
    _assert_same_tree(MerkleTree.new_with_inputs(field, depth, as_limbs(vals), ctx), want)
    mont = table.download(repr=1)
    _assert_same_tree(MerkleTree.new_with_inputs(field, depth, mont, ctx, repr=1), want)
    t = MerkleTree.new_with_inputs(field, depth, vals, ctx)
    assert np.array_equal(t.level_limbs(2, repr=1), ctx.upload(field, want.tree[2]).download(repr=1))
    with pytest.raises(ValueError):
        MerkleTree.new_with_inputs((field + 1) % 3, depth, table, ctx)  # another field
    with pytest.raises(ValueError):
        MerkleTree.new_with_inputs(field, 5, table, ctx)  # 50 inputs > 2^5
    other = zk_amd.Context(0)
    try:
        with pytest.raises(ValueError):
            MerkleTree.new_with_inputs(field, depth, table, other)  # another context
    finally:
        other.close()
    table.free()


# --- openings -----------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 11])
def test_openings(ctx, depth):
    ins = _inputs(FQ, depth)
    want = _checker(FQ, depth)
    t = MerkleTree.new_with_inputs(FQ, depth, list(ins), ctx)
    n = 1 << depth
    for leaf in (0, n - 1, n // 2 - 3 if depth > 3 else 5):
        proof = t.create_proof(ins[leaf], leaf)
        assert (proof.data, _pairs(proof)) == want.create_proof(ins[leaf], leaf)
        assert t.verify(proof) and merkle.verify_proof(want.root(), proof, FQ)
        assert want.verify(proof.data, _pairs(proof))
    ids = [(37 * k + 5) % n for k in range(64)]  # (repeats at depth 3: openings may share leaves)
    batch = t.create_proofs([ins[i] for i in ids], ids)
    assert len(batch) == 64
    for i, proof in zip(ids, batch):
        assert proof == t.create_proof(ins[i], i)
        assert (proof.data, _pairs(proof)) == want.create_proof(ins[i], i)
        assert t.verify(proof) and want.verify(proof.data, _pairs(proof))
    # wrong data / a bad id: ValueError, and the C entry point writes nothing (all or nothing)
    with pytest.raises(ValueError):
        t.create_proof(ins[1], 0)
    with pytest.raises(ValueError):
        t.create_proof(ins[0], n)
    with pytest.raises(ValueError):
        t.create_proofs([ins[0], ins[1], po.MODULI[FQ]], [0, 1, 2])
    sib = np.full((3 * depth, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    sides = np.full(3 * depth, 0x5A, np.uint8)
    for data, bad_ids in (([ins[0], ins[1], ins[3]], [0, 1, 2]), ([ins[0], ins[1], ins[2]], [0, 1, n])):
        rc = _lib.lib().zk_merkle_create_proofs(t.h, 0, ptr(as_limbs(data)), ptr(np.array(bad_ids, np.uint64)), 3,
                                                ptr(sib), ptr(sides))
        assert rc == _lib.ZK_EINVAL
        assert (sib == 0x5A5A5A5A5A5A5A5A).all() and (sides == 0x5A).all()


# --- updates ------------------------------------------------------------------------------
def test_batched_updates(ctx):
    depth, field = 11, FQ
    n = 1 << depth
    ins = _inputs(field, depth)
    t = MerkleTree.new_with_inputs(field, depth, list(ins), ctx)
    want = mo.Tree(field, depth, ins)  # a copy of its own: it is updated below
    # 50 distinct leaves: siblings (2k, 2k+1), cousins, both halves of the tree, the ends
    ids = [0, 1, 2, 3, 4, 6, n - 1, n - 2, n // 2, n // 2 - 1, 1024 + 7, 1024 + 6] + [(61 * k + 19) % n for k in range(38)]
    assert len(ids) == 50 == len(set(ids))
    p = po.MODULI[field]
    data = [int(v) for v in co.from_limbs(co.synth(field, 23, 1, 0, 50))]
    data[5], data[6] = 0, p - 1
    is_hash = [k % 3 == 0 for k in range(50)]
    t.update_leaves(ids, data, is_hash)
    for i, d, f in zip(ids, data, is_hash):  # distinct leaves: the sequential result does not depend on the order
        want.update_leaf(i, d, f)
    _assert_same_tree(t, want)
    for k in (0, 5, 49):
        assert t.leaves()[ids[k]] == (data[k] if is_hash[k] else mo.compute_hash(field, data[k]))
    with pytest.raises(ValueError):
        t.update_leaves([7, 9, 7], [1, 2, 3], [False, False, True])  # duplicate id
    _assert_same_tree(t, want)


@pytest.mark.parametrize("field", FIELDS)
def test_reset_leaf_restores_zero_tree(ctx, field):
    depth = 11
    zero = MerkleTree(field, depth, ctx)
    z = 0
    for _ in range(depth):
        z = mo.hash_pair(field, z, z)
    assert zero.get_root_hash() == z
    zero.update_leaves([0, 1500, 2047], [3, 4, 5], [False, True, False])
    assert zero.get_root_hash() != z
    zero.update_leaves([2047, 0, 1500], [0, 0, 0], [True, True, True])
    assert zero.get_root_hash() == z and zero.leaves() == [0] * (1 << depth)
