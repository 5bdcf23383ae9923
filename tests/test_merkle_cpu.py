"""CPU checks of the Merkle tree's host side (merkle_tree/src/merkle_tree.rs):
the checker against public Keccak-256 vectors and the pure-Python oracle, the
host-only C-ABI entry points (zk_merkle_hash_leaf / _hash_pair /
_verify_proof) against the checker on all three fields, and the committed
fixture tests/golden/merkle.json."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

import coracle as co
import merkle_oracle as mo
import pyoracle as po
from conftest import ROOT

from zk_amd import _lib, merkle
from zk_amd.elems import as_limbs, ptr, to_ints

FIELDS = [0, 1, 2]
CANON, MONT = 0, 1


def _values(field: int) -> list[int]:
    p = po.MODULI[field]
    return [0, 1, p - 1] + co.from_limbs(co.synth(field, 7, 0, 0, 64))


def _to_mont(field: int, v: int) -> np.ndarray:
    a, m = as_limbs([v]), np.zeros((1, 4), np.uint64)
    co.lib().or_fe_to_mont(field, a.ctypes.data, m.ctypes.data)
    return m


# --- the checker itself ------------------------------------------------------------
def test_checker_public_keccak_vectors():
    """Keccak-256 (not SHA3-256) of 32 and of 64 zero bytes, the widely published
    values (e.g. the zero-leaf hashes of Solidity Merkle trees)."""
    z32 = "290decd9548b62a8d60345a988386fc84ba6bc95484008f6362f93160ef3e563"
    z64 = "ad3228b676f7d3cd4284a5443f17f1962b36e491b30a40b2405849e597ba5fb5"
    for k in (co.keccak256, po.keccak256):
        assert k(bytes(32)).hex() == z32
        assert k(bytes(64)).hex() == z64


@pytest.mark.parametrize("field", FIELDS)
def test_checker_agrees_with_pure_python_keccak(field):
    vals = _values(field)[:8]
    for v in vals:
        assert mo.compute_hash(field, v) == mo.compute_hash(field, v, po.keccak256)
    for l, r in zip(vals, vals[1:]):
        assert mo.hash_pair(field, l, r) == mo.hash_pair(field, l, r, po.keccak256)


# --- host hash entry points ----------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_hash_leaf_and_pair_match_checker(field):
    L = _lib.lib()
    vals = _values(field)
    out = np.zeros((1, 4), np.uint64)
    for i, v in enumerate(vals):
        w = vals[(i + 1) % len(vals)]
        want1, want2 = mo.compute_hash(field, v), mo.hash_pair(field, v, w)
        assert merkle.compute_hash(v, field) == want1
        assert merkle.hash_pair(v, w, field) == want2
        # Montgomery in, Montgomery out == or_fe_to_mont of the canonical result
        assert L.zk_merkle_hash_leaf(field, MONT, ptr(_to_mont(field, v)), ptr(out)) == 0
        assert np.array_equal(out, _to_mont(field, want1))
        assert L.zk_merkle_hash_pair(field, MONT, ptr(_to_mont(field, v)), ptr(_to_mont(field, w)), ptr(out)) == 0
        assert np.array_equal(out, _to_mont(field, want2))


@pytest.mark.parametrize("field", FIELDS)
def test_hash_entry_points_reject_bad_arguments(field):
    L = _lib.lib()
    p = po.MODULI[field]
    out = np.full((1, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    before = out.copy()
    for repr_ in (CANON, MONT):
        assert L.zk_merkle_hash_leaf(field, repr_, ptr(as_limbs([p])), ptr(out)) == _lib.ZK_EINVAL
        assert L.zk_merkle_hash_pair(field, repr_, ptr(as_limbs([1])), ptr(as_limbs([p])), ptr(out)) == _lib.ZK_EINVAL
        assert L.zk_merkle_hash_pair(field, repr_, ptr(as_limbs([2**256 - 1])), ptr(as_limbs([1])), ptr(out)) == _lib.ZK_EINVAL
    assert L.zk_merkle_hash_leaf(field, CANON, None, ptr(out)) == _lib.ZK_EINVAL
    assert L.zk_merkle_hash_leaf(field, CANON, ptr(as_limbs([1])), None) == _lib.ZK_EINVAL
    assert L.zk_merkle_hash_leaf(7, CANON, ptr(as_limbs([1])), ptr(out)) == _lib.ZK_EINVAL
    assert np.array_equal(out, before)  # nothing written
    with pytest.raises(ValueError):
        merkle.compute_hash(p, field)
    with pytest.raises(ValueError):
        merkle.hash_pair(0, p, field)


# --- zk_merkle_verify_proof --------------------------------------------------------------
def _tree(field: int, depth: int) -> tuple:
    inputs = co.from_limbs(co.synth(field, 13, depth, 0, 1 << depth))
    return mo.Tree(field, depth, inputs), inputs


def _proof(data: int, pairs) -> merkle.MerkleProof:
    return merkle.MerkleProof(data, [merkle.ProofData(s, merkle.LeafSide(side)) for s, side in pairs])


@pytest.mark.parametrize("depth", [1, 3, 10])
@pytest.mark.parametrize("field", FIELDS)
def test_verify_proof_accepts_and_rejects(field, depth):
    t, inputs = _tree(field, depth)
    p = po.MODULI[field]
    root = t.root()
    for leaf in sorted({0, (1 << depth) - 1, (1 << depth) // 3}):
        data, pairs = t.create_proof(inputs[leaf], leaf)
        assert t.verify(data, pairs)
        assert merkle.verify_proof(root, _proof(data, pairs), field)
        for k in sorted({0, depth - 1}):
            sib, side = pairs[k]
            flipped = pairs[:k] + [(sib, 1 - side)] + pairs[k + 1:]
            assert not merkle.verify_proof(root, _proof(data, flipped), field)
            changed = pairs[:k] + [((sib + 1) % p, side)] + pairs[k + 1:]
            assert not merkle.verify_proof(root, _proof(data, changed), field)
        assert not merkle.verify_proof(root, _proof((data + 1) % p, pairs), field)
        assert not merkle.verify_proof((root + 1) % p, _proof(data, pairs), field)
    # the reference's dummy proof (:308-326): data 10, `depth` entries (0, Left)
    assert not merkle.verify_proof(root, _proof(10, [(0, mo.LEFT)] * depth), field)
    # ... and the length is not checked against a depth (:189): a longer or an empty proof just folds
    assert not merkle.verify_proof(root, _proof(inputs[0], t.create_proof(inputs[0], 0)[1] + [(0, mo.LEFT)]), field)
    assert merkle.verify_proof(mo.compute_hash(field, 5), _proof(5, []), field)


def test_verify_proof_montgomery_and_bad_arguments():
    field, depth = 1, 3
    L = _lib.lib()
    t, inputs = _tree(field, depth)
    data, pairs = t.create_proof(inputs[5], 5)
    sib = np.concatenate([_to_mont(field, s) for s, _ in pairs])
    sides = np.array([side for _, side in pairs], np.uint8)
    ok = C.c_int(-7)
    args = (ptr(_to_mont(field, t.root())), ptr(_to_mont(field, data)), ptr(sib), ptr(sides), depth, C.byref(ok))
    assert L.zk_merkle_verify_proof(field, MONT, *args) == 0 and ok.value == 1
    assert L.zk_merkle_verify_proof(field, CANON, ptr(as_limbs([t.root()])), ptr(as_limbs([data])), ptr(sib), ptr(sides),
                                    depth, C.byref(ok)) == 0 and ok.value == 0  # Montgomery images read as canonical
    ok = C.c_int(-7)
    bad_sides = sides.copy()
    bad_sides[1] = 2
    csib = as_limbs([s for s, _ in pairs])
    root, dat = ptr(as_limbs([t.root()])), ptr(as_limbs([data]))
    assert L.zk_merkle_verify_proof(field, CANON, root, dat, ptr(csib), ptr(bad_sides), depth, C.byref(ok)) == _lib.ZK_EINVAL
    big = as_limbs([s for s, _ in pairs[:-1]] + [po.MODULI[field]])
    assert L.zk_merkle_verify_proof(field, CANON, root, dat, ptr(big), ptr(sides), depth, C.byref(ok)) == _lib.ZK_EINVAL
    assert L.zk_merkle_verify_proof(field, CANON, root, dat, None, None, depth, C.byref(ok)) == _lib.ZK_EINVAL
    assert L.zk_merkle_verify_proof(field, CANON, root, dat, ptr(csib), ptr(sides), depth, None) == _lib.ZK_EINVAL
    assert ok.value == -7  # nothing written
    with pytest.raises(ValueError):
        merkle.verify_proof(t.root(), _proof(po.MODULI[field], pairs), field)


def test_tree_entry_points_need_a_context():
    """No tree without a device context: every device entry point fails cleanly on null handles."""
    L = _lib.lib()
    h = C.c_void_p()
    assert L.zk_merkle_new(None, 0, 3, CANON, None, 0, C.byref(h)) == _lib.ZK_EINVAL and not h.value
    assert L.zk_dev_merkle_new(None, 0, 3, None, 0, C.byref(h)) == _lib.ZK_EINVAL and not h.value
    out = np.zeros((1, 4), np.uint64)
    assert L.zk_merkle_root(None, CANON, ptr(out)) == _lib.ZK_EINVAL
    assert L.zk_merkle_download(None, -1, CANON, ptr(out)) == _lib.ZK_EINVAL
    assert L.zk_merkle_update_leaves(None, CANON, None, None, None, 1) == _lib.ZK_EINVAL
    assert L.zk_merkle_create_proofs(None, CANON, None, None, 1, None, None) == _lib.ZK_EINVAL
    L.zk_merkle_free(None)


# --- fixture -----------------------------------------------------------------------------
def test_golden_fixture_roots_and_quotient_sets():
    with open(os.path.join(ROOT, "tests", "golden", "merkle.json")) as fh:
        g = json.load(fh)
    assert (g["depth"], g["seed"], g["table"], g["index0"], g["count"]) == (10, 11, 0, 0, 1024)
    want_q = {0: [0, 1, 2, 3, 4, 5], 1: [0, 1, 2, 3, 4, 5], 2: [0, 1, 2]}
    for tr in g["trees"]:
        f = tr["field"]
        p = po.MODULI[f]
        # complete: every quotient a 256-bit digest can have, so a tree over these
        # inputs takes every branch of the digest reduction
        assert tr["quotients"] == want_q[f] == list(range((2**256 - 1) // p + 1))
        t = mo.Tree(f, g["depth"], co.from_limbs(co.synth(f, g["seed"], g["table"], g["index0"], g["count"])))
        assert t.root() == int(tr["root"], 16)
        assert sorted(t.quotients) == tr["quotients"]
    assert [tr["root"][:10] + tr["root"][-8:] for tr in g["trees"]] == [
        "0x2a690706494a32a1", "0x203a9270a6bcd245", "0x0b06ccf5c912cf7b"]
