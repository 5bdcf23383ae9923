"""Checker for the Merkle tree tests: merkle_tree/src/merkle_tree.rs restated in
Python over the oracle's Keccak-256 (coracle.keccak256; pyoracle.keccak256 is
the cross-check). Uses nothing of the library under test.

  compute_hash(x) = LEint(Keccak256(LE32(x))) mod p            :201-206
  hash_pair(l, r) = LEint(Keccak256(LE32(l) | LE32(r))) mod p  :208-214
"""
from __future__ import annotations

import coracle as co
import pyoracle as po

LEFT, RIGHT = 0, 1  # LeafSide :6-10


def le32(x: int) -> bytes:
    return int(x).to_bytes(32, "little")


def digest_int(data: bytes, keccak=co.keccak256) -> int:
    return int.from_bytes(keccak(data), "little")


def compute_hash(field: int, x: int, keccak=co.keccak256) -> int:
    return digest_int(le32(x), keccak) % po.MODULI[field]


def hash_pair(field: int, left: int, right: int, keccak=co.keccak256) -> int:
    return digest_int(le32(left) + le32(right), keccak) % po.MODULI[field]


class Tree:
    """MerkleTree<F> :25-29: leaves, tree[level], depth."""

    def __init__(self, field: int, depth: int, inputs=None):  # new :32-52 / new_with_inputs :54-82
        self.field, self.depth = field, depth
        n = 1 << depth
        inputs = [] if inputs is None else [int(v) for v in inputs]
        if len(inputs) > n:
            raise ValueError("Too many inputs for tree depth")
        self.leaves = [compute_hash(field, v) for v in inputs] + [0] * (n - len(inputs))
        self.quotients = {digest_int(le32(v)) // po.MODULI[field] for v in inputs}
        self.tree = []
        cur = self.leaves
        for _ in range(depth):
            nxt = []
            for j in range(0, len(cur), 2):
                d = digest_int(le32(cur[j]) + le32(cur[j + 1]))
                self.quotients.add(d // po.MODULI[field])
                nxt.append(d % po.MODULI[field])
            self.tree.append(nxt)
            cur = nxt

    def root(self) -> int:  # get_root_hash :134-136
        return self.tree[self.depth - 1][0]

    def _sibling(self, level: int, index: int) -> int:
        return self.leaves[index ^ 1] if level == 0 else self.tree[level - 1][index ^ 1]

    def update_leaf(self, leaf_id: int, data: int, is_hash: bool) -> None:  # :84-132
        if leaf_id >= 1 << self.depth:
            raise ValueError("Invalid leaf ID")
        cur = data if is_hash else compute_hash(self.field, data)
        self.leaves[leaf_id] = cur
        index = leaf_id
        for level in range(self.depth):
            sib = self._sibling(level, index)
            cur = hash_pair(self.field, cur, sib) if index % 2 == 0 else hash_pair(self.field, sib, cur)
            index //= 2
            self.tree[level][index] = cur

    def create_proof(self, data: int, leaf_id: int):  # :138-183 -> (data, [(sibling, side)])
        if leaf_id >= 1 << self.depth:
            raise ValueError("Invalid leaf ID")
        if self.leaves[leaf_id] != compute_hash(self.field, data):
            raise ValueError("Data does not match the leaf hash")
        proof, index = [], leaf_id
        for level in range(self.depth):
            proof.append((self._sibling(level, index), RIGHT if index % 2 == 0 else LEFT))
            index //= 2
        return data, proof

    def verify(self, data: int, proof) -> bool:  # :185-199
        return fold_proof(self.field, data, proof) == self.root()


def fold_proof(field: int, data: int, proof) -> int:
    cur = compute_hash(field, data)
    for sib, side in proof:
        cur = hash_pair(field, sib, cur) if side == LEFT else hash_pair(field, cur, sib)
    return cur
