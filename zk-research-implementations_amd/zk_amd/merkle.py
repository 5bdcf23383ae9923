"""Mirror of the reference Keccak Merkle tree (merkle_tree/src/merkle_tree.rs)
on the GPU through the C ABI: the tree lives in device memory and every hash
of a build, an update or an opening's check of the tree runs there.

Field elements are canonical Python ints. Where the reference returns `Err`
or would panic (depth 0, too many inputs, a bad leaf id, data that does not
match the leaf, a value >= p) these raise ValueError.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field as _dc_field
from enum import IntEnum

import numpy as np

from ._lib import lib
from .api import Field, _call, default_context
from .context import REPR_CANONICAL, Context, DeviceTable
from .elems import as_limbs, one, ptr, to_ints


class LeafSide(IntEnum):  # :6-10
    Left = 0
    Right = 1


@dataclass
class ProofData:  # :12-16
    data_hash: int
    data_side: LeafSide


@dataclass
class MerkleProof:  # :18-22
    data: int
    proof: list = _dc_field(default_factory=list)


def compute_hash(x: int, field: int = Field.BN254_FR) -> int:
    """compute_hash :201-206 (host)."""
    out = np.zeros((1, 4), np.uint64)
    _call(lib().zk_merkle_hash_leaf(int(field), REPR_CANONICAL, ptr(one(int(x))), ptr(out)))
    return to_ints(out)[0]


def hash_pair(left: int, right: int, field: int = Field.BN254_FR) -> int:
    """hash_pair :208-214 (host)."""
    out = np.zeros((1, 4), np.uint64)
    _call(lib().zk_merkle_hash_pair(int(field), REPR_CANONICAL, ptr(one(int(left))), ptr(one(int(right))), ptr(out)))
    return to_ints(out)[0]


def verify_proof(root: int, proof: MerkleProof, field: int = Field.BN254_FR) -> bool:
    """verify :185-199 against a given root (host); the proof's length is not checked."""
    n = len(proof.proof)
    sib = as_limbs([int(p.data_hash) for p in proof.proof]) if n else np.zeros((1, 4), np.uint64)
    sides = np.array([int(p.data_side) for p in proof.proof] or [0], np.uint8)
    ok = C.c_int(0)
    _call(lib().zk_merkle_verify_proof(int(field), REPR_CANONICAL, ptr(one(int(root))), ptr(one(int(proof.data))),
                                       ptr(sib), ptr(sides), n, C.byref(ok)))
    return bool(ok.value)


class MerkleTree:  # :25-29
    def __init__(self, field: int, depth: int, ctx: Context | None = None, _inputs=None, _repr: int = REPR_CANONICAL):
        """MerkleTree::new(depth) :32-52: all leaves the field element 0."""
        self.field = Field(field)
        self.depth = int(depth)
        self.h = None
        if self.depth < 0 or self.depth >= 1 << 32:
            raise ValueError("depth out of range")
        h = C.c_void_p()
        if isinstance(_inputs, DeviceTable):
            self.ctx = ctx or _inputs.ctx
            if _inputs.ctx is not self.ctx or _inputs.ctx.device != self.ctx.device:
                raise ValueError("the device table belongs to another context or device")
            if int(_inputs.field) != int(self.field):
                raise ValueError("the device table holds elements of another field")
            if not _inputs.ptr:
                raise ValueError("the device table has been freed")
            _call(lib().zk_dev_merkle_new(self.ctx.h, int(self.field), self.depth, _inputs.ptr, _inputs.count,
                                          C.byref(h)))
        else:
            self.ctx = ctx or default_context()
            a = None
            if _inputs is not None:
                a = as_limbs(_inputs if isinstance(_inputs, np.ndarray) else [int(v) for v in _inputs])
            n = 0 if a is None else a.shape[0]
            _call(lib().zk_merkle_new(self.ctx.h, int(self.field), self.depth, int(_repr), ptr(a) if n else None, n,
                                      C.byref(h)))
        self.h = h

    @classmethod
    def new_with_inputs(cls, field: int, depth: int, inputs, ctx: Context | None = None,
                        repr: int = REPR_CANONICAL) -> "MerkleTree":
        """new_with_inputs :54-82. `inputs`: ints, a uint64 [n, 4] array (in
        `repr`) or a DeviceTable of this context (hashed without leaving the device)."""
        return cls(field, depth, ctx, _inputs=inputs, _repr=repr)

    def close(self) -> None:
        if getattr(self, "h", None):
            if self.ctx.h:  # (a destroyed context has already released the device)
                lib().zk_merkle_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self.h:
            raise ValueError("the tree has been closed")
        return self.h

    # ---- reads ----
    def get_root_hash(self) -> int:  # :134-136
        out = np.zeros((1, 4), np.uint64)
        _call(lib().zk_merkle_root(self._handle(), REPR_CANONICAL, ptr(out)))
        return to_ints(out)[0]

    def level_limbs(self, level: int, repr: int = REPR_CANONICAL) -> np.ndarray:
        """tree[level] (level = -1: the leaves) as uint64 [n, 4]."""
        level = int(level)
        if not -1 <= level < self.depth:
            raise ValueError("no such level")
        out = np.zeros((1 << (self.depth - 1 - level), 4), np.uint64)
        _call(lib().zk_merkle_download(self._handle(), level, int(repr), ptr(out)))
        return out

    def leaves(self) -> list[int]:
        return to_ints(self.level_limbs(-1))

    def level(self, i: int) -> list[int]:
        return to_ints(self.level_limbs(i))

    # ---- update_leaf :84-104 ----
    def update_leaves(self, ids, data, is_hash) -> None:
        """update_leaf for every (ids[i], data[i], is_hash[i]) at once; the ids
        must be distinct (the reference applies updates one after another)."""
        ids = [int(i) for i in ids]
        data = [int(d) for d in data]
        flags = [bool(f) for f in is_hash]
        if not (len(ids) == len(data) == len(flags)):
            raise ValueError("ids, data and is_hash must have the same length")
        if not ids:
            return
        if any(i < 0 or i >= 1 << 64 for i in ids):
            raise ValueError("Invalid leaf ID")
        _call(lib().zk_merkle_update_leaves(self._handle(), REPR_CANONICAL, ptr(np.array(ids, np.uint64)),
                                            ptr(as_limbs(data)), ptr(np.array(flags, np.uint8)), len(ids)))

    def update_leaf(self, leaf_id: int, data: int, is_hash: bool) -> None:
        self.update_leaves([leaf_id], [data], [is_hash])

    # ---- create_proof :138-183 ----
    def create_proofs(self, data, ids) -> list[MerkleProof]:
        """create_proof for every (data[i], ids[i]) with one gather on the device; all or nothing."""
        ids = [int(i) for i in ids]
        data = [int(d) for d in data]
        if len(ids) != len(data):
            raise ValueError("data and ids must have the same length")
        if not ids:
            return []
        if any(i < 0 or i >= 1 << 64 for i in ids):
            raise ValueError("Invalid leaf ID")
        n, d = len(ids), self.depth
        sib = np.zeros((n * d, 4), np.uint64)
        sides = np.zeros(n * d, np.uint8)
        _call(lib().zk_merkle_create_proofs(self._handle(), REPR_CANONICAL, ptr(as_limbs(data)),
                                            ptr(np.array(ids, np.uint64)), n, ptr(sib), ptr(sides)))
        vals = to_ints(sib)
        return [MerkleProof(data[i], [ProofData(vals[i * d + k], LeafSide(int(sides[i * d + k]))) for k in range(d)])
                for i in range(n)]

    def create_proof(self, data_to_prove: int, leaf_id: int) -> MerkleProof:
        return self.create_proofs([data_to_prove], [leaf_id])[0]

    # ---- verify :185-199 ----
    def verify(self, proof: MerkleProof) -> bool:
        return verify_proof(self.get_root_hash(), proof, self.field)
