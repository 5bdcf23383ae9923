"""The R1CS prover without a GPU: host-only handles
(zk_r1cs_new with no context) on proofs the Python model (tests/r1cs_oracle.py)
makes — accepted on all three fields and, committed, on BLS12-381 Fr; rejected
for every kind of damage — the host matrix evaluation and multiplication against
the model, and every error path with nothing written."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import r1cs_cases as rc
import r1cs_oracle as ro
from pyoracle import MODULI, keccak256

import zk_amd
from zk_amd import R1CS, Transcript, UnivariatePoly
from zk_amd._lib import ZK_EDEVICE, ZK_EINVAL, ZK_EUNSUPPORTED, ZK_OK, lib
from zk_amd.elems import as_limbs, ptr, to_ints
from zk_amd.r1cs import R1csProof

UNCOMMITTED = ("1_1", "1_2", "2_2", "3_2", "3_4", "cubic", "chain5")
COMMITTED = ("1_2", "2_2", "cubic")  # sy = 2, 2, 3 (the pairing check of the model is slow: sy <= 3)


def _r1cs(inst) -> R1CS:
    return R1CS(inst.field, inst.nrows, inst.sy, inst.npub, inst.A, inst.B, inst.C)


def test_model_digest_layout():
    inst = ro.Instance(0, 1, 1, 0, [(0, 1, 5)], [], [(0, 0, 2), (0, 0, 3)])
    u32 = lambda x: x.to_bytes(4, "little")
    want = (b"zk-r1cs-v1" + u32(0) + u32(1) + u32(1) + u32(1) + u32(0) + u32(1) + u32(0) + u32(1)
            + (5).to_bytes(32, "little") + u32(0) + u32(2) + u32(0) + u32(0) + (2).to_bytes(32, "little") + u32(0)
            + u32(0) + (3).to_bytes(32, "little"))
    assert ro.digest(inst) == keccak256(want)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_shape_and_digest_match_the_model(field):
    for name in UNCOMMITTED:
        inst, _, _ = rc.case(name, field)
        r = _r1cs(inst)
        assert (r.sx, r.digest) == (inst.sx, ro.digest(inst)), name
        r.close()
    a, _, _ = rc.case("cubic", field)
    b = ro.Instance(field, a.nrows, a.sy, a.npub, list(reversed(a.A)), a.B, a.C)  # the caller's order is part of it
    assert ro.digest(a) != ro.digest(b)
    r = _r1cs(b)
    assert r.digest == ro.digest(b)
    r.close()


@pytest.mark.parametrize("name", UNCOMMITTED)
@pytest.mark.parametrize("field", [0, 1, 2])
def test_verifier_accepts_model_proofs(field, name):
    inst, w, io = rc.case(name, field)
    assert ro.is_satisfied(inst, w, io)
    proof = rc.model_proof(name, field)
    h = rc.handle(inst)
    rcode, ok, rx, ry, _ = rc.verify_raw(h, inst, proof, io)
    assert (rcode, ok) == (ZK_OK, 1) and rx == proof["rx"] and ry == proof["ry"]
    assert ro.verify(inst, proof, io, ro.Transcript(field)) == (True, proof["rx"], proof["ry"])
    lib().zk_r1cs_free(h)


@pytest.mark.parametrize("name", COMMITTED)
def test_verifier_accepts_committed_model_proofs(name):
    inst, w, io = rc.case(name, 2)
    proof = rc.model_proof(name, 2, committed=True)
    g2 = rc.setup(inst.sy - 1)[1]
    h = rc.handle(inst)
    assert rc.verify_raw(h, inst, proof, io, g2)[:2] == (ZK_OK, 1)
    assert rc.verify_raw(h, inst, proof, io, rc.other_g2(inst.sy - 1))[:2] == (ZK_OK, 0)   # a wrong setup
    assert rc.verify_raw(h, inst, proof, io, g2, pre=rc.PRE_BYTES)[:2] == (ZK_OK, 0)
    for how in list(rc.TAMPERINGS) + list(rc.TAMPERINGS_COMMITTED):
        res = rc.verify_raw(h, inst, rc.damaged(proof, 2, how), io, g2)
        assert res[:2] == (ZK_OK, 0) and res[4], how
    # an uncommitted proof of the same statement has another transcript: its rounds do not fit this one
    plain = dict(rc.model_proof(name, 2), commitment=proof["commitment"], opening=proof["opening"])
    assert rc.verify_raw(h, inst, plain, io, g2)[:2] == (ZK_OK, 0)
    lib().zk_r1cs_free(h)


def test_model_verifies_its_committed_proof():
    """the one pairing check in pure Python (slow): sy = 2"""
    inst, w, io = rc.case("1_2", 2)
    proof = rc.model_proof("1_2", 2, committed=True)
    assert ro.verify(inst, proof, io, ro.Transcript(2), rc.setup(1)[1])[0]
    assert not ro.verify(inst, rc.damaged(proof, 2, "vw"), io, ro.Transcript(2), rc.setup(1)[1])[0]


@pytest.mark.parametrize("how", sorted(rc.TAMPERINGS))
@pytest.mark.parametrize("name,field", [("3_4", 0), ("2_2", 1), ("chain5", 2)])
def test_damaged_proofs_are_rejected(name, field, how):
    inst, w, io = rc.case(name, field)
    h = rc.handle(inst)
    res = rc.verify_raw(h, inst, rc.damaged(rc.model_proof(name, field), field, how), io)
    assert res[:2] == (ZK_OK, 0) and res[4], "a rejection writes nothing but the verdict"
    lib().zk_r1cs_free(h)


@pytest.mark.parametrize("name,field", [("3_4", 0), ("cubic", 1), ("chain5", 2)])
def test_changed_statement_is_rejected(name, field):
    p = MODULI[field]
    inst, w, io = rc.case(name, field)
    proof = rc.model_proof(name, field)
    h = rc.handle(inst)
    assert rc.verify_raw(h, inst, proof, io)[:2] == (ZK_OK, 1)
    assert rc.verify_raw(h, inst, proof, [(io[0] + 1) % p] + io[1:])[:2] == (ZK_OK, 0)      # an io entry
    assert rc.verify_raw(h, inst, proof, io, pre=rc.PRE_BYTES)[:2] == (ZK_OK, 0)             # other bytes first
    lib().zk_r1cs_free(h)
    for t in range(3):                                                                        # a matrix entry
        mats = [list(m) for m in inst.matrices]
        if not mats[t]:
            continue
        r_, c_, v_ = mats[t][0]
        mats[t][0] = (r_, c_, (v_ + 1) % p)
        other = ro.Instance(field, inst.nrows, inst.sy, inst.npub, *mats)
        h2 = rc.handle(other)
        assert rc.verify_raw(h2, other, proof, io)[:2] == (ZK_OK, 0), t
        lib().zk_r1cs_free(h2)
    # a false witness: the model proves it, nobody accepts it
    bad = list(w)
    bad[0] = (bad[0] + 1) % p
    assert not ro.is_satisfied(inst, bad, io)
    false_proof = ro.prove(inst, bad, io, ro.Transcript(field))
    h = rc.handle(inst)
    assert rc.verify_raw(h, inst, false_proof, io)[:2] == (ZK_OK, 0)
    assert not ro.verify(inst, false_proof, io, ro.Transcript(field))[0]
    lib().zk_r1cs_free(h)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_host_mul_and_matrix_evals_match_the_model(field):
    p = MODULI[field]
    rng = random.Random(40 + field)
    for name in ("1_1", "3_4", "cubic", "chain5"):
        inst, w, io = rc.case(name, field)
        r = _r1cs(inst)
        z = ro.z_of(inst, w, io)
        assert r.z(w, io) == z and list(r.mul(z)) == ro.mul(inst, z)
        assert r.is_satisfied(w, io)
        for _ in range(2):
            rx = [rng.randrange(p) for _ in range(inst.sx)]
            ry = [rng.randrange(p) for _ in range(inst.sy)]
            assert r.matrix_evals(rx, ry) == ro.matrix_evals(inst, rx, ry)
        bits = lambda v, n: [(v >> (n - 1 - k)) & 1 for k in range(n)]
        dense = [[0] * (1 << inst.sy) for _ in range(3)]  # at a hypercube point it is the entry, duplicates added
        for t, m in enumerate(inst.matrices):
            for r_, c_, v_ in m:
                if r_ == 0:
                    dense[t][c_] = (dense[t][c_] + v_) % p
        for c_ in range(min(1 << inst.sy, 8)):
            assert r.matrix_evals(bits(0, inst.sx), bits(c_, inst.sy)) == [dense[t][c_] for t in range(3)]
        r.close()
    inst, w, io = rc.random_instance(field, 4, 3, 1, 2, 77, satisfied=False)
    r = _r1cs(inst)
    assert not r.is_satisfied(w, io)
    r.close()


def test_python_verify_on_a_host_only_handle():
    inst, w, io = rc.case("3_4", 0)
    m = rc.model_proof("3_4", 0)
    proof = R1csProof([UnivariatePoly(q, 0) for q in m["polys1"]], [UnivariatePoly(q, 0) for q in m["polys2"]],
                      m["va"], m["vb"], m["vc"], m["vw"])
    r = _r1cs(inst)
    res = r.verify(proof, io, Transcript(0))
    assert res.verified and res.rx == m["rx"] and res.ry == m["ry"]
    proof.vb = (proof.vb + 1) % MODULI[0]
    assert not r.verify(proof, io, Transcript(0)).verified
    with pytest.raises(zk_amd.ZkError) as e:
        r.prove(w, io, Transcript(0))
    assert e.value.code == ZK_EDEVICE
    r.close()
    assert zk_amd.R1CS is R1CS and zk_amd.R1csProof is R1csProof


# ---- error paths: the code, and nothing written --------------------------------
def test_new_error_paths():
    inst, _, _ = rc.case("3_4", 0)
    p = MODULI[0]
    rcode, h = rc.new_raw(inst)
    assert rcode == ZK_OK
    lib().zk_r1cs_free(h)
    lib().zk_r1cs_free(None)
    for null in ("nnz", "rows", "cols", "vals", "out"):
        if null == "out":
            assert lib().zk_r1cs_new(None, 0, 0, 1, 1, 0, ptr(np.zeros(3, np.uint32)), None, None, None, None) == ZK_EINVAL
        else:
            assert rc.new_raw(inst, null=(null,))[0] == ZK_EINVAL, null
    assert rc.new_raw(inst, field=3)[0] == ZK_EINVAL
    assert rc.new_raw(inst, repr_=2)[0] == ZK_EINVAL
    assert rc.new_raw(inst, nrows=0)[0] == ZK_EINVAL
    assert rc.new_raw(inst, sy=0)[0] == ZK_EINVAL
    assert rc.new_raw(inst, npub=8)[0] == ZK_EINVAL                 # npub + 1 > 2^(sy-1) = 8
    assert rc.new_raw(inst, nrows=4)[0] == ZK_EINVAL                # a row >= nrows (the instance has 5)
    assert rc.new_raw(inst, sy=3)[0] == ZK_EINVAL                   # a column >= 2^sy (and npub + 1 = 4 still fits)
    bad = ro.Instance(0, inst.nrows, inst.sy, inst.npub, [(0, 0, p)] + inst.A[1:], inst.B, inst.C)
    assert rc.new_raw(bad)[0] == ZK_EINVAL                          # a value >= p
    assert rc.new_raw(inst, sy=25)[0] == ZK_EUNSUPPORTED
    assert rc.new_raw(inst, nrows=(1 << 24) + 1)[0] == ZK_EUNSUPPORTED
    assert rc.new_raw(inst, nnz=[1 << 26, 1, 0])[0] == ZK_EUNSUPPORTED  # (the count is checked before an entry is read)
    empty = ro.Instance(0, 2, 1, 0, [], [], [])                     # no entries at all is an instance (0 0 = 0)
    r = _r1cs(empty)
    assert r.is_satisfied([5], []) and r.matrix_evals([3], [4]) == [0, 0, 0]
    r.close()


def _prove_raw_host_only(h, inst, w, io):
    L = lib()
    sx, sy = inst.sx, inst.sy
    bufs = [np.full((sx, 4, 4), rc.SENTINEL, np.uint64), np.full(sx, 0xA5, np.uint8),
            np.full((sy, 3, 4), rc.SENTINEL, np.uint64), np.full(sy, 0xA5, np.uint8),
            np.full((4, 4), rc.SENTINEL, np.uint64), np.full((sx, 4), rc.SENTINEL, np.uint64),
            np.full((sy, 4), rc.SENTINEL, np.uint64), np.full((1, 12), rc.SENTINEL, np.uint64),
            np.full((max(sy - 1, 1), 12), rc.SENTINEL, np.uint64)]
    t = L.zk_transcript_new()
    before = rc.transcript_bytes(t)
    code = L.zk_r1cs_prove(h, 0, ptr(as_limbs(list(w))), ptr(as_limbs(list(io))), None, None, t, *[ptr(b) for b in bufs])
    same = all(bool((b == (0xA5 if b.dtype == np.uint8 else rc.SENTINEL)).all()) for b in bufs)
    same = same and rc.transcript_bytes(t) == before
    L.zk_transcript_free(t)
    return code, same


def test_host_only_handle_cannot_prove_and_writes_nothing():
    inst, w, io = rc.case("3_4", 2)
    h = rc.handle(inst)
    assert _prove_raw_host_only(h, inst, w, io) == (ZK_EDEVICE, True)
    X, Y = 1 << inst.sx, 1 << inst.sy
    outs = [np.full((X, 4), rc.SENTINEL, np.uint64) for _ in range(3)]
    dummy = np.zeros((Y, 4), np.uint64)
    assert lib().zk_dev_r1cs_mul(h, ptr(dummy), ptr(outs[0]), ptr(outs[1]), ptr(outs[2])) == ZK_EDEVICE
    assert all(bool((o == rc.SENTINEL).all()) for o in outs)
    cols = [np.full((Y, 4), rc.SENTINEL, np.uint64) for _ in range(3)]
    x = np.zeros((X, 4), np.uint64)
    assert lib().zk_dev_r1cs_mul_t(h, ptr(x), ptr(cols[0]), ptr(cols[1]), ptr(cols[2])) == ZK_EDEVICE
    assert lib().zk_dev_r1cs_mul_t(h, None, ptr(cols[0]), ptr(cols[1]), ptr(cols[2])) == ZK_EINVAL
    assert all(bool((o == rc.SENTINEL).all()) for o in cols)
    lib().zk_r1cs_free(h)


def test_verify_error_paths_write_nothing():
    field = 2
    p = MODULI[field]
    inst, w, io = rc.case("cubic", field)
    proof = rc.model_proof("cubic", field, committed=True)
    g2 = rc.setup(inst.sy - 1)[1]
    h = rc.handle(inst)
    assert rc.verify_raw(h, inst, proof, io, g2)[:2] == (ZK_OK, 1)

    def code(pr=proof, io_=io, g2_=g2, **kw):
        res = rc.verify_raw(h, inst, pr, io_, g2_, **kw)
        return res[0], res[4]

    for null in ("io", "c1", "n1", "c2", "n2", "ev", "t", "ok", "rx", "ry", "cm", "op", "g2"):
        assert code(null=(null,)) == (ZK_EINVAL, True), null
    assert code(repr_=2) == (ZK_EINVAL, True)
    assert code(io_=[p]) == (ZK_EINVAL, True)
    for key in ("va", "vb", "vc", "vw"):
        assert code(pr=dict(proof, **{key: p})) == (ZK_EINVAL, True), key
    assert code(pr=dict(proof, polys1=[[p]] + proof["polys1"][1:])) == (ZK_EINVAL, True)
    assert code(pr=dict(proof, polys2=[[p]] + proof["polys2"][1:])) == (ZK_EINVAL, True)
    assert code(pr=dict(proof, commitment=(proof["commitment"][0], 1))) == (ZK_EINVAL, True)   # off the curve
    assert code(pr=dict(proof, opening=[proof["opening"][0], (5, 5)])) == (ZK_EINVAL, True)
    assert code(pr=dict(proof, polys1=[[1, 2, 3, 4, 5]] + proof["polys1"][1:])) == (ZK_OK, True)  # 5 coefficients: rejected
    lib().zk_r1cs_free(h)
    # a committed proof needs sy >= 2 and BLS12-381 Fr
    inst1, w1, io1 = rc.case("1_1", field)
    h1 = rc.handle(inst1)
    fake = dict(rc.model_proof("1_1", field), commitment=proof["commitment"], opening=[])
    assert rc.verify_raw(h1, inst1, fake, io1, [])[0] == ZK_EINVAL
    lib().zk_r1cs_free(h1)
    inst0, w0, io0 = rc.case("cubic", 0)
    h0 = rc.handle(inst0)
    fake = dict(rc.model_proof("cubic", 0), commitment=proof["commitment"], opening=proof["opening"])
    res = rc.verify_raw(h0, inst0, fake, io0, g2)
    assert (res[0], res[4]) == (ZK_EINVAL, True)
    lib().zk_r1cs_free(h0)


def test_mul_and_matrix_evals_error_paths_write_nothing():
    inst, w, io = rc.case("3_4", 1)
    p = MODULI[1]
    h = rc.handle(inst)
    X, Y = 1 << inst.sx, 1 << inst.sy
    outs = [np.full((X, 4), rc.SENTINEL, np.uint64) for _ in range(3)]
    z = as_limbs([1] * (Y - 1) + [p])
    L = lib()
    assert L.zk_r1cs_mul(h, 0, ptr(z), ptr(outs[0]), ptr(outs[1]), ptr(outs[2])) == ZK_EINVAL
    assert L.zk_r1cs_mul(h, 2, ptr(z), ptr(outs[0]), ptr(outs[1]), ptr(outs[2])) == ZK_EINVAL
    assert L.zk_r1cs_mul(h, 0, None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2])) == ZK_EINVAL
    assert L.zk_r1cs_mul(h, 0, ptr(z), ptr(outs[0]), None, ptr(outs[2])) == ZK_EINVAL
    assert L.zk_r1cs_mul(None, 0, ptr(z), ptr(outs[0]), ptr(outs[1]), ptr(outs[2])) == ZK_EINVAL
    assert all(bool((o == rc.SENTINEL).all()) for o in outs)
    out = np.full((3, 4), rc.SENTINEL, np.uint64)
    good, bad = as_limbs([1] * 4), as_limbs([p, 1, 2, 3])  # (sx = 3, sy = 4)
    assert L.zk_r1cs_matrix_evals(h, 0, ptr(bad), ptr(good), ptr(out)) == ZK_EINVAL
    assert L.zk_r1cs_matrix_evals(h, 0, ptr(good), ptr(bad), ptr(out)) == ZK_EINVAL
    assert L.zk_r1cs_matrix_evals(h, 2, ptr(good), ptr(good), ptr(out)) == ZK_EINVAL
    assert L.zk_r1cs_matrix_evals(h, 0, None, ptr(good), ptr(out)) == ZK_EINVAL
    assert L.zk_r1cs_matrix_evals(h, 0, ptr(good), ptr(good), None) == ZK_EINVAL
    assert bool((out == rc.SENTINEL).all())
    assert L.zk_r1cs_shape(None, None, None, None, None, None) == ZK_EINVAL
    sx = C.c_uint32(99)
    assert L.zk_r1cs_shape(h, C.byref(sx), None, None, None, None) == ZK_OK and sx.value == inst.sx
    L.zk_r1cs_free(h)
