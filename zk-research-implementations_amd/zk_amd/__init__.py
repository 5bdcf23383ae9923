"""zk_amd — MI355X-native sum-check / GKR sum-check prover.

Python mirror of the reference crates' API (obah/zk-research-implementations):
  fiat_shamir::fiat_shamir_transcript::{Transcript, fq_vec_to_bytes}
  multilinear_polynomial::{MultilinearPoly, ProductPoly, SumPoly}
  univariate_polynomial::UnivariatePoly
  sum_check::sum_check_protocol::{prove, verify, gkr_prove, gkr_verify, Proof, GkrProof, GkrVerify}
  gkr_prove / gkr_verify over every product and factor of a SumPoly: composed_prove, composed_verify, composed_combine
  the same with the tables KZG-committed and opened at once: committed_prove, committed_verify (zk_amd.committed)
  R1CS satisfiability over a committed witness: R1CS, R1csProof (zk_amd.r1cs)
  lookups (LogUp) over a committed column, batched field inversion: Lookup, LookupProof, batch_inverse (zk_amd.lookup)
  merkle_tree::{MerkleTree, MerkleProof, ProofData, LeafSide}  (zk_amd.merkle)
  fft::{fft_evaluate, fft_interpolate, split_poly, get_interpolation_roots}  (zk_amd.fft)
  univariate_polynomial::UnivariatePoly::{interpolate, evaluate} over many points  (zk_amd.poly)
  shamir_secret_sharing::{create_polynomia, recover_polynomial, get_secret, share_points}  (zk_amd.shamir)
over the C ABI of include/zk_sumcheck.h. Every table-sized operation runs in
the HIP library on a gfx950 GPU; this module only marshals arguments.

Field elements are canonical Python ints, or numpy uint64 arrays of shape
[n, 4] (little-endian limbs) for tables.
"""
from __future__ import annotations

from .api import (  # noqa: F401
    ComposedProof,
    Field,
    GkrProof,
    GkrVerify,
    MultilinearPoly,
    ProductPoly,
    Proof,
    SumPoly,
    Transcript,
    UnivariatePoly,
    blob_info,
    composed_combine,
    composed_prove,
    composed_verify,
    default_context,
    fq_vec_to_bytes,
    gkr_prove,
    gkr_verify,
    gkr_verify_blob,
    keccak256,
    modulus,
    prove,
    verify,
)
from .context import Context, DeviceTable  # noqa: F401
from . import gkr  # noqa: F401  (gkr crate mirror: Circuit, WiredCircuit, Operation, prove, verify)
from . import merkle  # noqa: F401  (merkle_tree crate mirror)
from .merkle import LeafSide, MerkleProof, MerkleTree, ProofData  # noqa: F401
from . import fft  # noqa: F401  (fft crate mirror, polynomial product)
from .fft import (  # noqa: F401
    dev_fft,
    fft_evaluate,
    fft_interpolate,
    get_interpolation_roots,
    get_root_of_unity,
    poly_mul,
    split_poly,
)
from . import poly  # noqa: F401  (interpolation and batch evaluation over arbitrary points)
from . import shamir  # noqa: F401  (shamir_secret_sharing crate mirror)
from .committed import CommittedProof, CommittedVerify, committed_prove, committed_verify  # noqa: F401
from .r1cs import R1CS, R1csProof, R1csVerify  # noqa: F401
from .lookup import Lookup, LookupProof, LookupVerify, batch_inverse  # noqa: F401
from ._lib import ZkError  # noqa: F401
