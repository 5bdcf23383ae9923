/*
 * zk_sumcheck.h — C ABI of the MI355X-native sum-check / GKR sum-check prover.
 *
 * Drop-in boundary for the reference crates `sum_check`, `multilinear_polynomial`
 * and `fiat_shamir` (obah/zk-research-implementations). Each entry point names
 * the Rust item it replaces (paths relative to the reference root). The
 * reference is generic over `F: PrimeField`; here the field is a runtime
 * `zk_field` and elements are 32-byte little-endian 4 x u64 limbs, either
 * canonical (what `fq_vec_to_bytes` serialises) or Montgomery (ark-ff 0.5.0's
 * in-memory `Fp<MontBackend<_,4>,4>`, R = 2^256), selected per call by
 * `zk_repr` so a Rust shim can pass `Vec<F>` memory directly.
 *
 * Conventions
 *  - every function returns ZK_OK (0) or an error code; where the reference
 *    would `panic!` (non-power-of-two tables, mismatched sizes, wrong number of
 *    evaluation points) the call returns ZK_EINVAL and writes nothing else;
 *  - verification failures are NOT errors: they return ZK_OK with
 *    *out_verified = 0, exactly as the reference returns `false`;
 *  - host buffers are caller-owned; `zk_dev_*` calls take HIP device pointers
 *    holding Montgomery elements (32 B each, 16-B aligned);
 *  - a zk_ctx is bound to one HIP device and is not thread-safe: one per
 *    host thread. All calls are synchronous on return;
 *  - compute runs on the GPU only. A ctx cannot be created without a usable
 *    gfx950 device (ZK_EDEVICE); there is no CPU fallback.
 */
#ifndef ZK_SUMCHECK_H
#define ZK_SUMCHECK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_ABI_VERSION 15u

typedef enum { ZK_BN254_FR = 0, ZK_BN254_FQ = 1, ZK_BLS12_381_FR = 2 } zk_field;
typedef enum { ZK_REPR_CANONICAL = 0, ZK_REPR_MONTGOMERY = 1 } zk_repr;

/* One field element: 4 x u64, little-endian limbs. */
typedef struct {
  uint64_t limb[4];
} zk_fe;

enum {
  ZK_OK = 0,
  ZK_EINVAL = 1,       /* reference would panic / bad argument */
  ZK_EDEVICE = 2,      /* HIP error or no usable device */
  ZK_ECOMM = 3,        /* collective failed */
  ZK_ENOMEM = 4,       /* device or host allocation failed */
  ZK_EUNSUPPORTED = 5  /* valid request outside what this build implements */
};

typedef struct zk_ctx zk_ctx;
typedef struct zk_transcript zk_transcript;

uint32_t zk_abi_version(void);
/* Message describing the last failing call on this host thread ("" if none). */
const char* zk_last_error(void);

/* ---------------------------------------------------------------------------
 * Context: HIP device + stream + device workspace (+ optional communicator).
 * ------------------------------------------------------------------------- */
int zk_ctx_create(int device, zk_ctx** out);
void zk_ctx_destroy(zk_ctx* ctx);

/* Per-kernel-kind counters; timing (HIP events around every launch on the
 * ctx stream) is collected only while enabled. */
enum {
  ZK_K_GKR_ROUND0 = 0, /* first GKR round: e0,e1,e2 over the input tables */
  ZK_K_GKR_ROUND = 1,  /* fused fold-by-r + next-round e0,e2 over 4 tables (k_gkr_round) */
  ZK_K_SC_ROUND = 2,   /* plain sum-check: (fold) + half sums */
  ZK_K_FOLD = 3,       /* MultilinearPoly::partial_evaluate */
  ZK_K_REDUCE = 4,     /* block partials -> limb-split sums */
  ZK_K_CONVERT = 5,    /* canonical <-> Montgomery */
  ZK_K_SYNTH = 6,      /* synthetic table generator */
  ZK_K_LAYER = 7,      /* GKR circuit: layer evaluation, gate weights, layer tables */
  ZK_K_MSM = 8,        /* KZG: bucket sort, bucket/window sums, fixed-base setup, normalisation */
  ZK_K_GKR_LANES = 9,  /* the same round for small tables, 8 lanes per pair (k_gkr_round_lanes) */
  ZK_K_GKR_TAIL = 10,  /* the small rounds of a proof in one persistent kernel (k_gkr_tail, ZK_DROUND=0) */
  ZK_K_GKR_DROUND = 11, /* two rounds per kernel: pending folds + round sums + next round's quadratics (k_gkr_dround) */
  ZK_K_GKR_DTAIL = 12, /* the small double rounds in one persistent kernel (k_gkr_dtail) */
  ZK_K_GKR_D0 = 13,    /* the input pass: rounds 0-2 (k_gkr_d0t) or rounds 0 and 1 (k_gkr_d0m), on the matrix cores */
  ZK_K_GKR_DM = 14,    /* two-round steps on the matrix cores that fold by two or three challenges (k_gkr_dm, k_gkr_dm3) */
  ZK_K_GKR_T33 = 15,   /* three-round steps on the matrix cores: fold by three + 27 moment sums (k_gkr_t33) */
  ZK_K_COLL = 16,      /* collectives of a sharded proof: RCCL all-reduce / all-gather (event-timed on the stream
                          when timing is on), or the host communicator's callback (host wall time, always) */
  ZK_K_KINDS = 17
};
typedef struct {
  uint64_t launches[ZK_K_KINDS];
  double kernel_ms[ZK_K_KINDS];  /* sum of event-timed durations */
  double alg_bytes[ZK_K_KINDS];  /* algorithmic HBM bytes */
  double field_muls[ZK_K_KINDS]; /* Montgomery multiplications issued */
  uint64_t host_syncs;           /* device->host round trips */
  uint64_t collectives;          /* all-reduce calls */
  double host_wait_us;           /* host time spent waiting for round results */
  double host_work_us;           /* host time from a round result to the next launch issued */
  uint64_t device_fs_rounds;     /* rounds whose challenge the device drew (ZK_DEVICE_FS), replayed by the host */
} zk_stats;
int zk_ctx_set_timing(zk_ctx* ctx, int enable);                /* all kinds on / off */
int zk_ctx_set_timing_mask(zk_ctx* ctx, uint32_t kind_mask);   /* bit k = time ZK_K_k launches */
int zk_ctx_get_stats(const zk_ctx* ctx, zk_stats* out);
int zk_ctx_reset_stats(zk_ctx* ctx);
/* The event-timed launches since the last zk_ctx_reset_stats, in launch order
 * (kind, duration, algorithmic bytes): *n gets the count, at most cap are copied. */
typedef struct {
  int kind;
  double ms;
  double alg_bytes;
} zk_launch;
int zk_ctx_get_launches(const zk_ctx* ctx, zk_launch* out, size_t cap, size_t* n);

/* ---------------------------------------------------------------------------
 * Fiat-Shamir transcript (host) — fiat_shamir/src/fiat_shamir_transcript.rs
 * ------------------------------------------------------------------------- */
zk_transcript* zk_transcript_new(void);                      /* Transcript::new        :12-17 */
zk_transcript* zk_transcript_clone(const zk_transcript* t);  /* #[derive(Clone)]       :5     */
void zk_transcript_free(zk_transcript* t);
int zk_transcript_append(zk_transcript* t, const uint8_t* data, size_t len); /* append :19-21 */
int zk_transcript_get_random_challenge(zk_transcript* t, zk_field field, zk_repr repr,
                                       zk_fe* out);          /* get_random_challenge   :23-29 */
/* Checkpoint / resume of a transcript mid-proof. The reference's
 * Transcript derives Clone (:5) but not serde; this is the byte image of that clone:
 *   "ZKTR" | u32 version (1) | u32 fill (< 136) | u32 0 | 25 x u64 LE Keccak lanes |
 *   136 bytes of the partial rate block (bytes >= fill are zero)
 * = ZK_TRANSCRIPT_STATE_BYTES. A deserialised transcript continues bit-exactly where the
 * serialised one stood (same challenges for the same appends). zk_transcript_deserialize
 * returns NULL on a bad magic / version / fill / non-zero padding or len != the size. */
#define ZK_TRANSCRIPT_STATE_BYTES 352
int zk_transcript_serialize(const zk_transcript* t, uint8_t* out, size_t cap, size_t* out_len);
zk_transcript* zk_transcript_deserialize(const uint8_t* data, size_t len);
/* fq_vec_to_bytes :32-37 — canonical LE, 32 bytes per element into out[32*n] */
int zk_fe_vec_to_bytes(zk_field field, zk_repr repr, const zk_fe* v, size_t n, uint8_t* out);

/* ---------------------------------------------------------------------------
 * MultilinearPoly — multilinear_polynomial/src/multilinear_polynomial_evaluation.rs
 * ------------------------------------------------------------------------- */
/* partial_evaluate(bit, value) :52-63; out has 2^(nvars-1) elements */
int zk_mle_partial_evaluate(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* evals, uint32_t nvars,
                            uint32_t bit, const zk_fe* value, zk_fe* out);
/* evaluate(values) :79-91; npoint must equal nvars (else ZK_EINVAL, the panic at :80-82) */
int zk_mle_evaluate(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* evals, uint32_t nvars,
                    const zk_fe* point, uint32_t npoint, zk_fe* out);

/* Table builders (multilinear_polynomial_evaluation.rs): op = ZK_MLE_ADD / MUL / SUB.
 *   zk_mle_binop   impl Add / Mul / Sub for MultilinearPoly :113-151 — element-wise over the
 *                  zip of a (2^nvars_a) and b (2^nvars_b): out has 2^min(nvars_a, nvars_b)
 *   zk_mle_scale   scale(value) :93-97 — out[i] = evals[i] * value, 2^nvars outputs
 *   zk_mle_tensor  tensor_add_mul_polynomials(a, b, op) :99-110 — out[i nb + j] = op(a[i], b[j]),
 *                  op ADD or MUL only (Operation :4-17); na * nb must be a nonzero power of
 *                  two (MultilinearPoly::new panics otherwise) — ZK_EINVAL */
typedef enum { ZK_MLE_ADD = 0, ZK_MLE_MUL = 1, ZK_MLE_SUB = 2 } zk_mle_op;
int zk_mle_binop(zk_ctx* ctx, zk_field field, zk_repr repr, zk_mle_op op, const zk_fe* a, uint32_t nvars_a,
                 const zk_fe* b, uint32_t nvars_b, zk_fe* out);
int zk_mle_scale(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* evals, uint32_t nvars,
                 const zk_fe* value, zk_fe* out);
int zk_mle_tensor(zk_ctx* ctx, zk_field field, zk_repr repr, zk_mle_op op, const zk_fe* a, uint64_t na,
                  const zk_fe* b, uint64_t nb, zk_fe* out);

/* ---------------------------------------------------------------------------
 * Sum-check — sum_check/src/sum_check_protocol.rs
 * ------------------------------------------------------------------------- */
/* prove :25-52 -> Proof{proof_polynomials: nvars x [s0, s1], claimed_sum} */
int zk_sumcheck_prove(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* evals, uint32_t nvars,
                      zk_fe* out_round_polys /* 2*nvars */, zk_fe* out_claimed_sum);
/* verify :54-84; round_polys = nrounds polys of poly_len elements each */
int zk_sumcheck_verify(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* evals, uint32_t nvars,
                       const zk_fe* round_polys, uint32_t nrounds, uint32_t poly_len, const zk_fe* claimed_sum,
                       int* out_verified);
/* gkr_prove :86-115 on SumPoly{[ProductPoly[t0,t1], ProductPoly[t2,t3]]}
 * (composed_polynomial.rs:88-103 — reduce uses exactly these four tables).
 * Mutates `transcript`; out_coeffs[3*k .. 3*k+ncoeffs[k]) are round k's trimmed
 * UnivariatePoly coefficients; claimed_sum is passed through (:110-114). */
int zk_gkr_sumcheck_prove(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* const tables[4], uint32_t nvars,
                          const zk_fe* claimed_sum, zk_transcript* transcript, zk_fe* out_coeffs /* 3*nvars */,
                          uint8_t* out_ncoeffs /* nvars */, zk_fe* out_challenges /* nvars */,
                          zk_fe* out_claimed_sum);
/* gkr_verify :117-150 (host-only, O(nrounds)). On failure *out_verified=0,
 * final claim 0 and a single zero challenge (:128-134). out_challenges needs
 * max(nrounds,1) slots. */
int zk_gkr_sumcheck_verify(zk_field field, zk_repr repr, const zk_fe* coeffs /* 3*nrounds */,
                           const uint8_t* ncoeffs, uint32_t nrounds, const zk_fe* claimed_sum,
                           zk_transcript* transcript, int* out_verified, zk_fe* out_final_claimed_sum,
                           zk_fe* out_challenges);

/* ---------------------------------------------------------------------------
 * GKR over a layered circuit (gkr_protocol.rs:31-227,
 * gkr_circuit.rs:1-144). Layers are given input -> output: gates[l] gates in
 * layer l, ops concatenated layer by layer (0 = Operation::Add, 1 = Mul), gate
 * g of layer l reading (in[2g], in[2g+1]). Supported shape (the one for which
 * the reference's table sizes agree; anything else is ZK_EINVAL): powers of
 * two, ninputs = 2 gates[0], gates[l+1] = gates[l] / 2, output layer of 1 or
 * 2 gates, 2 gates[0] <= 2^14.
 * The prover evaluates the circuit, builds every layer's four sum-check tables
 * (wiring folded at the verifier's points — sparse, instead of the reference's
 * dense 2^(3g+2) add_i / mul_i — and the tensor sum / product of w) and runs
 * the layer sum-checks on the GPU; the transcript is the reference's (fresh,
 * output poly absorbed first, alpha / beta per layer). The input layer's KZG
 * commitment (:92-118, row f3) is not made: the two input-MLE evaluations it
 * would open are returned instead, and the verifier recomputes them when
 * given the inputs.
 * Outputs (rounds in processing order: output layer first; layer l has
 * 2 log2(2 gates[l]) rounds, total from zk_gkr_circuit_rounds):
 *   out_output_poly[2], out_coeffs[3*total] + out_ncoeffs[total] (trimmed),
 *   out_challenges[total], out_claims[2*(nlayers-1)] = (o1, o2) per layer
 *   except the input layer, out_input_evals[2].
 * ZK_EINVAL, with no output written: a null pointer (out_claims may be NULL
 * when nlayers = 1), nlayers = 0 or > 24, an unsupported shape, ninputs !=
 * 2 gates[0], an op > 1, an input >= p in either representation, an unknown
 * field or repr.
 * ------------------------------------------------------------------------- */
int zk_gkr_circuit_rounds(uint32_t nlayers, const uint32_t* gates, uint32_t* out_total_rounds);
int zk_gkr_circuit_prove(zk_ctx* ctx, zk_field field, zk_repr repr, uint32_t nlayers, const uint32_t* gates,
                         const uint8_t* ops, const zk_fe* inputs, uint32_t ninputs, zk_fe* out_output_poly,
                         zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_claims,
                         zk_fe* out_input_evals);
/* gkr::verify (host). inputs may be NULL (then the input evaluations are not
 * re-derived, matching a verifier that trusts the commitment opening). */
int zk_gkr_circuit_verify(zk_field field, zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                          const zk_fe* inputs, uint32_t ninputs, const zk_fe* output_poly, const zk_fe* coeffs,
                          const uint8_t* ncoeffs, const zk_fe* claims, const zk_fe* input_evals, int* out_verified);

/* ---------------------------------------------------------------------------
 * GKR over a circuit with explicit wiring: the protocol above
 * (gkr_protocol.rs:31-126) for any layered circuit, not only the binary tree.
 * Layers are given input -> output: gates[l] >= 1 gates in layer l; ops, left
 * and right are concatenated layer by layer; gate g of layer l computes
 * in[left_g] op in[right_g] (0 = Add, 1 = Mul) over the n_below(l) values of
 * the layer below (n_below(0) = ninputs >= 1, else gates[l-1]). Counts need
 * not be powers of two, left == right is allowed, wires may be shared or
 * unused, a layer may be wider than the one below.
 *   kb(l) = max(1, ceil log2 n_below(l)), ka(l) = max(1, ceil log2 gates[l]).
 * A layer's value table is its inputs zero-padded to 2^kb(l); the wiring
 * predicates are zero on padding. The output polynomial is the last layer's
 * values zero-padded to 2^v, v = ka(nlayers-1): all 2^v values are absorbed,
 * v challenges r0 are drawn one after the other, m0 = MLE(out)(r0) (MSB
 * first) is absorbed. Layer l's sum-check (output layer first) has 2 kb(l)
 * rounds, the bits of b then those of c, over
 *   f(b,c) = sum_{g: left_g=b, right_g=c} wt_g (op_g = Add ? w(b)+w(c) : w(b) w(c)),
 * wt_g = eq(r0, g) for the output layer, alpha eq(r_b', g) + beta eq(r_c', g)
 * below it (r_b', r_c' the halves of the previous layer's challenges). After
 * every layer but the input layer o1 = w(r_b) is absorbed, alpha drawn,
 * o2 = w(r_c) absorbed, beta drawn. A tree-shaped wired circuit (left = 2g,
 * right = 2g+1, halving powers of two, ninputs = 2 gates[0]) gives the bytes
 * zk_gkr_circuit_prove gives.
 * ZK_EINVAL: a null array, nlayers = 0, ninputs = 0, a layer without gates, an
 * op > 1, a wire index >= n_below. ZK_EUNSUPPORTED: more than 256 layers, a
 * gates[l] or ninputs above 2^24, more than 2^26 gates in all. The largest
 * shape tested is 2^20 inputs feeding a 2^20-gate layer; between that and the
 * 2^24 cap nothing has been run or measured.
 *   zk_gkr_wired_new    validates and keeps the circuit with its context: the
 *                       wiring and its two groupings per layer (gates by left
 *                       input, gates by right input) live on the device.
 *   zk_gkr_wired_free   releases it (NULL is a no-op). Circuits still alive
 *                       when their context is destroyed are released with it
 *                       and must not be freed afterwards.
 *   zk_gkr_wired_shape  (host only) total rounds = sum of 2 kb(l), and v.
 *   zk_gkr_wired_prove  on the circuit's context. Outputs (rounds in processing
 *                       order, output layer first): out_output_poly[2^v],
 *                       out_coeffs[3*total] + out_ncoeffs[total] (trimmed),
 *                       out_challenges[total], out_claims[2*(nlayers-1)],
 *                       out_input_evals[2] = the input MLE at the last layer's
 *                       (r_b, r_c), which compose with zk_kzg_* as the tree
 *                       prover's do. Nothing is written on failure.
 *                       Layers with kb(l) <= ZK_CIRCUIT_HOST_LGL run on the
 *                       host; ZK_CIRCUIT_DENSE does not apply.
 *   zk_gkr_wired_verify (host only, no ctx) the verifier: the wiring extension
 *                       at a layer's point is sum_g wt_g eq(r_b, left_g)
 *                       eq(r_c, right_g) per op, from eq tables in O(gates +
 *                       2^k). inputs may be NULL (the input evaluations are
 *                       then not re-derived). A rejected proof is ZK_OK with
 *                       *out_verified = 0.
 * ------------------------------------------------------------------------- */
typedef struct zk_wired_circuit zk_wired_circuit;
int zk_gkr_wired_new(zk_ctx* ctx, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops, const uint32_t* left,
                     const uint32_t* right, uint32_t ninputs, zk_wired_circuit** out);
void zk_gkr_wired_free(zk_wired_circuit* circuit);
int zk_gkr_wired_shape(uint32_t nlayers, const uint32_t* gates, uint32_t ninputs, uint32_t* out_total_rounds,
                       uint32_t* out_output_vars);
int zk_gkr_wired_prove(zk_wired_circuit* circuit, zk_field field, zk_repr repr, const zk_fe* inputs,
                       zk_fe* out_output_poly, zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges,
                       zk_fe* out_claims, zk_fe* out_input_evals);
int zk_gkr_wired_verify(zk_field field, zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                        const uint32_t* left, const uint32_t* right, uint32_t ninputs, const zk_fe* inputs,
                        const zk_fe* output_poly, const zk_fe* coeffs, const uint8_t* ncoeffs, const zk_fe* claims,
                        const zk_fe* input_evals, int* out_verified);

/* ---------------------------------------------------------------------------
 * Sum-check over any sum of products of multilinear tables:
 * gkr_prove's loop (sum_check_protocol.rs:86-166) with SumPoly::reduce done in
 * full, beside zk_gkr_sumcheck_prove, which keeps the reference's four-table
 * reduce and its bytes. Given ntables distinct tables of 2^nvars elements and
 * nterms products of `degree` factors, each factor an index into the tables
 * (factors[t * degree + d], term-major; an index may repeat within a term and
 * across terms), the polynomial is f = sum_t prod_d table[factors[t][d]].
 * Round k: y_i = sum_j f_k(i, j) for i = 0..degree, variable 0 (the MSB) bound
 * to i as partial_evaluate(0, i) binds it; the polynomial of degree <= degree
 * through (i, y_i), trailing zeros trimmed; its coefficient bytes absorbed
 * (none when it trims to nothing); one challenge r_k; every table folded by
 * r_k. With ntables = 4 and factors = {0,1, 2,3} the outputs are
 * zk_gkr_sumcheck_prove's, byte for byte. claimed_sum is carried through and
 * influences no round polynomial.
 * Caps: ntables <= 16, nterms <= 16, nvars <= 26, and */
#define ZK_COMPOSED_MAX_DEGREE 4 /* degree <= 4: the highest whose round kernels were built and found free of scratch */
/* ZK_EINVAL: a null pointer, ntables, nterms or degree = 0, a factor index >=
 * ntables, an unknown field or repr, a value >= p. ZK_EUNSUPPORTED: a cap
 * exceeded. nvars = 0 is valid: no rounds, out_table_evals are the single
 * entries (out_coeffs, out_ncoeffs and out_challenges may then be NULL).
 * Nothing is written on failure.
 *   zk_composed_sumcheck_prove      tables in host memory. Outputs:
 *                       out_coeffs[(degree+1)*nvars] (round k at (degree+1)*k,
 *                       zero past its trimmed count out_ncoeffs[k]),
 *                       out_challenges[nvars], out_table_evals[ntables] = table
 *                       i at the challenge point (the fully folded table: the
 *                       verifier's final check is final_claim ==
 *                       combine(table_evals)), *out_claimed_sum = claimed_sum.
 *                       Rounds whose tables have at most 2^ZK_COMPOSED_HOST_LG
 *                       entries (default 6, read at zk_ctx_create; 0: every
 *                       round on the device) run on the host.
 *   zk_dev_composed_sumcheck_prove  the same over Montgomery tables already in
 *                       device memory (repr: the scalars in and out). The
 *                       inputs are only read; the folds live in the context's
 *                       workspace.
 *   zk_composed_sumcheck_verify     (host only, no ctx) gkr_verify with a
 *                       degree bound over coeffs[(degree+1)*nrounds]. A round
 *                       with ncoeffs[k] > degree + 1, or with s(0) + s(1) !=
 *                       claim, is ZK_OK with *out_verified = 0, final claim 0
 *                       and one zero challenge, as zk_gkr_sumcheck_verify.
 *   zk_composed_combine             (host only) sum_t prod_d
 *                       table_evals[factors[t][d]].
 * ------------------------------------------------------------------------- */
int zk_composed_sumcheck_prove(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* const* tables, uint32_t ntables,
                               uint32_t nvars, const uint8_t* factors, uint32_t nterms, uint32_t degree,
                               const zk_fe* claimed_sum, zk_transcript* transcript, zk_fe* out_coeffs,
                               uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_table_evals,
                               zk_fe* out_claimed_sum);
int zk_dev_composed_sumcheck_prove(zk_ctx* ctx, zk_field field, zk_repr repr, const void* const* d_tables,
                                   uint32_t ntables, uint32_t nvars, const uint8_t* factors, uint32_t nterms,
                                   uint32_t degree, const zk_fe* claimed_sum, zk_transcript* transcript,
                                   zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges,
                                   zk_fe* out_table_evals, zk_fe* out_claimed_sum);
int zk_composed_sumcheck_verify(zk_field field, zk_repr repr, uint32_t degree, const zk_fe* coeffs,
                                const uint8_t* ncoeffs, uint32_t nrounds, const zk_fe* claimed_sum,
                                zk_transcript* transcript, int* out_verified, zk_fe* out_final_claim,
                                zk_fe* out_challenges);
int zk_composed_combine(zk_field field, zk_repr repr, const zk_fe* table_evals, uint32_t ntables,
                        const uint8_t* factors, uint32_t nterms, uint32_t degree, zk_fe* out);

/* ---------------------------------------------------------------------------
 * Multilinear KZG over BLS12-381 G1 (pcs/src/kzg_pcs/kzg.rs).
 * Scalars are BLS12-381 Fr (zk_fe, repr as elsewhere). Points are affine with
 * canonical little-endian 48-byte coordinates; (0, 0) is the point at infinity.
 *   zk_kzg_setup       KZG::new / run_trusted_setup's G1 half (:18-49): the
 *                      Lagrange basis eq(taus, i) * G for every i (MSB-first
 *                      hypercube, generate_bhc :171-181), plus the bases over
 *                      every suffix of taus used by get_proof, and (host)
 *                      the G2 taus tau_i * G2 used by KZG::verify (below).
 *   zk_kzg_commit      KZG::commit (:51-53) = sum_i evals[i] * L_i (Pippenger MSM)
 *   zk_kzg_get_proof   KZG::get_proof (:59-95): nvars quotient commitments
 *   zk_kzg_lagrange_basis  the basis over the last nvars_suffix taus
 *   zk_msm_g1          sum_i scalars[i] * bases[i] for caller bases (checked on the curve)
 * KZG::open is MultilinearPoly::evaluate: zk_mle_evaluate.
 * ------------------------------------------------------------------------- */
typedef struct {
  uint64_t x[6];
  uint64_t y[6];
} zk_g1;
typedef struct zk_kzg zk_kzg;
int zk_kzg_setup(zk_ctx* ctx, zk_repr repr, const zk_fe* taus, uint32_t nvars, zk_kzg** out);
void zk_kzg_free(zk_kzg* kzg);
int zk_kzg_lagrange_basis(zk_ctx* ctx, const zk_kzg* kzg, uint32_t nvars_suffix, zk_g1* out /* 2^nvars_suffix */);
int zk_kzg_commit(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const zk_fe* evals /* 2^nvars */, zk_g1* out);
int zk_dev_kzg_commit(zk_ctx* ctx, const zk_kzg* kzg, const void* dev_evals /* Montgomery Fr */, zk_g1* out);
int zk_kzg_get_proof(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const zk_fe* evals, const zk_fe* opened_value,
                     const zk_fe* point /* nvars */, zk_g1* out /* nvars */);
/* KZG::get_proof with the evaluations already on the device (Montgomery Fr,
 * 2^nvars, as zk_dev_kzg_commit takes them; read only): no host upload. repr
 * applies to opened_value and point. */
int zk_dev_kzg_get_proof(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const void* dev_evals, const zk_fe* opened_value,
                         const zk_fe* point /* nvars */, zk_g1* out /* nvars */);
/* Setups of >= 2^16 points use a fixed-base table of G1 (654 MB of device
 * memory) built once per device and shared by every context of the process.
 * This frees it for `device` (-1: every device); the next large setup rebuilds
 * it (~50 ms). ZK_EINVAL while a setup on that device is using it. */
int zk_kzg_release_fixed_base_cache(int device);
int zk_msm_g1(zk_ctx* ctx, zk_repr repr, const zk_g1* bases, const zk_fe* scalars, size_t n, zk_g1* out);

/* Verifier half (host, O(nvars) pairings; pcs/src/kzg_pcs/kzg.rs:35-49, :97-129).
 * G2 points are affine over Fq2 = Fq[u]/(u^2+1): x = x[0] + x[1] u, canonical
 * 48-byte LE coordinates, all zero = infinity; inputs are checked on the twist
 * y^2 = x^3 + 4(1+u).
 *   zk_kzg_g2_taus     KZG::g2_taus (pub field): tau_i * G2, nvars points
 *   zk_kzg_verify      KZG::verify: 1 / 0 in *out_verified; nproof != npoint is
 *                      ZK_EINVAL (the panic at :104-106); g2_taus holds npoint points
 *   zk_g2_mul_generator  scalars[i] * G2 (G2Projective::mul_bigint)
 *   zk_bls12_381_pairing Bls12_381::pairing(p, q) as 6 Fq2 = 72 u64: the
 *                      Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (1+u)) element
 *                      c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each Fq2 as (re, im)
 *                      canonical 6 x u64 (ark's field order)
 *   zk_bls12_381_pairing_check  *out_ok = prod_i e(p_i, q_i) == 1 */
typedef struct {
  uint64_t x[2][6];
  uint64_t y[2][6];
} zk_g2;
int zk_kzg_g2_taus(const zk_kzg* kzg, zk_g2* out /* nvars */);
int zk_kzg_verify(zk_repr repr, const zk_g1* commitment, const zk_fe* opened_value, const zk_g1* proof,
                  uint32_t nproof, const zk_fe* point, uint32_t npoint, const zk_g2* g2_taus, int* out_verified);
int zk_g2_mul_generator(zk_repr repr, const zk_fe* scalars, size_t n, zk_g2* out);
int zk_bls12_381_pairing(const zk_g1* p, const zk_g2* q, uint64_t out[72]);
int zk_bls12_381_pairing_check(const zk_g1* p, const zk_g2* q, size_t n, int* out_ok);

/* gkr::prove WITH the input layer's KZG step (gkr_protocol.rs:92-118), so the
 * proof is the reference's GkrProof including input_proof. BLS12-381 Fr only
 * (the reference's KZG is over BLS12-381, kzg.rs:3). The reference draws the
 * taus from StdRng::from_entropy (:97-103); here they are the caller's
 * taus[log2 ninputs] so proofs are reproducible. Writes everything
 * zk_gkr_circuit_prove writes (out_input_evals = the two values KZG::open
 * returns at r_b and r_c), plus the commitment (KZG::commit :106), the two
 * get_proof results out_proofs[2 log2 ninputs] (w_b's then w_c's, :108-113)
 * and the verifier's setup out_g2_taus[log2 ninputs] (KZG::g2_taus). */
int zk_gkr_circuit_prove_kzg(zk_ctx* ctx, zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                             const zk_fe* inputs, uint32_t ninputs, const zk_fe* taus, zk_fe* out_output_poly,
                             zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_claims,
                             zk_fe* out_input_evals, zk_g1* out_commitment, zk_g1* out_proofs, zk_g2* out_g2_taus);
/* gkr::verify (:128-227) with the two KZG::verify checks of the input layer
 * (:155-175) at the verifier's own (r_b, r_c): needs no inputs.
 * SOUNDNESS: g2_taus must come from a trusted setup the verifier holds, NOT
 * from the proof. The reference passes the prover's kzg_setup.g2_taus
 * (gkr_protocol.rs:167,175), and this entry point keeps that behaviour for
 * parity. A prover who picks its own setup can satisfy both pairings, so
 * this check is not sound against a malicious prover unless the caller
 * supplies g2_taus of its own (zk_kzg_g2_taus of a setup it trusts). */
int zk_gkr_circuit_verify_kzg(zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                              const zk_fe* output_poly, const zk_fe* coeffs, const uint8_t* ncoeffs,
                              const zk_fe* claims, const zk_fe* opened_evals, const zk_g1* commitment,
                              const zk_g1* proofs, const zk_g2* g2_taus, int* out_verified);

/* ---------------------------------------------------------------------------
 * Sum-check over KZG-committed tables with one batched opening.
 * zk_composed_sumcheck_* ends with table_evals[i], table i at the challenge
 * point; these entry points tie those values to commitments, so that an
 * identity such as eq (a b - c) = 0 is an argument about committed a, b, c.
 * BLS12-381 Fr throughout, as all KZG here, except the two table builders,
 * which take any field.
 *
 * Table builders (device tables are Montgomery, as zk_dev_upload leaves them;
 * repr applies to the host scalars):
 *   zk_dev_mle_lincomb   d_out[j] = sum_i coeffs[i] table_i[j] + constant
 *                        (constant NULL = 0) for j < count. 1 <= ntables <= 16,
 *                        count >= 1; the same table may appear more than once;
 *                        d_out must be none of the inputs (pointers compared)
 *                        and must not overlap one. ZK_EINVAL: a null pointer,
 *                        ntables = 0, count = 0, d_out equal to an input, a
 *                        coefficient or constant >= p, an unknown field or
 *                        repr. ZK_EUNSUPPORTED: ntables > 16. Nothing is
 *                        written on failure.
 *   zk_dev_mle_eq_table  d_out[j] = eq(point, bits of j) for j < 2^n, bit
 *                        n-1-k of j against point[k] (MSB first, the order the
 *                        sum-checks bind variables in). n <= 26
 *                        (ZK_EUNSUPPORTED above); n = 0 gives the single entry 1.
 *   zk_mle_eq_table      the same into host memory.
 *   zk_mle_eq_eval       (host only, no ctx) prod_i (a_i b_i + (1 - a_i)(1 - b_i)):
 *                        the eq table of a at the point b, what a verifier
 *                        computes for a public eq table.
 *
 * Batched KZG (k tables over one setup, opened at ONE point by one proof, by
 * the random linear combination with weights rho^0 .. rho^(k-1) in the order
 * given; 1 <= ntables <= 16, ZK_EUNSUPPORTED above):
 *   zk_dev_kzg_commit_batch / zk_kzg_commit_batch   out[i] = KZG::commit of
 *                        table i: one MSM per table.
 *   zk_dev_kzg_batch_open / zk_kzg_batch_open       get_proof(v, point, g) for
 *                        g = sum_j rho^j table_j and v = sum_j rho^j
 *                        opened_values[j]: nvars quotient commitments. One
 *                        streaming pass over the tables, then the work of one
 *                        zk_dev_kzg_get_proof; with ntables = 1 its bytes,
 *                        whatever rho is.
 *   zk_kzg_batch_verify  (host only, no ctx) KZG::verify of C = sum_j rho^j
 *                        commitments[j] against the same v. Commitments must be
 *                        on the curve ((0, 0), infinity, is: an all-zero table
 *                        commits to it); nproof != npoint is ZK_EINVAL.
 *
 * The committed sum-check. Bit i of committed_mask says table i is committed;
 * the other tables are public (eq, selectors, a table of ones), and the
 * verifier evaluates those itself. The transcript, on the caller's handle:
 *   1. for each committed table in index order, append 96 bytes: x then y,
 *      each canonical little-endian 48 bytes, as zk_g1 holds them (infinity
 *      is 96 zero bytes);
 *   2. the composed sum-check, exactly as zk_composed_sumcheck_prove runs it;
 *   3. append(fq_vec_to_bytes(table_evals[0..ntables))), then rho =
 *      get_random_challenge;
 *   4. the j-th committed table (index order) gets rho^j; the opening is
 *      batch_open at the sum-check's challenges with the committed tables'
 *      table_evals as opened values (the sum-check binds variable 0, the MSB,
 *      first, and get_proof divides out the top variable first: the same point).
 *   zk_committed_sumcheck_prove      tables in host memory (uploaded once, for
 *                        the sum-check and the opening). Writes everything
 *                        zk_composed_sumcheck_prove writes, then
 *                        out_commitments[popcount(mask)] in table-index order
 *                        and out_opening[nvars]. commitments_in (NULL: compute
 *                        them) lets a prover reuse commitments made once: they
 *                        are absorbed and returned as given, not recomputed
 *                        (only checked to be on the curve).
 *   zk_dev_committed_sumcheck_prove  the same over Montgomery tables on the
 *                        device; the inputs are only read.
 *   zk_committed_sumcheck_verify     (host only, no ctx) *out_verified = 1
 *                        requires all of: the composed verifier accepts,
 *                        final_claim == combine(table_evals), and
 *                        zk_kzg_batch_verify accepts the opening at the
 *                        verifier's own challenges. A failed check is ZK_OK
 *                        with *out_verified = 0 and one zero challenge, as
 *                        zk_composed_sumcheck_verify. It does NOT check the
 *                        public tables' entries of table_evals: it returns
 *                        out_challenges[nrounds] so that the caller can
 *                        (zk_mle_evaluate, zk_mle_eq_eval), and must.
 *                        SOUNDNESS: the note on g2_taus at
 *                        zk_gkr_circuit_verify_kzg applies unchanged: they must
 *                        come from a setup the verifier trusts, not from the
 *                        prover.
 * ZK_EINVAL besides the composed sum-check's: committed_mask = 0, a mask bit
 * at or above ntables, nvars (nrounds) different from the setup's variable
 * count (so nvars = 0: KZG needs one variable), a point not on the curve. The
 * composed caps are unchanged. Nothing is written on failure, the transcript
 * included.
 * ------------------------------------------------------------------------- */
int zk_dev_mle_lincomb(zk_ctx* ctx, zk_field field, zk_repr repr, const void* const* d_tables, uint32_t ntables,
                       const zk_fe* coeffs /* ntables */, const zk_fe* constant /* may be NULL = 0 */, uint64_t count,
                       void* d_out);
int zk_dev_mle_eq_table(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* point, uint32_t n,
                        void* d_out /* 2^n */);
int zk_mle_eq_table(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* point, uint32_t n, zk_fe* out /* 2^n */);
int zk_mle_eq_eval(zk_field field, zk_repr repr, const zk_fe* a, const zk_fe* b, uint32_t n, zk_fe* out);
int zk_dev_kzg_commit_batch(zk_ctx* ctx, const zk_kzg* kzg, const void* const* d_tables, uint32_t ntables,
                            zk_g1* out /* ntables */);
int zk_kzg_commit_batch(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const zk_fe* const* tables, uint32_t ntables,
                        zk_g1* out /* ntables */);
int zk_dev_kzg_batch_open(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const void* const* d_tables, uint32_t ntables,
                          const zk_fe* rho, const zk_fe* opened_values /* ntables */, const zk_fe* point /* nvars */,
                          zk_g1* out /* nvars */);
int zk_kzg_batch_open(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const zk_fe* const* tables, uint32_t ntables,
                      const zk_fe* rho, const zk_fe* opened_values /* ntables */, const zk_fe* point /* nvars */,
                      zk_g1* out /* nvars */);
int zk_kzg_batch_verify(zk_repr repr, const zk_g1* commitments, uint32_t ntables, const zk_fe* rho,
                        const zk_fe* opened_values, const zk_g1* proof, uint32_t nproof, const zk_fe* point,
                        uint32_t npoint, const zk_g2* g2_taus, int* out_verified);
int zk_committed_sumcheck_prove(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const zk_fe* const* tables,
                                uint32_t ntables, uint32_t nvars, const uint8_t* factors, uint32_t nterms,
                                uint32_t degree, uint32_t committed_mask,
                                const zk_g1* commitments_in /* NULL: compute them */, const zk_fe* claimed_sum,
                                zk_transcript* transcript, zk_fe* out_coeffs, uint8_t* out_ncoeffs,
                                zk_fe* out_challenges, zk_fe* out_table_evals, zk_fe* out_claimed_sum,
                                zk_g1* out_commitments /* popcount(mask), table-index order */,
                                zk_g1* out_opening /* nvars */);
int zk_dev_committed_sumcheck_prove(zk_ctx* ctx, const zk_kzg* kzg, zk_repr repr, const void* const* d_tables,
                                    uint32_t ntables, uint32_t nvars, const uint8_t* factors, uint32_t nterms,
                                    uint32_t degree, uint32_t committed_mask, const zk_g1* commitments_in,
                                    const zk_fe* claimed_sum, zk_transcript* transcript, zk_fe* out_coeffs,
                                    uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_table_evals,
                                    zk_fe* out_claimed_sum, zk_g1* out_commitments, zk_g1* out_opening);
int zk_committed_sumcheck_verify(zk_repr repr, uint32_t degree, const zk_fe* coeffs, const uint8_t* ncoeffs,
                                 uint32_t nrounds, const zk_fe* claimed_sum, const uint8_t* factors, uint32_t nterms,
                                 uint32_t ntables, const zk_fe* table_evals, uint32_t committed_mask,
                                 const zk_g1* commitments, const zk_g1* opening, const zk_g2* g2_taus,
                                 zk_transcript* transcript, int* out_verified, zk_fe* out_challenges);

/* ---------------------------------------------------------------------------
 * R1CS satisfiability by two sum-checks over a committed witness (DESIGN.md
 * 6k; the Spartan reduction, Setty 2020, without the commitment to the
 * matrices: the verifier is O(entries)). Any field; the KZG closing is
 * BLS12-381 Fr, as all KZG here.
 *
 * The statement. nrows >= 1 constraints (A z)_i (B z)_i = (C z)_i. z has 2^sy
 * entries: the first half (MSB = 0) is the witness w of 2^(sy-1) entries, the
 * second half is (1, io_0 .. io_(npub-1), 0 ..), npub + 1 <= 2^(sy-1). Each
 * matrix is a list of (row, col, value) in any order; duplicates of a
 * (row, col) inside one matrix add up; zero values are allowed. sx =
 * max(1, ceil log2 nrows); rows are zero-padded to 2^sx.
 * Caps: sx, sy <= 24 and at most 2^26 entries in all (ZK_EUNSUPPORTED above).
 * ZK_EINVAL: nrows = 0, sy = 0, a row >= nrows, a column >= 2^sy, a value >= p,
 * npub + 1 > 2^(sy-1), an unknown field or repr, a null pointer.
 *
 * The transcript, on the caller's handle:
 *   1. digest = Keccak-256 of: the ASCII bytes "zk-r1cs-v1"; then as u32
 *      little-endian field, nrows, sx, sy, npub; then for A, B, C in turn the
 *      u32 entry count and each entry in the caller's order as u32 row, u32
 *      col and the value's 32 canonical little-endian bytes. Computed at
 *      handle creation;
 *   2. append(digest), append(fq_vec_to_bytes(io)) and, with a KZG setup, the
 *      96 bytes of the commitment of w (the committed sum-check's encoding,
 *      infinity 96 zero bytes);
 *   3. tau_0 .. tau_(sx-1) by sx consecutive get_random_challenge;
 *   4. sum-check 1, exactly as zk_composed_sumcheck_prove runs it: tables
 *      [eq(tau,.), Az, Bz, -eq(tau,.), Cz, 1], factors {0,1,2},{3,4,5}, degree
 *      3, claimed sum 0. Its challenges are rx; va, vb, vc = Az, Bz, Cz at rx;
 *   5. append(fq_vec_to_bytes([va, vb, vc])), rho = get_random_challenge;
 *   6. M(y) = sum_x eq(rx, x) (A + rho B + rho^2 C)(x, y) over the 2^sy columns;
 *   7. sum-check 2: tables [M, z], factors {0,1}, degree 2, claimed sum
 *      va + rho vb + rho^2 vc. Its challenges are ry;
 *   8. vw = w~(ry[1..]), append(fq_vec_to_bytes([vw])). With a KZG setup of
 *      sy - 1 variables (so sy >= 2) the opening is get_proof(w, vw, ry[1..]);
 *      without one the proof ends in the claim (ry[1..], vw), which the caller
 *      checks, as zk_composed_sumcheck_verify leaves table_evals to the caller.
 * A proof: coeffs1[4 sx] / ncoeffs1[sx] and coeffs2[3 sy] / ncoeffs2[sy] (the
 * round polynomials, degree + 1 slots per round, zero past the trimmed count),
 * evals[4] = (va, vb, vc, vw) and, committed, the commitment and sy - 1
 * quotient commitments.
 *
 *   zk_r1cs_new     nnz[3]: the entry counts of A, B, C; rows / cols / vals:
 *                   their entries concatenated, A's then B's then C's. With a
 *                   context the two groupings of the entries (by row, by
 *                   column) and their values go to the device; the handle
 *                   works through that context: use it only while the context
 *                   lives (zk_r1cs_free itself does not read the context). With
 *                   ctx == NULL the handle is host-only: it verifies, with an
 *                   O(entries) host evaluation of the three matrices, and
 *                   multiplies on the host, but cannot prove (ZK_EDEVICE).
 *   zk_r1cs_shape   sx, sy, the round counts of the two sum-checks (sx and
 *                   sy) and the digest; any output may be NULL.
 *   zk_r1cs_mul / zk_dev_r1cs_mul   z (2^sy) -> Az, Bz, Cz, 2^sx entries each
 *                   (zero in the padded rows). The device entry takes and
 *                   fills Montgomery tables on the device, none of them
 *                   overlapping another.
 *   zk_dev_r1cs_mul_t   the transposes: x (2^sx, Montgomery, on the device) ->
 *                   A^T x, B^T x, C^T x, 2^sy entries each (zero in columns
 *                   without entries): the column pass with the three sums kept
 *                   apart, which the prover runs on x = eq(rx, .).
 *   zk_r1cs_matrix_evals  out[3] = the multilinear extensions of A, B, C at
 *                   (rx[sx], ry[sy]): on the device when the handle has a
 *                   context (the column pass, then three dot products), on the
 *                   host otherwise.
 *   zk_r1cs_prove / zk_dev_r1cs_prove   witness: 2^(sy-1) entries in host /
 *                   device (Montgomery) memory, only read; io[npub] in host
 *                   memory (NULL when npub = 0). kzg NULL: uncommitted, and
 *                   commitment_in, out_commitment, out_opening are ignored.
 *                   With a setup (BLS12-381 Fr, sy - 1 variables; else
 *                   ZK_EINVAL) commitment_in (NULL: compute it) is absorbed and
 *                   returned as given, only checked to be on the curve. Writes
 *                   the proof, out_rx[sx] and out_ry[sy]. The instance need
 *                   not be satisfied: the proof of an unsatisfied one is
 *                   rejected.
 *   zk_r1cs_verify  *out_verified = 1 requires all of: zk_composed_sumcheck_verify
 *                   accepts both lists of rounds; final_1 == eq(tau, rx)
 *                   (va vb - vc); final_2 == (A~ + rho B~ + rho^2 C~)(rx, ry) vz
 *                   with vz = (1 - ry_0) vw + ry_0 pub~(ry[1..]), the public
 *                   part summed over its npub + 1 non-zero entries; and, with a
 *                   commitment, zk_kzg_verify of the opening at ry[1..].
 *                   commitment, opening and g2_taus are all given or all NULL;
 *                   uncommitted, the caller checks w~(out_ry[1..]) == evals[3].
 *                   A rejection is ZK_OK with *out_verified = 0 and nothing
 *                   else written, the transcript included.
 *                   SOUNDNESS: the note on g2_taus at zk_gkr_circuit_verify_kzg
 *                   applies unchanged: they must come from a setup the
 *                   verifier trusts, not from the prover.
 * Every call works on a copy of the transcript and hands it back only on
 * success: nothing is written on failure.
 * ------------------------------------------------------------------------- */
typedef struct zk_r1cs zk_r1cs;
int zk_r1cs_new(zk_ctx* ctx /* NULL: host-only */, zk_field field, zk_repr repr, uint32_t nrows, uint32_t sy,
                uint32_t npub, const uint32_t nnz[3], const uint32_t* rows, const uint32_t* cols, const zk_fe* vals,
                zk_r1cs** out);
void zk_r1cs_free(zk_r1cs* r);
int zk_r1cs_shape(const zk_r1cs* r, uint32_t* out_sx, uint32_t* out_sy, uint32_t* out_rounds1, uint32_t* out_rounds2,
                  uint8_t out_digest[32]);
int zk_r1cs_mul(zk_r1cs* r, zk_repr repr, const zk_fe* z /* 2^sy */, zk_fe* out_az, zk_fe* out_bz,
                zk_fe* out_cz /* 2^sx each */);
int zk_dev_r1cs_mul(zk_r1cs* r, const void* d_z, void* d_az, void* d_bz, void* d_cz);
int zk_dev_r1cs_mul_t(zk_r1cs* r, const void* d_x /* 2^sx */, void* d_atx, void* d_btx, void* d_ctx /* 2^sy each */);
int zk_r1cs_matrix_evals(zk_r1cs* r, zk_repr repr, const zk_fe* rx /* sx */, const zk_fe* ry /* sy */,
                         zk_fe out[3]);
int zk_r1cs_prove(zk_r1cs* r, zk_repr repr, const zk_fe* witness /* 2^(sy-1) */, const zk_fe* io /* npub */,
                  const zk_kzg* kzg /* may be NULL */, const zk_g1* commitment_in /* NULL: compute it */,
                  zk_transcript* transcript, zk_fe* out_coeffs1 /* 4 sx */, uint8_t* out_ncoeffs1 /* sx */,
                  zk_fe* out_coeffs2 /* 3 sy */, uint8_t* out_ncoeffs2 /* sy */, zk_fe out_evals[4],
                  zk_fe* out_rx /* sx */, zk_fe* out_ry /* sy */, zk_g1* out_commitment,
                  zk_g1* out_opening /* sy - 1 */);
int zk_dev_r1cs_prove(zk_r1cs* r, zk_repr repr, const void* d_witness, const zk_fe* io, const zk_kzg* kzg,
                      const zk_g1* commitment_in, zk_transcript* transcript, zk_fe* out_coeffs1,
                      uint8_t* out_ncoeffs1, zk_fe* out_coeffs2, uint8_t* out_ncoeffs2, zk_fe out_evals[4],
                      zk_fe* out_rx, zk_fe* out_ry, zk_g1* out_commitment, zk_g1* out_opening);
int zk_r1cs_verify(zk_r1cs* r, zk_repr repr, const zk_fe* io, const zk_fe* coeffs1, const uint8_t* ncoeffs1,
                   const zk_fe* coeffs2, const uint8_t* ncoeffs2, const zk_fe evals[4],
                   const zk_g1* commitment /* NULL: uncommitted */, const zk_g1* opening, const zk_g2* g2_taus,
                   zk_transcript* transcript, int* out_verified, zk_fe* out_rx /* sx */, zk_fe* out_ry /* sy */);

/* ---------------------------------------------------------------------------
 * Lookups (LogUp, Haboeck 2022) over committed columns: every
 * entry of a committed column lies in a public table. Range checks, byte
 * decompositions and fixed function tables reduce to it. The two device
 * primitives in front of it, the batched inversion and the multiplicity
 * count, take any field; proving and verifying are BLS12-381 Fr, as all KZG
 * here.
 *
 * The statement. f: a column of 2^n elements, 1 <= n <= 24 (ZK_EUNSUPPORTED
 * above). t: a public table of T elements, 1 <= T <= 2^n, duplicates allowed.
 * Claim: every f_i equals some t_j. t_pad[j] = t[min(j, T - 1)] for j < 2^n.
 * m_j = #{i : f_i = t_j} at the FIRST index j holding that value, 0 at every
 * later duplicate and at the padding. h_f = 1 / (alpha - f), h_t = m /
 * (alpha - t_pad).
 *
 * The transcript, on the caller's handle:
 *   1. digest = Keccak-256 of: the ASCII bytes "zk-lookup-v1"; then as u32
 *      little-endian field, T; then each t_j as its 32 canonical little-endian
 *      bytes. Computed at handle creation;
 *   2. append(digest), append(u32 little-endian n), then the 96 bytes of the
 *      commitment of f and of m (the committed sum-check's encoding);
 *   3. alpha = get_random_challenge;
 *   4. the helper columns h_f and h_t (1 / 0 is taken as 0: then identity (b)
 *      or (c) below fails and the proof is rejected);
 *   5. the 96 bytes of the commitment of h_f and of h_t;
 *   6. tau_0 .. tau_(n-1) by n consecutive get_random_challenge, then lambda =
 *      get_random_challenge;
 *   7. one zk_dev_committed_sumcheck_prove, unchanged, with the four
 *      commitments as commitments_in (it absorbs them again, in table order),
 *      claimed sum 0, degree 3, committed mask 0b1111, the eleven tables
 *        0 h_f   1 h_t   2 f   3 m   4 t_pad   5 ones   6 -ones
 *        7 alpha lambda eq(tau,.)     8 -lambda eq(tau,.)
 *        9 alpha lambda^2 eq(tau,.)   10 -lambda^2 eq(tau,.)
 *      and the eight terms {0,5,5} {1,6,5} {7,0,5} {8,0,2} {8,5,5} {9,1,5}
 *      {10,1,4} {10,3,5}: the sum is
 *        (a) sum (h_f - h_t)
 *        (b) + lambda   sum eq(tau,.) (h_f (alpha - f) - 1)
 *        (c) + lambda^2 sum eq(tau,.) (h_t (alpha - t_pad) - m).
 * A proof: coeffs[4 n] / ncoeffs[n] (the round polynomials, 4 slots per round,
 * zero past the trimmed count), table_evals[11], four commitments in table
 * order (h_f, h_t, f, m) and n quotient commitments.
 *
 *   zk_fe_batch_inverse / zk_dev_fe_batch_inverse   out[i] = in[i]^-1, and 0 -> 0,
 *                   over count >= 1 elements (any count, not only a power of
 *                   two): Montgomery's trick, one Fermat power per 64
 *                   elements. The host entry takes zk_fe arrays in `repr`; the
 *                   device entry Montgomery tables on the device. out == in is
 *                   allowed; a partial overlap is ZK_EINVAL.
 *   zk_lookup_new   validates the table (a value >= p, T = 0: ZK_EINVAL; T >
 *                   2^24: ZK_EUNSUPPORTED) and builds its hash on the host,
 *                   deterministically: 2^s slots, the power of two at least
 *                   2 T; slot of a value = ((low 32 bits of its canonical
 *                   form) * 0x9E3779B1 mod 2^32) >> (32 - s), so values equal
 *                   mod 2^32 collide; linear probing in index order; a slot
 *                   holds the first index of its value, or 0xFFFFFFFF when
 *                   empty. With a context the slots and the Montgomery table
 *                   go to the device and the handle works through that
 *                   context: use it only while the context lives
 *                   (zk_lookup_free itself does not read the context). With
 *                   ctx == NULL the handle is host-only: it counts, evaluates
 *                   and verifies on the host, but cannot prove (ZK_EDEVICE).
 *   zk_lookup_info  T, the slot count, the digest and the slots; any output
 *                   may be NULL.
 *   zk_lookup_multiplicities / zk_dev_lookup_multiplicities   m over all 2^n
 *                   slots (zero at or above T) from `count` column entries, 1
 *                   <= count <= 2^24, T <= 2^n; *out_missing = the number of
 *                   entries found nowhere in the table. The device entry takes
 *                   and fills Montgomery tables on the device that do not
 *                   overlap; a host-only handle counts on the host.
 *   zk_lookup_table_eval   t_pad~(point[n]) in O(T) products on the host:
 *                   c + sum_(j<T) (t_j - c) eq(point, j), c = t[T - 1].
 *   zk_lookup_prove / zk_dev_lookup_prove   f: 2^n entries in host / device
 *                   (Montgomery) memory, only read. kzg: a setup of n
 *                   variables. commitment_in (NULL: compute it) is f's
 *                   commitment, absorbed and returned as given, only checked to
 *                   be on the curve. Writes the proof, out_point[n] (the
 *                   sum-check's challenges) and *out_missing. A column with
 *                   non-members is not refused: out_missing reports them, and
 *                   the proof is rejected.
 *   zk_lookup_verify   works with a host-only handle. Replays steps 2 - 6,
 *                   calls zk_committed_sumcheck_verify, then checks the public
 *                   entries of table_evals itself: ones is 1, -ones is -1, the
 *                   four scaled eq entries by eq(tau, point), t_pad by the
 *                   handle. A rejection is ZK_OK with *out_verified = 0 and
 *                   nothing else written, the transcript included.
 *                   SOUNDNESS: the note on g2_taus at zk_gkr_circuit_verify_kzg
 *                   applies unchanged: they must come from a setup the
 *                   verifier trusts, not from the prover.
 * ZK_EINVAL: a null pointer, T = 0, T > 2^n, n = 0, a value >= p, a setup whose
 * variable count is not n, a field other than BLS12-381 Fr for prove or
 * verify, a point not on the curve. ZK_EUNSUPPORTED: n > 24. Every call works
 * on a copy of the transcript and hands it back only on success: nothing is
 * written on failure.
 * ------------------------------------------------------------------------- */
typedef struct zk_lookup zk_lookup;
int zk_fe_batch_inverse(zk_field field, zk_repr repr, const zk_fe* in, uint64_t count, zk_fe* out);
int zk_dev_fe_batch_inverse(zk_ctx* ctx, zk_field field, const void* d_in, uint64_t count, void* d_out);
int zk_lookup_new(zk_ctx* ctx /* NULL: host-only */, zk_field field, zk_repr repr, const zk_fe* table, uint32_t T,
                  zk_lookup** out);
void zk_lookup_free(zk_lookup* lk);
int zk_lookup_info(const zk_lookup* lk, uint32_t* out_T, uint32_t* out_nslots, uint8_t out_digest[32],
                   uint32_t* out_slots /* nslots */);
int zk_lookup_multiplicities(zk_lookup* lk, zk_repr repr, const zk_fe* f, uint64_t count, uint32_t n,
                             zk_fe* out_m /* 2^n */, uint64_t* out_missing);
int zk_dev_lookup_multiplicities(zk_lookup* lk, const void* d_f, uint64_t count, void* d_m /* 2^n */, uint32_t n,
                                 uint64_t* out_missing);
int zk_lookup_table_eval(zk_lookup* lk, zk_repr repr, const zk_fe* point /* n */, uint32_t n, zk_fe* out);
int zk_lookup_prove(zk_lookup* lk, zk_repr repr, const zk_fe* f /* 2^n */, uint32_t n, const zk_kzg* kzg,
                    const zk_g1* commitment_in /* NULL: compute it */, zk_transcript* transcript,
                    zk_fe* out_coeffs /* 4 n */, uint8_t* out_ncoeffs /* n */, zk_fe* out_table_evals /* 11 */,
                    zk_fe* out_point /* n */, zk_g1* out_commitments /* 4 */, zk_g1* out_opening /* n */,
                    uint64_t* out_missing);
int zk_dev_lookup_prove(zk_lookup* lk, zk_repr repr, const void* d_f, uint32_t n, const zk_kzg* kzg,
                        const zk_g1* commitment_in, zk_transcript* transcript, zk_fe* out_coeffs, uint8_t* out_ncoeffs,
                        zk_fe* out_table_evals, zk_fe* out_point, zk_g1* out_commitments, zk_g1* out_opening,
                        uint64_t* out_missing);
int zk_lookup_verify(zk_lookup* lk, zk_repr repr, uint32_t n, const zk_fe* coeffs, const uint8_t* ncoeffs,
                     const zk_fe* table_evals /* 11 */, const zk_g1* commitments /* 4 */, const zk_g1* opening /* n */,
                     const zk_g2* g2_taus, zk_transcript* transcript, int* out_verified, zk_fe* out_point /* n */);

/* ---------------------------------------------------------------------------
 * Proof blob: a canonical byte form of a proof, so a proof
 * produced on the CPU, on one GPU or on G GPUs can be compared as one digest
 * and shipped/verified elsewhere. The reference keeps proofs as in-memory
 * structs only (sum_check_protocol.rs:8-17); the blob holds exactly their
 * fields. All integers little-endian; field elements canonical 32-byte LE
 * (fq_vec_to_bytes, fiat_shamir_transcript.rs:32-37):
 *   [0,4)   "ZKSP"
 *   4       version = 1
 *   5       kind: ZK_BLOB_GKR (gkr_prove) or ZK_BLOB_SUMCHECK (prove)
 *   6       zk_field
 *   7       0
 *   [8,12)  nrounds (u32)
 *   [12,44) claimed_sum
 *   then per round: m (u8), m elements. For ZK_BLOB_GKR, m <= 3 is the trimmed
 *   coefficient count and the m elements are exactly the bytes the transcript
 *   absorbs that round; for ZK_BLOB_SUMCHECK they are the round's [s0, s1].
 * Parsing rejects (ZK_EINVAL) a bad magic/version/kind/field, truncation,
 * trailing bytes, m > 3 in a GKR blob, and elements >= p.
 * Serialisers return the size in *out_len; pass out = NULL to query it.
 * ------------------------------------------------------------------------- */
enum { ZK_BLOB_GKR = 1, ZK_BLOB_SUMCHECK = 2 };
int zk_gkr_proof_to_blob(zk_field field, zk_repr repr, const zk_fe* coeffs /* 3*nrounds */, const uint8_t* ncoeffs,
                         uint32_t nrounds, const zk_fe* claimed_sum, uint8_t* out, size_t cap, size_t* out_len);
int zk_sumcheck_proof_to_blob(zk_field field, zk_repr repr, const zk_fe* round_polys /* nrounds*poly_len */,
                              uint32_t nrounds, uint32_t poly_len, const zk_fe* claimed_sum, uint8_t* out,
                              size_t cap, size_t* out_len);
int zk_proof_blob_info(const uint8_t* blob, size_t len, int* out_kind, zk_field* out_field, uint32_t* out_nrounds);
int zk_gkr_proof_from_blob(const uint8_t* blob, size_t len, zk_repr repr, zk_fe* out_coeffs /* 3*cap_rounds */,
                           uint8_t* out_ncoeffs /* cap_rounds */, uint32_t cap_rounds, zk_fe* out_claimed_sum);
int zk_sumcheck_proof_from_blob(const uint8_t* blob, size_t len, zk_repr repr, zk_fe* out_round_polys,
                                size_t cap_elems, uint32_t* out_poly_len, zk_fe* out_claimed_sum);
/* gkr_verify of a GKR blob (claimed sum taken from the blob); outputs canonical. */
int zk_gkr_verify_blob(const uint8_t* blob, size_t len, zk_transcript* transcript, int* out_verified,
                       zk_fe* out_final_claimed_sum, zk_fe* out_challenges /* cap_rounds */, uint32_t cap_rounds);
/* Keccak-256 (the transcript's sponge: rate 136, pad 0x01..0x80) of a byte string */
int zk_keccak256(const uint8_t* data, size_t len, uint8_t out[32]);

/* ---------------------------------------------------------------------------
 * Device-resident API (tables already in HBM, Montgomery form)
 * ------------------------------------------------------------------------- */
int zk_dev_alloc(zk_ctx* ctx, size_t bytes, void** out);
int zk_dev_free(zk_ctx* ctx, void* p);
/* host (repr) -> device Montgomery, and back */
int zk_dev_upload(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* host, size_t n, void* dev);
int zk_dev_download(zk_ctx* ctx, zk_field field, zk_repr repr, const void* dev, size_t n, zk_fe* host);
/* synthetic table: dev[m] = synth(seed, table, index0 + m*stride) in Montgomery form */
int zk_dev_synth_fill(zk_ctx* ctx, zk_field field, void* dev, uint64_t count, uint64_t seed, uint32_t table,
                      uint64_t index0, uint64_t stride);
/* partial_evaluate on device buffers: d_out has 2^(nvars-1) elements (may not alias d_in) */
int zk_dev_mle_partial_evaluate(zk_ctx* ctx, zk_field field, const void* d_in, uint32_t nvars, uint32_t bit,
                                zk_repr repr, const zk_fe* value, void* d_out);
/* tensor_add_mul_polynomials on device buffers (Montgomery): d_out[i nb + j] = op(d_a[i], d_b[j]);
 * the GKR-shaped S = w (+) w and P = w (x) w tables built in HBM (d_out may not alias an input) */
int zk_dev_mle_tensor(zk_ctx* ctx, zk_field field, zk_mle_op op, const void* d_a, uint64_t na, const void* d_b,
                      uint64_t nb, void* d_out);
/* gkr_prove over device tables (read-only; the ctx workspace holds the folds) */
int zk_dev_gkr_sumcheck_prove(zk_ctx* ctx, zk_field field, const void* const d_tables[4], uint32_t nvars,
                              zk_repr repr, const zk_fe* claimed_sum, zk_transcript* transcript,
                              zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges);

/* ---------------------------------------------------------------------------
 * Keccak Merkle tree over field elements — merkle_tree/src/merkle_tree.rs
 * (MerkleTree<F> :25-29). With LE32 the canonical 32-byte image:
 *   compute_hash(x) = from_le_bytes_mod_order(Keccak256(LE32(x)))            :201-206
 *   hash_pair(l, r) = from_le_bytes_mod_order(Keccak256(LE32(l) | LE32(r)))  :208-214
 * leaves has 2^depth entries, tree[level] has 2^(depth-1-level) nodes, tree[0]
 * holds the parents of the leaves, the root is tree[depth-1][0]. The whole
 * tree lives in device memory ((2^(depth+1) - 1) * 32 B, one allocation; a
 * failed allocation is ZK_EDEVICE) and every hash runs on the GPU.
 * Where the reference returns Err or would panic the call returns ZK_EINVAL and
 * writes nothing: depth = 0 (get_root_hash indexes depth - 1), too many
 * inputs, a leaf id >= 2^depth, data that does not match the leaf, and any
 * value >= p. A tree belongs to its context: free it before the context.
 *   zk_merkle_new      new :32-52 (n_inputs = 0: all leaves the element 0, not
 *                      hashed) / new_with_inputs :54-82 (leaves[i] =
 *                      compute_hash(inputs[i]), the rest 0)
 *   zk_dev_merkle_new  new_with_inputs over a table already on the device
 *                      (Montgomery elements, as zk_dev_upload leaves them)
 *   zk_merkle_root     get_root_hash :134-136
 *   zk_merkle_download the leaves (level = -1) or tree[level] (0 .. depth-1)
 *   zk_merkle_update_leaves  update_leaf :84-104 for n leaves at once (is_hash[i]
 *                      != 0: the leaf becomes data[i], else compute_hash(data[i]));
 *                      every path is recomputed :106-132. The reference is
 *                      sequential, so ids must be distinct (else ZK_EINVAL)
 *   zk_merkle_create_proofs  create_proof :138-183 for n leaves, all or nothing:
 *                      out_siblings[i*depth + level] / out_sides[i*depth + level]
 *                      from the leaf level upward; side 0 = LeafSide::Left,
 *                      1 = Right (Right when the running index is even :165-169)
 * Host only (no context), as zk_gkr_sumcheck_verify:
 *   zk_merkle_hash_leaf / zk_merkle_hash_pair   compute_hash / hash_pair
 *   zk_merkle_verify_proof  verify :185-199 against a given root: folds
 *                      compute_hash(data) with the len entries; *out_ok = 1 / 0.
 *                      As in the reference, len is not checked against a depth;
 *                      a side other than 0 / 1 is ZK_EINVAL
 * ------------------------------------------------------------------------- */
typedef struct zk_merkle zk_merkle;
int zk_merkle_new(zk_ctx* ctx, zk_field field, uint32_t depth, zk_repr repr, const zk_fe* inputs, uint64_t n_inputs,
                  zk_merkle** out);
int zk_dev_merkle_new(zk_ctx* ctx, zk_field field, uint32_t depth, const void* dev_inputs, uint64_t n_inputs,
                      zk_merkle** out);
void zk_merkle_free(zk_merkle* tree);
int zk_merkle_root(zk_merkle* tree, zk_repr repr, zk_fe* out);
int zk_merkle_download(zk_merkle* tree, int level, zk_repr repr, zk_fe* out);
int zk_merkle_update_leaves(zk_merkle* tree, zk_repr repr, const uint64_t* ids, const zk_fe* data,
                            const uint8_t* is_hash, size_t n);
int zk_merkle_create_proofs(zk_merkle* tree, zk_repr repr, const zk_fe* data, const uint64_t* ids, size_t n,
                            zk_fe* out_siblings /* n*depth */, uint8_t* out_sides /* n*depth */);
int zk_merkle_hash_leaf(zk_field field, zk_repr repr, const zk_fe* x, zk_fe* out);
int zk_merkle_hash_pair(zk_field field, zk_repr repr, const zk_fe* left, const zk_fe* right, zk_fe* out);
int zk_merkle_verify_proof(zk_field field, zk_repr repr, const zk_fe* root, const zk_fe* data, const zk_fe* siblings,
                           const uint8_t* sides, size_t len, int* out_ok);

/* ---------------------------------------------------------------------------
 * FFT — fft/src/fft.rs: the radix-2 number-theoretic transform over a scalar
 * field and the polynomial product built on it. With w = F::get_root_of_unity(n)
 *   evaluate     y[k] = sum_j c[j] w^(jk)                       (dft :6-29, :31-41)
 *   interpolate  c[j] = n^-1 sum_k y[k] w^(-jk), all n of them, untrimmed  (:43-60)
 * both in natural order on both sides. The result is an exact field element, so
 * it equals the reference's bit for bit whatever the algorithm; here every
 * butterfly runs on the GPU, in ceil(log2 n / 8) passes over the table.
 * The root is defined for n a power of two up to 2^s, s the field's
 * two-adicity (BN254 Fr 28, BLS12-381 Fr 32, BN254 Fq 1): F::TWO_ADIC_ROOT_OF_UNITY
 * squared s - log2 n times. (ark's get_root_of_unity also knows 3 2^k and
 * 9 2^k through a small subgroup; fft.rs panics on those lengths before it
 * asks, so they are ZK_EINVAL here.)
 * ZK_EINVAL, where the reference panics: n = 0 or not a power of two, log2 n
 * above the two-adicity, a value >= p, a null pointer. ZK_EUNSUPPORTED: log2 n
 * > 28 (a 2^28 table is 8 GiB). Sizes above 2^24 (2^23-term operands for the
 * product) have not been measured or tested.
 *   zk_fft_root_of_unity        F::get_root_of_unity(n) (host)
 *   zk_fft_interpolation_roots  get_interpolation_roots :70-78 (host): the
 *                      reference's GeneralEvaluationDomain::new(n) rounds n up to
 *                      N = next_power_of_two(n); out[k] = w_N^(-k) N^-1, k < n, for
 *                      any n >= 1. ZK_EINVAL when N exceeds the two-adicity or 2^28
 *   zk_fft_evaluate    fft_evaluate :31-41
 *   zk_fft_interpolate fft_interpolate :43-60
 *   zk_dev_fft         the same transform (inverse != 0: interpolate) over a
 *                      table already on the device (Montgomery elements, as
 *                      zk_dev_upload leaves them). d_in is only read; d_out is
 *                      d_in itself or does not overlap it (else ZK_EINVAL)
 *   zk_poly_mul        impl Mul, univariate_polynomial_dense.rs:95-109: both
 *                      operands trimmed of trailing zeros as degree() does (:28-32;
 *                      a zero polynomial is ZK_EINVAL, its len() - 1 underflow);
 *                      *out_len = deg a + deg b + 1 values to out (cap < *out_len:
 *                      ZK_EINVAL with *out_len set). Computed as two forward
 *                      transforms of N = next_power_of_two(*out_len) points, a
 *                      pointwise product and one inverse, all on the device; an N
 *                      above the two-adicity or 2^28 is ZK_EUNSUPPORTED (BN254 Fq:
 *                      every product longer than 2)
 * ------------------------------------------------------------------------- */
int zk_fft_root_of_unity(zk_field field, zk_repr repr, uint64_t n, zk_fe* out);
int zk_fft_interpolation_roots(zk_field field, zk_repr repr, uint64_t n, zk_fe* out /* n */);
int zk_fft_evaluate(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* coeffs, uint64_t n, zk_fe* out /* n */);
int zk_fft_interpolate(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* evals, uint64_t n, zk_fe* out /* n */);
int zk_dev_fft(zk_ctx* ctx, zk_field field, const void* d_in, uint64_t n, int inverse, void* d_out);
int zk_poly_mul(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* a, uint64_t na, const zk_fe* b, uint64_t nb,
                zk_fe* out, uint64_t cap, uint64_t* out_len);

/* ---------------------------------------------------------------------------
 * Univariate polynomials over arbitrary points —
 * univariate_polynomial_dense.rs evaluate :20-26 and interpolate :48-74, which
 * are also all the arithmetic of the shamir_secret_sharing crate. Any field;
 * no evaluation domain is involved. Results are exact field elements: the
 * interpolant of n points with distinct x is unique, so it is bit-identical to
 * the reference's loop, trailing zeros trimmed (:71).
 *   zk_poly_evaluate      out[i] = sum_k coeffs[k] xs[i]^k, i < npoints, host
 *                         memory in and out. ncoeffs = 0: 0 everywhere (the
 *                         empty sum); npoints = 0: a successful no-op
 *   zk_dev_poly_evaluate  the same over device tables (Montgomery elements, as
 *                         zk_dev_upload leaves them); nothing crosses the host
 *                         boundary. out_tbl may be xs_tbl itself; any other
 *                         overlap with an input is ZK_EINVAL
 *   zk_poly_eval_plan     how an evaluation of that shape runs on this
 *                         context's device: *out_chunks runs of *out_chunk_len
 *                         coefficients each (1: one kernel; more: per-run cells
 *                         and a combining kernel). Host only
 *   zk_poly_interpolate   the polynomial of degree < n through (xs[i], ys[i]):
 *                         *out_ncoeffs <= n trimmed coefficients to out_coeffs
 *                         (n = 0: none; every y = 0: none). cap < n: ZK_EINVAL
 * ZK_EINVAL: a null buffer, an unknown field or representation, a value >= p,
 * two points with the same x (the reference divides by zero, :62-64).
 * ZK_EUNSUPPORTED: interpolation of more than 2^16 points (about 2.5 n^2 field
 * products: 10^10 at the cap); evaluation with more than 2^28 coefficients or
 * points, or npoints x ncoeffs above 2^40 (about ten seconds of products at
 * the measured 116 G/s). Sizes, field and representation are checked before
 * the context, the context before any value is read.
 * Calls with at most ZK_POLY_HOST_MAX points (read at zk_ctx_create; default
 * 96; evaluations: npoints x ncoeffs up to its square) run on the host in the
 * same O(n^2) formulation; 0 sends every call to the device.
 * ------------------------------------------------------------------------- */
int zk_poly_evaluate(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* coeffs, uint64_t ncoeffs, const zk_fe* xs,
                     uint64_t npoints, zk_fe* out /* npoints */);
int zk_dev_poly_evaluate(zk_ctx* ctx, zk_field field, const void* coeffs_tbl, uint64_t ncoeffs, const void* xs_tbl,
                         uint64_t npoints, void* out_tbl);
int zk_poly_eval_plan(const zk_ctx* ctx, uint64_t ncoeffs, uint64_t npoints, uint32_t* out_chunks, uint64_t* out_chunk_len);
int zk_poly_interpolate(zk_ctx* ctx, zk_field field, zk_repr repr, const zk_fe* xs, const zk_fe* ys, uint64_t n,
                        zk_fe* out_coeffs, uint64_t cap, uint64_t* out_ncoeffs);

/* ---------------------------------------------------------------------------
 * Multi-GPU: the hypercube is split over `world` ranks (one process or thread
 * per GPU, world a power of two). Rank g holds the sub-cube whose LOW
 * log2(world) index bits equal g: local m <-> global m*world + g. The first
 * nvars_local rounds fold purely locally; each round's partial sums are
 * combined with ONE all-reduce of at most 24 u64 (three elements split into
 * 32-bit limbs, so the u64 sum is exact); a last all-reduce of one-hot slots
 * gathers the 4 remaining elements of every rank so all ranks finish the last
 * log2(world) rounds identically. All-reduce (SUM, u64) is the only collective.
 * No broadcast is needed: every rank derives the same challenges from the
 * same transcript.
 * ------------------------------------------------------------------------- */
/* host-memory all-reduce supplied by the caller (e.g. torch.distributed/gloo).
 * With a host callback attached every step launches after its challenge
 * (pre-enqueue off): the callback's latency is unbounded and ranks may share
 * one device. */
typedef int (*zk_allreduce_u64_fn)(void* user, uint64_t* data, size_t count); /* in-place SUM, 0 = ok */
int zk_ctx_attach_host_comm(zk_ctx* ctx, int rank, int world, zk_allreduce_u64_fn allreduce, void* user);
/* RCCL over xGMI: rank 0 creates the id, every rank passes the same 128 bytes */
int zk_comm_get_unique_id(uint8_t out[128]);
int zk_ctx_attach_rccl(zk_ctx* ctx, int rank, int world, const uint8_t unique_id[128]);
int zk_ctx_detach_comm(zk_ctx* ctx);
/* The communicator the ctx holds: *out_kind = 0 none, 1 host callback, 2 RCCL;
 * *out_rank / *out_count = this rank and the number of ranks — for RCCL as the
 * communicator reports them (ncclCommUserRank / ncclCommCount), else the
 * attached rank / world (0 / 1 with none). */
int zk_ctx_comm_count(const zk_ctx* ctx, int* out_kind, int* out_rank, int* out_count);
/* Peer reduction (collective: every rank calls it, after attaching a
 * communicator; world <= 8, the ranks of one node). enable = 1: each rank
 * allocates an uncached receive buffer, the IPC handles are exchanged through
 * the attached communicator and opened, and one reduction of known values is
 * checked across the world. From then on each sharded step's sums are
 * summed by the step kernel itself — its publishing block writes them into
 * every rank's buffer and waits for the others' (replacing the step's
 * all-reduce of sum_check_protocol.rs:96-108's round sums; the early gather of
 * <= 4 x 2^12 elements per rank goes through a second such buffer).
 * enable = 0 releases it, as does attaching a communicator again. Proofs must
 * then run in the same order on every rank (the reductions carry a shared
 * sequence number); a proof that fails mid-way leaves the sequence unusable
 * until the next attach.
 * *out_ok (may be null) = 1 when enabled and the check passed. */
int zk_ctx_attach_peer_reduce(zk_ctx* ctx, int enable, int* out_ok);
/* gkr_prove over the global (nvars_local + log2(world))-variable SumPoly whose
 * local shard this rank holds; outputs are the global proof (identical on all
 * ranks). out arrays sized for nvars_local + log2(world) rounds. */
int zk_dev_gkr_sumcheck_prove_sharded(zk_ctx* ctx, zk_field field, const void* const d_local_tables[4],
                                      uint32_t nvars_local, zk_repr repr, const zk_fe* claimed_sum,
                                      zk_transcript* transcript, zk_fe* out_coeffs, uint8_t* out_ncoeffs,
                                      zk_fe* out_challenges);

#ifdef __cplusplus
}
#endif
#endif /* ZK_SUMCHECK_H */
