/*
 * rabe_hip.h -- C ABI of the MI355X (gfx950) batched ABE pairing / scalar-multiplication engine.
 *
 * This is the drop-in boundary for the hot path of Fraunhofer-AISEC/rabe: the per-attribute loops of
 * rabe::schemes::{ac17,bsw,lsw,aw11}::{keygen,encrypt,decrypt}.  In the reference all of that math
 * enters through `use rabe_bn::{Group, Gt, G1, G2, Fr, pairing}` (src/schemes/ac17/mod.rs:42,
 * bsw/mod.rs:23, lsw/mod.rs:23, aw11/mod.rs:27); a Rust host keeps policy parsing, MSP, pruning, KDF
 * and AES and binds these symbols over FFI (INTEGRATION.md shows the `extern "C"` block).
 * The convention follows the reference's own (stale) C FFI, src/ffi/bsw.rs:22-163: opaque context
 * pointers created/destroyed by paired functions, int32 status (0 ok, <0 error).
 *
 * Two levels:
 *   Level E  element batches -- `rabe_bn` operator semantics on arrays (n independent operations),
 *            used for parity against the oracle and for a `rabe-bn`-shaped shim.
 *   Level B  scheme batches -- whole encrypt / keygen / decrypt group-arithmetic of n independent calls.
 *
 * Wire format (all little-endian, canonical = fully reduced, NOT Montgomery):
 *   rhip_fr  32 B   integer < r
 *   rhip_g1  64 B   affine x || y, each an integer < p; the point at infinity is all-zero
 *   rhip_g2 128 B   affine x.c0 || x.c1 || y.c0 || y.c1  (Fq2 = c0 + c1*u); infinity all-zero
 *   rhip_gt 384 B   12 integers < p in tower order c0.a0.c0, c0.a0.c1, c0.a1.c0, ... c1.a2.c1
 *                   (Fq12 = c0 + c1*w, Fq6 = a0 + a1*v + a2*v^2, Fq2 = c0 + c1*u)
 * Every `dev` pointer below is DEVICE memory (hipMalloc / rhip_malloc / a torch CUDA tensor);
 * the call is asynchronous on the context's stream; rhip_sync() waits.
 */
#ifndef RABE_HIP_H
#define RABE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint32_t l[8]; } rhip_fr;
typedef struct { uint32_t l[16]; } rhip_g1;
typedef struct { uint32_t l[32]; } rhip_g2;
typedef struct { uint32_t l[96]; } rhip_gt;

typedef struct rhip_ctx rhip_ctx;

#define RHIP_OK 0
#define RHIP_ERR_NO_DEVICE (-1)   /* no HIP device / kernels not loadable: the engine never falls back to the CPU */
#define RHIP_ERR_HIP (-2)         /* a HIP runtime call failed; see rhip_last_error */
#define RHIP_ERR_ARG (-3)
#define RHIP_ERR_NOT_MEMBER (-4)  /* an input point is not on the curve (rabe_bn::FieldError::NotMember, src/error.rs:60-69) */

/* ---- context (one per host thread / per GPU; single owner) ------------------------------------ */
/* The first context of a device runs a known-answer self-test of the BN254 field / tower arithmetic on every SIMD (adversarial
 * carry patterns through every multiply-accumulate and carry-chain form; ~1 ms; bn254/selftest.h) and refuses the device
 * (RHIP_ERR_HIP, message in rhip_last_error(NULL)) on any mismatch.  RABE_NO_SELFTEST=1 skips it. */
int32_t rhip_ctx_create(int32_t device, rhip_ctx** out);
/* number of distinct SIMDs the self-test of this context's device ran on (diagnostic) */
int32_t rhip_ctx_selftest_info(rhip_ctx* ctx, uint32_t* simds_checked);
void rhip_ctx_destroy(rhip_ctx* ctx);
/* use an existing hipStream_t (e.g. torch's current stream); NULL = the context's own stream */
int32_t rhip_ctx_set_stream(rhip_ctx* ctx, void* hip_stream);
/* make the context's device the calling thread's current HIP device (a host thread that serves several contexts / devices) */
int32_t rhip_ctx_make_current(rhip_ctx* ctx);
int32_t rhip_sync(rhip_ctx* ctx);
const char* rhip_last_error(rhip_ctx* ctx);
/* per-kernel timing with HIP events on the launch stream (measurement only; off by default).
 * rhip_ctx_timing_read drains the record as "kernel_name total_ms launches\n" lines. */
int32_t rhip_ctx_timing(rhip_ctx* ctx, int32_t enable);
int32_t rhip_ctx_timing_read(rhip_ctx* ctx, char* buf, size_t len);
/* pairing kernels: 0 = auto (cooperating lanes for launches that would under-fill the chip, one lane per item and chunk
 * otherwise), 1 = always one lane, 3 = three lanes per pairing (pairwise paths), 6 = six lanes per Fq12 accumulator
 * (k_miller_c6 / k_final_exp_c6: one Fq2 coefficient per lane), 29 = one lane per item and chunk on the reduced-radix field core
 * (k_miller_multi_rr: 9 x 29-bit limbs; what mode 0 takes for launches that fill the chip).  Results are identical.
 * 99 = cross-check: every multi-pairing launch runs as mode 0 would run it (the caller gets that result) and again with modes 1, 6 and 29
 * forced -- Miller loops and final exponentiation of each family on the same pair lists -- and the results are compared on the device; a
 * difference fails the call (RHIP_ERR_HIP, the families named in rhip_last_error).  Synchronous and about four times the pairing work: a
 * self-check for tests and suspect devices, not a production mode.
 * RABE_PAIRING_MODE in the environment of rhip_ctx_create presets the mode (A/B runs). */
int32_t rhip_ctx_set_pairing_mode(rhip_ctx* ctx, int32_t mode);
/* number of compute units / device name of the context's GPU */
int32_t rhip_device_info(rhip_ctx* ctx, int32_t* n_cu, char* name, size_t name_len);

/* device memory helpers for hosts without their own allocator */
int32_t rhip_malloc(rhip_ctx* ctx, size_t bytes, void** dev);
int32_t rhip_free(rhip_ctx* ctx, void* dev);
int32_t rhip_upload(rhip_ctx* ctx, void* dev, const void* host, size_t bytes);
int32_t rhip_download(rhip_ctx* ctx, void* host, const void* dev, size_t bytes);
/* Pinned host memory and copies that are only ordered on the context's stream (rhip_sync waits for them): a caller with
 * several contexts overlaps the PCIe traffic of one batch with the kernels of the others. */
int32_t rhip_host_alloc(rhip_ctx* ctx, size_t bytes, void** host);
int32_t rhip_host_free(rhip_ctx* ctx, void* host);
int32_t rhip_upload_async(rhip_ctx* ctx, void* dev, const void* host_pinned, size_t bytes);
int32_t rhip_download_async(rhip_ctx* ctx, void* host_pinned, const void* dev, size_t bytes);
/* stream-ordered fill (the host layer wipes staging areas that held master-key-derived scalars) */
int32_t rhip_memset_async(rhip_ctx* ctx, void* dev, int32_t byte, size_t bytes);
/* cross-context ordering without a host round trip: work submitted to `ctx` after this call starts only when everything
 * submitted to `other` so far has finished (event record + stream wait): e.g. a copy context that drains one batch's
 * outputs while the compute context already runs the next kernels */
int32_t rhip_ctx_wait_for(rhip_ctx* ctx, rhip_ctx* other);
/* a point of a context's stream that a HOST thread can wait for without waiting for the stream's later work (rhip_event_wait blocks until
 * everything submitted to ctx before rhip_event_record has finished, and frees the event) */
typedef struct rhip_event rhip_event;
int32_t rhip_event_record(rhip_ctx* ctx, rhip_event** out);
int32_t rhip_event_wait(rhip_event* ev);
/* Pipelining two launch sets on two contexts (streams): `waiter`'s stream is held until ctx's NEXT decrypt (any entry point that runs
 * the shared-accumulator Miller kernel) has issued its Miller loops; what is left on ctx then is its final exponentiation (one wave per
 * item), beside which the waiter's encrypt kernels can run.  One-shot.  Typical use: a small launch set on ctx, the next large one on
 * waiter -- submit ctx first, then enqueue waiter's work; make waiter's decrypt wait for all of ctx with rhip_ctx_wait_for.  The request
 * is consumed by ctx's next final-exponentiation launch; waiter = NULL withdraws a pending one (a context must not be destroyed while
 * it is a pending waiter).  The hold is bounded: the waiter's stream polls for at most a few tens of milliseconds. */
int32_t rhip_ctx_release_before_final_exp(rhip_ctx* ctx, rhip_ctx* waiter);
/* The same hold, released as soon as ctx's Miller loops are DONE (no wait for the final exponentiation's blocks to be resident): for a
 * waiter with little work of its own -- the Gt membership checks of a packed decrypt run beside the final exponentiation this way. */
int32_t rhip_ctx_release_after_miller(rhip_ctx* ctx, rhip_ctx* waiter);
/* The hold for a SMALL launch set on ctx beside the waiter's large one: the waiter's stream goes on as soon as the blocks of ctx's next Miller
 * launch are RESIDENT -- they own their CUs, the waiter's encrypt kernels take the CUs that are left -- instead of when that launch is done.
 * Served by the reduced-radix Miller kernel on uniform pair lists (pairing mode 0 / 29); any other launch behaves as under
 * rhip_ctx_release_before_final_exp.  One-shot; same bytes either way. */
int32_t rhip_ctx_release_when_miller_resident(rhip_ctx* ctx, rhip_ctx* waiter);

/* ---- Level E: element batches (n independent operations) --------------------------------------
 * rabe_bn surface replaced ("rabe_bn API surface actually used"):
 *   Fr: + - * neg inverse            src/utils/secretsharing/mod.rs:25-28,66,218; ac17/mod.rs:213,229,240
 *   Fr::from_slice(SHA3 digest)      src/utils/hash/mod.rs:16,27
 *   G1/G2: + - neg, * Fr             ac17/mod.rs:219,235-240,300-302,343-348,406-415
 *   Gt: * inverse pow                ac17/mod.rs:357-360,418; bsw/mod.rs:234,291-294,308
 *   pairing(G1,G2)                   ac17/mod.rs:148,415-416; bsw/mod.rs:108,292-293,308
 * Scalars (rhip_fr operands of * Fr, pow, the MSM / selection coefficients of Level B) are canonical records (< r).  A record
 * that is not is brought below r where it is loaded, so `k * P` is the group's answer for every 256-bit word; nothing relies on
 * the caller having checked.  Group elements are NOT validated by the arithmetic entry points: rhip_g1_on_curve /
 * rhip_g2_in_subgroup / rhip_gt_is_member (which also reject non-canonical coordinates >= p) are the decoding checks.
 */
/* RHIP_FR_POW: out = a^b with b read as an integer (`Fr::pow(Fr)`, src/utils/secretsharing/mod.rs:218) */
enum { RHIP_FR_ADD = 0, RHIP_FR_SUB = 1, RHIP_FR_MUL = 2, RHIP_FR_NEG = 3, RHIP_FR_INV = 4, RHIP_FR_POW = 5 };
int32_t rhip_fr_op(rhip_ctx* ctx, int32_t op, size_t n, const rhip_fr* dev_a, const rhip_fr* dev_b, rhip_fr* dev_out);
/* `Fr::from_slice` of n 32-byte BIG-endian digests: integer mod r */
int32_t rhip_fr_from_be32_reduce(rhip_ctx* ctx, size_t n, const uint8_t* dev_digests, rhip_fr* dev_out);
/* Diagnostic: out[i] = a0[i] b0[i] + a1[i] b1[i] in the BASE field (canonical 32-byte records < p, the coordinate encoding of rhip_g1),
 * through the two-term dot product under one reduction that closes the G1 mixed addition (bn254/fp.h: mont_dot2_raw). */
int32_t rhip_fp_dot2(rhip_ctx* ctx, size_t n, const rhip_fr* dev_a0, const rhip_fr* dev_b0, const rhip_fr* dev_a1, const rhip_fr* dev_b1,
                     rhip_fr* dev_out);

int32_t rhip_g1_add(rhip_ctx* ctx, size_t n, const rhip_g1* dev_a, const rhip_g1* dev_b, rhip_g1* dev_out);
int32_t rhip_g1_neg(rhip_ctx* ctx, size_t n, const rhip_g1* dev_a, rhip_g1* dev_out);
int32_t rhip_g1_mul(rhip_ctx* ctx, size_t n, const rhip_g1* dev_p, const rhip_fr* dev_k, rhip_g1* dev_out);
int32_t rhip_g2_add(rhip_ctx* ctx, size_t n, const rhip_g2* dev_a, const rhip_g2* dev_b, rhip_g2* dev_out);
int32_t rhip_g2_neg(rhip_ctx* ctx, size_t n, const rhip_g2* dev_a, rhip_g2* dev_out);
int32_t rhip_g2_mul(rhip_ctx* ctx, size_t n, const rhip_g2* dev_p, const rhip_fr* dev_k, rhip_g2* dev_out);
/* Variable-base G2 multiplication of rows that share scalars: out[t] = k[i] * p[t] for the rows t in [item_row_off[i], item_row_off[i+1])
 * of item i (n_items + 1 non-decreasing offsets, item_row_off[0] = 0, item_row_off[n_items] = n_rows; an item may own no row).  What
 * ghw11::tkgen does to a key (every element times z^-1, src/schemes/ghw11/mod.rs:156-178), for n_items keys in one launch set.  The scalar
 * is split four ways over the twist endomorphism once per item (k = k0 + k1 L + k2 L^2 + k3 L^3 mod r, L = p mod r, |k_i| < 2^65) and
 * every row runs one joint chain of ~66 doublings (bn254/gls4.h) instead of rhip_g2_mul's 254.  Any 256-bit scalar word is accepted (0
 * and multiples of r give infinity); infinity in, infinity out.  The points must be members of G2 (rhip_g2_in_subgroup): for a twist
 * point outside the r-torsion the result is NOT k * p -- rhip_g2_mul is the entry point for those. */
int32_t rhip_g2_mul_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_g2* dev_p /*[n_rows]*/,
                         size_t n_items, const rhip_fr* dev_k /*[n_items]*/, rhip_g2* dev_out /*[n_rows]*/);
/* The same with a row index on both sides: out[row_dst[t]] = k[i] * p[row_src[t]].  A caller whose rows are ordered by scalar keeps each
 * point once (row_src[t] < the number of points) and has the results written where its records want them (row_dst: a permutation of
 * [0, n_rows); nothing is checked).  rhip_g2_mul_rows itself is unchanged. */
int32_t rhip_g2_mul_rows_at(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_g2* dev_p,
                            const uint32_t* dev_row_src /*[n_rows]*/, size_t n_items, const rhip_fr* dev_k /*[n_items]*/,
                            const uint32_t* dev_row_dst /*[n_rows]*/, rhip_g2* dev_out /*[n_rows]*/);
/* Variable-base G1 multiplication of rows that share scalars, the shape of rhip_g2_mul_rows: out[t] = k[i] * p[t] for the rows t of item i.
 * What bdabe::request_attribute_sk / mke08::request_authority_sk do to a user's u1 (bdabe/mod.rs:275-305), one scalar per attribute against
 * many users.  The GLV decomposition k = k1 + k2 lambda and the NAF masks of both halves are made once per item (k_glv_masks); every row
 * runs one joint chain over P and phi(P) = (beta x, y) of ~130 doublings, and a block shares one field inversion (rhip_g1_mul: one
 * decomposition and one inversion per element).  Any 256-bit scalar word is accepted (0 and multiples of r give infinity); infinity in,
 * infinity out; the points must be on the curve.  Same bytes as rhip_g1_mul.  _at: out[row_dst[t]] = k[i] * p[row_src[t]], as above. */
int32_t rhip_g1_mul_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_g1* dev_p /*[n_rows]*/,
                         size_t n_items, const rhip_fr* dev_k /*[n_items]*/, rhip_g1* dev_out /*[n_rows]*/);
int32_t rhip_g1_mul_rows_at(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_g1* dev_p,
                            const uint32_t* dev_row_src /*[n_rows]*/, size_t n_items, const rhip_fr* dev_k /*[n_items]*/,
                            const uint32_t* dev_row_dst /*[n_rows]*/, rhip_g1* dev_out /*[n_rows]*/);
/* the split alone, on the host (no GPU, no context; the code the kernel runs): mag[4 i .. 4 i + 4) = |k_i| as little-endian words,
 * neg[i] = 1 for a negative k_i */
int32_t rhip_host_fr_split4(const rhip_fr* k, uint32_t mag[16], uint8_t neg[4]);
/* per-element curve membership: dev_ok[i] = 1 if on the curve (or infinity) */
int32_t rhip_g1_on_curve(rhip_ctx* ctx, size_t n, const rhip_g1* dev_p, uint32_t* dev_ok);
int32_t rhip_g2_on_curve(rhip_ctx* ctx, size_t n, const rhip_g2* dev_p, uint32_t* dev_ok);
/* membership in the groups proper (what decoding an untrusted element has to establish; G1 has cofactor 1, so on-curve suffices
 * there): G2 = the r-torsion of the twist (on the curve and r * P = O), Gt = the order-r subgroup of Fq12* */
int32_t rhip_g2_in_subgroup(rhip_ctx* ctx, size_t n, const rhip_g2* dev_p, uint32_t* dev_ok);
/* the same verdicts by the definition r * Q = O (rhip_g2_in_subgroup uses the BN-specific test [u+1]Q + psi([u]Q) + psi^2([u]Q) =
 * psi^3([2u]Q): one multiplication by the 63-bit curve parameter instead of the 254-bit order) -- kept for cross-checks */
int32_t rhip_g2_in_subgroup_by_order(rhip_ctx* ctx, size_t n, const rhip_g2* dev_p, uint32_t* dev_ok);
/* rhip_g2_in_subgroup of the listed elements only: dev_ok[k] = the verdict of dev_p[dev_idx[k]], k < n_idx */
int32_t rhip_g2_in_subgroup_at(rhip_ctx* ctx, size_t n_idx, const uint32_t* dev_idx, const rhip_g2* dev_p, uint32_t* dev_ok);
/* G2 membership as a by-product of a decrypt's Miller loops.  One-shot: the NEXT pair-list decrypt on this context (the shared-
 * accumulator paths of rhip_{ac17_cp,bsw,lsw,aw11}_decrypt_batch*, rhip_pairing_jobs) examines every G2 argument it WALKS -- the
 * untrusted side of a decrypt: c_0 (ac17), Cy.g2 (bsw), D2 (lsw), C2 (aw11) of the selected rows -- after its Miller loops:
 * the running point then holds [6u+2]Q + psi(Q) - psi^2(Q), which is -psi^3(Q) exactly for the points of the twist that lie
 * in G2 (engine_jobs.hip: k_walk_verdicts has the argument).  dev_fail[i] becomes 1 if an argument of item i fails,
 * dev_count[i] grows by the number of arguments examined (a pair with an argument at infinity is skipped and not counted; a
 * launch that takes another path counts nothing): the caller zeroes both arrays, compares the counts with what it expected to
 * be examined and runs rhip_g2_in_subgroup(_at) on whatever was not.  Curve equation and coordinate range are not part of this
 * verdict (rhip_g2_on_curve).  NULL, NULL withdraws the request. */
int32_t rhip_ctx_collect_walk_verdicts(rhip_ctx* ctx, uint32_t* dev_fail, uint32_t* dev_count);
int32_t rhip_gt_is_member(rhip_ctx* ctx, size_t n, const rhip_gt* dev_a, uint32_t* dev_ok);
/* the same verdicts with the order test by the definition f^r = 1 (rhip_gt_is_member uses f^p = f^(6u^2) after the cyclotomic test) */
int32_t rhip_gt_is_member_by_order(rhip_ctx* ctx, size_t n, const rhip_gt* dev_a, uint32_t* dev_ok);
/* verdicts folded per item on the device: dev_out[s] = AND of dev_flags[scale * dev_seg_off[s] .. scale * dev_seg_off[s + 1]),
 * s < n_seg (dev_seg_off has n_seg + 1 entries: an item's rows; scale = elements per row) */
int32_t rhip_flags_all(rhip_ctx* ctx, size_t n_seg, const uint32_t* dev_seg_off, uint32_t scale, const uint32_t* dev_flags, uint32_t* dev_out);

int32_t rhip_gt_mul(rhip_ctx* ctx, size_t n, const rhip_gt* dev_a, const rhip_gt* dev_b, rhip_gt* dev_out);
/* out[i] = product of a[off[i] .. off[i+1]) (1 for an empty segment): the Gt accumulation loops of aw11::decrypt :320-352 */
int32_t rhip_gt_product(rhip_ctx* ctx, size_t n_items, const uint32_t* dev_off /*[n_items+1]*/, const rhip_gt* dev_a, rhip_gt* dev_out);
int32_t rhip_gt_inv(rhip_ctx* ctx, size_t n, const rhip_gt* dev_a, rhip_gt* dev_out);
int32_t rhip_gt_pow(rhip_ctx* ctx, size_t n, const rhip_gt* dev_a, const rhip_fr* dev_k, rhip_gt* dev_out);
/* Gt powers of rows that share exponents, the shape of rhip_g2_mul_rows: out[t] = (dev_mul ? mul[t] : 1) * a[t]^(+-k[i]) for the rows t in
 * [item_row_off[i], item_row_off[i+1]) of item i (n_items + 1 non-decreasing offsets, item_row_off[0] = 0, item_row_off[n_items] =
 * n_rows; an item may own no row); the sign is minus with RHIP_GT_POW_INVERT (an inverse in Gt is a conjugation: it costs nothing).
 * What a GHW11 client does with a transformed ciphertext (c * t^-z, src/schemes/ghw11/mod.rs decrypt_out), every record of a call under
 * the one z.  Frobenius is the power L = p mod r on Gt, so the exponent is split four ways once per item (k = k0 + k1 L + k2 L^2 +
 * k3 L^3 mod r, |k_i| < 2^65, the split of rhip_g2_mul_rows) and every row runs one joint chain of at most 66 cyclotomic squarings
 * (bn254/gtpow4.h) instead of rhip_gt_pow's 256.  Any 256-bit scalar word is accepted (0 and multiples of r give 1 -- times mul[t]).
 * The elements a[t] must be members of Gt (rhip_gt_is_member): for an element outside the order-r subgroup the result is NOT a^k --
 * rhip_gt_pow is the entry point for those; mul[t] may be any field element.  dev_out may be dev_a or dev_mul.  Same bytes as
 * rhip_gt_pow followed by rhip_gt_inv / rhip_gt_mul.  The per-item staging of the exponents is zeroed when the call's kernels are done. */
#define RHIP_GT_POW_INVERT 1u
int32_t rhip_gt_pow_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_gt* dev_a /*[n_rows]*/,
                         size_t n_items, const rhip_fr* dev_k /*[n_items]*/, const rhip_gt* dev_mul /*[n_rows] or NULL*/, uint32_t flags,
                         rhip_gt* dev_out /*[n_rows]*/);
/* Gt multi-exponentiation per item: out[i] = (dev_mul ? mul[i] : 1) * prod over the rows t in [item_row_off[i], item_row_off[i+1]) of
 * a[t]^(+-k[t]), minus with RHIP_GT_POW_INVERT; offsets as rhip_gt_pow_rows (an item without rows gives mul[i] or 1).  The shape of AW11's
 * leading factor c_0 * prod C1_e^(-c_e) (aw11/mod.rs:320-352).  Any 256-bit scalar word is accepted and brought below r where it is
 * loaded; zero and multiples of r give a factor of 1.  Every scalar is recoded on the device into width-4 signed odd digits (+-1, +-3, +-5,
 * +-7; 128 bytes of staging per scalar), every row gets the table a, a^3, a^5, a^7 in a work arena of the context (4 x 384 = 1536 bytes
 * per row), and lane (chunk, item) walks its chunk of at most C rows on ONE chain of cyclotomic squarings: a non-zero digit costs a table
 * load, a conjugation when it is negative and one multiplication (~51 per 254-bit scalar against ~85 over the plain NAF); a finish lane
 * per item multiplies the L partial products and mul[i].  chunk_terms = 0 lets the engine choose (L, C) from the compute-unit count and the
 * longest item; another value forces C.  The offsets are read back once for that (the call synchronises its stream).
 * The elements a[t] must be members of Gt (rhip_gt_is_member): the routine squares cyclotomically and inverts by conjugation, so for
 * anything else rhip_gt_pow + rhip_gt_product is the route; mul[i] may be any field element.  dev_out may be dev_mul.  Same bytes as
 * rhip_gt_pow -> (rhip_gt_inv) -> rhip_gt_product -> rhip_gt_mul.  The digit staging is zeroed when the call's kernels are done. */
int32_t rhip_gt_multiexp_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_gt* dev_a /*[n_rows]*/,
                              const rhip_fr* dev_k /*[n_rows]*/, size_t n_items, const rhip_gt* dev_mul /*[n_items] or NULL*/, uint32_t flags,
                              uint32_t chunk_terms /*0 = the engine's choice*/, rhip_gt* dev_out /*[n_items]*/);

/* n independent pairings e(p_i, q_i) */
int32_t rhip_pairing(rhip_ctx* ctx, size_t n, const rhip_g1* dev_p, const rhip_g2* dev_q, rhip_gt* dev_out);
/* n_items products of pairings: out[i] = prod_{j in [off[i], off[i+1])} e(p_j, q_j), with ONE final
 * exponentiation per item (the restructuring of SURVEY.md Appendix B).  dev_off has n_items+1 entries. */
int32_t rhip_pairing_product(rhip_ctx* ctx, size_t n_items, const uint32_t* dev_off, size_t n_pairs,
                             const rhip_g1* dev_p, const rhip_g2* dev_q, rhip_gt* dev_out);

/* The general form the decrypts of bsw / lsw / aw11 / ghw11 reduce to (coefficient-folded products of pairings):
 *   out[i] = lead[i] * FE( prod_{j in [pair_off[i], pair_off[i+1])} ML(scal[j] * base[j], q[j])  *  ML( sum_{t in [sum_off[i], sum_off[i+1])} s_scal[t] * s_base[t], s_q[i] ) )
 * in one launch set: the G1 arguments are scaled over the NAF of their coefficients (the shorter of c and r - c), the sum runs with
 * shared doublings, all pairs of an item share a few Fq12 accumulators, one final exponentiation per item.  dev_scal NULL: all 1;
 * dev_sum_off NULL: no summed pair (dev_s_* ignored); dev_lead NULL: no leading factor.  max_pairs / max_terms: the largest per-item
 * counts (they size the launch). */
int32_t rhip_pairing_jobs(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t n_pairs, const uint32_t* dev_pair_off /*[n_items+1]*/,
                          const rhip_g1* dev_base, const rhip_fr* dev_scal, const rhip_g2* dev_q, size_t max_terms, size_t n_terms,
                          const uint32_t* dev_sum_off /*[n_items+1] or NULL*/, const rhip_g1* dev_s_base, const rhip_fr* dev_s_scal,
                          const rhip_g2* dev_s_q /*[n_items]*/, const rhip_gt* dev_lead /*[n_items] or NULL*/, rhip_gt* dev_out /*[n_items]*/);

/* ---- Level E, host-value forms: ONE element per call, host pointers (upload, launch, download).  These are what an
 * operator-overloading replacement of the `rabe_bn` crate binds (`impl Mul<Fr> for G1`, `pairing(p, q)`, ...; see
 * INTEGRATION.md section 2 and integration/rabe-bn-shim/): whole-program parity runs of unmodified rabe, not throughput. */
int32_t rhip_host_fr_op(rhip_ctx* ctx, int32_t op, const rhip_fr* a, const rhip_fr* b /* NULL for NEG / INV */, rhip_fr* out);
int32_t rhip_host_fr_pow(rhip_ctx* ctx, const rhip_fr* a, const rhip_fr* e, rhip_fr* out);
int32_t rhip_host_fr_from_be32_reduce(rhip_ctx* ctx, const uint8_t digest[32], rhip_fr* out);
/* curve membership of a decoded point (what makes `FieldError::NotMember`, src/error.rs:66): *ok = 1 on the curve or infinity */
int32_t rhip_host_g1_on_curve(rhip_ctx* ctx, const rhip_g1* p, int32_t* ok);
int32_t rhip_host_g2_on_curve(rhip_ctx* ctx, const rhip_g2* p, int32_t* ok);
/* the full decoding checks of one element: canonical coordinates, on the twist and r * P = O / in the order-r subgroup of Fq12 */
int32_t rhip_host_g2_in_subgroup(rhip_ctx* ctx, const rhip_g2* p, int32_t* ok);
int32_t rhip_host_gt_is_member(rhip_ctx* ctx, const rhip_gt* a, int32_t* ok);
int32_t rhip_host_g1_add(rhip_ctx* ctx, const rhip_g1* a, const rhip_g1* b, rhip_g1* out);
int32_t rhip_host_g1_neg(rhip_ctx* ctx, const rhip_g1* a, rhip_g1* out);
int32_t rhip_host_g1_mul(rhip_ctx* ctx, const rhip_g1* p, const rhip_fr* k, rhip_g1* out);
int32_t rhip_host_g2_add(rhip_ctx* ctx, const rhip_g2* a, const rhip_g2* b, rhip_g2* out);
int32_t rhip_host_g2_neg(rhip_ctx* ctx, const rhip_g2* a, rhip_g2* out);
int32_t rhip_host_g2_mul(rhip_ctx* ctx, const rhip_g2* p, const rhip_fr* k, rhip_g2* out);
int32_t rhip_host_gt_mul(rhip_ctx* ctx, const rhip_gt* a, const rhip_gt* b, rhip_gt* out);
int32_t rhip_host_gt_inv(rhip_ctx* ctx, const rhip_gt* a, rhip_gt* out);
int32_t rhip_host_gt_pow(rhip_ctx* ctx, const rhip_gt* a, const rhip_fr* k, rhip_gt* out);
int32_t rhip_host_pairing(rhip_ctx* ctx, const rhip_g1* p, const rhip_g2* q, rhip_gt* out);

/* ---- fixed-base tables (per public key; resident in HBM) --------------------------------------
 * Every G1/G2 element the schemes create is a known-scalar multiple of a generator from the public
 * key (hash-to-group is g * Fr(SHA3(label)), src/utils/hash/mod.rs:10-20), and every Gt power is of a
 * public-key constant, so the engine keeps 8-bit window tables of those bases. */
typedef struct rhip_g1_table rhip_g1_table;
typedef struct rhip_g2_table rhip_g2_table;
typedef struct rhip_gt_table rhip_gt_table;
int32_t rhip_g1_table_create(rhip_ctx* ctx, const rhip_g1* host_base, rhip_g1_table** out);
int32_t rhip_g2_table_create(rhip_ctx* ctx, const rhip_g2* host_base, rhip_g2_table** out);
int32_t rhip_gt_table_create(rhip_ctx* ctx, const rhip_gt* host_base, rhip_gt_table** out);
/* adds 16-bit windows (16 x 65535 entries, 67 MB) to a G1 table: halves the additions of rhip_g1_table_mul-style
 * kernels; rhip_ac17_pk_create does this for the public generator g */
int32_t rhip_g1_table_add_w16(rhip_ctx* ctx, rhip_g1_table* t);
/* adds signed w_bits-wide windows (17 <= w_bits <= 27): a fixed-base multiplication then costs ceil(254 / w_bits)
 * mixed additions (11 at 24 bits, 10 at 26) for 64 B x 2^(w_bits-1) x ceil(254 / w_bits) of HBM (5.4 GB at 24 bits,
 * 19 GB at 26) -- memory traded for work on a 288 GB part.  Results are the same group elements, hence the same bytes. */
int32_t rhip_g1_table_add_wide(rhip_ctx* ctx, rhip_g1_table* t, int32_t w_bits);
/* the same for a G2 base (16 x 65535 x 128 B = 134 MB; rhip_ac17_pk_create does this for h_a[0..2]) */
int32_t rhip_g2_table_add_w16(rhip_ctx* ctx, rhip_g2_table* t);
/* the same for a Gt base (16 x 65535 x 384 B = 402 MB): halves the multiplications of a fixed-base Gt power */
int32_t rhip_gt_table_add_w16(rhip_ctx* ctx, rhip_gt_table* t);
void rhip_g1_table_destroy(rhip_g1_table* t);
void rhip_g2_table_destroy(rhip_g2_table* t);
void rhip_gt_table_destroy(rhip_gt_table* t);
/* out[i] = base * k[i]  /  base ^ k[i] */
int32_t rhip_g1_table_mul(rhip_ctx* ctx, const rhip_g1_table* t, size_t n, const rhip_fr* dev_k, rhip_g1* dev_out);
int32_t rhip_g2_table_mul(rhip_ctx* ctx, const rhip_g2_table* t, size_t n, const rhip_fr* dev_k, rhip_g2* dev_out);
int32_t rhip_gt_table_pow(rhip_ctx* ctx, const rhip_gt_table* t, size_t n, const rhip_fr* dev_k, rhip_gt* dev_out);

/* ---- Level B: AC17 (FAME) CP-ABE -------------------------------------------------------------- */
/* Public key side of ac17::cp_encrypt (Ac17PublicKey, src/schemes/ac17/mod.rs:62-66). */
typedef struct rhip_ac17_pk rhip_ac17_pk;
int32_t rhip_ac17_pk_create(rhip_ctx* ctx, const rhip_g1* host_g, const rhip_g2* host_h_a /*[3]*/,
                            const rhip_gt* host_e_gh_ka /*[2]*/, rhip_ac17_pk** out);
/* switches the public generator's table of pk to signed w_bits-wide windows (rhip_g1_table_add_wide) */
int32_t rhip_ac17_pk_set_g_window(rhip_ctx* ctx, rhip_ac17_pk* pk, int32_t w_bits);
void rhip_ac17_pk_destroy(rhip_ac17_pk* pk);

/* Group arithmetic of n_items calls of ac17::cp_encrypt (src/schemes/ac17/mod.rs:274-376).
 * The host has parsed each policy and built its MSP; per distinct policy it supplies the Fr table
 *   A[row][l][t] = h(pi_row || l || t) + sum_j M[row][j] * h("0" || (j+1) || l || t)   (mod r)
 * (h = Fr::from_slice(SHA3-256), src/utils/hash/mod.rs:16) for row < n_rows(policy), l < 3, t < 2; the
 * tables of all policies used by the batch are concatenated in dev_A and item i points at the first row
 * of its policy with item_A_off[i].  Ciphertext i owns output rows [ct_row_off[i], ct_row_off[i+1])
 * (n_rows of its policy).  Per item the explicit randomness is s[i][0..2) (drawn at :292) and the Gt
 * `msg` (drawn at :362).  Outputs:
 *   c_0[i][0..3)  = (h_a0*s0, h_a1*s1, h_a2*(s0+s1))                       (:297-302)
 *   c[row][l]     = g * (s0*A[a][l][0] + s1*A[a][l][1])                    (:330-356)
 *   c_p[i]        = e_gh_ka0^s0 * e_gh_ka1^s1 * msg                        (:357-368)
 */
int32_t rhip_ac17_cp_encrypt_batch(rhip_ctx* ctx, const rhip_ac17_pk* pk, size_t n_items,
                                   const rhip_fr* dev_A /*[policy rows][3][2]*/, const uint32_t* dev_item_A_off /*[n_items]*/,
                                   const uint32_t* dev_ct_row_off /*[n_items+1]*/, size_t total_rows,
                                   const rhip_fr* dev_s /*[n_items][2]*/, const rhip_gt* dev_msg /*[n_items]*/,
                                   rhip_g2* dev_c0 /*[n_items][3]*/, rhip_g1* dev_c /*[total_rows][3]*/, rhip_gt* dev_cp /*[n_items]*/);

/* Group arithmetic of n_items calls of ac17::cp_keygen (src/schemes/ac17/mod.rs:191-264).
 * Host supplies per attribute y the hashes H[y][l][t] = h(y||l||t) and, once, H01[l][t] = h("01"||l||t);
 * per item the randomness r0, r1, sigma_y (one per attribute), sigma'.  a_inv[t] = a_t^-1, b[t] from the msk.
 * Outputs per item: k_0[3] (G2), k[y][3] (G1), k_p[3] (G1).  g_k[3] are the msk's G1 elements. */
int32_t rhip_ac17_cp_keygen_batch(rhip_ctx* ctx, const rhip_g1_table* g_table, const rhip_g2_table* h_table,
                                  const rhip_g1* dev_g_k /*[3]*/, const rhip_fr* dev_a_inv /*[2]*/, const rhip_fr* dev_b /*[2]*/,
                                  size_t n_items, size_t n_attrs, const rhip_fr* dev_H /*[n_attrs][3][2]*/,
                                  const rhip_fr* dev_H01 /*[3][2]*/, const rhip_fr* dev_r /*[n_items][2]*/,
                                  const rhip_fr* dev_sigma /*[n_items][n_attrs]*/, const rhip_fr* dev_sigma_p /*[n_items]*/,
                                  rhip_g2* dev_k0 /*[n_items][3]*/, rhip_g1* dev_k /*[n_items][n_attrs][3]*/,
                                  rhip_g1* dev_kp /*[n_items][3]*/);

/* Group arithmetic of n_items calls of ac17::cp_decrypt (src/schemes/ac17/mod.rs:385-430).
 * Ciphertext i occupies rows [ct_row_off[i], ct_row_off[i+1]) of dev_ct_c; it is decrypted with secret
 * key sk_idx[i], whose attribute rows are [sk_row_off[k], sk_row_off[k+1]) of dev_sk_k.  The host has run
 * traverse_policy / calc_pruned (string work) and hands over, per item, the matched row indices:
 * ct_sel / sk_sel hold row numbers relative to the item's ciphertext / key, delimited by sel_off
 * (one (ct,sk) index list pair per item; entries are summed once per occurrence exactly as the
 * reference's name-matching loops do, :403-414).  Output: the Gt handed to decrypt_symmetric (:418). */
int32_t rhip_ac17_cp_decrypt_batch(rhip_ctx* ctx, size_t n_items,
                                   const rhip_g2* dev_ct_c0 /*[n_items][3]*/, const rhip_g1* dev_ct_c /*[rows][3]*/,
                                   const uint32_t* dev_ct_row_off /*[n_items+1]*/, const rhip_gt* dev_ct_cp /*[n_items]*/,
                                   const rhip_g2* dev_sk_k0 /*[n_sk][3]*/, const rhip_g1* dev_sk_k /*[sk rows][3]*/,
                                   const uint32_t* dev_sk_row_off /*[n_sk+1]*/, const rhip_g1* dev_sk_kp /*[n_sk][3]*/,
                                   const uint32_t* dev_sk_idx /*[n_items]*/,
                                   const uint32_t* dev_ct_sel, const uint32_t* dev_ct_sel_off /*[n_items+1]*/,
                                   const uint32_t* dev_sk_sel, const uint32_t* dev_sk_sel_off /*[n_items+1]*/,
                                   rhip_gt* dev_out /*[n_items]*/);

/* Prepared secret keys.  k_0 is fixed per key, so the G2 side of the three pairings e(.., k_0[j]) of cp_decrypt (:416)
 * -- the Miller-loop line coefficients -- is computed once per key and replayed by every decryption with it (the
 * role of rabe-bn's G2 precomputation inside `pairing`; 3 x 88 x 192 B per key).  rhip_ac17_cp_decrypt_batch_prepared
 * takes the handle in place of dev_sk_k0 and returns exactly the values of rhip_ac17_cp_decrypt_batch; it runs the two
 * pairings of each index j on one accumulator (3 lanes per item, one Fq12 squaring per doubling step for both).
 * rhip_ac17_sk_prepare returns after the lines are complete, so the handle may be used from any context at once. */
typedef struct rhip_ac17_sk_lines rhip_ac17_sk_lines;
int32_t rhip_ac17_sk_prepare(rhip_ctx* ctx, size_t n_sk, const rhip_g2* dev_sk_k0 /*[n_sk][3]*/, rhip_ac17_sk_lines** out);
void rhip_ac17_sk_lines_destroy(rhip_ac17_sk_lines* p);
int32_t rhip_ac17_cp_decrypt_batch_prepared(rhip_ctx* ctx, size_t n_items,
                                            const rhip_g2* dev_ct_c0, const rhip_g1* dev_ct_c, const uint32_t* dev_ct_row_off,
                                            const rhip_gt* dev_ct_cp, const rhip_ac17_sk_lines* sk_lines,
                                            const rhip_g1* dev_sk_k, const uint32_t* dev_sk_row_off, const rhip_g1* dev_sk_kp,
                                            const uint32_t* dev_sk_idx, const uint32_t* dev_ct_sel, const uint32_t* dev_ct_sel_off,
                                            const uint32_t* dev_sk_sel, const uint32_t* dev_sk_sel_off, rhip_gt* dev_out);

/* ---- prepared G2 arguments (generic form of rhip_ac17_sk_prepare) -----------------------------------------------
 * The Miller-loop line coefficients of n G2 points (88 triples of Fq2 each, 16.9 KB per point): what `pairing` spends on
 * the G2 side, paid once for a G2 element that many pairings share (a secret key's components, a public key element).
 * Returns after the lines are complete, so the handle may be used from any context. */
typedef struct rhip_g2_lines rhip_g2_lines;
int32_t rhip_g2_lines_prepare(rhip_ctx* ctx, size_t n, const rhip_g2* dev_q, rhip_g2_lines** out);
void rhip_g2_lines_destroy(rhip_g2_lines* p);
/* device memory the handle holds, in bytes: the line triples, the reduced-radix copy the contexts that run those kernels keep beside
 * them, one flag per point */
size_t rhip_g2_lines_bytes(const rhip_g2_lines* p);
/* ---- a handle of fixed capacity, filled and emptied by ranges of blocks (a block = one point's 88 triples, its reduced-radix copy and
 * its flag): what a key store that adds and revokes keys in place is made of.  rhip_g2_lines_reserve makes a handle with room for
 * `capacity` points in which every block is EMPTY: zero line words in both copies and the flag of the point at infinity, so a pair that
 * names an empty block contributes 1.  rhip_g2_lines_bytes reports the reserved size, which is that of rhip_g2_lines_prepare over
 * `capacity` points; a handle from rhip_g2_lines_prepare is a handle of capacity n and takes the three range calls too.
 * rhip_g2_lines_prepare_range: the lines of dev_q[0 .. n) into blocks [first, first + n) -- for points of G2 the bytes
 *   rhip_g2_lines_prepare makes for them at blocks 0 .. n, in both copies; a block whose point is the point at infinity is left empty.
 *   Nothing outside the range is written.
 * rhip_g2_lines_scrub_range: blocks [first, first + n) back to empty, with a kernel of plain vector stores (key material, wiped as the
 *   session secrets are).
 * rhip_g2_lines_range_is_zero: *out_zero = 1 iff every line word of blocks [first, first + n) is zero in BOTH copies and every flag
 *   says empty, 0 otherwise.
 * All return after their device work is complete (rhip_g2_lines_prepare's rule), so the handle may be used from any context of its
 * device afterwards; the caller lets no batch that names the range run beside a call that writes it.  first + n > capacity:
 * RHIP_ERR_ARG, nothing is touched.  n = 0: nothing is done (*out_zero = 1). */
int32_t rhip_g2_lines_reserve(rhip_ctx* ctx, size_t capacity, rhip_g2_lines** out);
int32_t rhip_g2_lines_prepare_range(rhip_ctx* ctx, rhip_g2_lines* lines, size_t first, size_t n, const rhip_g2* dev_q);
int32_t rhip_g2_lines_scrub_range(rhip_ctx* ctx, rhip_g2_lines* lines, size_t first, size_t n);
int32_t rhip_g2_lines_range_is_zero(rhip_ctx* ctx, const rhip_g2_lines* lines, size_t first, size_t n, int32_t* out_zero);

/* ---- Level B: BSW CP-ABE (src/schemes/bsw/mod.rs) ---------------------------------------------------------------
 * Flattened policy trees (the host has parsed the policy text; everything below is numbers).  The leaves of a policy
 * are numbered in DFS order -- the order gen_shares_policy emits shares (src/utils/secretsharing/mod.rs:82-122) --
 * and the tables of all distinct policies of a batch are concatenated:
 *   path_off[leaf .. leaf+1]      the leaf's path entries, root first
 *   path_gate[e], path_x[e]       "child number x (1-based) of gate `gate`" (gate numbered relative to the policy's first gate)
 *   gate_k[g]                     threshold of gate g: its child count for AND, 1 for OR (:98-110)
 *   gate_coef_off[g]              where the gate's k-1 polynomial coefficients start in an item's draw list (DFS pre-order,
 *                                 the reference's draw order :128-134)
 *   leaf_hash[leaf]               Fr(SHA3(name)) of the leaf's attribute (src/utils/hash/mod.rs:23-31)
 * Item i uses the policy whose first leaf row / first gate row are item_tree_leaf[i] / item_tree_gate[i], owns output
 * leaf rows [item_leaf_off[i], item_leaf_off[i+1]) and the draws coef[item_coef_off[i] ..].
 */
typedef struct rhip_bsw_pk rhip_bsw_pk;       /* window tables of g1, g2, h, e_gg_alpha (CpAbePublicKey, bsw/mod.rs:43-49) */
int32_t rhip_bsw_pk_create(rhip_ctx* ctx, const rhip_g1* host_g1, const rhip_g2* host_g2, const rhip_g1* host_h,
                           const rhip_gt* host_e_gg_alpha, rhip_bsw_pk** out);
void rhip_bsw_pk_destroy(rhip_bsw_pk* pk);
/* Group arithmetic of n_items calls of bsw::encrypt (bsw/mod.rs:217-251): explicit randomness per item = secret (:228),
 * the Gt `msg` (:229) and the gate coefficients.  Outputs: c = h * secret, c_p = e_gg_alpha^secret * msg, and per leaf
 * row (g1 * q_y, (g2 * h(name_y)) * q_y) with q_y the leaf's share of `secret`. */
int32_t rhip_bsw_encrypt_batch(rhip_ctx* ctx, const rhip_bsw_pk* pk, size_t n_items, size_t total_leaves,
                               const uint32_t* dev_item_leaf_off /*[n_items+1]*/, const uint32_t* dev_item_tree_leaf /*[n_items]*/,
                               const uint32_t* dev_item_tree_gate /*[n_items]*/, const uint32_t* dev_path_off, const uint32_t* dev_path_gate,
                               const uint32_t* dev_path_x, const uint32_t* dev_gate_k, const uint32_t* dev_gate_coef_off,
                               const rhip_fr* dev_leaf_hash, const rhip_fr* dev_secret /*[n_items]*/, const rhip_fr* dev_coef,
                               const uint32_t* dev_item_coef_off /*[n_items]*/, const rhip_gt* dev_msg /*[n_items]*/,
                               rhip_g1* dev_c /*[n_items]*/, rhip_gt* dev_cp /*[n_items]*/, rhip_g1* dev_cy_g1 /*[total_leaves]*/,
                               rhip_g2* dev_cy_g2 /*[total_leaves]*/);
/* Group arithmetic of n_items calls of bsw::decrypt (bsw/mod.rs:260-318).  The host has run traverse_policy / calc_pruned /
 * calc_coefficients (string and Fr work, per distinct (policy, key attribute set)) and hands over selection tables: entry e
 * names a pruned leaf by its row in the ciphertext (sel_ct_leaf, relative to the item's first leaf row), the matching
 * attribute row of the key (sel_sk_attr, relative to the key's first row) and the leaf's Lagrange coefficient z
 * (sel_coeff).  Item i uses entries sel_start[i] .. sel_start[i] + m_i - 1 and owns pairs [pair_off[i], pair_off[i+1]),
 * pair_off[i+1] - pair_off[i] = 2 m_i + 1 (max_pairs = the largest such count).  Ciphertext i: c, c_p and leaf rows
 * [ct_leaf_off[i], ct_leaf_off[i+1]); key sk_idx[i]: d and attribute rows [sk_attr_off[k], sk_attr_off[k+1]).
 *   out[i] = c_p * FE( ML(-c, d) * prod_e ML(z_e Cy.g1, Dj.g2) ML(-z_e Dj.g1, Cy.g2) )     
 * i.e. the Gt handed to decrypt_symmetric (:308-311).  sk_lines (optional, rhip_bsw_sk_prepare): prepared lines of the
 * keys' G2 components -- the same values, without the G2 arithmetic of the key-side pairings. */
typedef struct rhip_bsw_sk_lines rhip_bsw_sk_lines;
int32_t rhip_bsw_sk_prepare(rhip_ctx* ctx, size_t n_sk, size_t total_attrs, const rhip_g2* dev_sk_d /*[n_sk]*/,
                            const rhip_g2* dev_sk_dj_g2 /*[total_attrs]*/, rhip_bsw_sk_lines** out);
void rhip_bsw_sk_lines_destroy(rhip_bsw_sk_lines* p);
int32_t rhip_bsw_decrypt_batch(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs,
                               const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                               const uint32_t* dev_sel_ct_leaf, const uint32_t* dev_sel_sk_attr, const rhip_fr* dev_sel_coeff,
                               const rhip_g1* dev_ct_c /*[n_items]*/, const rhip_gt* dev_ct_cp /*[n_items]*/,
                               const rhip_g1* dev_ct_cy_g1, const rhip_g2* dev_ct_cy_g2, const uint32_t* dev_ct_leaf_off /*[n_items+1]*/,
                               const rhip_g2* dev_sk_d /*[n_sk]*/, const rhip_g1* dev_sk_dj_g1, const rhip_g2* dev_sk_dj_g2,
                               const uint32_t* dev_sk_attr_off /*[n_sk+1]*/, const uint32_t* dev_sk_idx /*[n_items]*/,
                               const rhip_bsw_sk_lines* sk_lines /* or NULL */, rhip_gt* dev_out /*[n_items]*/);

/* The same with ONE secret key for every item (dev_sk_d [1], dev_sk_dj_* = its attribute rows, dev_sk_attr_off = {0, n}) -- what
 * rabe_bsw_decrypt_packed does and BASELINE config 3 measures.  The key-side G1 arguments -z_e * Dj.g1 then depend on the selection
 * entry alone: ciphertexts that share a policy share their entries (dev_sel_start), so those scalings are computed once per ENTRY (n_sel
 * of them) instead of once per pair.  Results are those of rhip_bsw_decrypt_batch with dev_sk_idx = all zero. */
int32_t rhip_bsw_decrypt_batch_one_sk(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                      const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                      const uint32_t* dev_sel_ct_leaf, const uint32_t* dev_sel_sk_attr, const rhip_fr* dev_sel_coeff,
                                      const rhip_g1* dev_ct_c /*[n_items]*/, const rhip_gt* dev_ct_cp /*[n_items]*/,
                                      const rhip_g1* dev_ct_cy_g1, const rhip_g2* dev_ct_cy_g2, const uint32_t* dev_ct_leaf_off /*[n_items+1]*/,
                                      const rhip_g2* dev_sk_d /*[1]*/, const rhip_g1* dev_sk_dj_g1, const rhip_g2* dev_sk_dj_g2,
                                      const uint32_t* dev_sk_attr_off /*[2]*/, const rhip_bsw_sk_lines* sk_lines /* or NULL */, rhip_gt* dev_out /*[n_items]*/);

/* ---- Level B: LSW KP-ABE (src/schemes/lsw/mod.rs) ----------------------------------------------------------------
 * rhip_lsw_keygen_batch: positive leaves; rhip_lsw_keygen_batch_signed: positive and negative ("!x", :137-146).  The reference's
 * decrypt has no negative branch at all (a TODO, :265-278): the host layer reproduces what it does instead. */
typedef struct rhip_lsw_pk rhip_lsw_pk;       /* window tables of g1, g2 (KpAbePublicKey, lsw/mod.rs:44-51) */
int32_t rhip_lsw_pk_create(rhip_ctx* ctx, const rhip_g1* host_g1, const rhip_g2* host_g2, rhip_lsw_pk** out);
void rhip_lsw_pk_destroy(rhip_lsw_pk* pk);
/* Group arithmetic of n_items calls of lsw::keygen (lsw/mod.rs:121-170): shares q_y of alpha1 over the item's policy
 * (flattened trees as for bsw; draws = the gate coefficients), then per leaf the explicit `random` r_y (:136):
 *   d1[row] = g1 * (alpha2 * q_y + h(y) * r_y)   ( = g1*(alpha2 q_y) + (g1*h(y))*r_y, :149-154 ),   d2[row] = g2 * r_y
 * dev_alpha = (alpha1, alpha2) of the master key. */
int32_t rhip_lsw_keygen_batch(rhip_ctx* ctx, const rhip_lsw_pk* pk, size_t n_items, size_t total_leaves,
                              const uint32_t* dev_item_leaf_off /*[n_items+1]*/, const uint32_t* dev_item_tree_leaf, const uint32_t* dev_item_tree_gate,
                              const uint32_t* dev_path_off, const uint32_t* dev_path_gate, const uint32_t* dev_path_x, const uint32_t* dev_gate_k,
                              const uint32_t* dev_gate_coef_off, const rhip_fr* dev_leaf_hash, const rhip_fr* dev_alpha /*[2]*/,
                              const rhip_fr* dev_coef, const uint32_t* dev_item_coef_off /*[n_items]*/, const rhip_fr* dev_rand /*[total_leaves]*/,
                              rhip_g1* dev_d1 /*[total_leaves]*/, rhip_g2* dev_d2 /*[total_leaves]*/);
/* The same with negative leaves ("!x", lsw/mod.rs:137-146): leaf_neg[leaf] (per policy leaf, beside leaf_hash) != 0 marks them.
 * A positive row gets (d1, d2) as above and the identity in d3..d5; a negative row gets the identity in d1, d2 and
 *   d3 = g1 * q_y + g1_b2 * r_y,   d4 = g1_b * (h(y) r_y) + h_g1 * r_y,   d5 = g1 * (-r_y)
 * with g1_b = g1 * b, g1_b2 = g1 * b^2 (dev_b = the master key's b, host_h_g1 its h_g1; a window table of h_g1 is built per call). */
int32_t rhip_lsw_keygen_batch_signed(rhip_ctx* ctx, const rhip_lsw_pk* pk, size_t n_items, size_t total_leaves,
                                     const uint32_t* dev_item_leaf_off /*[n_items+1]*/, const uint32_t* dev_item_tree_leaf, const uint32_t* dev_item_tree_gate,
                                     const uint32_t* dev_path_off, const uint32_t* dev_path_gate, const uint32_t* dev_path_x, const uint32_t* dev_gate_k,
                                     const uint32_t* dev_gate_coef_off, const rhip_fr* dev_leaf_hash, const uint32_t* dev_leaf_neg,
                                     const rhip_fr* dev_alpha /*[2]*/, const rhip_fr* dev_b /*[1]*/, const rhip_g1* host_h_g1, const rhip_fr* dev_coef,
                                     const uint32_t* dev_item_coef_off /*[n_items]*/, const rhip_fr* dev_rand /*[total_leaves]*/,
                                     rhip_g1* dev_d1, rhip_g2* dev_d2, rhip_g1* dev_d3, rhip_g1* dev_d4, rhip_g1* dev_d5 /*[total_leaves] each*/);
/* Group arithmetic of n_items calls of lsw::decrypt (lsw/mod.rs:228-290).  Selection entry e: the key's leaf row
 * (sel_sk_leaf, relative to the key's first row), the ciphertext's attribute row (sel_ct_attr, relative) and the leaf's
 * coefficient c.  Item i: entries sel_start[i] .. + m_i - 1, pairs [pair_off[i], pair_off[i+1]) with m_i + 1 of them; its
 * key is sk_idx[i] (NULL: i) with leaf rows [sk_leaf_off[k], ..), its ciphertext ct_idx[i] (NULL: i) with attribute rows
 * [ct_attr_off[c], ..).  n_sel = total number of selection entries.
 *   out[i] = e1 * FE( ML( sum_e -c_e D1_e, e2 ) * prod_e ML( c_e E1_e, D2_e ) )               
 * (the factors that share e2 collapse into one pairing of a multi-scalar sum with shared doublings).
 * ct_e2_lines (optional): prepared lines of dev_ct_e2 (rhip_g2_lines_prepare over the same array). */
int32_t rhip_lsw_decrypt_batch(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                               const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                               const uint32_t* dev_sel_sk_leaf, const uint32_t* dev_sel_ct_attr, const rhip_fr* dev_sel_coeff,
                               const rhip_gt* dev_ct_e1 /*[n_items]: item i's e1*/, const rhip_g2* dev_ct_e2 /*[n_ct]*/,
                               const rhip_g1* dev_ct_e1j /*[ct attribute rows]: ej.1*/, const uint32_t* dev_ct_attr_off /*[n_ct+1]*/,
                               const uint32_t* dev_ct_idx /*[n_items] or NULL*/, const rhip_g1* dev_sk_d1, const rhip_g2* dev_sk_d2,
                               const uint32_t* dev_sk_leaf_off /*[n_sk+1]*/, const uint32_t* dev_sk_idx /*[n_items] or NULL*/,
                               const rhip_g2_lines* ct_e2_lines /* or NULL */, rhip_gt* dev_out /*[n_items]*/);

/* The same with ONE ciphertext for every item (dev_ct_e2 [1], dev_ct_e1j = its attribute rows) -- n fresh keys against one ciphertext, what
 * BASELINE config 4 measures and rabe_lsw_decrypt_packed does.  The scaled G1 arguments c_e * E1_e then depend on the selection entry
 * alone: items that share a policy share their entries (dev_sel_start), so the scalings are computed once per ENTRY (n_sel of them)
 * instead of once per pair.  Results are those of rhip_lsw_decrypt_batch with dev_ct_idx = all zero. */
int32_t rhip_lsw_decrypt_batch_one_ct(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                      const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                      const uint32_t* dev_sel_sk_leaf, const uint32_t* dev_sel_ct_attr, const rhip_fr* dev_sel_coeff,
                                      const rhip_gt* dev_ct_e1 /*[n_items]: e1 replicated*/, const rhip_g2* dev_ct_e2 /*[1]*/,
                                      const rhip_g1* dev_ct_e1j /*[the ciphertext's attribute rows]*/, const rhip_g1* dev_sk_d1, const rhip_g2* dev_sk_d2,
                                      const uint32_t* dev_sk_leaf_off /*[n_sk+1]*/, const uint32_t* dev_sk_idx /*[n_items] or NULL*/,
                                      const rhip_g2_lines* ct_e2_lines /* or NULL */, rhip_gt* dev_out /*[n_items]*/);

/* The same with ONE secret key for every item and a ciphertext of its own per item (ciphertext i = item i: dev_ct_e2 [n_items], attribute rows
 * [ct_attr_off[i], ct_attr_off[i+1]) of dev_ct_e1j) -- what a KP-ABE key holder does and rabe_lsw_decrypt_one_sk_packed runs.  Every D2 is the
 * key's: sk_d2_lines = rhip_g2_lines_prepare over the key's D2 rows (block = leaf row, what sel_sk_leaf names), so the m_i key-side Miller loops
 * of an item replay prepared lines and the only walked G2 argument is the item's own e2 (whose walk verdict rhip_ctx_collect_walk_verdicts
 * hands out).  sum_e -c_e D1_e depends on the selection alone and is computed once per selection GROUP, stated by the caller: the n_sel entries
 * are the concatenation of the groups' entries, group g owning [group_off[g], group_off[g+1]); item i belongs to group item_group[i], i.e.
 * sel_start[i] = group_off[item_group[i]] and m_i = the group's entry count.  Without sharing: one group per item (n_groups = n_items).  What
 * stays per pair is the scaling c_e * E1_{i,e}.  Results are those of rhip_lsw_decrypt_batch with dev_sk_idx = all zero. */
int32_t rhip_lsw_decrypt_batch_one_sk(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                      const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                      const uint32_t* dev_sel_sk_leaf, const uint32_t* dev_sel_ct_attr, const rhip_fr* dev_sel_coeff,
                                      size_t n_groups, const uint32_t* dev_group_off /*[n_groups+1]*/, const uint32_t* dev_item_group /*[n_items]*/,
                                      const rhip_gt* dev_ct_e1 /*[n_items]*/, const rhip_g2* dev_ct_e2 /*[n_items]*/,
                                      const rhip_g1* dev_ct_e1j /*[ct attribute rows]: ej.1*/, const uint32_t* dev_ct_attr_off /*[n_items+1]*/,
                                      const rhip_g1* dev_sk_d1 /*[the key's leaf rows]*/, const rhip_g2_lines* sk_d2_lines, rhip_gt* dev_out /*[n_items]*/);
/* The attribute rows of n_items calls of lsw::encrypt (lsw/mod.rs:201-208), one lane per row (k_lsw_enc_rows).  The four tables are window
 * tables with 16-bit windows (rhip_g1_table_add_w16) of the public key's g1, g1_b, g1_b2 and h_b.  Item i owns rows
 * [item_row_off[i], item_row_off[i+1]); row t of it has the attribute hash h = dev_hash[item_hash_off[i] + t - item_row_off[i]] (items with
 * the same attribute list share their hashes) and the scalar dev_sx[t], which the caller supplies as the reference's loop leaves it (:197-200:
 * the first row's loses sx[i], not the new element -- zero for a list of one attribute).  The products h secret and sx h are formed on the device.
 *   out[3 t] = e3 = g1 * (h secret_i)     out[3 t + 1] = e4 = g1_b * sx     out[3 t + 2] = e5 = g1_b2 * (sx h) + h_b * sx
 * e5 is two walks on one accumulator; the three conversions of a row share one inversion, and a block its rows'.  An element that is the
 * identity (sx = 0, h secret = 0, or the two halves of e5 cancelling) is 64 zero bytes, and its neighbours in the row are unaffected.  The
 * bytes are those of rhip_g1_table_mul over host-formed products followed by rhip_g1_add.  The item-level elements (e1, e2) are not
 * computed here. */
int32_t rhip_lsw_encrypt_rows(rhip_ctx* ctx, const rhip_g1_table* g1, const rhip_g1_table* g1_b, const rhip_g1_table* g1_b2, const rhip_g1_table* h_b,
                              size_t n_items, size_t total_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/,
                              const uint32_t* dev_item_hash_off /*[n_items]*/, const rhip_fr* dev_hash, const rhip_fr* dev_secret /*[n_items]*/,
                              const rhip_fr* dev_sx /*[total_rows]*/, rhip_g1* dev_out /*[3 total_rows]: e3, e4, e5 per row*/);

/* ---- Level B: GHW11 outsourced decryption (src/schemes/ghw11/mod.rs:227-295) ----------------------
 * Group arithmetic of n_items calls of ghw11::transform under ONE transform key.  tk_lines = rhip_g2_lines_prepare over the key's G2
 * elements in the order k_z, l_z, k_x[0], k_x[1], ... : every Miller loop of the batch replays prepared lines (no G2 arithmetic).
 * Selection entry e: the ciphertext row (sel_ct_row, relative to the item's first row), the key attribute (sel_tk_attr) and the leaf's
 * coefficient w.  Item i: entries sel_start[i] .. + m_i - 1, pairs [pair_off[i], pair_off[i+1]) with m_i + 2 of them.
 *   out[i] = t = e(c1, k_z) / ( prod_e e(w_e D_e, K_e) * e(sum_e w_e C_e, l_z) )   as ONE product of m_i + 2 Miller values and one
 * final exponentiation (the factors that share l_z collapse into one pairing of a multi-scalar sum). */
int32_t rhip_ghw11_transform_batch(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                   const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                   const uint32_t* dev_sel_ct_row, const uint32_t* dev_sel_tk_attr, const rhip_fr* dev_sel_coeff,
                                   const rhip_g1* dev_ct_c1 /*[n_items]*/, const rhip_g1* dev_ct_c /*[rows]: ci*/, const rhip_g1* dev_ct_d /*[rows]: di*/,
                                   const uint32_t* dev_ct_row_off /*[n_items+1]*/, const rhip_g2_lines* tk_lines, rhip_gt* dev_out /*[n_items]*/);
/* The same batch under MANY transform keys -- a proxy's mixed queue, item i served under its own user's key.  store_lines = ONE
 * rhip_g2_lines_prepare over the elements of all keys, key after key, each in the order k_z, l_z, k_x[0], k_x[1], ...;
 * dev_item_line_base[i] = the index, in that array, of the k_z of item i's key, so the item's pairs replay the blocks base, base + 1 and
 * base + 2 + sel_tk_attr[e].  The other arguments are rhip_ghw11_transform_batch's, and out[i] is what that call returns for item i under
 * its key's own handle, bit for bit: only the gather kernel differs (k_ghw11_pairs_keyed), the sum, the Miller loops and the final
 * exponentiation are the same launches.  dev_item_ok (may be NULL: every item is served): an item with dev_item_ok[i] = 0 contributes no
 * pair and its output is zeros -- what a caller that zeroed dev_out finds there (the launch set ends by writing them); its arrays are
 * still read, so they must be valid.  A pair whose block index lies beyond the handle's count is skipped, never read.  RHIP_ERR_ARG: a
 * handle of 2^32 - 2 or more elements (the two largest 32-bit values mark skipped and walking pairs). */
int32_t rhip_ghw11_transform_batch_keyed(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                         const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                         const uint32_t* dev_sel_ct_row, const uint32_t* dev_sel_tk_attr, const rhip_fr* dev_sel_coeff,
                                         const rhip_g1* dev_ct_c1 /*[n_items]*/, const rhip_g1* dev_ct_c /*[rows]: ci*/, const rhip_g1* dev_ct_d /*[rows]: di*/,
                                         const uint32_t* dev_ct_row_off /*[n_items+1]*/, const uint32_t* dev_item_line_base /*[n_items]*/,
                                         const uint32_t* dev_item_ok /*[n_items], may be NULL*/, const rhip_g2_lines* store_lines,
                                         rhip_gt* dev_out /*[n_items]*/);
/* ghw11 decrypt for the HOLDER of the secret key (no proxy): arguments of rhip_ghw11_transform_batch with sk_lines = rhip_g2_lines_prepare over
 * k, l, k_x[0], k_x[1], ... of the Ghw11SecretKey (a transform key has that layout), plus c of every item.
 *   msg[i] = c[i] * t_1[i]^-1,  t_1 = the transform's expression on the secret key's own elements
 * which is decrypt_out(transform(ct, tk), rk) for every z tkgen may draw (t_z = t_1^(1/z); ghw11/mod.rs:252-282, :302).  One launch set: the
 * G1 arguments enter the Miller loops with the opposite sign (t_1^-1 costs nothing), and c is the leading factor of the final-exponentiation
 * kernel of whichever pairing family the context selects -- t_1 is never written to device memory and no Gt power is taken. */
int32_t rhip_ghw11_decrypt_batch(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                 const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                 const uint32_t* dev_sel_ct_row, const uint32_t* dev_sel_sk_attr, const rhip_fr* dev_sel_coeff,
                                 const rhip_g1* dev_ct_c1 /*[n_items]*/, const rhip_g1* dev_ct_c /*[rows]: ci*/, const rhip_g1* dev_ct_d /*[rows]: di*/,
                                 const uint32_t* dev_ct_row_off /*[n_items+1]*/, const rhip_g2_lines* sk_lines,
                                 const rhip_gt* dev_c /*[n_items]*/, rhip_gt* dev_msg /*[n_items]*/);
/* GHW11 encrypt (ghw11/mod.rs:189-225) over the flattened policy trees of the BSW block above.  rhip_ghw11_pk: window tables
 * (8-bit and 16-bit) of g1, g1_a and e_gg_alpha (Ghw11PublicKey).  Explicit randomness per item = secret, the Gt `msg` and the gate
 * coefficients, plus one draw t per leaf row.  Outputs: c = e_gg_alpha^secret * msg, c1 = g1 * secret, and per leaf row
 * cd[2 row] = C = g1_a * lambda + g1 * (-H(j) t), cd[2 row + 1] = D = g1 * t, with lambda the leaf's share of `secret` and
 * H(j) = leaf_hash = Fr(SHA3(remove_index(name_col))) -- one lane per row (k_ghw11_enc_rows). */
typedef struct rhip_ghw11_pk rhip_ghw11_pk;
int32_t rhip_ghw11_pk_create(rhip_ctx* ctx, const rhip_g1* host_g1, const rhip_g1* host_g1_a, const rhip_gt* host_e_gg_alpha, rhip_ghw11_pk** out);
void rhip_ghw11_pk_destroy(rhip_ghw11_pk* pk);
int32_t rhip_ghw11_encrypt_batch(rhip_ctx* ctx, const rhip_ghw11_pk* pk, size_t n_items, size_t total_leaves,
                                 const uint32_t* dev_item_leaf_off /*[n_items+1]*/, const uint32_t* dev_item_tree_leaf /*[n_items]*/,
                                 const uint32_t* dev_item_tree_gate /*[n_items]*/, const uint32_t* dev_path_off, const uint32_t* dev_path_gate,
                                 const uint32_t* dev_path_x, const uint32_t* dev_gate_k, const uint32_t* dev_gate_coef_off,
                                 const rhip_fr* dev_leaf_hash, const rhip_fr* dev_secret /*[n_items]*/, const rhip_fr* dev_coef,
                                 const uint32_t* dev_item_coef_off /*[n_items]*/, const rhip_fr* dev_t /*[total_leaves]*/,
                                 const rhip_gt* dev_msg /*[n_items]*/, rhip_gt* dev_c /*[n_items]*/, rhip_g1* dev_c1 /*[n_items]*/,
                                 rhip_g1* dev_cd /*[2 total_leaves]: C, D per row*/);
/* GHW11 keygen (ghw11/mod.rs:123-152) for n_items keys under one master key.  rhip_ghw11_keys: 8- and 16-bit window tables of g2 and g2_a
 * (Ghw11PublicKey) and the master key's g2_alpha -- the G2 side of the key pair, beside rhip_ghw11_pk (the G1 / Gt side encrypt uses).
 * Item i owns output rows [item_row_off[i], item_row_off[i+1]) = 2 + (its number of attributes): L = g2 * r_i, K = g2_alpha + g2_a * r_i,
 * then K_x = g2 * (h(x) r_i) per attribute with h(x) = dev_hash[item_hash_off[i] + x] (Fr(SHA3(name)); items with the same attribute list
 * share their hashes).  One lane per row (k_ghw11_keygen_rows), one inversion per block, canonical wire form out. */
typedef struct rhip_ghw11_keys rhip_ghw11_keys;
int32_t rhip_ghw11_keys_create(rhip_ctx* ctx, const rhip_g2* host_g2, const rhip_g2* host_g2_a, const rhip_g2* host_g2_alpha, rhip_ghw11_keys** out);
void rhip_ghw11_keys_destroy(rhip_ghw11_keys* keys);
int32_t rhip_ghw11_keygen_batch(rhip_ctx* ctx, const rhip_ghw11_keys* keys, size_t n_items, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/,
                                const uint32_t* dev_item_hash_off /*[n_items]*/, const rhip_fr* dev_hash, const rhip_fr* dev_r /*[n_items]*/,
                                rhip_g2* dev_out /*[n_rows]*/);
/* GHW11 keygen + tkgen (ghw11/mod.rs:123-178) fused, for an authority that issues a user's secret key and the transform key of that user's
 * proxy in one go: it knows r_i and z_i, so every transform-key element is a fixed-base multiple as well.  Rows as in
 * rhip_ghw11_keygen_batch, for both outputs:
 *   dev_out_tk: L_z = g2 * (r z^-1), K_z = g2_alpha * z^-1 + g2_a * (r z^-1), K_x_z = g2 * (h(x) r z^-1)
 *   dev_out_sk: the rows rhip_ghw11_keygen_batch writes for the same r (that kernel, unchanged); NULL: not computed
 * z_i^-1 and r_i z_i^-1 are formed on the device (k_ghw11_tk_scalars: one Fr inversion per block); dev_flags[i] = 1 where z_i = 0 (that
 * item's transform-key rows are then the point at infinity), else 0.  One lane per transform-key row (k_ghw11_provision_rows), row 1 as
 * two walks on one accumulator.  The 16-bit window table of g2_alpha is built on the first call with a handle and kept in it (134 MB;
 * rhip_ghw11_keys_create alone does not build it); the build is serialised, so contexts may share the handle. */
int32_t rhip_ghw11_provision_batch(rhip_ctx* ctx, rhip_ghw11_keys* keys, size_t n_items, size_t n_rows,
                                   const uint32_t* dev_item_row_off /*[n_items+1]*/, const uint32_t* dev_item_hash_off /*[n_items]*/,
                                   const rhip_fr* dev_hash, const rhip_fr* dev_r /*[n_items]*/, const rhip_fr* dev_z /*[n_items]*/,
                                   rhip_g2* dev_out_sk /*[n_rows] or NULL*/, rhip_g2* dev_out_tk /*[n_rows]*/, uint32_t* dev_flags /*[n_items]*/);
/* BDABE / MKE08 keygen (bdabe/mod.rs:201-222, mke08/mod.rs:185-206) for n_items users under one authority key (MKE08: the master key).
 * rhip_dnf_keys: 8- and 16-bit window tables of p1, g1, p2, g2 and the authority's a1 / a2 (MKE08: msk.g1 / msk.g2).  Item i owns rows
 * 2 i, 2 i + 1 of both outputs: out_g1 = sk.u1 = a1 + p1 * r_i, pk.u1 = g1 * r_i; out_g2 = sk.u2 = a2 + p2 * r_i, pk.u2 = g2 * r_i.
 * One lane per element (k_dnf_keygen_g1, k_dnf_keygen_g2), one inversion per block, canonical wire form out. */
typedef struct rhip_dnf_keys rhip_dnf_keys;
int32_t rhip_dnf_keys_create(rhip_ctx* ctx, const rhip_g1* host_p1, const rhip_g1* host_g1, const rhip_g2* host_p2, const rhip_g2* host_g2,
                             const rhip_g1* host_a1, const rhip_g2* host_a2, rhip_dnf_keys** out);
void rhip_dnf_keys_destroy(rhip_dnf_keys* keys);
int32_t rhip_dnf_keygen_batch(rhip_ctx* ctx, const rhip_dnf_keys* keys, size_t n_items, const rhip_fr* dev_r /*[n_items]*/,
                              rhip_g1* dev_out_g1 /*[2 n_items]*/, rhip_g2* dev_out_g2 /*[2 n_items]*/);
/* BDABE / MKE08 encrypt (bdabe/mod.rs:317-358, mke08/mod.rs:290-334).  Every group element of their ciphertexts is a fixed-base product
 * with the draw r of its row (one row per (item, DNF term)):  p1 * r, p2 * r (public key) and T1 * r, T2 * r, Tgt_g^r * msg_g with the
 * term's folded attribute keys T1 = sum a1_k (G1), T2 = sum a2_k (G2), Tgt_g = prod of the keys' Gt component g (BDABE: n_gt = 1, a3;
 * MKE08: n_gt = 2, gt1 and gt2).
 * rhip_dnf_pk: 8- and 16-bit window tables of p1 (G1) and p2 (G2), walked by every row.
 * rhip_dnf_terms: 8-bit window tables of n_terms term bases -- host_t1 [n_terms], host_t2 [n_terms], host_tgt [n_gt][n_terms] -- built
 * in three launches (G1, G2, Gt; 522 KB + 1 MB + n_gt x 3.1 MB per term), and the device array of table pointers the row kernels index
 * by term.
 * rhip_dnf_encrypt_batch: one launch set over the n_rows rows of a call whose items may use several policies.  The term sets
 * sets[0 .. n_sets) are concatenated: dev_row_term[j] < (sum of their n_terms) names row j's term in that order, dev_row_item[j] its item,
 * dev_r[j] its draw; dev_msg [n_gt][n_items] the items' Gt messages (BDABE msg; MKE08 msg1, msg2).  Outputs, laid out for the records:
 *   dev_gt [n_rows][n_gt]:  Tgt_g^r * msg_g                         (BDABE e1; MKE08 j1, j2)      -- k_dnf_enc_gt
 *   dev_g1 [n_rows][2]:     p1 * r, T1 * r                          (BDABE e2, e4; MKE08 j3, j5)  -- k_dnf_enc_g1
 *   dev_g2 [n_rows][2]:     p2 * r, T2 * r                          (BDABE e3, e5; MKE08 j4, j6)  -- k_dnf_enc_g2
 * The G1 and G2 kernels run one lane per row, park the first point in the row's output and convert both with one inversion per block. */
typedef struct rhip_dnf_pk rhip_dnf_pk;
int32_t rhip_dnf_pk_create(rhip_ctx* ctx, const rhip_g1* host_p1, const rhip_g2* host_p2, rhip_dnf_pk** out);
void rhip_dnf_pk_destroy(rhip_dnf_pk* pk);
typedef struct rhip_dnf_terms rhip_dnf_terms;
int32_t rhip_dnf_terms_create(rhip_ctx* ctx, size_t n_terms, uint32_t n_gt, const rhip_g1* host_t1, const rhip_g2* host_t2, const rhip_gt* host_tgt,
                              rhip_dnf_terms** out);
void rhip_dnf_terms_destroy(rhip_dnf_terms* terms);
int32_t rhip_dnf_encrypt_batch(rhip_ctx* ctx, const rhip_dnf_pk* pk, size_t n_sets, const rhip_dnf_terms* const* sets, size_t n_items, size_t n_rows,
                               const uint32_t* dev_row_term /*[n_rows]*/, const uint32_t* dev_row_item /*[n_rows]*/, const rhip_fr* dev_r /*[n_rows]*/,
                               const rhip_gt* dev_msg /*[n_gt][n_items]*/, rhip_gt* dev_gt /*[n_rows][n_gt]*/, rhip_g1* dev_g1 /*[n_rows][2]*/,
                               rhip_g2* dev_g2 /*[n_rows][2]*/);
/* BDABE / MKE08 decrypt (bdabe/mod.rs:377-380, mke08/mod.rs:385-388) of n_items ciphertext conjunctions under ONE user key, in the four-pair
 * form: with S1 = sum au1_k and S2 = sum au2_k over the conjunction's attribute keys (sums of the KEY's elements: fixed per distinct
 * conjunction, a CLASS, stated by the caller)
 *   out[i] = lead[i] * e(e2, S2) * e(S1, e3) * e(-e4, u2) * e(-u1, e5)          (MKE08: lead = j1 j2; e2 .. e5 = j3 .. j6)
 * which is the element the per-attribute form prod_k e(e2, au2_k) ... gives (rhip_pairing_jobs as the host's plan_term fills it).  Four Miller
 * loops per item whatever the conjunction's length: pairs 0 and 2 replay prepared lines -- key_lines = rhip_g2_lines_prepare over
 * [sk.u2, S2_0, S2_1, ...], block 0 the user key's u2 and block 1 + c the S2 of class c -- and pairs 1 and 3 walk the item's own e3 and e5,
 * whose membership verdicts rhip_ctx_collect_walk_verdicts hands out.  dev_class_skip[c]: bit 0 = S1 of the class is the identity, bit 1 =
 * S2 is (dev_class_s1[c] is not read then); a pair with an argument at infinity -- those two, a ciphertext element, u1 or u2 -- contributes 1.
 * dev_item_class[i] < n_classes (an item that names no class has all four pairs skipped).  One gather kernel (k_dnf_dec_pairs: uniform pair
 * map, four pairs per item, no scalar multiplication), then the Miller dispatch and the final exponentiation of every multi-pairing launch.
 * dev_lead may be NULL (no leading factor) or dev_out (in place). */
int32_t rhip_dnf_decrypt_batch_one_uk(rhip_ctx* ctx, size_t n_items, size_t n_classes, const uint32_t* dev_item_class /*[n_items]*/,
                                      const rhip_g1* dev_class_s1 /*[n_classes]*/, const uint8_t* dev_class_skip /*[n_classes]: bit 0 S1 = O, bit 1 S2 = O*/,
                                      const rhip_g1* dev_neg_u1 /*[1]*/, const rhip_g2_lines* key_lines /* block 0: sk.u2, block 1 + c: S2 of class c */,
                                      const rhip_g1* dev_ct_g1 /*[n_items][2]: e2, e4*/, const rhip_g2* dev_ct_g2 /*[n_items][2]: e3, e5*/,
                                      const rhip_gt* dev_lead /*[n_items]*/, rhip_gt* dev_out /*[n_items]*/);

/* ---- Level B: AW11 multi-authority CP-ABE (src/schemes/aw11/mod.rs) -----------------------------------------------
 * rhip_aw11_pk: gk (g1, g2), the constant e(g1, g2) and, for each of the n_attrs attributes of the authorities in play,
 * (egg_alpha_x, g2 * y_x) (Aw11PublicKey.attr, :56-61) as window tables.  leaf_attr[leaf] (per policy leaf, beside the
 * flattened tree tables) = the attribute's index in those arrays.  The per-attribute tables are 8-bit windows (4.2 MB per
 * attribute) plus, by default, SIGNED 10-bit windows built from them (26 x 512 entries = 6.8 MB per attribute, 1.4 GB for 200: 26 instead
 * of 32 table entries per power, a negative digit is a conjugation in Gt / a negated y in G2; RABE_AW11_ATTR_BITS = 9 ... 14 picks another
 * width, 8 none; only built while they leave half of the device memory free).  16-bit windows (536 MB per attribute, 107 GB for 200: 16
 * entries per power) are OPT-IN through RABE_AW11_ATTR_W16=1, and even then only built while they leave a quarter of the device memory
 * free.  Results do not depend on any of it. */
typedef struct rhip_aw11_pk rhip_aw11_pk;
int32_t rhip_aw11_pk_create(rhip_ctx* ctx, const rhip_g1* host_g1, const rhip_g2* host_g2, size_t n_attrs,
                            const rhip_gt* host_egg_alpha /*[n_attrs]*/, const rhip_g2* host_g2_y /*[n_attrs]*/, rhip_aw11_pk** out);
void rhip_aw11_pk_destroy(rhip_aw11_pk* pk);
/* The form the per-attribute tables of a handle took (read-only; the fallbacks above are silent otherwise): 0 plain 8-bit windows, 1 16-bit
 * windows per attribute, 9 ... 14 signed windows of that width. */
int32_t rhip_aw11_pk_table_form(const rhip_aw11_pk* pk, int32_t* form);
/* Group arithmetic of n_items calls of aw11::encrypt (aw11/mod.rs:241-289).  Explicit randomness per item, in the
 * reference's draw order: s (:257), the gate coefficients of the s-shares then of the 0-shares (item_n_coef[i] each,
 * consecutive in dev_coef from item_coef_off[i]; :259-260), the Gt `msg` (:262), and one r_x per row (dev_rand, :267).
 *   c_0 = msg * E^s ;  per row: c1 = E^lambda_x * egg_alpha_x^r_x,  c2 = g2 * r_x,  c3 = (g2*y_x) * r_x + g2 * omega_x */
int32_t rhip_aw11_encrypt_batch(rhip_ctx* ctx, const rhip_aw11_pk* pk, size_t n_items, size_t total_rows,
                                const uint32_t* dev_item_row_off /*[n_items+1]*/, const uint32_t* dev_item_tree_leaf, const uint32_t* dev_item_tree_gate,
                                const uint32_t* dev_item_n_coef /*[n_items]*/, const uint32_t* dev_path_off, const uint32_t* dev_path_gate,
                                const uint32_t* dev_path_x, const uint32_t* dev_gate_k, const uint32_t* dev_gate_coef_off,
                                const uint32_t* dev_leaf_attr, const rhip_fr* dev_s /*[n_items]*/, const rhip_fr* dev_coef,
                                const uint32_t* dev_item_coef_off /*[n_items]*/, const rhip_fr* dev_rand /*[total_rows]*/,
                                const rhip_gt* dev_msg /*[n_items]*/, rhip_gt* dev_c0 /*[n_items]*/, rhip_gt* dev_c1 /*[total_rows]*/,
                                rhip_g2* dev_c2 /*[total_rows]*/, rhip_g2* dev_c3 /*[total_rows]*/);
/* Group arithmetic of n_items calls of aw11::decrypt (aw11/mod.rs:298-366).  Selection entry e: ciphertext row (sel_ct_row,
 * relative to the item's first row), key attribute row (sel_sk_attr, relative to the key's first row), coefficient c.
 * dev_sk_hash[k] = g1 * h(gid_k) (the reference hashes the gid inside decrypt, :318).
 *   out[i] = c_0 * prod_e C1_e^(-c_e) * FE( ML( -H(gid), sum_e c_e C3_e ) * prod_e ML( c_e K_e, C2_e ) )   
 * The G2 sum and the Gt product run with shared doublings / squarings over the NAFs of the coefficients. */
int32_t rhip_aw11_decrypt_batch(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                const uint32_t* dev_sel_ct_row, const uint32_t* dev_sel_sk_attr, const rhip_fr* dev_sel_coeff,
                                const rhip_gt* dev_ct_c0 /*[n_items]*/, const rhip_gt* dev_ct_c1, const rhip_g2* dev_ct_c2, const rhip_g2* dev_ct_c3,
                                const uint32_t* dev_ct_row_off /*[n_items+1]*/, const rhip_g1* dev_sk_hash /*[n_sk]*/, const rhip_g1* dev_sk_k,
                                const uint32_t* dev_sk_attr_off /*[n_sk+1]*/, const uint32_t* dev_sk_idx /*[n_items] or NULL*/,
                                rhip_gt* dev_out /*[n_items]*/);
/* The same call, same arguments, same bytes, with the leading factor c_0 * prod_e C1_e^(-c_e) over width-4 signed windows (the routine of
 * rhip_gt_multiexp_rows: k_gtmexp4_digits, k_gtmexp4_table, k_gt_mexp4_partial, k_gt_mexp4_finish) in place of k_gt_multiexp_partial +
 * k_gt_lead; every other launch is rhip_aw11_decrypt_batch's.  Measured slower on AW11's own coefficients (docs/tried.md): no call of the host
 * layer takes it unless RABE_AW11_LEAD_W4 is set (rabe_aw11_decaps_packed, tools/bench_aw11_kem.py). */
int32_t rhip_aw11_decrypt_batch_w4(rhip_ctx* ctx, size_t n_items, size_t max_pairs, size_t total_pairs, size_t n_sel,
                                   const uint32_t* dev_pair_off /*[n_items+1]*/, const uint32_t* dev_sel_start /*[n_items]*/,
                                   const uint32_t* dev_sel_ct_row, const uint32_t* dev_sel_sk_attr, const rhip_fr* dev_sel_coeff,
                                   const rhip_gt* dev_ct_c0 /*[n_items]*/, const rhip_gt* dev_ct_c1, const rhip_g2* dev_ct_c2, const rhip_g2* dev_ct_c3,
                                   const uint32_t* dev_ct_row_off /*[n_items+1]*/, const rhip_g1* dev_sk_hash /*[n_sk]*/, const rhip_g1* dev_sk_k,
                                   const uint32_t* dev_sk_attr_off /*[n_sk+1]*/, const uint32_t* dev_sk_idx /*[n_items] or NULL*/,
                                   rhip_gt* dev_out /*[n_items]*/);

/* ---- Level S: the KEM -> DEM step and label hashing on the device (rabe_amd/csrc/engine_sym.hip) ------------------------------
 * Replaces, for batches, src/utils/aes/mod.rs:10-55 (`encrypt_symmetric` :10, `decrypt_symmetric` :29, `kdf` :47: key = SHA3-256(bytes(Gt)),
 * AES-256-GCM, sealed form = nonce(12) || ciphertext || tag(16)) and src/utils/hash/mod.rs:10-31 (`sha3_hash_fr`: Fr::from_slice(SHA3-256)).
 * The Gt of an encrypt / decrypt stays in HBM; only plaintext and record bytes cross PCIe.  No memory table is indexed by a secret
 * (the AES S-box lives in a register of the wave and is read through the lane crossbar).
 *
 * Offsets are byte offsets into the named blob; dev_len[i] = plaintext length of item i.  The host states the shape of the batch:
 * dev_blk_off[n+1] = prefix sums of ceil(len/16) (one lane per 16-byte block), dev_seg_off[n+1] = prefix sums of ceil(blocks/64) (GHASH runs
 * per 64-block segment, folded with powers of H).  dev_ws: rhip_seal_workspace_bytes(n, total_segments) bytes of device scratch. */
/* SHA3-256 (FIPS 202) of n byte strings data[off[i] .. off[i+1]); digests 32 bytes each */
int32_t rhip_sha3_256_batch(rhip_ctx* ctx, size_t n, const uint8_t* dev_data, const uint64_t* dev_off /*[n+1]*/, uint8_t* dev_digest /*[n][32]*/);
/* hash/mod.rs:23-31 sha3_hash_fr: the digest as a big-endian integer reduced mod r, canonical little-endian rhip_fr */
int32_t rhip_sha3_fr_batch(rhip_ctx* ctx, size_t n, const uint8_t* dev_data, const uint64_t* dev_off /*[n+1]*/, rhip_fr* dev_out /*[n]*/);
/* aes/mod.rs:47-55 kdf: key_i = SHA3-256(bytes(gt[idx ? idx[i] : i])), bytes = 12 coefficients as 32 big-endian bytes each */
int32_t rhip_gt_kdf_batch(rhip_ctx* ctx, size_t n, const rhip_gt* dev_gt, const uint32_t* dev_gt_idx /*[n] or NULL*/, uint8_t* dev_keys /*[n][32]*/);
/* The same KDF behind per-item verdicts (the ending of rabe_{ac17_cp,bsw}_decaps_packed): key_i = SHA3-256(bytes(gt[row[i]])) where
 * row[i] < n_gt, 32 zero bytes where it is not (RHIP_KDF_NO_ROW: the item failed) -- a failed item's slot never holds a key derived from
 * what its pairings left.  dev_gt must be a valid device pointer even when n_gt = 0. */
#define RHIP_KDF_NO_ROW 0xFFFFFFFFu
int32_t rhip_gt_kdf_rows(rhip_ctx* ctx, size_t n, const rhip_gt* dev_gt, size_t n_gt, const uint32_t* dev_row /*[n]*/, uint8_t* dev_keys /*[n][32]*/);
/* AES-256 (FIPS 197) of n blocks under n keys (known-answer tests) */
int32_t rhip_aes256_encrypt_blocks(rhip_ctx* ctx, size_t n, const uint8_t* dev_keys /*[n][32]*/, const uint8_t* dev_in /*[n][16]*/, uint8_t* dev_out /*[n][16]*/);
size_t rhip_seal_workspace_bytes(size_t n, size_t total_segments);
/* AES-256-GCM (SP 800-38D; 96-bit nonce, no AAD) with explicit keys.  seal != 0: in = plaintext at dev_in_off[i], out = nonce || ct || tag at
 * dev_out_off[i] (len_prefix != 0 also writes the u32 length len + 28 in the four bytes BEFORE it: the record's length field);
 * seal == 0: in = the sealed bytes at dev_in_off[i] (nonce read from there), out = plaintext at dev_out_off[i], dev_ok[i] = tag verified
 * (a failed item's plaintext bytes are zeros). */
int32_t rhip_aes256_gcm_batch(rhip_ctx* ctx, int32_t seal, size_t n, const uint8_t* dev_keys /*[n][32]*/, const uint8_t* dev_nonce /*[n][12], seal only*/,
                              const uint8_t* dev_in, const uint64_t* dev_in_off /*[n]*/, uint8_t* dev_out, const uint64_t* dev_out_off /*[n]*/,
                              const uint32_t* dev_len /*[n]*/, const uint32_t* dev_blk_off /*[n+1]*/, size_t total_blocks,
                              const uint32_t* dev_seg_off /*[n+1]*/, size_t total_segments, int32_t len_prefix, uint32_t* dev_ok /*[n], open only*/,
                              void* dev_ws);
/* n calls of encrypt_symmetric(gt_i, plaintext_i) with explicit nonces (the reference draws them from thread_rng, aes/mod.rs:17) */
int32_t rhip_seal_batch(rhip_ctx* ctx, size_t n, const rhip_gt* dev_gt /*[n]*/, const uint8_t* dev_nonce /*[n][12]*/, const uint8_t* dev_pt,
                        const uint64_t* dev_pt_off /*[n]*/, uint8_t* dev_out, const uint64_t* dev_sealed_off /*[n]*/, const uint32_t* dev_len /*[n]*/,
                        const uint32_t* dev_blk_off /*[n+1]*/, size_t total_blocks, const uint32_t* dev_seg_off /*[n+1]*/, size_t total_segments,
                        int32_t len_prefix, void* dev_ws);
/* n calls of decrypt_symmetric(gt[idx ? idx[i] : i], sealed_i); dev_len[i] = sealed length - 28 */
int32_t rhip_open_batch(rhip_ctx* ctx, size_t n, const rhip_gt* dev_gt, const uint32_t* dev_gt_idx /*[n] or NULL*/, const uint8_t* dev_blob,
                        const uint64_t* dev_sealed_off /*[n]*/, uint8_t* dev_pt, const uint64_t* dev_pt_off /*[n]*/, const uint32_t* dev_len /*[n]*/,
                        const uint32_t* dev_blk_off /*[n+1]*/, size_t total_blocks, const uint32_t* dev_seg_off /*[n+1]*/, size_t total_segments,
                        uint32_t* dev_ok /*[n]*/, void* dev_ws);
/* Records of a batch written from their parts on the device (the struct layouts of src/schemes/ac17/mod.rs:58-135 etc. in the canonical byte
 * form of rabe_obj_serialize): byte b of item i's record = dev_map[dev_layout_off[dev_layout[i]] + b], where a map word 0xFF0000vv is the
 * literal byte vv (policy text, names, counts -- one template per distinct policy) and k << 24 | o is byte o of item i's part in source
 * k: dev_src[k] + dev_src_item_off[k * n + i].  rhip_gather_parts is the reverse for a decrypt: part p of a layout copies dev_part_len[p]
 * bytes from record offset dev_part_src[p] to dev_dst[dev_part_k[p]] + dev_dst_item_off[k * n + i] + dev_part_dst[p]. */
int32_t rhip_assemble_records(rhip_ctx* ctx, size_t n, uint8_t* dev_out, const uint64_t* dev_out_off /*[n]*/, const uint32_t* dev_layout /*[n]*/,
                              const uint32_t* dev_layout_off, const uint32_t* dev_map, uint32_t n_src, const uint8_t* const* dev_src,
                              const uint64_t* dev_src_item_off /*[n_src][n]*/);
int32_t rhip_gather_parts(rhip_ctx* ctx, size_t n, const uint8_t* dev_blob, const uint64_t* dev_rec_off /*[n]*/, const uint32_t* dev_layout /*[n]*/,
                          const uint32_t* dev_layout_off, const uint32_t* dev_part_src, const uint32_t* dev_part_dst, const uint32_t* dev_part_len,
                          const uint32_t* dev_part_k, uint8_t* const* dev_dst, const uint64_t* dev_dst_item_off /*[n_dst][n]*/);

/* ---- measurement helper: integer-multiply issue-rate microbenchmark (the roofline denominator) --
 * Runs `iters` dependent-free v_mad_u64_u32 per lane on every CU and returns elapsed milliseconds
 * and the number of multiply-adds executed. */
int32_t rhip_calibrate_mad(rhip_ctx* ctx, int32_t variant, uint32_t iters, double* ms, double* n_ops);

#ifdef __cplusplus
}
#endif
#endif /* RABE_HIP_H */
