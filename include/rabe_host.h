/*
 * rabe_host.h -- C interface of the C++ host layer (rabe::schemes::* mirror, rabe_amd/csrc/host/).
 *
 * Same convention as the reference's own C FFI (src/ffi/bsw.rs:22-163): opaque object pointers created by
 * one call and destroyed by a paired free, int32 status, out-buffers returned through out-pointers.
 * Status: 0 ok; 1 = `None` (the reference returns Option::None: bsw::keygen :132-134, aw11::authgen :127-129);
 * -1 = RabeError (text via rabe_host_last_error); -2 = a condition on which the reference panics
 * (malformed policy shapes, unwrap on None).  Group arithmetic always runs on the HIP engine.
 */
#ifndef RABE_HOST_H
#define RABE_HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rabe_host rabe_host;

enum {   /* object kinds for rabe_obj_free / rabe_obj_serialize / rabe_obj_deserialize */
  RABE_AC17_PK = 1, RABE_AC17_MSK = 2, RABE_AC17_CP_SK = 3, RABE_AC17_CP_CT = 4, RABE_AC17_KP_SK = 5, RABE_AC17_KP_CT = 6,
  RABE_BSW_PK = 10, RABE_BSW_MSK = 11, RABE_BSW_SK = 12, RABE_BSW_CT = 13,
  RABE_LSW_PK = 20, RABE_LSW_MSK = 21, RABE_LSW_SK = 22, RABE_LSW_CT = 23,
  RABE_AW11_GK = 30, RABE_AW11_PK = 31, RABE_AW11_MSK = 32, RABE_AW11_SK = 33, RABE_AW11_CT = 34,
  RABE_GHW11_PK = 40, RABE_GHW11_MSK = 41, RABE_GHW11_SK = 42, RABE_GHW11_TK = 43, RABE_GHW11_RK = 44, RABE_GHW11_CT = 45, RABE_GHW11_TCT = 46,
  RABE_GHW11_TK_STORE = 47,   /* rabe_ghw11_tk_store_create's / _open's handle: rabe_obj_free only, no byte form */
  /* bdabe / mke08: public key, master key, secret AUTHORITY key, user key (with its attribute keys), public attribute key, ciphertext */
  RABE_BDABE_PK = 50, RABE_BDABE_MSK = 51, RABE_BDABE_SKA = 52, RABE_BDABE_UK = 53, RABE_BDABE_PKA = 54, RABE_BDABE_CT = 55,
  RABE_MKE08_PK = 60, RABE_MKE08_MSK = 61, RABE_MKE08_SKA = 62, RABE_MKE08_UK = 63, RABE_MKE08_PKA = 64, RABE_MKE08_CT = 65
};
enum { RABE_JSON_POLICY = 0, RABE_HUMAN_POLICY = 1 };   /* PolicyLanguage, src/utils/policy/pest/mod.rs:18-23 */

/* ABI revision of this header.  An argument list that changes keeps its symbol name only together with a bump of this number (revision 3
 * inserted ct_len and flags into the packed decrypts): a caller passes the revision it was COMPILED against -- rabe_host_open is the macro
 * for that -- and a library of another revision refuses with -3 instead of reading shifted arguments.  rabe_host_create does not check. */
#define RABE_HOST_ABI_VERSION 5
int32_t rabe_host_abi_version(void);
int32_t rabe_host_create_checked(int32_t abi_version, int32_t device, rabe_host** out);
#define rabe_host_open(device, out) rabe_host_create_checked(RABE_HOST_ABI_VERSION, (device), (out))
int32_t rabe_host_create(int32_t device, rabe_host** out);
/* ---- device group: ONE host over several GPUs of a node ----------------------------------------------------------------------
 * Every encrypt / keygen / decrypt call is independent (the reference's schemes are pure functions of their arguments and fresh
 * randomness), so a batch shards by item.  The SHARDED calls:
 *   the four BASELINE schemes: rabe_ac17_cp_encrypt_packed, rabe_ac17_cp_decrypt_packed, rabe_bsw_encrypt_packed, rabe_bsw_decrypt_packed,
 *     rabe_lsw_keygen_packed, rabe_lsw_decrypt_packed, rabe_lsw_decrypt_one_sk_packed, rabe_aw11_encrypt_packed, rabe_aw11_decrypt_packed;
 *   AC17 KP: rabe_ac17_kp_encrypt_packed, rabe_ac17_kp_decrypt_packed;
 *   the KEM pair of both schemes: rabe_ac17_cp_encaps_packed, rabe_ac17_cp_decaps_packed, rabe_bsw_encaps_packed, rabe_bsw_decaps_packed;
 *   the GHW11 KEM: rabe_ghw11_encaps_packed, rabe_ghw11_decaps_out_packed, rabe_ghw11_decaps_packed;
 *   the key-policy KEMs: rabe_ac17_kp_encaps_packed, rabe_ac17_kp_decaps_packed, rabe_lsw_decaps_packed;
 *   the AW11 KEM: rabe_aw11_encaps_packed, rabe_aw11_decaps_packed;
 *   the GHW11 service: rabe_ghw11_encrypt_packed, rabe_ghw11_transform_packed, rabe_ghw11_decrypt_out_packed, rabe_ghw11_decrypt_packed,
 *     rabe_ghw11_keygen_packed, rabe_ghw11_provision_packed, rabe_ghw11_transform_keyed (rabe_ghw11_tk_store_create itself runs on devices[0]);
 *   the DNF schemes' encrypt: rabe_bdabe_encrypt_packed, rabe_mke08_encrypt_packed;
 *   the DNF schemes' KEM: rabe_bdabe_kem_encaps, rabe_bdabe_kem_decaps, rabe_mke08_kem_encaps, rabe_mke08_kem_decaps.
 * Each cuts its n_items into one contiguous block per device (sizes differ by at most one, blocks in device order; fewer items than
 * devices: one item each for the first), runs every block on its own host thread with its engine's device current (each device builds its
 * replica of a key's window tables / prepared lines on first use and keeps it), and the records / plaintexts / fixed-size slots (the
 * 768-byte transform records, the 32-byte keys) / status entries land in the caller's buffers exactly where the single-device call puts them;
 * rabe_host_last_error is the first failing item's text in item order.  Randomness is drawn block after block from the host's one source
 * (rabe_ghw11_provision_packed: its two runs r_0 .., z_0 .. are drawn in that order before the blocks start), so on a tape
 * (rabe_host_set_tape) the bytes do not depend on the number of devices.  Every engine that held secrets zeroes its staging when the call
 * ends.  No data-path collective: the only exchange is the results arriving in host memory.  A device may be listed more than once (two
 * engines, i.e. two streams with their own workspaces, on one GPU) -- how a one-GPU box tests the split.
 * PLAINTEXT CAPACITY under a group: a decrypt-shaped call that is cut needs the total size of the well-formed records, not of their
 * sealed parts (every block is handed the slice its records span); see the calls' own comments.
 * NOT sharded, on devices[0]: rabe_ghw11_tkgen_packed (what it draws depends on which records decode on the host; the call is
 * host-bound), the bulk keygen_packed calls of ac17 / bsw / aw11 / bdabe / mke08, the request_*_sk_packed pair, rabe_bsw_delegate_packed,
 * rabe_lsw_encrypt_packed, rabe_lsw_encaps_packed, rabe_{bdabe,mke08}_decrypt_packed, the object API and the submission queue.
 * Status: as rabe_host_create_checked. */
int32_t rabe_host_open_group_checked(int32_t abi_version, size_t n_devices, const int32_t* devices, rabe_host** out);
#define rabe_host_open_group(n_devices, devices, out) rabe_host_open_group_checked(RABE_HOST_ABI_VERSION, (n_devices), (devices), (out))
int32_t rabe_host_group_size(rabe_host* h);          /* engines of the host: 1 for rabe_host_open */
/* out[k] = the number of items whose block has run to its end on engine k since the host was opened, over all sharded calls (cumulative; a
 * plain host counts the same calls in out[0]; a call that returns 1 for a short buffer counts nothing).  Shows that a node is in use -- and
 * the tests that a call was cut at all.  Returns the group size, or -1 when cap is smaller than that. */
int32_t rabe_host_group_items(rabe_host* h, uint64_t* out /*[cap]*/, size_t cap);
void rabe_host_destroy(rabe_host* h);
/* ---- submission queue: one call at a time, many callers ------------------------------------------------------------------------
 * The reference's API is one call per ciphertext (src/schemes/ac17/mod.rs:274-279, :385-388; rabe-console/src/mod.rs:1098, 1310) and one
 * call is one small launch set: milliseconds of latency for microseconds of chip time.  With the queue ON, the one-call encrypt / decrypt
 * entry points of ac17 (CP), bsw, lsw and aw11 below may be called from MANY THREADS on one rabe_host: calls that arrive while a batch is
 * running are collected and run as one packed batch (group commit: the batch grows with the load; window_us > 0 additionally holds every
 * batch open for that long).  Randomness is drawn in arrival order: one caller on a fixed tape gets the bytes of the unqueued path.
 * Errors of a threaded caller: rabe_host_last_error(NULL) (per thread).  Every other entry point stays single-owner.
 * The *_submit forms queue a call and return at once; rabe_ticket_wait blocks until the result is there (and may run the queued batch
 * itself -- there is no service thread), hands out the ciphertext object (encrypt) or the plaintext (decrypt, rabe_bytes_free) and frees
 * the ticket.  Key objects and, for decrypts, the ciphertext object must stay alive until the wait returns; plaintexts are copied. */
typedef struct rabe_ticket rabe_ticket;
int32_t rabe_host_set_coalescing(rabe_host* h, int32_t on, uint32_t window_us);
/* what the queue has done so far: batches run, requests in them, groups (= packed calls), requests that ran singly, microseconds spent
 * inside batches, largest batch */
int32_t rabe_host_queue_stats(rabe_host* h, uint64_t out[6]);
int32_t rabe_ac17_cp_encrypt_submit(rabe_host* h, const void* pk, const char* policy, int32_t language, const uint8_t* pt, size_t len, rabe_ticket** ticket);
int32_t rabe_ac17_cp_decrypt_submit(rabe_host* h, const void* sk, const void* ct, rabe_ticket** ticket);
int32_t rabe_bsw_encrypt_submit(rabe_host* h, const void* pk, const char* policy, int32_t language, const uint8_t* pt, size_t len, rabe_ticket** ticket);
int32_t rabe_bsw_decrypt_submit(rabe_host* h, const void* sk, const void* ct, rabe_ticket** ticket);
int32_t rabe_lsw_encrypt_submit(rabe_host* h, const void* pk, const char* const* attributes, size_t n, const uint8_t* pt, size_t len, rabe_ticket** ticket);
int32_t rabe_lsw_decrypt_submit(rabe_host* h, const void* sk, const void* ct, rabe_ticket** ticket);
int32_t rabe_aw11_encrypt_submit(rabe_host* h, const void* gk, const void* const* pks, size_t n_pks, const char* policy, int32_t language,
                                 const uint8_t* data, size_t len, rabe_ticket** ticket);
int32_t rabe_aw11_decrypt_submit(rabe_host* h, const void* gk, const void* sk, const void* ct, rabe_ticket** ticket);
int32_t rabe_ticket_wait(rabe_host* h, rabe_ticket* ticket, void** obj /*encrypt*/, uint8_t** out, size_t* len /*decrypt*/);
/* measurement helper: `threads` native host threads issue rabe_ac17_cp_encrypt + rabe_ac17_cp_decrypt one call at a time on this host
 * (depth 1), or keep `depth` submitted calls in flight each, for `seconds`; *ops = verified encrypt+decrypt cycles, *bad = the others */
int32_t rabe_bench_ac17_threads(rabe_host* h, const void* pk, const void* sk, const char* const* policies, size_t n_policies, int32_t language,
                                uint32_t threads, uint32_t depth, double seconds, uint64_t* ops, uint64_t* bad);
const char* rabe_host_last_error(rabe_host* h);          /* h may be NULL: error of the last host-free call on this thread */
/* Explicit randomness: the next calls draw their Fr values from this tape, in the reference's
 * draw order, instead of the OS generator.  n = 0 switches back to OS randomness. */
int32_t rabe_host_set_tape(rabe_host* h, const uint8_t* fr_le32, size_t n);

/* The per-kernel launch record of the host's own engine (include/rabe_hip.h: rhip_ctx_timing on the calling thread's lane, main stream): while
 * enabled every kernel launch there is timed; _read waits for the stream and drains the record as "kernel_name total_ms launches\n" lines
 * (truncated to len).  For measurements and for tests that assert WHICH kernels a call launched; launches on the side stream (the
 * membership pass) are not recorded. */
int32_t rabe_host_kernel_timing(rabe_host* h, int32_t enable);
int32_t rabe_host_kernel_timing_read(rabe_host* h, char* buf, size_t len);

/* G*Fr / Gt^Fr elements that share one base are served from a cached fixed-base window table once n of them have been seen,
 * in one call or accumulated over calls (default 1024); the results do not depend on it.  Tests set 1 / SIZE_MAX to force
 * either path. */
int32_t rabe_host_set_fixed_base_min(rabe_host* h, size_t n);

void rabe_obj_free(int32_t kind, void* obj);
/* canonical byte form of a key / ciphertext (layout: rabe_amd/csrc/host/host_abi.cpp); free with rabe_bytes_free */
int32_t rabe_obj_serialize(int32_t kind, const void* obj, uint8_t** out, size_t* len);
int32_t rabe_obj_deserialize(int32_t kind, const uint8_t* data, size_t len, void** obj);
/* rabe_obj_deserialize checks structure and ranges (lengths of the fixed-size AC17 vectors, scalars < r, coordinates < p);
 * the _checked form additionally establishes group membership of every element on the GPU (G1 on the curve, G2 in the r-torsion
 * of the twist, Gt in the order-r subgroup): use it for keys / ciphertexts that arrive from outside */
int32_t rabe_obj_deserialize_checked(rabe_host* h, int32_t kind, const uint8_t* data, size_t len, void** obj);
void rabe_bytes_free(void* p);

/* ---- ac17 (src/schemes/ac17/mod.rs:141-430) */
int32_t rabe_ac17_setup(rabe_host* h, void** pk, void** msk);
int32_t rabe_ac17_cp_keygen(rabe_host* h, const void* msk, const char* const* attributes, size_t n, void** sk);
int32_t rabe_ac17_cp_encrypt(rabe_host* h, const void* pk, const char* policy, int32_t language, const uint8_t* plaintext, size_t len, void** ct);
int32_t rabe_ac17_cp_decrypt(rabe_host* h, const void* sk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_ac17_cp_decrypt_gt(rabe_host* h, const void* sk, const void* ct, uint8_t out_gt[384]);
/* n independent cp_encrypt calls in one launch set; cts receives n object pointers */
int32_t rabe_ac17_cp_encrypt_batch(rabe_host* h, const void* pk, size_t n, const char* const* policies, int32_t language,
                                   const uint8_t* const* plaintexts, const size_t* lens, void** cts);
/* n independent cp_decrypt calls; status[i] = 0 ok / -1 error; plaintexts[i] malloc'd (rabe_bytes_free) */
int32_t rabe_ac17_cp_decrypt_batch(rabe_host* h, size_t n, const void* const* sks, const void* const* cts, int32_t* status,
                                   uint8_t** plaintexts, size_t* lens);
/* The same two batches with packed input and output -- no per-item objects on either side of the boundary, every buffer
 * caller-allocated (and reusable across calls).  Ciphertexts are ONE blob of canonical records (the byte form rabe_obj_serialize
 * gives an Ac17CpCiphertext) delimited by an offset array of n_items + 1 entries; plaintexts likewise.
 *   encrypt: item i uses policies[item_policy[i]] (distinct policy texts are parsed once, and cached across calls).  ct_off is
 *            always filled; return 1 (nothing done, no randomness drawn) when ct_cap < ct_off[n_items], the size the records need.
 *   decrypt: status[i] = 0 / -1 per item (a key that does not satisfy a policy, a malformed record or an authentication failure
 *            fails that item only; its plaintext is empty).  pt_cap >= the sum of the sizes of the records whose bounds are valid always suffices (<= ct_len unless records overlap);
 *            return 1 when it is smaller. */
int32_t rabe_ac17_cp_encrypt_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                                    const uint32_t* item_policy /*[n_items]*/, const uint8_t* pt_blob, const uint64_t* pt_off /*[n_items+1]*/,
                                    uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off /*[n_items+1]*/);
/* decrypt reads UNTRUSTED bytes: ct_len is the size of ct_blob, and ct_off must be monotone inside it (an item whose bounds are not
 * fails alone with status -1; nothing outside [0, ct_len) is read).  Unless RABE_PACKED_TRUSTED is set in `flags`, every decoded element
 * goes through one batched membership pass on the GPU -- coordinates < p, rows on the G1 curve, c_0 in the r-torsion of the twist, c_p in
 * the order-r subgroup of Fq12 (rabe-bn: FieldError::NotMember) -- and a non-member fails its item only.  Set the flag only for
 * ciphertexts this process produced itself. */
#define RABE_PACKED_TRUSTED 1u
/* Environment of the packed entry points (read per call; defaults are what the measurements in DESIGN.md section 7 favour):
 *   RABE_PACKED_CHUNK   cut a packed call into chunks of at least this many items that run RABE_PACKED_LANES (default 2) at a time, each on
 *                       its own engine lane; off by default -- measured no faster than one launch set once the unchunked call was tuned
 *   RABE_MEMBER_INLINE  run the decoding checks on the main stream before the kernels instead of beside them (A/B)
 *   RABE_G_WINDOW       signed window width of AC17's g table in this layer (default 20 = +0.44 GB per public key; 16 = none extra)
 *   RABE_NO_ARENA       every device buffer of a call its own hipMalloc again (diagnostics)
 *   RABE_ARENA_MAX_GB   cap of the grow-only device block a lane keeps between packed calls (default 16)
 *   RABE_HOST_TIMING    stage timings on stderr
 * Results never depend on any of them. */
/* A key authority issuing keys in bulk: n_items calls of ac17::cp_keygen (src/schemes/ac17/mod.rs:191-264) under one master key.  The
 * attribute lists are given once (n_sets lists, list s = the next counts[s] entries of `attributes`), item i gets list item_set[i].
 * sk_buf receives the Ac17CpSecretKey records (sk_off: n_items + 1 offsets, always filled; returns 1 when sk_cap is too small, before any
 * randomness is drawn).  Items that share a list are one launch of the Level B keygen kernels; the master key's window tables are kept. */
int32_t rabe_ac17_cp_keygen_packed(rabe_host* h, const void* msk, const char* const* attributes, const size_t* counts, size_t n_sets, size_t n_items,
                                   const uint32_t* item_set /*[n_items]*/, uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off /*[n_items+1]*/);
int32_t rabe_ac17_cp_decrypt_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                    const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* pt_buf,
                                    size_t pt_cap, uint64_t* pt_off /*[n_items+1]*/);

/* ---- key encapsulation: the packed pair WITHOUT payloads.  A caller that seals large objects where they live (files, streams, rows) wants per
 * item the ciphertext HEADER and the 32-byte content key the reference's kdf derives (src/utils/aes/mod.rs:47-55), and on the other side the same
 * 32 bytes back from the header and a secret key.  Not functions of the reference but compositions of functions that are (as
 * rabe_ghw11_provision_packed is).  Built for ac17 (CP) and bsw here, for ac17 (KP), lsw and ghw11 below; all four calls are sharded over a device group (a block's headers at their
 * offsets, its keys and verdicts at key_buf + 32 lo and status + lo).
 *   key = SHA3-256(bytes(Gt)): bytes(Gt) is the byte form the reference's kdf hashes -- the 12 coefficients in wire order, each as 32 BIG-endian
 *   bytes -- i.e. exactly the AES key rabe_encrypt_symmetric / rabe_decrypt_symmetric derive from that Gt.
 * ENCAPS.  Item i's header at hdr_buf + hdr_off[i] is the Ac17CpCiphertext record rabe_ac17_cp_encrypt_packed writes for the same draws with a
 *   sealed part of length ZERO: the record's length field is 0 and no nonce, ciphertext or tag follows.  key_buf + 32 i = SHA3-256(bytes(msg_i)).
 *   DRAW ORDER: rabe_ac17_cp_encrypt_packed's minus the AES nonce -- per item s0, s1, msg -- so a tape that drives encrypt_packed with the nonce
 *   draws removed drives encaps_packed.  hdr_off is always filled; returns 1, with nothing drawn and nothing written, when
 *   hdr_cap < hdr_off[n_items].  Arguments otherwise as rabe_ac17_cp_encrypt_packed.  The record-assembly template ends in the zero length field
 *   and takes no sealed source; the keys come from the KDF kernel alone (rhip_gt_kdf_batch straight out of the msg array): no AES context, CTR,
 *   GHASH or tag kernel is launched.  The staging that held the scalars, msg and the keys is zeroed, host and device, when the call ends.
 * DECAPS.  key_buf + 32 i = SHA3-256(bytes(X)) where X is what rabe_ac17_cp_decrypt_gt(sk, record i) returns, for ANY well-formed
 *   Ac17CpCiphertext record, whatever its sealed part: headers from encaps and full records from rabe_ac17_cp_encrypt_packed are both valid input.
 *   The sealed bytes are skipped by their length field (which must lie inside the record); they are not read and NOT authenticated.  An item
 *   fails alone -- status[i] = -1, 32 zero bytes in its slot, the first error in rabe_host_last_error: bad bounds, a malformed record, a
 *   non-member element unless RABE_PACKED_TRUSTED, a key that does not satisfy the policy.  Nothing outside [0, ct_len) is read; no randomness
 *   is drawn.  The launch set is rabe_ac17_cp_decrypt_packed's up to the final Gt (one upload of the blob, the cached plans and prepared key
 *   lines); its ending is the KDF behind the verdict mask (rhip_gt_kdf_rows: a failed item's key is never computed) and one download of
 *   32 n_items bytes -- no gather of sealed parts, no open.
 * THE EXISTING PARSERS and the empty sealed part: rabe_obj_deserialize and the packed decrypts already ACCEPT a record whose sealed part is
 *   empty -- the length field is read and the bytes it announces must lie inside the record -- and fail such a record only later, at the tag
 *   ("decryption error: aead::Error": nonce + tag need 28 bytes).  They are unchanged; decaps parses with the same code and stops before the tag. */
int32_t rabe_ac17_cp_encaps_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                                   const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap, uint64_t* hdr_off /*[n_items+1]*/,
                                   uint8_t* key_buf /*32 n_items*/);
int32_t rabe_ac17_cp_decaps_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                   const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);

/* KP-ABE variant (src/schemes/ac17/mod.rs:439-675) */
int32_t rabe_ac17_kp_keygen(rabe_host* h, const void* msk, const char* policy, int32_t language, void** sk);
/* n_items calls of ac17::kp_keygen (src/schemes/ac17/mod.rs:439-547) under one master key, item i under policies[item_policy[i]]: the triple
 * loop over rows x columns x (l, t) (:479-538) is Fr work on all host cores, the 3 rows + 3 elements per key are ONE fixed-base launch set,
 * the records (Ac17KpSecretKey: policy, k_0, rows, an empty k_p) are written on the device.  Buffers / return value as
 * rabe_ac17_cp_keygen_packed (1 = sk_cap too small, sk_off[n_items] says what is needed). */
int32_t rabe_ac17_kp_keygen_packed(rabe_host* h, const void* msk, const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                                   const uint32_t* item_policy /*[n_items]*/, uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off /*[n_items+1]*/);
int32_t rabe_ac17_kp_encrypt(rabe_host* h, const void* pk, const char* const* attributes, size_t n, const uint8_t* data, size_t len, void** ct);
int32_t rabe_ac17_kp_decrypt(rabe_host* h, const void* sk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_ac17_kp_decrypt_gt(rabe_host* h, const void* sk, const void* ct, uint8_t out_gt[384]);
/* The KP pair packed (conventions of rabe_ac17_cp_{encrypt,decrypt}_packed; records = Ac17KpCiphertext): n_items encrypts, item i under the
 * attribute list item_set[i] of the n_sets lists given once (list s = the next counts[s] entries of `attributes`); n_items decrypts
 * with ONE key (whose policy is checked against every ciphertext's attribute list).  Same kernels as the CP pair
 * (src/schemes/ac17/mod.rs:556-675).  The decrypt returns 1 when pt_cap is below the total size of the well-formed records -- one engine or
 * a device group alike; for this call the two sizes coincide.  A group that cuts the batch needs the total size of the well-formed
 * records, not of their sealed parts: the call returns 1, and pt_off[n_items] holds the size to come back with. */
int32_t rabe_ac17_kp_encrypt_packed(rabe_host* h, const void* pk, const char* const* attributes, const size_t* counts, size_t n_sets, size_t n_items,
                                    const uint32_t* item_set /*[n_items]*/, const uint8_t* pt_blob, const uint64_t* pt_off /*[n_items+1]*/,
                                    uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off /*[n_items+1]*/);
int32_t rabe_ac17_kp_decrypt_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                    const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* pt_buf, size_t pt_cap,
                                    uint64_t* pt_off /*[n_items+1]*/);
/* Key encapsulation for the KP pair: everything said at rabe_ac17_cp_{encaps,decaps}_packed, with Ac17KpCiphertext records,
 * rabe_ac17_kp_encrypt_packed / rabe_ac17_kp_decrypt_packed as the calls composed (their arguments minus the payloads, plus key_buf) and
 * rabe_ac17_kp_decrypt_gt as the definition of X.  ENCAPS DRAW ORDER: rabe_ac17_kp_encrypt_packed's minus the AES nonce -- per item s0, s1,
 * msg.  The kernels are the CP pair's.  Both calls are cut over a device group where the calls they compose are cut. */
int32_t rabe_ac17_kp_encaps_packed(rabe_host* h, const void* pk, const char* const* attributes, const size_t* counts, size_t n_sets, size_t n_items,
                                   const uint32_t* item_set /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap, uint64_t* hdr_off /*[n_items+1]*/,
                                   uint8_t* key_buf /*32 n_items*/);
int32_t rabe_ac17_kp_decaps_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                   const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);
/* n independent kp_encrypt / kp_decrypt calls in one launch set; item i's attributes are the next counts[i] entries of `attributes` */
int32_t rabe_ac17_kp_encrypt_batch(rabe_host* h, const void* pk, size_t n, const char* const* attributes, const size_t* counts,
                                   const uint8_t* const* datas, const size_t* lens, void** cts);
int32_t rabe_ac17_kp_decrypt_batch(rabe_host* h, size_t n, const void* const* sks, const void* const* cts, int32_t* status,
                                   uint8_t** plaintexts, size_t* lens);

/* ---- bsw (src/schemes/bsw/mod.rs:92-318) */
int32_t rabe_bsw_setup(rabe_host* h, void** pk, void** msk);
int32_t rabe_bsw_keygen(rabe_host* h, const void* pk, const void* msk, const char* const* attributes, size_t n, void** sk);
int32_t rabe_bsw_delegate(rabe_host* h, const void* pk, const void* sk, const char* const* subset, size_t n, void** out_sk);
int32_t rabe_bsw_encrypt(rabe_host* h, const void* pk, const char* policy, int32_t language, const uint8_t* plaintext, size_t len, void** ct);
int32_t rabe_bsw_decrypt(rabe_host* h, const void* sk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_bsw_decrypt_gt(rabe_host* h, const void* sk, const void* ct, uint8_t out_gt[384]);
/* n independent encrypt / decrypt calls, the group work of all items in one launch per operation type
 * (BASELINE config 3); conventions as rabe_ac17_cp_{encrypt,decrypt}_batch */
int32_t rabe_bsw_encrypt_batch(rabe_host* h, const void* pk, size_t n, const char* const* policies, int32_t language,
                               const uint8_t* const* plaintexts, const size_t* lens, void** cts);
int32_t rabe_bsw_decrypt_batch(rabe_host* h, size_t n, const void* const* sks, const void* const* cts, int32_t* status,
                               uint8_t** plaintexts, size_t* lens);
/* The same two batches packed (conventions of rabe_ac17_cp_{encrypt,decrypt}_packed: one blob of canonical CpAbeCiphertext records +
 * n_items + 1 offsets per side, caller-allocated buffers, per-item status, ct_len / RABE_PACKED_TRUSTED for untrusted input).  These
 * feed the device-resident path (rhip_bsw_{encrypt,decrypt}_batch): share generation, fixed-base multiplications, the folded
 * pairing product and one final exponentiation per item all happen on HBM-resident arrays (src/schemes/bsw/mod.rs:217-318). */
/* Bulk key issuing for bsw (conventions of rabe_ac17_cp_keygen_packed): n_items calls of bsw::keygen (src/schemes/bsw/mod.rs:125-152) under one
 * master key, records = CpAbeSecretKey.  Every key element is a fixed-base multiple of a generator (d = g2_alpha/beta + g2*(r/beta)):
 * three window-table launches for the whole batch.  An empty attribute list (for which bsw::keygen returns None) fails the call. */
int32_t rabe_bsw_keygen_packed(rabe_host* h, const void* pk, const void* msk, const char* const* attributes, const size_t* counts, size_t n_sets,
                               size_t n_items, const uint32_t* item_set /*[n_items]*/, uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off /*[n_items+1]*/);
/* n_items calls of bsw::delegate (src/schemes/bsw/mod.rs:162-206) on ONE key: item i delegates `sk` to the attribute list item_subset[i] of the
 * n_subsets lists given once (flattened in `attributes`, `counts` each).  d' = d + f * r, rows D_j + (g1 * r_j, g2 * (h(j) r_j + r)): window-table
 * launches and batched additions for the whole batch, records (CpAbeSecretKey) written on the device.  A subset that is empty or not contained
 * in the key (delegate returns None) fails the call; buffers / return value as rabe_bsw_keygen_packed. */
int32_t rabe_bsw_delegate_packed(rabe_host* h, const void* pk, const void* sk, const char* const* attributes, const size_t* counts, size_t n_subsets,
                                 size_t n_items, const uint32_t* item_subset /*[n_items]*/, uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off /*[n_items+1]*/);
int32_t rabe_bsw_encrypt_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                                const uint32_t* item_policy /*[n_items]*/, const uint8_t* pt_blob, const uint64_t* pt_off /*[n_items+1]*/,
                                uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off /*[n_items+1]*/);
int32_t rabe_bsw_decrypt_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* pt_buf, size_t pt_cap,
                                uint64_t* pt_off /*[n_items+1]*/);
/* Key encapsulation for bsw: everything said at rabe_ac17_cp_{encaps,decaps}_packed, with CpAbeCiphertext records, rabe_bsw_encrypt_packed /
 * rabe_bsw_decrypt_packed as the calls composed and rabe_bsw_decrypt_gt as the definition of X.  ENCAPS DRAW ORDER: rabe_bsw_encrypt_packed's
 * minus the AES nonce -- per item secret, msg, the gate coefficients of gen_shares_policy.  The existing parser accepts an empty sealed part
 * here too and fails it at the tag; it is unchanged. */
int32_t rabe_bsw_encaps_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                               const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap, uint64_t* hdr_off /*[n_items+1]*/,
                               uint8_t* key_buf /*32 n_items*/);
int32_t rabe_bsw_decaps_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                               const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);

/* ---- lsw (src/schemes/lsw/mod.rs:86-290) */
int32_t rabe_lsw_setup(rabe_host* h, void** pk, void** msk);
int32_t rabe_lsw_keygen(rabe_host* h, const void* pk, const void* msk, const char* policy, int32_t language, void** sk);
int32_t rabe_lsw_encrypt(rabe_host* h, const void* pk, const char* const* attributes, size_t n, const uint8_t* plaintext, size_t len, void** ct);
int32_t rabe_lsw_decrypt(rabe_host* h, const void* sk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_lsw_decrypt_gt(rabe_host* h, const void* sk, const void* ct, uint8_t out_gt[384]);
/* BASELINE config 4: n keygen / decrypt calls in one launch set */
int32_t rabe_lsw_keygen_batch(rabe_host* h, const void* pk, const void* msk, size_t n, const char* const* policies, int32_t language, void** sks);
int32_t rabe_lsw_decrypt_batch(rabe_host* h, size_t n, const void* const* sks, const void* const* cts, int32_t* status,
                               uint8_t** plaintexts, size_t* lens);
/* Packed forms over the device-resident path (rhip_lsw_{keygen,decrypt}_batch; src/schemes/lsw/mod.rs:121-290): keygen writes n
 * KpAbeSecretKey records (item i's policy = policies[item_policy[i]]) into one caller-allocated blob; decrypt takes n such records
 * and ONE ciphertext object (BASELINE config 4) and returns n plaintexts.  Size / status / ct_len / RABE_PACKED_TRUSTED conventions as
 * rabe_ac17_cp_{encrypt,decrypt}_packed.  keygen handles negative leaves ("!x", lsw/mod.rs:137-146) on the device as well; a decrypt
 * whose pruned selection reaches a negative attribute fails that item -- the reference's own decrypt has no negative branch (a TODO,
 * :265-278), and rabe_lsw_decrypt reproduces what it does instead. */
/* n_items calls of lsw::encrypt (src/schemes/lsw/mod.rs:180-219), item i under the attribute list item_set[i] of the n_sets lists given once;
 * records = KpAbeCiphertext (conventions of rabe_ac17_cp_encrypt_packed).  Every element is a fixed-base multiple of a public-key element
 * (the reference's sx[0] index quirk :197-200 included): window-table launches for the whole batch. */
int32_t rabe_lsw_encrypt_packed(rabe_host* h, const void* pk, const char* const* attributes, const size_t* counts, size_t n_sets, size_t n_items,
                                const uint32_t* item_set /*[n_items]*/, const uint8_t* pt_blob, const uint64_t* pt_off /*[n_items+1]*/,
                                uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off /*[n_items+1]*/);
int32_t rabe_lsw_keygen_packed(rabe_host* h, const void* pk, const void* msk, const char* const* policies, size_t n_policies, int32_t language,
                               size_t n_items, const uint32_t* item_policy /*[n_items]*/, uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off /*[n_items+1]*/);
int32_t rabe_lsw_decrypt_packed(rabe_host* h, const void* ct, size_t n_items, const uint8_t* sk_blob, size_t sk_len,
                                const uint64_t* sk_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* pt_buf, size_t pt_cap,
                                uint64_t* pt_off /*[n_items+1]*/);
/* The shape of a KP-ABE key holder: ONE key of the holder's own against n_items ciphertexts from outside -- KpAbeCiphertext records as
 * rabe_obj_serialize writes them and rabe_lsw_encrypt_packed emits them (conventions of rabe_bsw_decrypt_packed: nothing outside
 * [0, ct_len) is read; bad bounds, a malformed record, attributes that do not satisfy the key's policy, a tag that does not verify fail
 * that item alone: status -1, an empty plaintext slot, the first error in rabe_host_last_error).  Over rhip_lsw_decrypt_batch_one_sk: the
 * key-side Miller loops replay the key's prepared lines (built once per key and engine), sum_e -c_e D1_e is computed once per distinct
 * list of row names, the sealed parts are opened on the device.  Records that list the same names in the same order share one plan
 * (calc_pruned + coefficients, the reference's FIRST-row lookups :249-263); another order or a duplicated name is a list of its own.
 * Unless RABE_PACKED_TRUSTED is set every decoded element is checked: e1 in Gt, the row elements on the G1 curve with canonical
 * coordinates, e2 in G2 (out of its own Miller loop, or the stand-alone test).  A selected negative attribute fails the item as in
 * rabe_lsw_decrypt_packed.  No randomness is drawn.  Returns 1 when pt_cap is below the total of the well-formed records' sealed
 * lengths (a device group that cuts the batch: below their total record size); pt_off[n_items] then holds the size to come back with. */
int32_t rabe_lsw_decrypt_one_sk_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                       const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/,
                                       uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off /*[n_items+1]*/);
/* Key encapsulation for lsw: everything said at rabe_ac17_cp_{encaps,decaps}_packed about the format, the key, the failure of an item alone,
 * RABE_PACKED_TRUSTED, the bounds and the scrubbed staging, with KpAbeCiphertext records and rabe_lsw_decrypt_gt as the definition of X.
 * ENCAPS: arguments of rabe_lsw_encrypt_packed minus the payloads, plus key_buf.  Header i is the record rabe_lsw_encrypt_packed writes for the
 *   same draws with a sealed part of length zero.  DRAW ORDER: rabe_lsw_encrypt_packed's minus the AES nonce -- per item secret, one sx per
 *   attribute, the msg exponent.  The attribute rows come from ONE fused kernel (rhip_lsw_encrypt_rows: one lane per row, the products
 *   h secret and sx h formed on the device, 32 uploaded bytes per row, one inversion per block) where rabe_lsw_encrypt_packed runs four table
 *   launches and an addition; the bytes are the same.  e1 and e2 keep their table calls; no AES kernel is launched.  Like
 *   rabe_lsw_encrypt_packed the call is NOT cut over a device group: it runs on the group's first device.
 * DECAPS: ONE key of the holder's own against n_items records, arguments of rabe_lsw_decrypt_one_sk_packed with key_buf in place of the
 *   plaintext buffers.  Headers and full records are both valid input.  The launch set is rabe_lsw_decrypt_one_sk_packed's up to the final Gt
 *   (shared plans per list of row names, the key's prepared lines, the membership checks), then the KDF behind the verdict mask and one
 *   download of 32 n_items bytes.  A selected negative attribute fails the item.  Cut over a device group as rabe_lsw_decrypt_one_sk_packed is. */
int32_t rabe_lsw_encaps_packed(rabe_host* h, const void* pk, const char* const* attributes, const size_t* counts, size_t n_sets, size_t n_items,
                               const uint32_t* item_set /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap, uint64_t* hdr_off /*[n_items+1]*/,
                               uint8_t* key_buf /*32 n_items*/);
int32_t rabe_lsw_decaps_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                               const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);

/* ---- aw11 (src/schemes/aw11/mod.rs:100-390) */
int32_t rabe_aw11_setup(rabe_host* h, void** gk);
int32_t rabe_aw11_authgen(rabe_host* h, const void* gk, const char* const* attributes, size_t n, void** pk, void** msk);
int32_t rabe_aw11_keygen(rabe_host* h, const void* gk, const void* msk, const char* name, const char* const* attributes, size_t n, void** sk);
int32_t rabe_aw11_add_to_attribute(rabe_host* h, const void* gk, const void* msk, const char* attribute, void* sk);
int32_t rabe_aw11_encrypt(rabe_host* h, const void* gk, const void* const* pks, size_t n_pks, const char* policy, int32_t language,
                          const uint8_t* data, size_t len, void** ct);
int32_t rabe_aw11_decrypt(rabe_host* h, const void* gk, const void* sk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_aw11_decrypt_gt(rabe_host* h, const void* gk, const void* sk, const void* ct, uint8_t out_gt[384]);
/* BASELINE config 5: n encrypt / decrypt calls in one launch set (all items encrypt under the same authority keys) */
int32_t rabe_aw11_encrypt_batch(rabe_host* h, const void* gk, const void* const* pks, size_t n_pks, size_t n, const char* const* policies,
                                int32_t language, const uint8_t* const* datas, const size_t* lens, void** cts);
int32_t rabe_aw11_decrypt_batch(rabe_host* h, const void* gk, size_t n, const void* const* sks, const void* const* cts, int32_t* status,
                                uint8_t** plaintexts, size_t* lens);
/* Packed forms over the device-resident path (rhip_aw11_{encrypt,decrypt}_batch; src/schemes/aw11/mod.rs:241-366), conventions as
 * rabe_ac17_cp_{encrypt,decrypt}_packed.  Every policy leaf must name an attribute of one of the authority keys (the reference drops
 * other rows silently, :269-271; rabe_aw11_encrypt reproduces that). */
/* Bulk key issuing by one authority (conventions of rabe_ac17_cp_keygen_packed): n_items calls of aw11::keygen (src/schemes/aw11/mod.rs:165-231),
 * user gids[i] gets the attribute list item_set[i]; records = Aw11SecretKey.  No randomness: K_x = g1 * (alpha_x + h(gid) y_x), one
 * window-table launch for the whole batch. */
int32_t rabe_aw11_keygen_packed(rabe_host* h, const void* gk, const void* msk, const char* const* gids /*[n_items]*/, const char* const* attributes,
                                const size_t* counts, size_t n_sets, size_t n_items, const uint32_t* item_set /*[n_items]*/, uint8_t* sk_buf, size_t sk_cap,
                                uint64_t* sk_off /*[n_items+1]*/);
int32_t rabe_aw11_encrypt_packed(rabe_host* h, const void* gk, const void* const* pks, size_t n_pks, const char* const* policies, size_t n_policies,
                                 int32_t language, size_t n_items, const uint32_t* item_policy /*[n_items]*/, const uint8_t* pt_blob,
                                 const uint64_t* pt_off /*[n_items+1]*/, uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off /*[n_items+1]*/);
int32_t rabe_aw11_decrypt_packed(rabe_host* h, const void* gk, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                 const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* pt_buf, size_t pt_cap,
                                 uint64_t* pt_off /*[n_items+1]*/);
/* Key encapsulation for aw11: everything said at rabe_ac17_cp_{encaps,decaps}_packed about the format, the key, the failure of an item alone
 * (status -1 and 32 zero bytes: bounds, membership unless RABE_PACKED_TRUSTED, a key that lacks the attributes), the bounds and the scrubbed
 * staging, with Aw11Ciphertext records and rabe_aw11_decrypt_gt as the definition of X.  Compositions: the reference has neither function.
 * ENCAPS: arguments of rabe_aw11_encrypt_packed minus the payloads, plus key_buf.  Header i is the record rabe_aw11_encrypt_packed writes for
 *   the same draws with a sealed part of length zero; key i = SHA3-256(bytes(msg_i)).  DRAW ORDER: rabe_aw11_encrypt_packed's minus the AES
 *   nonce -- per item s, the gate coefficients of the s-shares then of the 0-shares, msg, one r_x per share.  No AES kernel is launched.
 * DECAPS: ONE key against n_items records, arguments of rabe_aw11_decrypt_packed with key_buf in place of the plaintext buffers.  Headers and
 *   full records are both valid input; the sealed part is neither read nor authenticated.  The launch set is rabe_aw11_decrypt_packed's up to
 *   the final Gt -- parsing, membership passes, selection, k_aw11_dec_pairs, the G2 sum, the leading factor and the pairings unchanged -- then
 *   the KDF behind the verdict mask and one download of 32 n_items bytes.  No Gt element crosses PCIe.  The leading factor
 *   c_0 * prod C1_e^(-c_e) over width-4 windows (rhip_aw11_decrypt_batch_w4, the kernels of rhip_gt_multiexp_rows) was built for this call and
 *   measured SLOWER on this scheme's coefficients (products of 2 and -1: docs/tried.md), so k_gt_multiexp_partial + k_gt_lead stay; the
 *   environment variable RABE_AW11_LEAD_W4 puts the windowed routine in their place for measurements (same keys).
 * Both calls are cut over a device group where the calls they compose are cut. */
int32_t rabe_aw11_encaps_packed(rabe_host* h, const void* gk, const void* const* pks, size_t n_pks, const char* const* policies, size_t n_policies,
                                int32_t language, size_t n_items, const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap,
                                uint64_t* hdr_off /*[n_items+1]*/, uint8_t* key_buf /*32 n_items*/);
int32_t rabe_aw11_decaps_packed(rabe_host* h, const void* gk, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);

/* ---- ghw11, CP-ABE with outsourced decryption (src/schemes/ghw11/mod.rs:92-305): `transform` is the server's part
 * (m + 2 pairings per ciphertext), `decrypt_out` the client's (one Gt power) */
int32_t rabe_ghw11_setup(rabe_host* h, void** pk, void** msk);
int32_t rabe_ghw11_keygen(rabe_host* h, const void* pk, const void* msk, const char* const* attributes, size_t n, void** sk);
int32_t rabe_ghw11_tkgen(rabe_host* h, const void* sk, void** tk, void** rk);
int32_t rabe_ghw11_encrypt(rabe_host* h, const void* pk, const char* policy, int32_t language, const uint8_t* plaintext, size_t len, void** ct);
int32_t rabe_ghw11_transform(rabe_host* h, const void* ct, const void* tk, void** tct);
/* n independent transforms in one launch set; status[i] = 0 ok / -1 (tk i does not satisfy ct i; tcts[i] = NULL) */
int32_t rabe_ghw11_transform_batch(rabe_host* h, size_t n, const void* const* cts, const void* const* tks, int32_t* status, void** tcts);
/* n_items calls of encrypt (ghw11/mod.rs:189-225) in the form of rabe_bsw_encrypt_packed: item i encrypts plaintext i of pt_blob under
 * policies[item_policy[i]]; ct_buf receives the Ghw11Ciphertext records (rabe_obj_serialize's bytes), built and sealed on the device (one lane
 * per ciphertext row: share, C on one accumulator over the tables of g1_a and g1, D).  Draw order per item: secret, msg, gate coefficients,
 * one t per share in share order, AES nonce.  Returns 1 when ct_cap is too small; ct_off[n_items] = the size needed. */
int32_t rabe_ghw11_encrypt_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language,
                                  size_t n_items, const uint32_t* item_policy /*[n_items]*/, const uint8_t* pt_blob, const uint64_t* pt_off /*[n_items+1]*/,
                                  uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off /*[n_items+1]*/);
/* The outsourced half as a service: n_items Ghw11Ciphertext records in one blob (+ n_items + 1 offsets, ct_len; bounds and --
 * unless RABE_PACKED_TRUSTED -- group membership of every decoded element are checked, an item fails alone with status -1) transformed under
 * ONE transform key.  tct_buf + 768 i receives item i's Ghw11TransformCiphertext record (c | t; zeros where status[i] = -1); returns 1 when
 * tct_cap < 768 n_items.  Under a device group a block writes its slots and verdicts in place (tct_buf + 768 lo, status + lo).  Device-resident: every G2 argument is the key's, so all m + 2 Miller loops of an item replay the key's prepared
 * lines (kept across calls) and the rows that share l_z collapse into one pairing of a multi-scalar sum (ghw11/mod.rs:227-295).
 * The sealed part of a record is skipped by its length field and never read: the headers rabe_ghw11_encaps_packed writes (an empty sealed
 * part) pass through this call as full records do, with the same 768-byte output. */
int32_t rabe_ghw11_transform_packed(rabe_host* h, const void* tk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                    const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* tct_buf, size_t tct_cap);
/* ---- the proxy's call for a MIXED queue: a device-resident store of many users' transform keys, and a batch in which item i belongs to
 * user item_key[i].  (rabe_ghw11_transform_packed serves a batch under ONE key: a queue sorted by user becomes one small launch set per user.)
 * STORE: tk_blob (+ n_keys + 1 offsets, tk_len) holds Ghw11TransformKey records exactly as rabe_ghw11_tkgen_packed / rabe_ghw11_provision_packed
 *   write them.  The blob is UNTRUSTED, with the conventions of rabe_ghw11_tkgen_packed: nothing outside [0, tk_len) is read, a record has to end
 *   where its offsets say, and unless RABE_PACKED_TRUSTED every G2 element goes through the batched membership pass.  A bad key fails alone:
 *   key_status[u] = -1 (0 otherwise), the first error in rabe_host_last_error, and every item that later names it fails.  The elements of all
 *   keys go to the device once and ONE set of prepared lines is made over them (16.9 KB per element for the line triples plus the reduced-radix
 *   copy; rabe_ghw11_tk_store_bytes reports what the store holds on all devices).  The store made this way has room for exactly the blocks
 *   of its well-formed keys; keys are added and revoked in place with the MUTABLE STORE calls below.  It may be used by any number of
 *   calls on the host that made it.  Free it with rabe_obj_free(RABE_GHW11_TK_STORE, store) BEFORE rabe_host_destroy: the device memory is
 *   released at once when the host is idle, and after the calls that may still use it have ended otherwise.
 * TRANSFORM: DEFINITION -- tct_buf + 768 i and status[i] are what rabe_ghw11_transform_packed writes for record i ALONE under key item_key[i],
 *   byte for byte; the bounds, the membership checks (unless RABE_PACKED_TRUSTED), the error texts and the pass-through of the headers
 *   rabe_ghw11_encaps_packed writes are that call's.  An item_key out of range, or one that names a failed key, fails that item only: status -1
 *   and 768 zero bytes.  Returns 1, with nothing written, when tct_cap < 768 n_items.  No randomness is drawn.  The selection plan of a policy
 *   text is made once per distinct attribute-name list among the keys the batch names, not once per key.  On the device the batch is ONE launch
 *   set whatever the number of keys (rhip_ghw11_transform_batch_keyed: a line base per item into the store's lines).  Under a device group the
 *   items are cut as rabe_ghw11_transform_packed cuts them; every engine prepares its replica of the store's lines on first use and keeps it
 *   until the store is freed.  The store prepares ONE replica at a time: in the first call on a group the engines' preparations run one
 *   after the other (the other blocks wait), and rabe_ghw11_tk_store_bytes waits for a preparation in progress.  An item that names a
 *   revoked key fails alone like one that names a failed key, with the message "transform key revoked"; it never reaches the device.
 * MUTABLE STORE: one store for the life of the proxy.  rabe_ghw11_tk_store_open makes an empty store with room for capacity_blocks BLOCKS
 *   (>= 1) on devices[0]; a block is one G2 element's prepared lines (29.6 KB with the reduced-radix copy), and a key of a attributes takes
 *   a + 2 CONTIGUOUS blocks (k_z, l_z, k_x[..]), placed first-fit at the lowest address.  The capacity is fixed and nothing is compacted: a
 *   key needs one free range of its size, whatever the free total.
 *   rabe_ghw11_tk_store_add takes records as rabe_ghw11_tk_store_create does (untrusted blob, bounds, the membership pass unless
 *   RABE_PACKED_TRUSTED).  A bad key fails alone: key_status[u] = -1, key_id[u] = UINT32_MAX, the first error in rabe_host_last_error, and it
 *   holds no block.  A good key gets key_status 0 and its id in key_id[u] -- what item_key names in rabe_ghw11_transform_keyed.  Ids count up
 *   from 0 in the order of successful addition and are never reused (a store from rabe_ghw11_tk_store_create has given its n_keys records the
 *   ids 0 .. n_keys - 1, the failed ones included).  Returns 1 when the well-formed keys of the call do not ALL fit: nothing is added, nothing is
 *   written to key_status or key_id, the store, its ids and its stat are unchanged.  Per call: one upload of the new elements only, one
 *   membership pass over them only, the lines of the new ranges only (on every engine that holds a replica).
 *   rabe_ghw11_tk_store_revoke: status[j] = 0 when key_id[j] is revoked now; -1, alone and with a message, for an id never issued, failed or
 *   revoked already.  Before the call returns the key's blocks are overwritten with zeros on EVERY device that holds a replica, the host-side
 *   copy of its elements and -- with its last user -- of its attribute names is wiped, and its range is free again, merged with free neighbours.
 *   rabe_ghw11_tk_store_stat: out = live keys, capacity in blocks, blocks in use, largest free contiguous range; -1 for a null argument.
 *   open, add and revoke are single-owner calls like every entry point that is not a _submit: no rabe_ghw11_transform_keyed on the store may
 *   run beside them.  They return after their device work is complete.  An engine of a device group that first meets the store after a
 *   change prepares its replica from the store as it is then; empty ranges stay reserved and empty. */
int32_t rabe_ghw11_tk_store_create(rabe_host* h, size_t n_keys, const uint8_t* tk_blob, size_t tk_len, const uint64_t* tk_off /*[n_keys+1]*/,
                                   uint32_t flags, int32_t* key_status /*[n_keys]*/, void** store);
uint64_t rabe_ghw11_tk_store_bytes(const void* store);
int32_t rabe_ghw11_tk_store_open(rabe_host* h, uint64_t capacity_blocks, void** store);
int32_t rabe_ghw11_tk_store_add(rabe_host* h, void* store, size_t n_keys, const uint8_t* tk_blob, size_t tk_len, const uint64_t* tk_off /*[n_keys+1]*/,
                                uint32_t flags, int32_t* key_status /*[n_keys]*/, uint32_t* key_id /*[n_keys]*/);
int32_t rabe_ghw11_tk_store_revoke(rabe_host* h, void* store, size_t n, const uint32_t* key_id, int32_t* status /*[n]*/);
int32_t rabe_ghw11_tk_store_stat(const void* store, uint64_t out[4]);
int32_t rabe_ghw11_transform_keyed(rabe_host* h, const void* store, size_t n_items, const uint32_t* item_key /*[n_items]*/, const uint8_t* ct_blob,
                                   size_t ct_len, const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/,
                                   uint8_t* tct_buf, size_t tct_cap);
/* Bulk key issuing (conventions of rabe_bsw_keygen_packed): n_items calls of ghw11::keygen (ghw11/mod.rs:123-152) under one master key, item i
 * with the attribute list item_set[i]; records = Ghw11SecretKey (k, l, rows (name, k_x)), written on the device.  Draw order: one r per item, in
 * item order.  Every element is a fixed-base multiple (L = g2 * r, K = g2_alpha + g2_a * r, K_x = g2 * (h(x) r)): one lane per element over window
 * tables of g2 and g2_a that are built once per key pair and kept.  sk_off is always filled; returns 1, with nothing drawn, when
 * sk_cap < sk_off[n_items].  An empty attribute list (keygen returns None) or an item_set out of range fails the call before any draw. */
int32_t rabe_ghw11_keygen_packed(rabe_host* h, const void* pk, const void* msk, const char* const* attributes, const size_t* counts,
                                 size_t n_sets, size_t n_items, const uint32_t* item_set /*[n_items]*/,
                                 uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off /*[n_items+1]*/);
/* n_items calls of ghw11::tkgen (ghw11/mod.rs:156-178), one per Ghw11SecretKey record of sk_blob.  The blob is UNTRUSTED (conventions of
 * rabe_ac17_cp_decrypt_packed): nothing outside [0, sk_len) is read; an item with bad bounds or a malformed record fails alone -- status[i] = -1,
 * an empty tk slot, 32 zero bytes of rk; unless RABE_PACKED_TRUSTED, every decoded G2 element goes through the batched membership pass
 * (coordinates < p, on the twist, in the r-torsion) and a non-member fails its item only.  With the flag a non-member is not rejected and its
 * transform key is NOT z^-1 times its elements (the multiplication relies on membership): set it only for keys this process issued.
 * Output: item i's Ghw11TransformKey record (k_z, l_z, rows (name, k_x_z): the secret key's layout, names copied) at tk_buf + tk_off[i], its
 * Ghw11RetrieveKey record (z, 32 bytes) at rk_buf + 32 i.  Returns 1, with nothing drawn, when tk_cap is below the total size of the well-formed
 * records (tk_off[n_items] = that size).
 * DRAW ORDER: one z per item whose record decodes ON THE HOST (bounds + parse), in item order; the membership verdicts arrive later and do
 * not change what is drawn (a non-member's z is spent).  z = 0 fails the whole call, as tkgen's inverse().unwrap() does.
 * Every element times z^-1 is a variable-base G2 multiplication: z^-1 is split four ways over the twist endomorphism once per item and each
 * element runs one joint chain of ~66 doublings (rhip_g2_mul_rows).  The staging that held z / z^-1 is zeroed when the call ends. */
int32_t rabe_ghw11_tkgen_packed(rabe_host* h, size_t n_items, const uint8_t* sk_blob, size_t sk_len, const uint64_t* sk_off /*[n_items+1]*/,
                                uint32_t flags, int32_t* status /*[n_items]*/,
                                uint8_t* tk_buf, size_t tk_cap, uint64_t* tk_off /*[n_items+1]*/, uint8_t* rk_buf /*32 n_items*/);
/* Bulk provisioning for an authority that issues a user's secret key and the transform / retrieve keys of that user's proxy in one go:
 * BY DEFINITION rabe_ghw11_keygen_packed followed by rabe_ghw11_tkgen_packed on its output, byte for byte and draw for draw (arguments as
 * rabe_ghw11_keygen_packed; item i's Ghw11SecretKey record at sk_buf + sk_off[i], its Ghw11TransformKey record -- the secret key's layout --
 * at tk_buf + tk_off[i], its Ghw11RetrieveKey record z_i at rk_buf + 32 i).  sk_off = NULL: transform and retrieve keys only -- sk_buf is
 * ignored, no secret-key row is computed, the draws are the same.
 * DRAW ORDER: r_0 .. r_{n-1}, then z_0 .. z_{n-1}: a tape that drives the two calls back to back drives this one.  z = 0 fails the whole call,
 * as tkgen's inverse().unwrap() does, and writes no record.
 * The authority knows r and z, so every transform-key element is a fixed-base multiple too (L_z = g2 * (r z^-1), K_z = g2_alpha * z^-1 +
 * g2_a * (r z^-1), K_x_z = g2 * (h(x) r z^-1)): no parse, no membership pass, no variable-base chain; z^-1 and r z^-1 are formed on the
 * device, the elements never leave it between the two halves, both record sets are written there.  The key tables are the ones
 * rabe_ghw11_keygen_packed caches; the window table of g2_alpha is added to them on the first provision call.
 * tk_off, and sk_off if given, are always filled; returns 1, with nothing drawn, when tk_cap < tk_off[n_items] or sk_cap < sk_off[n_items].
 * An empty attribute list or an item_set out of range fails the call before any draw.  The staging that held r, z, z^-1 or r z^-1 is zeroed,
 * on the host and on the device, when the call ends. */
int32_t rabe_ghw11_provision_packed(rabe_host* h, const void* pk, const void* msk, const char* const* attributes, const size_t* counts,
                                    size_t n_sets, size_t n_items, const uint32_t* item_set /*[n_items]*/,
                                    uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off /*[n_items+1] or NULL*/,
                                    uint8_t* tk_buf, size_t tk_cap, uint64_t* tk_off /*[n_items+1]*/, uint8_t* rk_buf /*32 n_items*/);
/* `data` of the reference's decrypt_out is the ciphertext's data field: pass the ciphertext object */
int32_t rabe_ghw11_decrypt_out(rabe_host* h, const void* tct, const void* rk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_ghw11_decrypt_out_gt(rabe_host* h, const void* tct, const void* rk, uint8_t out_gt[384]);
/* The client's half in bulk: n_items calls of decrypt_out (ghw11/mod.rs:297-305) under ONE retrieve key.  tct_buf + 768 i = item i's c | t
 * record exactly as rabe_ghw11_transform_packed writes it; record i of ct_blob (+ offsets) is item i's ciphertext, which carries the sealed
 * data.  msg = c * t^(-z), KDF and AES-GCM open run on the device; only plaintexts come back (pt_buf + pt_off).  Unless RABE_PACKED_TRUSTED,
 * c and t must be members of Gt.  An all-zero tct record, a malformed ciphertext record, a non-member or a tag that does not verify (e.g. a
 * wrong rk) fails that item alone: status -1, empty or zeroed plaintext slot, the first error in rabe_host_last_error.  Returns 1 when pt_cap
 * is below the total size of the well-formed ciphertext records; pt_off[n_items] = that size.  Under a device group both inputs are cut at
 * the same item boundaries (tct_buf + 768 lo, record lo of the blob).  A group that cuts the batch needs the total size of the well-formed
 * records, not of their sealed parts: the call returns 1, and pt_off[n_items] holds the size to come back with. */
int32_t rabe_ghw11_decrypt_out_packed(rabe_host* h, const void* rk, size_t n_items, const uint8_t* tct_buf /*768 n_items*/,
                                      const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags,
                                      int32_t* status /*[n_items]*/, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off /*[n_items+1]*/);

/* GHW11 for a key holder WITHOUT a proxy: n_items Ghw11Ciphertext records (one blob + n_items + 1 offsets, ct_len) under ONE secret key of
 * the holder's own.  DEFINITION: the plaintexts and verdicts of rabe_ghw11_tkgen -> rabe_ghw11_transform_packed -> rabe_ghw11_decrypt_out_packed,
 * for ANY z tkgen may draw.  With k_z = k / z, l_z = l / z, k_x_z = k_x / z the transform returns t_z = t_1^(1/z), where t_1 is the transform's own
 * expression on the secret key's elements (ghw11/mod.rs:252-282), and decrypt_out computes c * (t_z^z)^-1 = c * t_1^-1 (:302): the blinding
 * cancels.  Like rabe_ghw11_provision_packed this is not a function of the reference but a composition of functions that are.
 * SKIPPED against the three calls: z and its inversion, the m + 2 variable-base G2 multiplications of tkgen, the Gt power t^z, the second parse of
 * the blob, the 384 bytes per item that transform_packed brings back and the 768 that decrypt_out_packed sends again.  The records are parsed once,
 * the blob goes to the device once, every Miller loop replays the secret key's prepared lines (kept across calls, keyed on the key's bytes), the
 * G1 arguments enter with the opposite sign so that the Miller product is t_1^-1, c is the leading factor of the same final-exponentiation
 * kernel, and the KDF + AES-GCM open reads the device copy of the blob: no Gt element leaves the device, only plaintexts and verdicts come back.
 * Conventions of rabe_bsw_decrypt_packed and rabe_ghw11_decrypt_out_packed: nothing outside [0, ct_len) is read; bad bounds, a malformed record,
 * a key whose attributes do not satisfy the record's policy, a row name missing from the record, a non-member element, trailing bytes or a tag
 * that does not verify fail that item alone -- status -1, an EMPTY plaintext slot, the first error in rabe_host_last_error (the texts of
 * rabe_ghw11_transform_packed / rabe_ghw11_decrypt_out_packed).  Unless RABE_PACKED_TRUSTED: rabe_ghw11_transform_packed's membership checks
 * (c1, every C_i and D_i on the G1 curve with canonical coordinates, c in Gt).  No randomness is drawn; a seeded source or tape is left
 * untouched.  Returns 1 when pt_cap is below the total of the well-formed records' sealed lengths; pt_off[n_items] = that size.
 * A group that cuts the batch needs the total size of the well-formed records, not of their sealed parts: the call returns 1, and
 * pt_off[n_items] holds the size to come back with. */
int32_t rabe_ghw11_decrypt_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                  const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/,
                                  uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off /*[n_items+1]*/);
/* ---- GHW11 as a key encapsulation: the packed service WITHOUT payloads (what is said at rabe_ac17_cp_{encaps,decaps}_packed about the format
 * holds here with Ghw11Ciphertext records).  Outsourced decryption exists so that a thin client does almost nothing: a KEM client holds its
 * 32-byte z, is handed c | t (768 bytes per item) by the proxy, and computes one Gt power per item -- no ciphertext blob, no policy text, no
 * G1 element ever reaches it.
 * ENCAPS: header i is the Ghw11Ciphertext record rabe_ghw11_encrypt_packed writes for the same draws with a sealed part of length zero,
 *   key_buf + 32 i = SHA3-256(bytes(msg_i)) (the KDF of encrypt_symmetric).  Draw order: encrypt_packed's minus the AES nonce -- per item the
 *   secret, msg, the gate coefficients, then one t per share.  No seal kernel is launched.  hdr_off is always filled; returns 1, with nothing
 *   drawn and nothing written, when hdr_cap < hdr_off[n_items].  The staging that held the scalars, msg and the keys is scrubbed.
 * DECAPS_OUT (the client's half): tct_buf + 768 i = item i's c | t record as rabe_ghw11_transform_packed writes it; key_buf + 32 i =
 *   SHA3-256(bytes(c_i * t_i^-z)), BY DEFINITION the KDF of what rabe_ghw11_decrypt_out_gt returns.  The power runs over a four-way split of
 *   z along the Frobenius map (rhip_gt_pow_rows: one split for the call, z uploaded once, at most 66 squarings per item instead of 256, the
 *   inverse a conjugation, c multiplied in by the same kernel), then the KDF behind the verdict mask.  An item fails alone -- status -1 and
 *   32 zero bytes -- on an all-zero record (the transform's failure mark) and, unless RABE_PACKED_TRUSTED, when c or t is not a member of Gt.
 *   With the flag a non-member is not rejected and its key is UNSPECIFIED (the split relies on membership): set it only for records this
 *   process transformed.  A wrong rk gives another key with status 0: a KEM has no tag.  The staging that held z is zeroed when the call ends.
 * DECAPS (the holder without a proxy): rabe_ghw11_decrypt_packed's launch set up to c * t_1^-1, then the KDF.  Headers and full records are
 *   both valid input; the sealed bytes are skipped by their length field, neither read nor authenticated.  Failures and texts are those of
 *   rabe_ghw11_decrypt_packed; a failed item has status -1 and 32 zero bytes.  No Gt power and no AES kernel is launched.
 * Under a device group all three are cut as the AC17 / BSW pair is: headers through the producing pipeline, key slots and verdicts in place. */
int32_t rabe_ghw11_encaps_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                                 const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap, uint64_t* hdr_off /*[n_items+1]*/,
                                 uint8_t* key_buf /*32 n_items*/);
int32_t rabe_ghw11_decaps_out_packed(rabe_host* h, const void* rk, size_t n_items, const uint8_t* tct_buf /*768 n_items*/, uint32_t flags,
                                     int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);
int32_t rabe_ghw11_decaps_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len,
                                 const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/,
                                 uint8_t* key_buf /*32 n_items*/);
/* the same for one ciphertext object (one pairing job through rhip_pairing_jobs, as rabe_ghw11_transform); _gt returns c * t_1^-1 */
int32_t rabe_ghw11_decrypt(rabe_host* h, const void* sk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_ghw11_decrypt_gt(rabe_host* h, const void* sk, const void* ct, uint8_t out_gt[384]);

/* ---- bdabe (src/schemes/bdabe/mod.rs:149-399) and mke08 (src/schemes/mke08/mod.rs:130-380): DNF policies, attributes named
 * "authority::attribute".  `request_attribute_sk` / `request_authority_sk` APPEND the new secret attribute key to the user key
 * (the reference returns it and its callers push it onto `sk.sk_a`: bdabe/mod.rs:21, mke08 tests).  decrypt: every item's
 * pairing factors on one accumulator, one final exponentiation (rhip_pairing_jobs). */
int32_t rabe_bdabe_setup(rabe_host* h, void** pk, void** msk);
int32_t rabe_bdabe_authgen(rabe_host* h, const void* pk, const void* msk, const char* name, void** ska);
int32_t rabe_bdabe_keygen(rabe_host* h, const void* pk, const void* ska, const char* name, void** uk);
int32_t rabe_bdabe_request_attribute_pk(rabe_host* h, const void* pk, const void* ska, const char* attribute, void** pka);
int32_t rabe_bdabe_request_attribute_sk(rabe_host* h, void* uk, const void* ska, const char* attribute);
int32_t rabe_bdabe_encrypt(rabe_host* h, const void* pk, const void* const* attr_pks, size_t n_pks, const char* policy, int32_t language,
                           const uint8_t* plaintext, size_t len, void** ct);
int32_t rabe_bdabe_decrypt(rabe_host* h, const void* uk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_bdabe_decrypt_gt(rabe_host* h, const void* uk, const void* ct, uint8_t out_gt[384]);
int32_t rabe_bdabe_decrypt_batch(rabe_host* h, size_t n, const void* const* uks, const void* const* cts, int32_t* status, uint8_t** plaintexts,
                                 size_t* lens);
/* bdabe::decrypt (bdabe/mod.rs:359-399) / mke08::decrypt (mke08/mod.rs:343-380) of n_items serialized ciphertexts (one blob + n_items + 1
 * offsets, ct_len) under ONE user key -- same conventions as rabe_ac17_cp_decrypt_packed: bounds and, unless RABE_PACKED_TRUSTED, group
 * membership of every decoded element (one batched pass per group over the whole blob); status[i] = 0 / -1, plaintexts back to back in
 * pt_buf at pt_off[i] (nothing for a failed item); returns 1 when pt_cap is too small (sum of the sealed lengths always suffices).  The
 * pairings of the whole batch are one rhip_pairing_jobs launch set (<= 2 m + 3 Miller loops per item on a few accumulators, one final
 * exponentiation per item), the sealed plaintexts are opened on the device (Level S): no Gt crosses PCIe. */
int32_t rabe_bdabe_decrypt_packed(rabe_host* h, const void* uk, size_t n_items, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, uint32_t flags,
                                  int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off);
int32_t rabe_mke08_decrypt_packed(rabe_host* h, const void* uk, size_t n_items, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, uint32_t flags,
                                  int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off);
/* n_items calls of encrypt (bdabe/mod.rs:317-358, mke08/mod.rs:290-334) in the form of rabe_aw11_encrypt_packed: item i is
 * encrypt(pk, attr_pks, policies[item_policy[i]], language, pt_blob[pt_off[i] .. pt_off[i+1])).  ct_buf receives the BdabeCiphertext /
 * Mke08Ciphertext records (rabe_obj_serialize's bytes), built and sealed on the device: one row per (item, DNF term), every element a
 * fixed-base product with the row's r_j (tables of p1, p2 and of each term's folded attribute keys, cached per engine).
 * Draw order per item -- BDABE: a, b (msg = e(G1::one(), G2::one())^(ab)), one r_j per DNF term in json_to_dnf's order, the AES nonce;
 * MKE08: a, b, c (msg1 = gen^(ab), msg2 = msg1^c, the data sealed under msg1 * msg2), the r_j, the AES nonce.
 * Errors fail the whole call and write no record: a policy not in DNF or naming an attribute attr_pks lacks (the object API's messages,
 * with the index of the policy), an item_policy out of range.  Returns 1 when ct_cap is too small; ct_off[n_items] = the size needed. */
int32_t rabe_bdabe_encrypt_packed(rabe_host* h, const void* pk, const void* const* attr_pks, size_t n_pks,
                                  const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                                  const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off,
                                  uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off);
int32_t rabe_mke08_encrypt_packed(rabe_host* h, const void* pk, const void* const* attr_pks, size_t n_pks,
                                  const char* const* policies, size_t n_policies, int32_t language, size_t n_items,
                                  const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off,
                                  uint8_t* ct_buf, size_t ct_cap, uint64_t* ct_off);
/* Key encapsulation for bdabe / mke08: everything said at rabe_ac17_cp_{encaps,decaps}_packed about the format, the key (SHA3-256(bytes(Gt))),
 * the failure of an item alone (status -1, 32 zero bytes, the first error's text), the bounds and the scrubbed staging, with BdabeCiphertext /
 * Mke08Ciphertext records and rabe_{bdabe,mke08}_decrypt_gt as the definition of X.  Compositions: the reference has neither function.  (The
 * names do not end in _packed: the table of rabe_*_packed symbols is a recorded contract; the calls are packed calls in every other respect.)
 * ENCAPS: arguments of rabe_{bdabe,mke08}_encrypt_packed minus the payloads, plus key_buf.  Header i is the record encrypt_packed writes for the
 *   same draws with a sealed part of length zero; key i = SHA3-256(bytes(msg_i)) (MKE08: msg = msg1 * msg2, the element encrypt_packed seals
 *   under).  DRAW ORDER: encrypt_packed's minus the AES nonce -- BDABE a, b, the r_j; MKE08 a, b, c, the r_j.  Call-level errors, hdr_off and
 *   the return of 1 on a short buffer (nothing drawn) are encrypt_packed's.  The launch set is rhip_dnf_encrypt_batch; no AES kernel is launched.
 * DECAPS: ONE user key against n_items records; headers and full records are both valid input, the sealed part is skipped by its length field,
 *   neither read nor authenticated.  Item verdicts are those of rabe_{bdabe,mke08}_decrypt_packed's decoding (bounds, a malformed record,
 *   trailing bytes; unless RABE_PACKED_TRUSTED a non-member among ANY decoded element of the record, the conjunctions that are not chosen
 *   included) and of the reference's traverse_policy ("attributes in sk do not match policy in ct").  ONE DIFFERENCE from decrypt_gt: a record
 *   whose policy text the key satisfies but none of whose conjunction lists it does fails with a message of its own -- decrypt_gt returns
 *   Gt::one() there, which the AES layer of a decrypt then rejects; a KEM has no such layer and must not hand out the KDF of one.
 *   The chosen conjunction is the first in record order whose names the key holds; its attribute list as stated (order and repetitions
 *   included) is its CLASS.  Per class S1 = sum au1, S2 = sum au2 over the first key row of each name, on the device; per call one set of
 *   prepared lines over [sk.u2, S2 of every class]; then FOUR Miller loops per item whatever the conjunction's length
 *   (rhip_dnf_decrypt_batch_one_uk: e(e2, S2) and e(-e4, u2) on prepared lines, e(S1, e3) and e(-u1, e5) walked, their walks giving the
 *   membership verdicts of e3 and e5) where rabe_*_decrypt_packed runs m + 3, the KDF behind the verdict mask and one download of
 *   32 n_items bytes.  No Gt element crosses PCIe.
 * Both calls are cut over a device group (encaps like encrypt_packed; decaps block by block, each engine with its own lines). */
int32_t rabe_bdabe_kem_encaps(rabe_host* h, const void* pk, const void* const* attr_pks, size_t n_pks, const char* const* policies, size_t n_policies,
                              int32_t language, size_t n_items, const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap,
                              uint64_t* hdr_off /*[n_items+1]*/, uint8_t* key_buf /*32 n_items*/);
int32_t rabe_bdabe_kem_decaps(rabe_host* h, const void* uk, size_t n_items, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off /*[n_items+1]*/,
                              uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);
int32_t rabe_mke08_kem_encaps(rabe_host* h, const void* pk, const void* const* attr_pks, size_t n_pks, const char* const* policies, size_t n_policies,
                              int32_t language, size_t n_items, const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap,
                              uint64_t* hdr_off /*[n_items+1]*/, uint8_t* key_buf /*32 n_items*/);
int32_t rabe_mke08_kem_decaps(rabe_host* h, const void* uk, size_t n_items, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off /*[n_items+1]*/,
                              uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);
/* Bulk key issuing of the two schemes (conventions of rabe_ghw11_keygen_packed / rabe_ghw11_tkgen_packed).
 * keygen_packed: n_items calls of keygen (bdabe/mod.rs:201-222, mke08/mod.rs:185-206) under one authority key (MKE08: the master key), item i
 * for the user names[i].  Record i = rabe_obj_serialize's bytes of the user key with an empty sk_a: sk.u1 | sk.u2 | name | pk.u1 | pk.u2 | u32 0.
 * Draw order: one r_u (mk_u) per item, in item order.  Every element is a fixed-base multiple (a1 + p1 r, a2 + p2 r, g1 r, g2 r): one lane per
 * element over window tables of p1, g1, p2, g2 that are built once per key and kept; records are written on the device.  uk_off is always
 * filled; returns 1, with nothing drawn, when uk_cap < uk_off[n_items]. */
int32_t rabe_bdabe_keygen_packed(rabe_host* h, const void* pk, const void* ska, const char* const* names /*[n_items]*/, size_t n_items,
                                 uint8_t* uk_buf, size_t uk_cap, uint64_t* uk_off /*[n_items+1]*/);
int32_t rabe_mke08_keygen_packed(rabe_host* h, const void* pk, const void* msk, const char* const* names /*[n_items]*/, size_t n_items,
                                 uint8_t* uk_buf, size_t uk_cap, uint64_t* uk_off /*[n_items+1]*/);
/* Secret attribute keys in bulk: what n_items x (attributes of a list) calls of request_attribute_sk (bdabe/mod.rs:275-305) /
 * request_authority_sk (mke08/mod.rs:248-278) give under one authority key.  Item i is a user's PUBLIC key record, name | u1 (64) | u2 (128) --
 * the bytes of BdabePublicUserKey / Mke08PublicUserKey inside a user-key record -- and receives every attribute of the list item_set[i] (lists
 * as in rabe_ghw11_keygen_packed: flat attributes, counts, n_sets; an empty list is allowed).  Output record i: u32 count, then count rows
 * (attribute, au1 (64), au2 (128)) in list order -- byte for byte the sk_a tail of the user-key record, so keygen record[:-4] + this record
 * is the object API's user key after the same calls.  Nothing is drawn.
 * The blob is UNTRUSTED: an item with bad bounds, a malformed record or trailing bytes fails alone -- status[i] = -1, an empty output slot, the
 * first error in rabe_host_last_error; unless RABE_PACKED_TRUSTED, u1 must be on the curve with canonical coordinates and u2 a member of G2
 * (one batched pass beside the multiplications), and a non-member fails its item only.  With the flag a non-member is not rejected and its
 * keys are unspecified.  Call-level errors, before any work and with no output: an attribute that is not from_authority() for this key (the
 * object API's message and the index of its list), an item_set out of range, more than 2^32 rows.  Returns 1 when out_cap is below the total
 * size of the well-formed items' records (out_off[n_items] = that size).
 * exp = h(attribute) h(authority) a3 (MKE08: r) is formed once per (list, position) on the host; its rows -- the users of that list -- are
 * adjacent in the launch (rhip_g1_mul_rows_at, rhip_g2_mul_rows_at), results land item-major and the records are written on the device. */
int32_t rabe_bdabe_request_attribute_sk_packed(rabe_host* h, const void* ska, const char* const* attributes, const size_t* counts, size_t n_sets,
                                               size_t n_items, const uint32_t* item_set /*[n_items]*/, const uint8_t* upk_blob, size_t upk_len,
                                               const uint64_t* upk_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/,
                                               uint8_t* out_buf, size_t out_cap, uint64_t* out_off /*[n_items+1]*/);
int32_t rabe_mke08_request_authority_sk_packed(rabe_host* h, const void* ska, const char* const* attributes, const size_t* counts, size_t n_sets,
                                               size_t n_items, const uint32_t* item_set /*[n_items]*/, const uint8_t* upk_blob, size_t upk_len,
                                               const uint64_t* upk_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/,
                                               uint8_t* out_buf, size_t out_cap, uint64_t* out_off /*[n_items+1]*/);
int32_t rabe_mke08_setup(rabe_host* h, void** pk, void** msk);
int32_t rabe_mke08_keygen(rabe_host* h, const void* pk, const void* msk, const char* name, void** uk);
int32_t rabe_mke08_authgen(rabe_host* h, const char* name, void** ska);
int32_t rabe_mke08_request_authority_pk(rabe_host* h, const void* pk, const char* attribute, const void* ska, void** pka);
int32_t rabe_mke08_request_authority_sk(rabe_host* h, void* uk, const char* attribute, const void* ska);
int32_t rabe_mke08_encrypt(rabe_host* h, const void* pk, const void* const* attr_pks, size_t n_pks, const char* policy, int32_t language,
                           const uint8_t* plaintext, size_t len, void** ct);
int32_t rabe_mke08_decrypt(rabe_host* h, const void* uk, const void* ct, uint8_t** plaintext, size_t* len);
int32_t rabe_mke08_decrypt_gt(rabe_host* h, const void* uk, const void* ct, uint8_t out_gt[384]);
int32_t rabe_mke08_decrypt_batch(rabe_host* h, size_t n, const void* const* uks, const void* const* cts, int32_t* status, uint8_t** plaintexts,
                                 size_t* lens);
/* dnf.rs:203-243 and :186-201 on attribute names only: result 1 / 0; the terms as JSON [[attr, ..], ..] (keys = one name per public attribute key) */
int32_t rabe_policy_in_dnf(const char* policy, int32_t language, int32_t* result);
int32_t rabe_policy_dnf_terms(const char* policy, int32_t language, const char* const* key_attrs, size_t n, char** out);

/* ---- host-only policy utilities (no GPU needed): results as small JSON texts, free with rabe_bytes_free.
 *   rabe_policy_parse      -> serialize_policy(parse(policy, language), out_language)       pest/mod.rs:40-114
 *   rabe_policy_msp        -> {"m": [[..]], "pi": [..], "c": n}                             msp.rs:78-147
 *   rabe_policy_pruned     -> {"match": bool, "list": [[name, name_col], ..]}               secretsharing/mod.rs:143-199
 *   rabe_policy_traverse   -> 1 / 0                                                         tools/mod.rs:31-61
 *   rabe_policy_shares     -> [[name_col, hex(fr_le)], ..] for secret + coefficient tape    secretsharing/mod.rs:82-141
 *   rabe_policy_coeffs     -> [[name_col, hex(fr_le)], ..]                                  secretsharing/mod.rs:9-72
 */
int32_t rabe_policy_parse(const char* policy, int32_t language, int32_t out_language, char** out);
int32_t rabe_policy_msp(const char* policy, int32_t language, char** out);
int32_t rabe_policy_pruned(const char* policy, int32_t language, const char* const* attributes, size_t n, char** out);
int32_t rabe_policy_traverse(const char* policy, int32_t language, const char* const* attributes, size_t n, int32_t* result);
int32_t rabe_policy_shares(const char* policy, int32_t language, const uint8_t secret_le32[32], const uint8_t* tape_le32, size_t n_tape, char** out);
int32_t rabe_policy_coeffs(const char* policy, int32_t language, char** out);
/* sha3_hash_fr (src/utils/hash/mod.rs:23-31): Fr::from_slice(SHA3-256(label)), little-endian canonical */
int32_t rabe_hash_fr(const char* label, uint8_t out_le32[32]);
/* test hook: x mod r of a 512-bit little-endian x by the fast path and by plain long division */
int32_t rabe_fr_reduce512(const uint8_t in_le64[64], uint8_t out_fast[32], uint8_t out_division[32]);
/* test hook, no GPU needed: the four-way split k = k0 + k1 L + k2 L^2 + k3 L^3 (mod r), L = p mod r, that rabe_ghw11_tkgen_packed's kernel
 * applies to z^-1 (the same routine, run on the host): mag[i] = |k_i| little-endian, neg[i] = 1 for a negative k_i */
int32_t rabe_fr_split4(const uint8_t k[32], uint8_t mag[4][16] /*little-endian magnitudes*/, uint8_t neg[4]);
/* KDF + AES-256-GCM of src/utils/aes/mod.rs with an explicit nonce; out = nonce || ct || tag */
int32_t rabe_encrypt_symmetric(const uint8_t gt[384], const uint8_t* data, size_t len, const uint8_t nonce[12], uint8_t** out, size_t* out_len);
int32_t rabe_decrypt_symmetric(const uint8_t gt[384], const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);
/* the raw primitives under the two functions above (sha3 0.10.8 / aes-gcm 0.10.3 in the reference, Cargo.toml:28,36), exported
 * so that public known-answer vectors can pin them; out of rabe_aes256_gcm_encrypt = ciphertext || tag(16) */
int32_t rabe_sha3_256(const uint8_t* data, size_t len, uint8_t out[32]);
int32_t rabe_aes256_gcm_encrypt(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);
int32_t rabe_aes256_gcm_decrypt(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);

#ifdef __cplusplus
}
#endif
#endif
