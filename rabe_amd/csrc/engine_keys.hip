// engine_keys.hip -- bulk key issuing: the GHW11 keygen row kernel (fixed-base) and the variable-base G2 multiplication over rows that
// share a scalar (four-way split over the twist endomorphism, bn254/gls4.h), which serves ghw11::tkgen; the user-key row kernels of
// BDABE / MKE08 (fixed-base) and the variable-base G1 multiplication over rows that share a scalar (GLV, bn254/curve.h), which with the G2
// one serves their secret attribute keys; GHW11's fused keygen + tkgen for an authority that knows r and z (fixed-base again: an Fr kernel
// that inverts the z of a block together, and a row kernel over a third window table); the LSW ciphertext rows (fixed-base: three elements
// per lane, four walks, one inversion per block -- bn254/lsw_rows.h).
//
// A translation unit of its own: docs/rr29.md records that adding a kernel to a unit can move its neighbours' register allocation, and
// engine_jobs.hip holds the kernels BASELINE configs 3 - 5 time.
#include "engine_internal.h"
#include "bn254/gls4.h"
#include "bn254/lsw_rows.h"
#include <mutex>

// Montgomery records are 128 bytes and 16-byte aligned: 128-bit accesses
__device__ __forceinline__ Fp ld_fp_q(const uint4* p) {
  const uint4 a = p[0], b = p[1];
  Fp r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_fp_q(uint4* p, const Fp& a) {
  p[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  p[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
__device__ __forceinline__ G2Aff ld_g2_q(const G2M* p) {
  const uint4* q = (const uint4*)p;
  return G2Aff{Fp2{ld_fp_q(q), ld_fp_q(q + 2)}, Fp2{ld_fp_q(q + 4), ld_fp_q(q + 6)}};
}
__device__ __forceinline__ void st_g2_q(G2M* p, const G2Aff& a) {
  uint4* q = (uint4*)p;
  st_fp_q(q, a.x.c0); st_fp_q(q + 2, a.x.c1); st_fp_q(q + 4, a.y.c0); st_fp_q(q + 6, a.y.c1);
}
// item owning flat index t: the i with off[i] <= t < off[i+1] (off non-decreasing, off[0] <= t < off[n])
__device__ __forceinline__ size_t owner_of(const uint32_t* off, size_t n, size_t t) {
  size_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------ GHW11 keygen
struct rhip_ghw11_keys {
  rhip_ctx* ctx;
  rhip_g2_table* g2;
  rhip_g2_table* g2_a;
  rhip_g2* g2_alpha;          // device, wire form
  // rhip_ghw11_provision_batch alone walks a table of g2_alpha: built on its first call (134 MB, a launch over 2^20 entries -- a process
  // that only issues secret keys pays neither), from the host copy, under the mutex (the lanes of an engine share the handle)
  rhip_g2 g2_alpha_host;
  std::mutex mu;
  rhip_g2_table* g2_alpha_tbl;
};
extern "C" void rhip_ghw11_keys_destroy(rhip_ghw11_keys* k) {
  if (!k) return;
  rhip_g2_table_destroy(k->g2);
  rhip_g2_table_destroy(k->g2_a);
  rhip_g2_table_destroy(k->g2_alpha_tbl);
  if (k->g2_alpha) (void)hipFree(k->g2_alpha);
  delete k;
}
extern "C" int32_t rhip_ghw11_keys_create(rhip_ctx* ctx, const rhip_g2* g2, const rhip_g2* g2_a, const rhip_g2* g2_alpha, rhip_ghw11_keys** out) {
  if (!ctx || !g2 || !g2_a || !g2_alpha || !out) return RHIP_ERR_ARG;
  *out = nullptr;
  rhip_ghw11_keys* k = new rhip_ghw11_keys{ctx, nullptr, nullptr, nullptr, *g2_alpha, {}, nullptr};
  int32_t rc = rhip_g2_table_create(ctx, g2, &k->g2);
  if (!rc) rc = rhip_g2_table_add_w16(ctx, k->g2);
  if (!rc) rc = rhip_g2_table_create(ctx, g2_a, &k->g2_a);
  if (!rc) rc = rhip_g2_table_add_w16(ctx, k->g2_a);
  if (!rc) {
    hipError_t he = hipMalloc((void**)&k->g2_alpha, sizeof(rhip_g2));
    if (he == hipSuccess) he = hipMemcpy(k->g2_alpha, g2_alpha, sizeof(rhip_g2), hipMemcpyHostToDevice);
    if (he != hipSuccess) rc = fail(ctx, he, "rhip_ghw11_keys_create");
  }
  if (rc) { rhip_ghw11_keys_destroy(k); return rc; }
  *out = k;
  return RHIP_OK;
}
// one lane per key element (ghw11/mod.rs:123-152); rows of item i are [item_row_off[i], item_row_off[i+1]) = L, K, then its attributes:
//   row 0: L   = g2 * r
//   row 1: K   = g2_alpha + g2_a * r
//   row y: K_x = (g2 * h(x)) * r = g2 * (h(x) r),  h(x) = hash[item_hash_off[i] + y - 2]
// Every element is one walk over the 16-bit windows of g2 or g2_a; the product h(x) r is formed in the lane.  One inversion per block.
__global__ void __launch_bounds__(128, RB_G2_WAVES) k_ghw11_keygen_rows(const G2M* g2_tbl, const G2M* g2a_tbl, const rhip_g2* g2_alpha, size_t n_items,
                                                                       size_t n_rows, const uint32_t* item_row_off, const uint32_t* item_hash_off,
                                                                       const rhip_fr* hash, const rhip_fr* r, rhip_g2* out) {
  __shared__ uint32_t sh[2 * 8 * 128];
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_rows;
  if (!active) t = n_rows - 1;        // inactive lanes shadow the last row (no stores) and still join the block inversion
  const size_t item = owner_of(item_row_off, n_items, t);
  const uint32_t row = (uint32_t)(t - item_row_off[item]);
  uint32_t kk[8];
  if (row < 2) {
    ld_scalar(kk, r + item);
  } else {
    const Fr e = mul_inl(load_fr(hash[(size_t)item_hash_off[item] + (row - 2)].l), load_fr(r[item].l));
    from_mont_inl<FrParams>(kk, e);
  }
  G2Jac a = table_mul_g2_w16(row == 1 ? g2a_tbl : g2_tbl, kk);
  if (row == 1) a = jac_add_aff(a, load_g2(g2_alpha->l));
  store_g2_block128(sh, active, out + t, a);
}
extern "C" int32_t rhip_ghw11_keygen_batch(rhip_ctx* ctx, const rhip_ghw11_keys* keys, size_t n_items, size_t n_rows, const uint32_t* item_row_off,
                                           const uint32_t* item_hash_off, const rhip_fr* hash, const rhip_fr* r, rhip_g2* out) {
  NEED(ctx);
  if (!keys) return RHIP_ERR_ARG;
  if (!n_items || !n_rows) return RHIP_OK;
  if (!item_row_off || !item_hash_off || !hash || !r || !out) return RHIP_ERR_ARG;
  KLAUNCH(ctx, "k_ghw11_keygen_rows", k_ghw11_keygen_rows, dim3(blocks_for(n_rows, 128)), dim3(128), 0, ctx->stream, (const G2M*)keys->g2->dev16,
          (const G2M*)keys->g2_a->dev16, (const rhip_g2*)keys->g2_alpha, n_items, n_rows, item_row_off, item_hash_off, hash, r, out);
  return RHIP_OK;
}

// ------------------------------------------------------------------------------------------------ GHW11 keygen + tkgen, r and z known
// block_batch_inverse_n (engine_internal.h) over Fr: every thread of the NT = 64 E thread block contributes one non-zero scalar and gets
// its inverse back for ONE field inversion, computed by wave 0 on a wave-uniform value.  lds: 2 x 8 x NT words.  All NT threads must call.
__device__ __forceinline__ Fr shfl_up_fr(const Fr& x, int d) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_up((int)x.v[i], d);
  return r;
}
__device__ __forceinline__ Fr shfl_down_fr(const Fr& x, int d) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_down((int)x.v[i], d);
  return r;
}
__device__ __forceinline__ Fr shfl_fr(const Fr& x, int src) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl((int)x.v[i], src);
  return r;
}
__device__ __forceinline__ Fr sel_fr(bool c, const Fr& a, const Fr& b) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
template <int NT>
__device__ __noinline__ Fr block_batch_inverse_fr(uint32_t* lds, const Fr& mine) {
  uint32_t (*val)[NT] = (uint32_t (*)[NT])lds;
  uint32_t (*pre)[NT] = (uint32_t (*)[NT])(lds + 8 * NT);
  constexpr int E = NT / 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; i++) val[i][tid] = mine.v[i];
  __syncthreads();
  if (tid < 64) {
    Fr run;
#pragma unroll
    for (int i = 0; i < 8; i++) run.v[i] = val[i][tid];
#pragma unroll 1
    for (int e = 1; e < E; e++) {
      Fr v;
#pragma unroll
      for (int i = 0; i < 8; i++) { pre[i][tid + 64 * (e - 1)] = run.v[i]; v.v[i] = val[i][tid + 64 * e]; }
      run = mul(run, v);
    }
    Fr prefix = run, suffix = run;
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
      const Fr u = shfl_up_fr(prefix, d);
      const Fr w = shfl_down_fr(suffix, d);
      const Fr pu = mul(prefix, u);
      const Fr sw = mul(suffix, w);
      prefix = sel_fr(tid >= d, pu, prefix);
      suffix = sel_fr(tid + d < 64, sw, suffix);
    }
    const Fr total_inv = inv(shfl_fr(prefix, 63));
    Fr ex_pre = shfl_up_fr(prefix, 1), ex_suf = shfl_down_fr(suffix, 1);
    ex_pre = sel_fr(tid >= 1, ex_pre, one<FrParams>());
    ex_suf = sel_fr(tid < 63, ex_suf, one<FrParams>());
    Fr inv_run = mul(total_inv, mul(ex_pre, ex_suf));       // 1 / (product of this lane's E elements)
#pragma unroll 1
    for (int e = E - 1; e >= 1; e--) {
      Fr v, p;
#pragma unroll
      for (int i = 0; i < 8; i++) { v.v[i] = val[i][tid + 64 * e]; p.v[i] = pre[i][tid + 64 * (e - 1)]; }
      const Fr r = mul(inv_run, p);                          // 1 / v_e
      inv_run = mul(inv_run, v);                             // 1 / (v_0 .. v_{e-1})
#pragma unroll
      for (int i = 0; i < 8; i++) val[i][tid + 64 * e] = r.v[i];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) val[i][tid] = inv_run.v[i];
  }
  __syncthreads();
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = val[i][tid];
  return r;
}
// one lane per item: zinv[i] = z_i^-1, rz[i] = r_i z_i^-1 (canonical), one inversion per block.  z_i = 0 sets flags[i] and gives
// zinv[i] = rz[i] = 0; in the block's product it is replaced by one, as are the lanes past n, so its neighbours' inverses stand.
__global__ void __launch_bounds__(128, RB_MIN_WAVES) k_ghw11_tk_scalars(size_t n, const rhip_fr* r, const rhip_fr* z, rhip_fr* zinv, rhip_fr* rz,
                                                                       uint32_t* flags) {
  __shared__ uint32_t sh[2 * 8 * 128];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  uint32_t zz[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (active) ld_scalar(zz, z + i);          // below the group order: zero is the word 0
  const bool z0 = (zz[0] | zz[1] | zz[2] | zz[3] | zz[4] | zz[5] | zz[6] | zz[7]) == 0;
  Fr zi = block_batch_inverse_fr<128>(sh, z0 ? one<FrParams>() : to_mont<FrParams>(zz));
  if (!active) return;
  if (z0) zi = zero<FrParams>();
  flags[i] = z0 ? 1u : 0u;
  store_fr(zinv[i].l, zi);
  store_fr(rz[i].l, mul(load_fr(r[i].l), zi));
}
// two fixed-base products on one accumulator: tbl1 * k1 + tbl2 * k2 over the 16-bit windows of both tables, without leaving Jacobian form
// in between and with ONE call site of the G2 addition; a lane with k2 = 0 adds nothing in the second half
__device__ __forceinline__ G2Jac table_mul2_g2_w16(const G2M* tbl1, const uint32_t k1[8], const G2M* tbl2, const uint32_t k2[8]) {
  G2Jac acc = jac_inf<Fp2>();
  walk16_two(k1, k2, [&](bool second, int w, uint32_t d) { acc = jac_add_aff(acc, ld_g2_m((second ? tbl2 : tbl1) + (size_t)w * TBL16_DIGITS + (d - 1))); });
  return acc;
}
// one lane per transform-key element (ghw11/mod.rs:156-178 on the elements of :123-152), rows as in k_ghw11_keygen_rows; with
// u = z^-1 and v = r z^-1 of the row's item (k_ghw11_tk_scalars):
//   row 0: L_z   = g2 * v
//   row 1: K_z   = g2_alpha * u + g2_a * v          (two walks on one accumulator)
//   row y: K_x_z = g2 * (h(x) v),  h(x) = hash[item_hash_off[i] + y - 2]
// One inversion per block.
__global__ void __launch_bounds__(128, RB_G2_WAVES) k_ghw11_provision_rows(const G2M* g2_tbl, const G2M* g2a_tbl, const G2M* alpha_tbl, size_t n_items,
                                                                          size_t n_rows, const uint32_t* item_row_off, const uint32_t* item_hash_off,
                                                                          const rhip_fr* hash, const rhip_fr* zinv, const rhip_fr* rz, rhip_g2* out) {
  __shared__ uint32_t sh[2 * 8 * 128];
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_rows;
  if (!active) t = n_rows - 1;        // inactive lanes shadow the last row (no stores) and still join the block inversion
  const size_t item = owner_of(item_row_off, n_items, t);
  const uint32_t row = (uint32_t)(t - item_row_off[item]);
  uint32_t k1[8], k2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row == 0) {
    ld_scalar(k1, rz + item);
  } else if (row == 1) {
    ld_scalar(k1, zinv + item);
    ld_scalar(k2, rz + item);
  } else {
    const Fr e = mul_inl(load_fr(hash[(size_t)item_hash_off[item] + (row - 2)].l), load_fr(rz[item].l));
    from_mont_inl<FrParams>(k1, e);
  }
  const G2Jac a = table_mul2_g2_w16(row == 1 ? alpha_tbl : g2_tbl, k1, g2a_tbl, k2);
  store_g2_block128(sh, active, out + t, a);
}
extern "C" int32_t rhip_ghw11_provision_batch(rhip_ctx* ctx, rhip_ghw11_keys* keys, size_t n_items, size_t n_rows, const uint32_t* item_row_off,
                                              const uint32_t* item_hash_off, const rhip_fr* hash, const rhip_fr* r, const rhip_fr* z, rhip_g2* out_sk,
                                              rhip_g2* out_tk, uint32_t* flags) {
  NEED(ctx);
  if (!keys) return RHIP_ERR_ARG;
  if (!n_items || !n_rows) return RHIP_OK;
  if (!item_row_off || !item_hash_off || !hash || !r || !z || !out_tk || !flags) return RHIP_ERR_ARG;
  {
    std::lock_guard<std::mutex> lock(keys->mu);          // the build waits for its stream: the table is whole when the lock is released
    if (!keys->g2_alpha_tbl) {
      rhip_g2_table* tbl = nullptr;
      int32_t rc = rhip_g2_table_create(ctx, &keys->g2_alpha_host, &tbl);
      if (!rc) rc = rhip_g2_table_add_w16(ctx, tbl);
      if (rc) { rhip_g2_table_destroy(tbl); return rc; }
      keys->g2_alpha_tbl = tbl;
    }
  }
  if (out_sk) {
    const int32_t rc = rhip_ghw11_keygen_batch(ctx, keys, n_items, n_rows, item_row_off, item_hash_off, hash, r, out_sk);
    if (rc) return rc;
  }
  // z^-1 | r z^-1 per item: the per-item slot of rhip_g2_mul_rows (both are scratch of key issuing, in stream order on this context),
  // zeroed behind the row kernel -- the pair is the retrieve key and the key's r in another form
  void* work = nullptr;
  const int32_t rc = rhip_ensure_work(ctx, WORK_ROWS_MASKS, 2 * n_items * sizeof(rhip_fr), &work);
  if (rc) return rc;
  rhip_fr* zinv = (rhip_fr*)work;
  rhip_fr* rz = zinv + n_items;
  KLAUNCH(ctx, "k_ghw11_tk_scalars", k_ghw11_tk_scalars, dim3(blocks_for(n_items, 128)), dim3(128), 0, ctx->stream, n_items, r, z, zinv, rz, flags);
  KLAUNCH(ctx, "k_ghw11_provision_rows", k_ghw11_provision_rows, dim3(blocks_for(n_rows, 128)), dim3(128), 0, ctx->stream,
          (const G2M*)keys->g2->dev16, (const G2M*)keys->g2_a->dev16, (const G2M*)keys->g2_alpha_tbl->dev16, n_items, n_rows, item_row_off,
          item_hash_off, hash, (const rhip_fr*)zinv, (const rhip_fr*)rz, out_tk);
  HIP_TRY(ctx, hipMemsetAsync(work, 0, 2 * n_items * sizeof(rhip_fr), ctx->stream));
  return RHIP_OK;
}

// ------------------------------------------------------------------------------------------------ variable-base G2, rows sharing a scalar
// the split and the NAF masks, once per item (bn254/gls4.h): masks[24 i ..]
__global__ void __launch_bounds__(256, RB_MIN_WAVES) k_gls4_masks(size_t n, const rhip_fr* k, uint32_t* masks) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kk[8], m[24];
  ld_scalar(kk, k + i);
  gls4_masks(kk, m);
#pragma unroll
  for (int w = 0; w < 24; w++) masks[24 * i + w] = m[w];
}
// psi^i(P) of a lane: img[i * stride], Montgomery
struct Gls4Bases {
  const G2M* img;
  size_t stride;
  __device__ __forceinline__ G2Aff base(int i) const { return ld_g2_q(img + (size_t)i * stride); }
};
// one lane per row: out[t] = k[item of t] * p[t].  The lane computes the three images of its point once and keeps all four bases in
// global memory (img[i][lane], read back where an addition needs one -- the chain's accumulator and temporaries fill the register file);
// the masks are read through the item index, so the digit tests are uniform wherever a wave holds rows of one item.  Rows
// [row0, row0 + cnt) of the call; lanes past cnt shadow the last row with an image slot of their own (stride >= the launch's lanes).
__global__ void __launch_bounds__(128, RB_G2_WAVES) k_g2_mul_rows(size_t row0, size_t cnt, size_t n_items, const uint32_t* item_row_off, const rhip_g2* p,
                                                                 const uint32_t* masks, G2M* img, size_t stride, rhip_g2* out) {
  __shared__ uint32_t sh[2 * 8 * 128];
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = lane < cnt;
  const size_t t = row0 + (active ? lane : cnt - 1);
  const size_t item = owner_of(item_row_off, n_items, t);
  {
    const G2Aff P = load_g2(p[t].l);          // infinity (0, 0) maps to itself under psi and is skipped by every addition
    const G2Aff P2 = g2_frob2(P);
    st_g2_q(img + lane, P);
    st_g2_q(img + stride + lane, g2_frob1(P));
    st_g2_q(img + 2 * stride + lane, P2);
    st_g2_q(img + 3 * stride + lane, g2_frob1(P2));
  }
  const G2Jac acc = gls4_chain(Gls4Bases{img + lane, stride}, masks + 24 * item);
  store_g2_block128(sh, active, out + t, acc);
}
#define RB_G2_ROWS_CHUNK ((size_t)1 << 20)          // rows per launch: bounds the image workspace at 512 MB
extern "C" int32_t rhip_g2_mul_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* item_row_off, const rhip_g2* p, size_t n_items, const rhip_fr* k,
                                    rhip_g2* out) {
  NEED(ctx);
  if (!n_rows) return RHIP_OK;
  if (!n_items || !item_row_off || !p || !k || !out) return RHIP_ERR_ARG;
  void* masks = nullptr;
  void* img = nullptr;
  int32_t rc = rhip_ensure_work(ctx, WORK_ROWS_MASKS, n_items * 24 * sizeof(uint32_t), &masks);
  if (rc) return rc;
  const size_t stride = ((n_rows < RB_G2_ROWS_CHUNK ? n_rows : RB_G2_ROWS_CHUNK) + 127) / 128 * 128;
  rc = rhip_ensure_work(ctx, WORK_ROWS_IMAGES, stride * 4 * sizeof(G2M), &img);
  if (rc) return rc;
  KLAUNCH(ctx, "k_gls4_masks", k_gls4_masks, dim3(blocks_for(n_items, 256)), dim3(256), 0, ctx->stream, n_items, k, (uint32_t*)masks);
  for (size_t row0 = 0; row0 < n_rows; row0 += RB_G2_ROWS_CHUNK) {
    const size_t cnt = n_rows - row0 < RB_G2_ROWS_CHUNK ? n_rows - row0 : RB_G2_ROWS_CHUNK;
    KLAUNCH(ctx, "k_g2_mul_rows", k_g2_mul_rows, dim3(blocks_for(cnt, 128)), dim3(128), 0, ctx->stream, row0, cnt, n_items, item_row_off, p,
            (const uint32_t*)masks, (G2M*)img, stride, out);
  }
  return RHIP_OK;
}
// the split alone, on the host (the RB_HD code the kernel above runs): |k_i| as four little-endian words each, neg[i] = 1 for a negative k_i
extern "C" int32_t rhip_host_fr_split4(const rhip_fr* k, uint32_t mag[16], uint8_t neg_[4]) {
  if (!k || !mag || !neg_) return RHIP_ERR_ARG;
  uint32_t kk[8];
  for (int i = 0; i < 8; i++) kk[i] = k->l[i];
  for (int t = 0; t < 6; t++) {          // as ld_scalar: any 256-bit word is brought below r
    uint32_t d[8], borrow = 0;
    for (int i = 0; i < 8; i++) d[i] = subb32(kk[i], FrParams::mod(i), borrow);
    if (borrow) break;
    for (int i = 0; i < 8; i++) kk[i] = d[i];
  }
  uint32_t m[4][4];
  bool sg[4];
  gls4_split(kk, m, sg);
  for (int i = 0; i < 4; i++) {
    for (int w = 0; w < 4; w++) mag[4 * i + w] = m[i][w];
    neg_[i] = sg[i] ? 1 : 0;
  }
  return RHIP_OK;
}

// ------------------------------------------------------------------------------------------------ the same with a row index on both sides
// out[row_dst[t]] = k[item of t] * p[row_src[t]]: the rows of a call are ordered by scalar (the digit tests of a wave stay uniform) while
// the points are stored once per owner and the results land where the record writer wants them (each owner's rows adjacent).  The body of
// k_g2_mul_rows, repeated so that kernel's code object does not change.
__global__ void __launch_bounds__(128, RB_G2_WAVES) k_g2_mul_rows_at(size_t row0, size_t cnt, size_t n_items, const uint32_t* item_row_off, const rhip_g2* p,
                                                                    const uint32_t* row_src, const uint32_t* masks, G2M* img, size_t stride,
                                                                    const uint32_t* row_dst, rhip_g2* out) {
  __shared__ uint32_t sh[2 * 8 * 128];
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = lane < cnt;
  const size_t t = row0 + (active ? lane : cnt - 1);
  const size_t item = owner_of(item_row_off, n_items, t);
  {
    const G2Aff P = load_g2(p[row_src[t]].l);
    const G2Aff P2 = g2_frob2(P);
    st_g2_q(img + lane, P);
    st_g2_q(img + stride + lane, g2_frob1(P));
    st_g2_q(img + 2 * stride + lane, P2);
    st_g2_q(img + 3 * stride + lane, g2_frob1(P2));
  }
  const G2Jac acc = gls4_chain(Gls4Bases{img + lane, stride}, masks + 24 * item);
  store_g2_block128(sh, active, out + row_dst[t], acc);
}
extern "C" int32_t rhip_g2_mul_rows_at(rhip_ctx* ctx, size_t n_rows, const uint32_t* item_row_off, const rhip_g2* p, const uint32_t* row_src, size_t n_items,
                                       const rhip_fr* k, const uint32_t* row_dst, rhip_g2* out) {
  NEED(ctx);
  if (!n_rows) return RHIP_OK;
  if (!n_items || !item_row_off || !p || !row_src || !k || !row_dst || !out) return RHIP_ERR_ARG;
  void* masks = nullptr;
  void* img = nullptr;
  int32_t rc = rhip_ensure_work(ctx, WORK_ROWS_MASKS, n_items * 24 * sizeof(uint32_t), &masks);
  if (rc) return rc;
  const size_t stride = ((n_rows < RB_G2_ROWS_CHUNK ? n_rows : RB_G2_ROWS_CHUNK) + 127) / 128 * 128;
  rc = rhip_ensure_work(ctx, WORK_ROWS_IMAGES, stride * 4 * sizeof(G2M), &img);
  if (rc) return rc;
  KLAUNCH(ctx, "k_gls4_masks", k_gls4_masks, dim3(blocks_for(n_items, 256)), dim3(256), 0, ctx->stream, n_items, k, (uint32_t*)masks);
  for (size_t row0 = 0; row0 < n_rows; row0 += RB_G2_ROWS_CHUNK) {
    const size_t cnt = n_rows - row0 < RB_G2_ROWS_CHUNK ? n_rows - row0 : RB_G2_ROWS_CHUNK;
    KLAUNCH(ctx, "k_g2_mul_rows_at", k_g2_mul_rows_at, dim3(blocks_for(cnt, 128)), dim3(128), 0, ctx->stream, row0, cnt, n_items, item_row_off, p, row_src,
            (const uint32_t*)masks, (G2M*)img, stride, row_dst, out);
  }
  return RHIP_OK;
}

// ------------------------------------------------------------------------------------------------ variable-base G1, rows sharing a scalar
// GLV (bn254/curve.h: k = k1 + k2 lambda, |k1|, |k2| < 2^130) with the decomposition and the NAF masks made once per scalar:
// masks[20 i ..] = pos1[5], neg1[5], pos2[5], neg2[5], the signs of k1 / k2 folded in (a negative half swaps its two masks).
#define RB_GLV_MASK_WORDS 20
__global__ void __launch_bounds__(256, RB_MIN_WAVES) k_glv_masks(size_t n, const rhip_fr* k, uint32_t* masks) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kk[8], k1[8], k2[8], p1[8], n1[8], p2[8], n2[8];
  bool neg1, neg2;
  ld_scalar(kk, k + i);
  glv_decompose(kk, k1, neg1, k2, neg2);
  naf_masks(k1, p1, n1);
  naf_masks(k2, p2, n2);
  uint32_t* m = masks + RB_GLV_MASK_WORDS * i;
#pragma unroll
  for (int w = 0; w < 5; w++) {
    m[w] = neg1 ? n1[w] : p1[w];
    m[5 + w] = neg1 ? p1[w] : n1[w];
    m[10 + w] = neg2 ? n2[w] : p2[w];
    m[15 + w] = neg2 ? p2[w] : n2[w];
  }
}
// the joint chain of jac_mul_glv_g1 over P and phi(P) = (beta x, y), digits read from the scalar's masks: ~130 doublings + ~86 mixed additions.
// g1_madd_inl handles an infinite accumulator and the doubling / cancelling cases (k = 1, 2, lambda +- 1, ...); infinity in, infinity out.
__device__ __forceinline__ G1Jac glv_chain_rows(const G1Aff& base, const uint32_t* m) {
  G1Jac acc = jac_inf<Fp>();
  if (aff_is_inf(base)) return acc;
  constexpr uint32_t BETA[8] = RB_GLV_BETA;
  Fp beta;
#pragma unroll
  for (int i = 0; i < 8; i++) beta.v[i] = BETA[i];
  const Fp bx = mul(base.x, beta);
  bool started = false;
#pragma unroll 1
  for (int w = 4; w >= 0; w--) {
    const uint32_t pw1 = m[w], nw1 = m[5 + w], pw2 = m[10 + w], nw2 = m[15 + w];
    if (!started && !(pw1 | nw1 | pw2 | nw2)) continue;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      if (started) acc = g1_dbl_inl(acc);
      const uint32_t d1p = (pw1 >> b) & 1u, d1n = (nw1 >> b) & 1u, d2p = (pw2 >> b) & 1u, d2n = (nw2 >> b) & 1u;
      if (d1p | d1n) {
        acc = g1_madd_inl(acc, G1Aff{base.x, d1n ? neg(base.y) : base.y});
        started = true;
      }
      if (d2p | d2n) {
        acc = g1_madd_inl(acc, G1Aff{bx, d2n ? neg(base.y) : base.y});
        started = true;
      }
    }
  }
  return acc;
}
// one lane per row: out[row_dst ? row_dst[t] : t] = k[item of t] * p[row_src ? row_src[t] : t].  The masks are read through the item index,
// so the digit tests are uniform wherever a wave holds rows of one item.  One inversion per block; lanes past n_rows shadow the last row.
__global__ void __launch_bounds__(256, RB_G1_WAVES) k_g1_mul_rows(size_t n_rows, size_t n_items, const uint32_t* item_row_off, const rhip_g1* p,
                                                                 const uint32_t* row_src, const uint32_t* masks, const uint32_t* row_dst, rhip_g1* out) {
  __shared__ uint32_t lds[2 * 8 * 256];
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_rows;
  if (!active) t = n_rows - 1;
  const size_t item = owner_of(item_row_off, n_items, t);
  const G1Jac r = glv_chain_rows(load_g1(p[row_src ? row_src[t] : t].l), masks + RB_GLV_MASK_WORDS * item);
  const bool inf = !active || jac_is_inf(r);
  const Fp zinv = block_batch_inverse_n<256>(lds, inf ? one<FpParams>() : r.z);
  if (!active) return;
  store_g1(out[row_dst ? row_dst[t] : t].l, inf ? aff_inf<Fp>() : jac_to_aff_with_zinv(r, zinv));
}
static int32_t g1_mul_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* item_row_off, const rhip_g1* p, const uint32_t* row_src, size_t n_items,
                           const rhip_fr* k, const uint32_t* row_dst, rhip_g1* out) {
  void* masks = nullptr;
  const int32_t rc = rhip_ensure_work(ctx, WORK_G1_ROWS_MASKS, n_items * RB_GLV_MASK_WORDS * sizeof(uint32_t), &masks);
  if (rc) return rc;
  KLAUNCH(ctx, "k_glv_masks", k_glv_masks, dim3(blocks_for(n_items, 256)), dim3(256), 0, ctx->stream, n_items, k, (uint32_t*)masks);
  KLAUNCH(ctx, "k_g1_mul_rows", k_g1_mul_rows, dim3(blocks_for(n_rows, 256)), dim3(256), 0, ctx->stream, n_rows, n_items, item_row_off, p, row_src,
          (const uint32_t*)masks, row_dst, out);
  return RHIP_OK;
}
extern "C" int32_t rhip_g1_mul_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* item_row_off, const rhip_g1* p, size_t n_items, const rhip_fr* k,
                                    rhip_g1* out) {
  NEED(ctx);
  if (!n_rows) return RHIP_OK;
  if (!n_items || !item_row_off || !p || !k || !out) return RHIP_ERR_ARG;
  return g1_mul_rows(ctx, n_rows, item_row_off, p, nullptr, n_items, k, nullptr, out);
}
extern "C" int32_t rhip_g1_mul_rows_at(rhip_ctx* ctx, size_t n_rows, const uint32_t* item_row_off, const rhip_g1* p, const uint32_t* row_src, size_t n_items,
                                       const rhip_fr* k, const uint32_t* row_dst, rhip_g1* out) {
  NEED(ctx);
  if (!n_rows) return RHIP_OK;
  if (!n_items || !item_row_off || !p || !row_src || !k || !row_dst || !out) return RHIP_ERR_ARG;
  return g1_mul_rows(ctx, n_rows, item_row_off, p, row_src, n_items, k, row_dst, out);
}

// ------------------------------------------------------------------------------------------------ BDABE / MKE08 user keys
struct rhip_dnf_keys {
  rhip_ctx* ctx;
  rhip_g1_table* p1;
  rhip_g1_table* g1;
  rhip_g2_table* p2;
  rhip_g2_table* g2;
  rhip_g1* a1;          // device, wire form: the authority's a1 (MKE08: msk.g1)
  rhip_g2* a2;
};
extern "C" void rhip_dnf_keys_destroy(rhip_dnf_keys* k) {
  if (!k) return;
  rhip_g1_table_destroy(k->p1);
  rhip_g1_table_destroy(k->g1);
  rhip_g2_table_destroy(k->p2);
  rhip_g2_table_destroy(k->g2);
  if (k->a1) (void)hipFree(k->a1);
  if (k->a2) (void)hipFree(k->a2);
  delete k;
}
extern "C" int32_t rhip_dnf_keys_create(rhip_ctx* ctx, const rhip_g1* p1, const rhip_g1* g1, const rhip_g2* p2, const rhip_g2* g2, const rhip_g1* a1,
                                        const rhip_g2* a2, rhip_dnf_keys** out) {
  if (!ctx || !p1 || !g1 || !p2 || !g2 || !a1 || !a2 || !out) return RHIP_ERR_ARG;
  *out = nullptr;
  rhip_dnf_keys* k = new rhip_dnf_keys{ctx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int32_t rc = rhip_g1_table_create(ctx, p1, &k->p1);
  if (!rc) rc = rhip_g1_table_add_w16(ctx, k->p1);
  if (!rc) rc = rhip_g1_table_create(ctx, g1, &k->g1);
  if (!rc) rc = rhip_g1_table_add_w16(ctx, k->g1);
  if (!rc) rc = rhip_g2_table_create(ctx, p2, &k->p2);
  if (!rc) rc = rhip_g2_table_add_w16(ctx, k->p2);
  if (!rc) rc = rhip_g2_table_create(ctx, g2, &k->g2);
  if (!rc) rc = rhip_g2_table_add_w16(ctx, k->g2);
  if (!rc) {
    hipError_t he = hipMalloc((void**)&k->a1, sizeof(rhip_g1));
    if (he == hipSuccess) he = hipMemcpy(k->a1, a1, sizeof(rhip_g1), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMalloc((void**)&k->a2, sizeof(rhip_g2));
    if (he == hipSuccess) he = hipMemcpy(k->a2, a2, sizeof(rhip_g2), hipMemcpyHostToDevice);
    if (he != hipSuccess) rc = fail(ctx, he, "rhip_dnf_keys_create");
  }
  if (rc) { rhip_dnf_keys_destroy(k); return rc; }
  *out = k;
  return RHIP_OK;
}
// one lane per key element (bdabe/mod.rs:201-222, mke08/mod.rs:185-206); item i owns rows 2 i, 2 i + 1 of each group:
//   row 2 i:     sk.u1 = a1 + p1 * r_i     (G2: sk.u2 = a2 + p2 * r_i)
//   row 2 i + 1: pk.u1 = g1 * r_i          (G2: pk.u2 = g2 * r_i)
// Every element is one walk over the 16-bit windows of its base; one inversion per block.
__global__ void __launch_bounds__(256, RB_G1_WAVES) k_dnf_keygen_g1(const G1M* p1_tbl, const G1M* g1_tbl, const rhip_g1* a1, size_t n_rows, const rhip_fr* r,
                                                                   rhip_g1* out) {
  __shared__ uint32_t lds[2 * 8 * 256];
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_rows;
  if (!active) t = n_rows - 1;
  uint32_t kk[8];
  ld_scalar(kk, r + (t >> 1));
  G1Jac acc = table_mul_g1_w16((t & 1) ? g1_tbl : p1_tbl, kk);
  if (!(t & 1)) acc = g1_madd_inl(acc, load_g1(a1->l));
  const bool inf = !active || jac_is_inf(acc);
  const Fp zinv = block_batch_inverse_n<256>(lds, inf ? one<FpParams>() : acc.z);
  if (!active) return;
  store_g1(out[t].l, inf ? aff_inf<Fp>() : jac_to_aff_with_zinv(acc, zinv));
}
__global__ void __launch_bounds__(128, RB_G2_WAVES) k_dnf_keygen_g2(const G2M* p2_tbl, const G2M* g2_tbl, const rhip_g2* a2, size_t n_rows, const rhip_fr* r,
                                                                   rhip_g2* out) {
  __shared__ uint32_t sh[2 * 8 * 128];
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_rows;
  if (!active) t = n_rows - 1;
  uint32_t kk[8];
  ld_scalar(kk, r + (t >> 1));
  G2Jac a = table_mul_g2_w16((t & 1) ? g2_tbl : p2_tbl, kk);
  if (!(t & 1)) a = jac_add_aff(a, load_g2(a2->l));
  store_g2_block128(sh, active, out + t, a);
}
extern "C" int32_t rhip_dnf_keygen_batch(rhip_ctx* ctx, const rhip_dnf_keys* keys, size_t n_items, const rhip_fr* r, rhip_g1* out_g1, rhip_g2* out_g2) {
  NEED(ctx);
  if (!keys) return RHIP_ERR_ARG;
  if (!n_items) return RHIP_OK;
  if (!r || !out_g1 || !out_g2) return RHIP_ERR_ARG;
  const size_t n_rows = 2 * n_items;
  KLAUNCH(ctx, "k_dnf_keygen_g1", k_dnf_keygen_g1, dim3(blocks_for(n_rows, 256)), dim3(256), 0, ctx->stream, (const G1M*)keys->p1->dev16,
          (const G1M*)keys->g1->dev16, (const rhip_g1*)keys->a1, n_rows, r, out_g1);
  KLAUNCH(ctx, "k_dnf_keygen_g2", k_dnf_keygen_g2, dim3(blocks_for(n_rows, 128)), dim3(128), 0, ctx->stream, (const G2M*)keys->p2->dev16,
          (const G2M*)keys->g2->dev16, (const rhip_g2*)keys->a2, n_rows, r, out_g2);
  return RHIP_OK;
}

// ------------------------------------------------------------------------------------------------ LSW ciphertext rows
// the lane routine and the three-point conversion are host + device code (bn254/lsw_rows.h): the CPU check runs the same text
struct W16Table {
  const G1M* t;
  __device__ __forceinline__ G1Aff entry(int w, uint32_t d) const { return ld_g1_m(t + (size_t)w * TBL16_DIGITS + (d - 1)); }
};
// one lane per ciphertext row (lsw/mod.rs:201-208); row t belongs to the item i with item_row_off[i] <= t < item_row_off[i+1], its
// attribute hash is h = hash[item_hash_off[i] + t - item_row_off[i]], its scalar sx[t]:
//   out[3 t]     = e3 = g1 * (h secret_i)
//   out[3 t + 1] = e4 = g1_b * sx
//   out[3 t + 2] = e5 = g1_b2 * (sx h) + h_b * sx          both walks on ONE accumulator (no point buffer, no separate addition)
// The two products are formed in the lane.  ONE accumulator is live at a time: e3 and e4 are PARKED, as Jacobian Montgomery values, in the
// row's own output slots (3 x 64 B of affine output = 2 x 96 B) while the next element is walked, and read back into registers before the
// first affine point is stored over them.  The three conversions of a lane share one inversion, and the block's lanes share theirs: ONE
// field inversion per block.  An element that is the identity -- sx = 0 (the row of a one-attribute list, as the reference's loop is written),
// h secret = 0, or the two halves of e5 cancelling -- enters the shared product as one and is stored as 64 zero bytes (bn254/lsw_rows.h).
__global__ void __launch_bounds__(RB_ROWS_BLOCK, 2) k_lsw_enc_rows(const G1M* g1_tbl, const G1M* g1b_tbl, const G1M* g1b2_tbl, const G1M* hb_tbl, size_t n_items,
                                                                   size_t total_rows, const uint32_t* item_row_off, const uint32_t* item_hash_off,
                                                                   const rhip_fr* hash, const rhip_fr* secret, const rhip_fr* sx, rhip_g1* out) {
  __shared__ uint32_t sh[2 * 8 * RB_ROWS_BLOCK];
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < total_rows;
  if (!active) t = total_rows - 1;          // inactive lanes shadow the last row (no stores) and still join the block inversion
  const size_t item = owner_of(item_row_off, n_items, t);
  const rhip_fr* hp = hash + ((size_t)item_hash_off[item] + (t - item_row_off[item]));
  G1Jac* park = (G1Jac*)(out + 3 * t);
  G1Jac r = lsw_row_e3(W16Table{g1_tbl}, load_fr(hp->l), load_fr(secret[item].l));
  if (active) park[0] = r;
  uint32_t kk[8];
  ld_scalar(kk, sx + t);
  r = lsw_row_e4(W16Table{g1b_tbl}, kk);
  if (active) park[1] = r;
  r = lsw_row_e5(W16Table{g1b2_tbl}, W16Table{hb_tbl}, load_fr(hp->l), kk);
  G1Jac a = jac_inf<Fp>(), b = jac_inf<Fp>();
  if (active) { a = park[0]; b = park[1]; }
  G1Three z;
  const Fp abc = g1_three_product(z, a, b, r);
  const Fp inv_abc = block_batch_inverse_n<RB_ROWS_BLOCK>(sh, active ? abc : one<FpParams>());
  if (!active) return;
  G1Aff e[3];
  g1_three_to_aff(z, inv_abc, a, b, r, e);
  store_g1(out[3 * t].l, e[0]);
  store_g1(out[3 * t + 1].l, e[1]);
  store_g1(out[3 * t + 2].l, e[2]);
}
static_assert(2 * sizeof(G1Jac) == 3 * sizeof(rhip_g1), "two parked Jacobian points fill a row's three output records");
extern "C" int32_t rhip_lsw_encrypt_rows(rhip_ctx* ctx, const rhip_g1_table* g1, const rhip_g1_table* g1_b, const rhip_g1_table* g1_b2, const rhip_g1_table* h_b,
                                         size_t n_items, size_t total_rows, const uint32_t* item_row_off, const uint32_t* item_hash_off, const rhip_fr* hash,
                                         const rhip_fr* secret, const rhip_fr* sx, rhip_g1* out) {
  NEED(ctx);
  if (!g1 || !g1_b || !g1_b2 || !h_b) return RHIP_ERR_ARG;
  if (!n_items || !total_rows) return RHIP_OK;
  if (!item_row_off || !item_hash_off || !hash || !secret || !sx || !out) return RHIP_ERR_ARG;
  if (!g1->dev16 || !g1_b->dev16 || !g1_b2->dev16 || !h_b->dev16)
    return fail(ctx, hipErrorInvalidValue, "rhip_lsw_encrypt_rows: the G1 tables have no 16-bit windows (rhip_g1_table_add_w16)");
  KLAUNCH(ctx, "k_lsw_enc_rows", k_lsw_enc_rows, dim3(blocks_for(total_rows, RB_ROWS_BLOCK)), dim3(RB_ROWS_BLOCK), 0, ctx->stream, (const G1M*)g1->dev16,
          (const G1M*)g1_b->dev16, (const G1M*)g1_b2->dev16, (const G1M*)h_b->dev16, n_items, total_rows, item_row_off, item_hash_off, hash, secret, sx, out);
  return RHIP_OK;
}
