// engine_gtpow.hip -- variable-base Gt powers over rows that share an exponent: the four-way split over the Frobenius map
// (bn254/gtpow4.h), which serves the GHW11 key-encapsulation calls (one t^-z per item of a call, every item under the one z); and Gt
// multi-exponentiations over width-4 signed windows (bn254/gtmexp4.h): rhip_gt_multiexp_rows, and the leading factor of
// rhip_aw11_decrypt_batch_w4.
//
// A translation unit of its own: docs/rr29.md records that adding a kernel to a unit can move its neighbours' register allocation, and the
// other units' instruction streams are what was measured.
#include "engine_internal.h"
#include "bn254/gtpow4.h"
#include "bn254/gtmexp4.h"

// item owning flat index t: the i with off[i] <= t < off[i+1] (off non-decreasing, off[0] <= t < off[n])
__device__ __forceinline__ size_t owner_of(const uint32_t* off, size_t n, size_t t) {
  size_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// the split and the NAF masks, once per item: masks[24 i ..], the digits of -k[i] when `invert`
__global__ void __launch_bounds__(256, RB_MIN_WAVES) k_gtpow4_masks(size_t n, const rhip_fr* k, uint32_t invert, uint32_t* masks) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kk[8], m[24];
#pragma unroll
  for (int w = 0; w < 8; w++) kk[w] = k[i].l[w];
  gtpow4_masks(kk, invert != 0, m);
#pragma unroll
  for (int w = 0; w < 24; w++) masks[24 * i + w] = m[w];
}
// a^(p^i) of a lane: img[i * stride], Montgomery
struct GtPow4Bases {
  const GtM* img;
  size_t stride;
  __device__ __forceinline__ GtMOperand operand(int i, bool conj) const { return GtMOperand{img + (size_t)i * stride, conj}; }
};
// a multiplicand in wire form, converted where a multiplication fetches it
struct GtWireOperand {
  const rhip_gt* e;
  __device__ __forceinline__ Fp6 half(int h) const {
    const uint32_t* p = e->l + 48 * h;
    return Fp6{load_fp2(p), load_fp2(p + 16), load_fp2(p + 32)};
  }
};
// one lane per row: out[t] = (mul ? mul[t] : 1) * a[t]^(+-k[item of t]).  The lane computes the three Frobenius images of its base once and
// keeps all four columns in global memory (img[i][lane], read back where a multiplication needs one); the accumulator lives in the lane's
// LDS home (engine_internal.h: blocks of ONE wave), squared and multiplied in place -- the shape of the fixed-base Gt table kernels.  The
// masks are read through the item index, so the digit tests are uniform wherever a wave holds rows of one item.  Rows [row0, row0 + cnt)
// of the call; lanes past cnt leave (no barrier in this kernel).  A lane reads a[t] first and mul[t] last, before its one store: out may
// be a or mul.
__global__ void __launch_bounds__(64, RB_MIN_WAVES) k_gt_pow_rows(size_t row0, size_t cnt, size_t n_items, const uint32_t* item_row_off, const rhip_gt* a,
                                                                 const uint32_t* masks, GtM* img, size_t stride, const rhip_gt* mul_in, rhip_gt* out) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= cnt) return;
  const size_t t = row0 + lane;
  const size_t item = owner_of(item_row_off, n_items, t);
  {
    const Fp12 A = load_gt(a[t].l);
    st_gt_m(img + lane, A);
    st_gt_m(img + stride + lane, fp12_frob_fn(A, 1));
    st_gt_m(img + 2 * stride + lane, fp12_frob_fn(A, 2));
    st_gt_m(img + 3 * stride + lane, fp12_frob_fn(A, 3));
  }
  const LdsHome home{};
  bool started = gt_pow_split4(home, GtPow4Bases{img + lane, stride}, masks + 24 * item);
  if (mul_in) {
    if (started) facc_mul(home, GtWireOperand{mul_in + t});
    else { facc_set(home, GtWireOperand{mul_in + t}); started = true; }
  }
  store_gt(out[t].l, home_result(started));
}
#define RB_GT_ROWS_CHUNK ((size_t)1 << 17)          // rows per launch: bounds the image workspace at 192 MB
extern "C" int32_t rhip_gt_pow_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* item_row_off, const rhip_gt* a, size_t n_items, const rhip_fr* k,
                                    const rhip_gt* mul_in, uint32_t flags, rhip_gt* out) {
  NEED(ctx);
  if (flags & ~RHIP_GT_POW_INVERT) return RHIP_ERR_ARG;
  if (!n_rows) return RHIP_OK;
  if (!n_items || !item_row_off || !a || !k || !out) return RHIP_ERR_ARG;
  // the masks and the images take the two slots of rhip_g2_mul_rows (scratch of one call, in stream order on this context)
  void* masks = nullptr;
  void* img = nullptr;
  const size_t mask_bytes = n_items * 24 * sizeof(uint32_t);
  int32_t rc = rhip_ensure_work(ctx, WORK_ROWS_MASKS, mask_bytes, &masks);
  if (rc) return rc;
  const size_t stride = ((n_rows < RB_GT_ROWS_CHUNK ? n_rows : RB_GT_ROWS_CHUNK) + 63) / 64 * 64;
  rc = rhip_ensure_work(ctx, WORK_ROWS_IMAGES, stride * 4 * sizeof(GtM), &img);
  if (rc) return rc;
  KLAUNCH(ctx, "k_gtpow4_masks", k_gtpow4_masks, dim3(blocks_for(n_items, 256)), dim3(256), 0, ctx->stream, n_items, k, flags & RHIP_GT_POW_INVERT,
          (uint32_t*)masks);
  for (size_t row0 = 0; row0 < n_rows; row0 += RB_GT_ROWS_CHUNK) {
    const size_t cnt = n_rows - row0 < RB_GT_ROWS_CHUNK ? n_rows - row0 : RB_GT_ROWS_CHUNK;
    KLAUNCH(ctx, "k_gt_pow_rows", k_gt_pow_rows, dim3(blocks_for(cnt, 64)), dim3(64), 0, ctx->stream, row0, cnt, n_items, item_row_off, a,
            (const uint32_t*)masks, (GtM*)img, stride, mul_in, out);
  }
  // the masks are the exponents in another form (a transform key's z): zeroed behind the row kernel
  HIP_TRY(ctx, hipMemsetAsync(masks, 0, mask_bytes, ctx->stream));
  return RHIP_OK;
}

// ------------------------------------------------------------------------------------------------ multi-exponentiation, width-4 windows
// out[i] = (mul) * prod over the item's terms of base^(+-k) (bn254/gtmexp4.h): the digits once per scalar, the table x, x^3, x^5, x^7 once
// per term, then the two-kernel shape of k_gt_multiexp_partial / k_gt_lead (engine_jobs.hip) -- lane (chunk, item) walks its chunk on one
// chain of cyclotomic squarings, a finish lane per item multiplies the L partial products.  The accumulator lives in the lane's LDS home,
// table entries are fetched from HBM where a multiplication consumes them.
__global__ void __launch_bounds__(256, RB_MIN_WAVES) k_gtmexp4_digits(size_t n, const rhip_fr* k, uint32_t invert, uint32_t* dg) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kk[8];
#pragma unroll
  for (int w = 0; w < 8; w++) kk[w] = k[i].l[w];
  gtmexp4_digits(kk, invert != 0, dg + RB_GTMEXP4_WORDS * i);
}
struct GtMexp4Slots {
  GtM* tbl;
  __device__ __forceinline__ GtMOperand entry(int i) const { return GtMOperand{tbl + i}; }
  __device__ __forceinline__ void put(int i, const Fp12& v) const { st_gt_m(tbl + i, v); }
};
// lane = term: tbl[4 t ..] = x, x^3, x^5, x^7 (Montgomery) of the term's base, read in wire form (a_wire) or in Montgomery form (a_mont)
__global__ void __launch_bounds__(64, RB_MIN_WAVES) k_gtmexp4_table(size_t n_terms, const rhip_gt* a_wire, const GtM* a_mont, GtM* tbl) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_terms) return;
  GtM* mine = tbl + RB_GTMEXP4_TABLE * t;
  st_gt_m(mine, a_wire ? load_gt(a_wire[t].l) : ld_gt_m(a_mont + t));
  gt_mexp4_table(LdsHome{}, GtMexp4Slots{mine});
}
struct GtMexp4Terms {
  const GtM* tbl;            // of the chunk's first term
  const uint32_t* dg;        // of the chunk's first scalar
  int cnt;
  __device__ __forceinline__ int count() const { return cnt; }
  __device__ __forceinline__ uint32_t digit_word(int j, int w) const { return dg[RB_GTMEXP4_WORDS * j + w]; }
  __device__ __forceinline__ GtMOperand entry(int j, int i, bool conj) const { return GtMOperand{tbl + RB_GTMEXP4_TABLE * j + i, conj}; }
};
// lane t = chunk * n_items + item: the product over terms [term_off[item] + c C, ...) of the item, at most C of them; the scalars of item
// i start at k_start[i] (term_off[i] when k_start is NULL).  A lane whose chunk is empty writes 1.
__global__ void __launch_bounds__(64, RB_MIN_WAVES) k_gt_mexp4_partial(size_t n_items, uint32_t L, uint32_t C, const uint32_t* term_off, const uint32_t* k_start,
                                                                      const GtM* tbl, const uint32_t* dg, GtM* part) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items * L) return;
  const size_t c = t / n_items, item = t % n_items;
  const uint32_t lo = term_off[item], hi = term_off[item + 1];
  const uint64_t first = (uint64_t)lo + (uint64_t)c * C;
  int cnt = 0;
  if (first < hi) cnt = (int)((hi - first < C) ? (hi - first) : C);
  const size_t k0 = (size_t)(k_start ? k_start[item] : lo) + c * C;
  const bool started = gt_mexp4_chunk(LdsHome{}, GtMexp4Terms{tbl + RB_GTMEXP4_TABLE * first, dg + RB_GTMEXP4_WORDS * k0, cnt});
  st_gt_m(part + item * L + c, home_result(started));
}
// out[i] = (mul ? mul[i] : 1) * prod_c part[i][c], canonical.  mul[i] is read before the one store: out may be mul.
__global__ void __launch_bounds__(64, RB_MIN_WAVES) k_gt_mexp4_finish(size_t n_items, uint32_t L, const rhip_gt* mul, const GtM* part, rhip_gt* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  Fp12 acc = mul ? load_gt(mul[i].l) : ld_gt_m(part + i * L);
  for (uint32_t c = mul ? 0 : 1; c < L; c++) acc = fp12_mul_fn(acc, ld_gt_m(part + i * L + c));
  store_gt(out[i].l, acc);
}
int32_t rhip_gt_mexp4_run(rhip_ctx* ctx, size_t n_items, size_t max_terms, size_t n_terms, const uint32_t* term_off, const rhip_gt* a_wire, const GtM* a_mont,
                          size_t n_k, const rhip_fr* k, const uint32_t* k_start, const rhip_gt* mul, uint32_t flags, uint32_t chunk_terms, rhip_gt* out) {
  if (!n_items) return RHIP_OK;
  if (n_terms && ((!a_wire) == (!a_mont) || !k || !n_k)) return RHIP_ERR_ARG;
  uint32_t L, C;
  if (chunk_terms) {
    C = chunk_terms;
    L = (uint32_t)(((max_terms ? max_terms : 1) + C - 1) / C);
  } else {
    rb_gtmexp4_chunks((size_t)ctx->n_cu * 4, n_items, max_terms, &L, &C);
  }
  void *dg = nullptr, *tbl = nullptr, *part = nullptr;
  const size_t dg_bytes = (n_k ? n_k : 1) * RB_GTMEXP4_WORDS * sizeof(uint32_t);
  int32_t rc = rhip_ensure_work(ctx, WORK_GTMEXP4_DIGITS, dg_bytes, &dg);
  if (!rc) rc = rhip_ensure_work(ctx, WORK_GTMEXP4_TABLES, (n_terms ? n_terms : 1) * RB_GTMEXP4_TABLE * sizeof(GtM), &tbl);
  if (!rc) rc = rhip_ensure_work(ctx, WORK_GTMEXP4_PARTS, n_items * L * sizeof(GtM), &part);
  if (rc) return rc;
  if (n_k)
    KLAUNCH(ctx, "k_gtmexp4_digits", k_gtmexp4_digits, dim3(blocks_for(n_k, 256)), dim3(256), 0, ctx->stream, n_k, k, flags & RHIP_GT_POW_INVERT, (uint32_t*)dg);
  if (n_terms)
    KLAUNCH(ctx, "k_gtmexp4_table", k_gtmexp4_table, dim3(blocks_for(n_terms, 64)), dim3(64), 0, ctx->stream, n_terms, a_wire, a_mont, (GtM*)tbl);
  KLAUNCH(ctx, "k_gt_mexp4_partial", k_gt_mexp4_partial, dim3(blocks_for(n_items * L, 64)), dim3(64), 0, ctx->stream, n_items, L, C, term_off, k_start,
          (const GtM*)tbl, (const uint32_t*)dg, (GtM*)part);
  KLAUNCH(ctx, "k_gt_mexp4_finish", k_gt_mexp4_finish, dim3(blocks_for(n_items, 64)), dim3(64), 0, ctx->stream, n_items, L, mul, (const GtM*)part, out);
  // the digits are the scalars in another form (Lagrange coefficients derive from a key's attribute set): zeroed behind the kernels
  if (n_k) HIP_TRY(ctx, hipMemsetAsync(dg, 0, dg_bytes, ctx->stream));
  return RHIP_OK;
}
extern "C" int32_t rhip_gt_multiexp_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* item_row_off, const rhip_gt* a, const rhip_fr* k, size_t n_items,
                                         const rhip_gt* mul, uint32_t flags, uint32_t chunk_terms, rhip_gt* out) {
  NEED(ctx);
  if (flags & ~RHIP_GT_POW_INVERT) return RHIP_ERR_ARG;
  if (!n_items) return n_rows ? RHIP_ERR_ARG : RHIP_OK;
  if (!item_row_off || !out || (n_rows && (!a || !k)) || n_rows > 0xFFFFFFFFull) return RHIP_ERR_ARG;
  // the chunking needs the longest item: the offsets come back once (4 (n_items + 1) bytes, the call's one synchronisation) and are
  // checked on the way -- the kernels index the rows through them
  std::vector<uint32_t> off(n_items + 1);
  HIP_TRY(ctx, hipMemcpyAsync(off.data(), item_row_off, off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (off[0] != 0 || off[n_items] != n_rows) return RHIP_ERR_ARG;
  size_t max_terms = 0;
  for (size_t i = 0; i < n_items; i++) {
    if (off[i] > off[i + 1]) return RHIP_ERR_ARG;
    if ((size_t)(off[i + 1] - off[i]) > max_terms) max_terms = off[i + 1] - off[i];
  }
  return rhip_gt_mexp4_run(ctx, n_items, max_terms, n_rows, item_row_off, a, nullptr, n_rows, k, nullptr, mul, flags, chunk_terms, out);
}
