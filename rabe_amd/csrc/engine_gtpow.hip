// engine_gtpow.hip -- variable-base Gt powers over rows that share an exponent: the four-way split over the Frobenius map
// (bn254/gtpow4.h), which serves the GHW11 key-encapsulation calls (one t^-z per item of a call, every item under the one z).
//
// A translation unit of its own: docs/rr29.md records that adding a kernel to a unit can move its neighbours' register allocation, and the
// other units' instruction streams are what was measured.
#include "engine_internal.h"
#include "bn254/gtpow4.h"

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
  int32_t rc = rhip_ensure_work(ctx, 16, mask_bytes, &masks);
  if (rc) return rc;
  const size_t stride = ((n_rows < RB_GT_ROWS_CHUNK ? n_rows : RB_GT_ROWS_CHUNK) + 63) / 64 * 64;
  rc = rhip_ensure_work(ctx, 17, stride * 4 * sizeof(GtM), &img);
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
