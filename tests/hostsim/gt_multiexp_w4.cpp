// TEST INFRASTRUCTURE: the Gt multi-exponentiation over width-4 signed windows (rabe_amd/csrc/bn254/gtmexp4.h: what k_gtmexp4_digits,
// k_gtmexp4_table, k_gt_mexp4_partial and k_gt_mexp4_finish run per lane) on the CPU, beside the plain NAF walk of k_gt_multiexp_partial +
// k_gt_lead restated over the same headers' naf_masks / fp12_cyclotomic_sqr / fp12_mul.  Stand-alone (own main, no Python loading): it can
// be built with a host sanitizer.  Driven by tests/test_gt_multiexp_w4_host.py, which holds the oracle's answers.
//
// stdin:  a mode word (4 bytes), then
//   mode 0 (digits):   records of 36 bytes: k (32, any 256-bit little-endian word), flags (4: bit 0 invert)
//   mode 1 (products): per item  n_terms (4), C (4: terms per chunk, >= 1), flags (4: bit 0 invert, bit 1 multiply by mul), mul (384,
//                      canonical wire form), then n_terms x (a (384), k (32)).
// stdout: mode 0: 128 bytes per record, the 32 digit words;  mode 1: 384 + 384 bytes per item, the windowed routine's result and the
//         NAF walk's.
// exit:   0 when the two routines agree on every item, 1 otherwise, 2 on malformed input.
// Built with -DRB_COUNT_MULS it prints per item the Fp multiplications of both routines on stderr (conversions of the harness not
// counted): "muls item=.. w4=.. w4_table=.. w4_walk=.. w4_finish=.. naf=.. naf_walk=.. naf_finish=..".
#include "../../rabe_amd/csrc/bn254/io.h"
#include "../../rabe_amd/csrc/bn254/gtmexp4.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#ifdef RB_COUNT_MULS
extern "C" { unsigned long long rb_mul_counter = 0; }
#endif

using namespace rabe::bn254;

// the accumulator's home (LDS on the device): two halves + the parked Fq6
struct HostHome {
  Fp6* F;
  Fp6 ld_f6(int h) const { return F[h]; }
  void st_f6(int h, const Fp6& v) const { F[h] = v; }
  Fp6 ld_x() const { return F[2]; }
  void st_x(const Fp6& v) const { F[2] = v; }
  Fp2 ld_f2(int i) const { return (&F[i / 3].a0)[i % 3]; }
  void st_f2(int i, const Fp2& v) const { (&F[i / 3].a0)[i % 3] = v; }
  void fence() const {}
};
struct HostOperand {
  const Fp12* e;
  bool conj;
  Fp6 half(int h) const { return h ? (conj ? fp6_neg(e->c1) : e->c1) : e->c0; }
};
// the four entries of one base, kept in memory as the kernel keeps them
struct HostSlots {
  Fp12* tbl;
  HostOperand entry(int i) const { return HostOperand{tbl + i, false}; }
  void put(int i, const Fp12& v) const { tbl[i] = v; }
};
struct HostTerms {
  const Fp12* tbl;          // 4 per term
  const uint32_t* dg;       // 32 per term
  int cnt;
  int count() const { return cnt; }
  uint32_t digit_word(int j, int w) const { return dg[RB_GTMEXP4_WORDS * j + w]; }
  HostOperand entry(int j, int i, bool conj) const { return HostOperand{tbl + RB_GTMEXP4_TABLE * j + i, conj}; }
};

static unsigned long long counter() {
#ifdef RB_COUNT_MULS
  return rb_mul_counter;
#else
  return 0;
#endif
}

static bool read_exact(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }

// what k_naf_masks writes for a scalar word: the masks of the SHORTER of k and r - k, exchanged when the scalar was negated
static void naf_entry(const uint32_t k_in[8], uint32_t m[16]) {
  uint32_t k[8], d[8];
  memcpy(k, k_in, 32);
  for (int t = 0; t < 5; t++) {
    uint32_t borrow = 0;
    for (int i = 0; i < 8; i++) d[i] = subb32(k[i], FrParams::mod(i), borrow);
    if (borrow) break;
    memcpy(k, d, 32);
  }
  bool zero = true;
  for (int i = 0; i < 8; i++) zero = zero && !k[i];
  uint32_t borrow = 0, ng[8];
  for (int i = 0; i < 8; i++) ng[i] = subb32(FrParams::mod(i), k[i], borrow);
  bool flip = false;
  if (!zero) {
    for (int i = 7; i >= 0; i--) {
      if (ng[i] != k[i]) { flip = ng[i] < k[i]; break; }
    }
  }
  if (flip) memcpy(k, ng, 32);
  uint32_t pos[8], neg_[8];
  naf_masks(k, pos, neg_);
  for (int w = 0; w < 8; w++) { m[w] = flip ? neg_[w] : pos[w]; m[8 + w] = flip ? pos[w] : neg_[w]; }
}

int main() {
  uint32_t mode;
  if (!read_exact(&mode, 4) || mode > 1) return 2;
  if (mode == 0) {
    uint32_t rec[9];
    size_t got;
    while ((got = fread(rec, 1, 36, stdin)) == 36) {
      uint32_t dg[RB_GTMEXP4_WORDS];
      gtmexp4_digits(rec, (rec[8] & 1u) != 0, dg);
      if (fwrite(dg, 1, sizeof(dg), stdout) != sizeof(dg)) return 2;
    }
    return got ? 2 : 0;
  }
  size_t bad = 0, item = 0;
  for (;; item++) {
    uint32_t head[3];
    const size_t got = fread(head, 1, 12, stdin);
    if (got == 0) break;
    if (got != 12 || head[1] < 1) return 2;
    const uint32_t n_terms = head[0], C = head[1];
    const bool invert = (head[2] & 1u) != 0, has_mul = (head[2] & 2u) != 0;
    std::vector<uint32_t> raw(96 + (size_t)n_terms * 104);
    if (!read_exact(raw.data(), raw.size() * 4)) return 2;
    const Fp12 mul_in = load_gt(raw.data());
    std::vector<Fp12> a(n_terms);
    for (uint32_t t = 0; t < n_terms; t++) a[t] = load_gt(raw.data() + 96 + 104 * (size_t)t);
    auto scalar = [&](uint32_t t) { return raw.data() + 96 + 104 * (size_t)t + 96; };
    const uint32_t L = n_terms ? (n_terms + C - 1) / C : 1;
    uint32_t out[192];
    unsigned long long w4_table, w4_walk, w4_finish, naf_walk, naf_finish;
    {
      // digits and tables once per term, a lane per chunk, the finish over the L partials
      unsigned long long c0 = counter();
      std::vector<uint32_t> dg((size_t)n_terms * RB_GTMEXP4_WORDS);
      std::vector<Fp12> tbl((size_t)n_terms * RB_GTMEXP4_TABLE);
      Fp6 F[3];
      const HostHome home{F};
      for (uint32_t t = 0; t < n_terms; t++) {
        gtmexp4_digits(scalar(t), invert, dg.data() + (size_t)RB_GTMEXP4_WORDS * t);
        tbl[(size_t)RB_GTMEXP4_TABLE * t] = a[t];
        gt_mexp4_table(home, HostSlots{tbl.data() + (size_t)RB_GTMEXP4_TABLE * t});
      }
      w4_table = counter() - c0;
      c0 = counter();
      std::vector<Fp12> part(L);
      for (uint32_t c = 0; c < L; c++) {
        const uint32_t first = c * C;
        const int cnt = first < n_terms ? (int)(n_terms - first < C ? n_terms - first : C) : 0;
        const bool started = gt_mexp4_chunk(home, HostTerms{tbl.data() + (size_t)RB_GTMEXP4_TABLE * first, dg.data() + (size_t)RB_GTMEXP4_WORDS * first, cnt});
        part[c] = started ? facc_get(home) : fp12_one();
      }
      w4_walk = counter() - c0;
      c0 = counter();
      Fp12 acc = has_mul ? fp12_mul_fn(mul_in, part[0]) : part[0];
      for (uint32_t c = 1; c < L; c++) acc = fp12_mul_fn(acc, part[c]);
      w4_finish = counter() - c0;
      store_gt(out, acc);
    }
    {
      // k_gt_multiexp_partial (flip = invert) and k_gt_lead on the same chunks
      unsigned long long c0 = counter();
      std::vector<uint32_t> masks((size_t)n_terms * 16);
      for (uint32_t t = 0; t < n_terms; t++) naf_entry(scalar(t), masks.data() + 16 * (size_t)t);
      std::vector<Fp12> part(L);
      for (uint32_t c = 0; c < L; c++) {
        const uint32_t first = c * C;
        const int cnt = first < n_terms ? (int)(n_terms - first < C ? n_terms - first : C) : 0;
        const uint32_t* mk = masks.data() + 16 * (size_t)first;
        Fp12 acc = fp12_one();
        bool started = false;
        for (int w = 7; w >= 0; w--)
          for (int bit = 31; bit >= 0; bit--) {
            if (started) acc = fp12_cyclotomic_sqr(acc);
            for (int j = 0; j < cnt; j++) {
              const uint32_t pw = mk[16 * j + (invert ? 8 : 0) + w], nw = mk[16 * j + (invert ? 0 : 8) + w];
              const uint32_t pb = (pw >> bit) & 1u, nb = (nw >> bit) & 1u;
              if (pb | nb) {
                Fp12 x = a[first + j];
                if (nb) x = fp12_conj(x);
                acc = started ? fp12_mul(acc, x) : x;
                started = true;
              }
            }
          }
        part[c] = acc;
      }
      naf_walk = counter() - c0;
      c0 = counter();
      Fp12 acc = has_mul ? fp12_mul_fn(mul_in, part[0]) : part[0];
      for (uint32_t c = 1; c < L; c++) acc = fp12_mul_fn(acc, part[c]);
      naf_finish = counter() - c0;
      store_gt(out + 96, acc);
    }
    if (memcmp(out, out + 96, 384) != 0 && bad++ < 8) fprintf(stderr, "gt_multiexp_w4: item %zu differs\n", item);
    if (fwrite(out, 1, sizeof(out), stdout) != sizeof(out)) return 2;
#ifdef RB_COUNT_MULS
    fprintf(stderr, "muls item=%zu terms=%u C=%u w4=%llu w4_table=%llu w4_walk=%llu w4_finish=%llu naf=%llu naf_walk=%llu naf_finish=%llu\n", item, n_terms, C,
            w4_table + w4_walk + w4_finish, w4_table, w4_walk, w4_finish, naf_walk + naf_finish, naf_walk, naf_finish);
#else
    (void)w4_table; (void)w4_walk; (void)w4_finish; (void)naf_walk; (void)naf_finish;
#endif
  }
  fprintf(stderr, "gt_multiexp_w4: %zu items, %zu differ\n", item, bad);
  return bad ? 1 : 0;
}
