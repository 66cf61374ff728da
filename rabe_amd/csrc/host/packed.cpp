// Packed batch entry points (include/rabe_host.h: rabe_*_packed): n independent calls of one of the reference's scheme functions with ONE blob
// of canonical records + offsets on each side of the boundary, fed to the device-resident Level B paths (rhip_*_batch, include/rabe_hip.h)
// instead of the per-object pairing jobs.  In file order: AC17 bulk keygen (CP, KP) / encrypt / decrypt (CP and KP: one body each); BSW keygen /
// delegate / encrypt / decrypt; LSW encrypt / keygen / decrypt (n keys, one ciphertext) / decrypt (n ciphertexts, one key); AW11 encrypt /
// keygen / decrypt; GHW11 encrypt / decrypt_out / transform / decrypt / keygen / tkgen / provision; BDABE and MKE08 (one body, dnfabe) encrypt /
// keygen / secret attribute keys / decaps.  The key-encapsulation forms (rabe_{ac17_cp,ac17_kp,bsw,...}_{encaps,decaps}_packed) are a mode of the encrypt /
// decrypt bodies: same caches, plans and launch sets, another ending.
// What stays on the host is what the reference does with strings and bytes: policy parsing, flattening the tree into the index tables the
// share kernels walk, traverse / calc_pruned / calc_coefficients per distinct policy, the selection tables, record layouts.  Records are the
// byte form rabe_obj_serialize gives the corresponding struct (host_abi.cpp), so packed and object APIs interoperate.
// The seven "many records under one key" decrypts (ac17, bsw, lsw x 2, aw11, ghw11 transform and decrypt) are top-to-bottom functions -- bounds,
// parse + plan, lists, shapes, buffers, checks, launch, verdicts -- over check_offsets / Cursor / same (ac17_record.h, with AC17's record reader)
// and the helpers of the anonymous namespace below: PlanCache, for_each_record, Selection, WalkScope, gather_record.  AC17 differs in two
// places: its plans are kept ACROSS calls (Ac17PlanCache: a PlanCache per key fingerprint), and its selection is two plain index lists copied
// on all cores instead of a Selection.  The issuers size their output with record_offsets, say where an item's parts lie with a RecordSources
// (record_layout.h) and the encrypts end in finish_encrypt (records.h); the four that walk share trees (bsw / ghw11 / aw11 encrypt, lsw keygen)
// keep them in a ShareTrees.
#include "schemes.h"
#include "records.h"
#include "ac17_record.h"

#include <algorithm>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace rabe {
using namespace host;
PolicyNode parse_or_error(const std::string& policy, PolicyLanguage lang);          // schemes.cpp
void parallel_for(size_t n, const std::function<void(size_t)>& fn);                // schemes.cpp

namespace schemes {
namespace {

// A policy text as the device-level paths want it (include/rabe_hip.h, "Flattened policy trees"): leaves in DFS order -- the order
// gen_shares_policy emits shares (src/utils/secretsharing/mod.rs:82-122) -- each with its root-to-leaf path of (gate, 1-based child
// number); gates in DFS pre-order with their threshold and the offset of their k - 1 coefficient draws (:128-134); per leaf the
// share's name `name_col` (node_index, :74-76), Fr(SHA3(remove_index(name_col))) (what the schemes hash, e.g. bsw/mod.rs:239) and
// the reconstruction coefficient (calc_coefficients, :9-57).  Cached across calls by (language, text).
struct FlatPolicy {
  PolicyNode tree;
  std::vector<std::string> leaf_name, leaf_name_col;
  std::vector<uint32_t> path_off{0}, path_gate, path_x, gate_k, gate_coef_off;
  uint32_t n_coef = 0;
  std::vector<Fr> leaf_hash, leaf_coeff;
  bool has_negative = false;
  size_t names_bytes = 0;          // sum of name_col lengths (record sizes)
};
void flatten_walk(FlatPolicy& f, const PolicyNode& n, std::vector<std::pair<uint32_t, uint32_t>>& path) {
  if (n.type == PolicyType::Leaf) {
    f.leaf_name.push_back(n.name);
    f.leaf_name_col.push_back(node_index(n));
    for (auto& pe : path) { f.path_gate.push_back(pe.first); f.path_x.push_back(pe.second); }
    f.path_off.push_back((uint32_t)f.path_gate.size());
    return;
  }
  if (n.children.size() < 2)
    throw PolicyPanic(n.type == PolicyType::And ? "Error: Invalid policy (AND with just a single child)." : "Error: Invalid policy (OR with just a single child).");
  const uint32_t g = (uint32_t)f.gate_k.size();
  const uint32_t k = n.type == PolicyType::And ? (uint32_t)n.children.size() : 1u;
  f.gate_k.push_back(k);
  f.gate_coef_off.push_back(f.n_coef);
  f.n_coef += k - 1;
  for (size_t i = 0; i < n.children.size(); i++) {
    path.push_back({g, (uint32_t)i + 1});
    flatten_walk(f, n.children[i], path);
    path.pop_back();
  }
}
std::shared_ptr<const FlatPolicy> flat_policy(const std::string& pol, PolicyLanguage language) {
  static std::mutex mu;
  static std::map<std::pair<int, std::string>, std::shared_ptr<const FlatPolicy>> cache;
  const auto key = std::make_pair((int)language, pol);
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  auto f = std::make_shared<FlatPolicy>();
  f->tree = parse_or_error(pol, language);
  std::vector<std::pair<uint32_t, uint32_t>> path;
  flatten_walk(*f, f->tree, path);
  NamedFr coeff;
  calc_coefficients(f->tree, fr_one(), &coeff);
  for (size_t i = 0; i < f->leaf_name_col.size(); i++) {
    f->leaf_hash.push_back(sha3_hash_fr(remove_index(f->leaf_name_col[i])));
    f->leaf_coeff.push_back(coeff[i].second);
    f->has_negative = f->has_negative || is_negative(f->leaf_name[i]);
    f->names_bytes += f->leaf_name_col[i].size();
  }
  std::lock_guard<std::mutex> g(mu);
  if (cache.size() >= 1024) cache.clear();
  cache[key] = f;
  return f;
}

// uploads that tolerate empty vectors (the device entry points are never handed a null array)
DBuf up32(Engine& eng, const std::vector<uint32_t>& v) {
  static const uint32_t zero = 0;
  return v.empty() ? DBuf(&eng, &zero, 4) : DBuf(&eng, v.data(), v.size() * 4);
}
DBuf up_bytes(Engine& eng, const std::vector<uint8_t>& v) {
  static const uint8_t zero[32] = {0};
  return v.empty() ? DBuf(&eng, zero, 32) : DBuf(&eng, v.data(), v.size());
}

// The share trees of one issuing call (bsw / ghw11 / aw11 encrypt, lsw keygen).  add() flattens the call's distinct policies, in their order;
// place() says where item i's leaves and coefficient draws start -- an AW11 item draws two coefficients per gate draw (the s-shares, then the
// 0-shares) -- and which tree it walks; upload(), after the draws, puts those arrays and the concatenated tables of the trees on the
// device, where d_* point to them: the tree arguments of rhip_*_batch, in that order.
struct ShareTrees {
  std::vector<std::shared_ptr<const FlatPolicy>> pols;
  std::vector<uint32_t> leaf_off, coef_off, tree_leaf, tree_gate;          // per item
  size_t total = 0, total_coef = 0;
  const uint32_t *d_leaf_off = nullptr, *d_tree_leaf = nullptr, *d_tree_gate = nullptr, *d_path_off = nullptr, *d_path_gate = nullptr, *d_path_x = nullptr,
                 *d_gate_k = nullptr, *d_gate_coef_off = nullptr, *d_coef_off = nullptr;
  const rhip_fr* d_leaf_hash = nullptr;
  const FlatPolicy& add(const std::string& policy, PolicyLanguage language) { pols.push_back(flat_policy(policy, language)); return *pols.back(); }
  void place(size_t n, const uint32_t* item_policy, uint32_t coefs_per_gate_draw) {
    std::vector<uint32_t> first_leaf(pols.size() + 1, 0), first_gate(pols.size() + 1, 0);
    for (size_t p = 0; p < pols.size(); p++) {
      first_leaf[p + 1] = first_leaf[p] + (uint32_t)pols[p]->leaf_name.size();
      first_gate[p + 1] = first_gate[p] + (uint32_t)pols[p]->gate_k.size();
    }
    leaf_off.assign(n + 1, 0); coef_off.assign(n + 1, 0); tree_leaf.resize(n); tree_gate.resize(n);
    for (size_t i = 0; i < n; i++) {
      const uint32_t p = item_policy[i];
      leaf_off[i + 1] = leaf_off[i] + (first_leaf[p + 1] - first_leaf[p]);
      coef_off[i + 1] = coef_off[i] + coefs_per_gate_draw * pols[p]->n_coef;
      tree_leaf[i] = first_leaf[p];
      tree_gate[i] = first_gate[p];
    }
    total = leaf_off[n];
    total_coef = coef_off[n];
  }
  void upload(Engine& eng) {
    std::vector<uint32_t> po{0}, pg, px, gk, gc;
    std::vector<Fr> lh;
    for (const auto& f : pols) {
      const uint32_t base = (uint32_t)pg.size();
      for (size_t i = 1; i < f->path_off.size(); i++) po.push_back(base + f->path_off[i]);
      pg.insert(pg.end(), f->path_gate.begin(), f->path_gate.end());
      px.insert(px.end(), f->path_x.begin(), f->path_x.end());
      gk.insert(gk.end(), f->gate_k.begin(), f->gate_k.end());
      gc.insert(gc.end(), f->gate_coef_off.begin(), f->gate_coef_off.end());
      lh.insert(lh.end(), f->leaf_hash.begin(), f->leaf_hash.end());
    }
    d_path_off = dev32(eng, po); d_path_gate = dev32(eng, pg); d_path_x = dev32(eng, px); d_gate_k = dev32(eng, gk); d_gate_coef_off = dev32(eng, gc);
    bufs_.push_back(up_bytes(eng, flatten_fr(lh)));
    d_leaf_hash = bufs_.back().as<rhip_fr>();
    d_leaf_off = dev32(eng, leaf_off); d_tree_leaf = dev32(eng, tree_leaf); d_tree_gate = dev32(eng, tree_gate); d_coef_off = dev32(eng, coef_off);
  }
 private:
  std::vector<DBuf> bufs_;
  const uint32_t* dev32(Engine& eng, const std::vector<uint32_t>& v) { bufs_.push_back(up32(eng, v)); return bufs_.back().as<uint32_t>(); }
};

// common.h's draw_items for these schemes: an item draws hundreds of values (one per gate coefficient and leaf), hence the small blocks
template <class DRAW>
void draw_items(Rng& rng, size_t n, DRAW draw) { rabe::draw_items(rng, n, 256, 16, draw); }

// The plans of one call by (language, key text), looked up WITHOUT copying the text and without serialising the readers: every item of a
// batch asks for its policy's plan, the texts are kilobytes (a 200-leaf policy: ~10 KB), and a mutex around a std::map of strings made the
// parse stage of a 4096-item call 8 ms long.  A miss runs `make(plan, text, lang)` under plans_mu -- once per distinct key, so no plan is
// built twice -- and keeps what it threw in the plan's `err`: the items of that key then fail with it, one by one.
template <class Plan>
class PlanCache {
 public:
  template <class MAKE>
  std::shared_ptr<Plan> get(const char* txt, size_t len, PolicyLanguage lang, MAKE make) {
    const uint64_t h = hash(txt, len, lang);
    if (auto hit = find(h, txt, len, lang)) return hit;
    std::lock_guard<std::mutex> g(plans_mu);
    if (auto hit = find(h, txt, len, lang)) return hit;
    auto pl = std::make_shared<Plan>();
    std::string text(txt, len);
    try {
      make(*pl, text, lang);
    } catch (const std::exception& ex) {
      pl->err = ex.what();
      if (pl->err.empty()) pl->err = "policy error";
    }
    std::unique_lock<std::shared_mutex> w(mu_);
    tab_[h].push_back(Entry{std::move(text), lang, pl});
    n_++;
    return pl;
  }
  // the same for a caller that keeps the cache itself alive for as long as it uses the plans (a cache kept across calls): a plain pointer,
  // no reference count that every thread of the parse stage would touch once per record
  template <class MAKE>
  Plan* get_kept(const char* txt, size_t len, PolicyLanguage lang, MAKE make) {
    { std::shared_lock<std::shared_mutex> g(mu_); if (const auto* hit = at(hash(txt, len, lang), txt, len, lang)) return hit->get(); }
    return get(txt, len, lang, make).get();
  }
  size_t size() const { return n_.load(); }          // plans made so far (a cache kept across calls is bounded by it)
 private:
  struct Entry { std::string text; PolicyLanguage lang; std::shared_ptr<Plan> plan; };
  std::shared_ptr<Plan> find(uint64_t h, const char* txt, size_t len, PolicyLanguage lang) {
    std::shared_lock<std::shared_mutex> g(mu_);
    const auto* hit = at(h, txt, len, lang);
    return hit ? *hit : nullptr;
  }
  const std::shared_ptr<Plan>* at(uint64_t h, const char* txt, size_t len, PolicyLanguage lang) const {          // under mu_
    auto it = tab_.find(h);
    if (it != tab_.end())
      for (const auto& e : it->second) if (e.lang == lang && e.text.size() == len && memcmp(e.text.data(), txt, len) == 0) return &e.plan;
    return nullptr;
  }
  static uint64_t hash(const char* txt, size_t len, PolicyLanguage lang) {
    uint64_t h = 1469598103934665603ull ^ (uint64_t)lang;
    for (size_t i = 0; i + 8 <= len; i += 8) { uint64_t w; memcpy(&w, txt + i, 8); h = (h ^ w) * 1099511628211ull; }
    for (size_t i = len & ~(size_t)7; i < len; i++) h = (h ^ (uint8_t)txt[i]) * 1099511628211ull;
    return h;
  }
  std::mutex plans_mu;          // the makers, one at a time
  std::shared_mutex mu_;
  std::unordered_map<uint64_t, std::vector<Entry>> tab_;
  std::atomic<size_t> n_{0};
};

// fn(i) for every record that has no error yet, on the host's cores; what it throws is that record's error
template <class FN>
void for_each_record(size_t n, std::vector<std::string>* errors, FN fn) {
  parallel_for(n, [&](size_t i) {
    std::string& err = (*errors)[i];
    if (!err.empty()) return;
    try {
      fn(i);
    } catch (const std::exception& ex) {
      err = ex.what();
      if (err.empty()) err = "malformed record";
    }
  });
}

// The selection tables of a "many records against one key" decrypt (include/rabe_hip.h: rhip_*_decrypt_batch_one_sk and kin).  Live item j
// (record live[j] of the call) has its rows at [row_off[j], row_off[j + 1]) of the gathered arrays, its pairs at [pair_off[j], pair_off[j + 1])
// and its entries at sel_start[j]: entry e pairs row sel_rec[e] of the record with row sel_one[e] of the call's ONE object (the key; the
// ciphertext of lsw::decrypt_packed), weighted by sel_z[e].  Records in the standard layout of one plan share their entries.
struct Selection {
  const uint32_t per_entry, extra;          // an item of m entries takes per_entry * m + extra pairs
  std::vector<size_t> live;
  std::vector<uint8_t> standard;            // per live item
  std::vector<uint32_t> row_off{0}, pair_off{0}, sel_start, sel_rec, sel_one;
  std::vector<Fr> sel_z;
  size_t max_pairs;
  Selection(uint32_t per_entry_, uint32_t extra_) : per_entry(per_entry_), extra(extra_), max_pairs(extra_) {}
  uint32_t entries(size_t j) const { return (pair_off[j + 1] - pair_off[j] - extra) / per_entry; }
  // record i with `rows` rows; entries(emit) calls emit(record row, row of the one object, weight) per entry of THIS record -- it is not
  // called for a standard-layout record whose plan's entries are there already
  template <class ENTRIES>
  void add(size_t i, uint32_t rows, const void* plan, bool std_layout, ENTRIES entries) {
    live.push_back(i);
    standard.push_back(std_layout);
    row_off.push_back(row_off.back() + rows);
    auto emit = [&](uint32_t rec_row, uint32_t one_row, const Fr& z) { sel_rec.push_back(rec_row); sel_one.push_back(one_row); sel_z.push_back(z); };
    std::pair<uint32_t, uint32_t> at{(uint32_t)sel_rec.size(), 0};          // start, count
    auto it = std_layout ? shared_start.find(plan) : shared_start.end();
    if (it != shared_start.end()) {
      at = it->second;
    } else {
      entries(emit);
      at.second = (uint32_t)sel_rec.size() - at.first;
      if (std_layout) shared_start.insert({plan, at});
    }
    sel_start.push_back(at.first);
    const uint32_t pairs = per_entry * at.second + extra;
    pair_off.push_back(pair_off.back() + pairs);
    if (pairs > max_pairs) max_pairs = pairs;
  }
 private:
  std::map<const void*, std::pair<uint32_t, uint32_t>> shared_start;
};

// The membership checks of one untrusted batch (common.h: MemberChecks beside the decrypt, WalkedG2 out of its own Miller loops) and what
// they refer to.  ONE lifetime rule: the walk's verdicts are read after the open (records.h: retract_item), so this object -- the checks,
// the index lists WalkedG2 points to and the device array it reads -- is declared before the launch block and outlives it.
struct WalkScope {
  std::unique_ptr<MemberChecks> mc;
  std::unique_ptr<WalkedG2> walked;
  std::vector<uint32_t> walked_idx, walked_off;
  DBuf d_g2;                                // the array whose elements the decrypt walks
  size_t k_alone = (size_t)-1;              // without walk verdicts: the index of d_g2's stand-alone test among mc's checks
  // Does the decrypt walk EVERY row of every item's G2 array (the rows its selection names)?  Only where it is verified: a record in the
  // standard layout, as many entries as rows, the selected rows distinct and in range -- rows matched by name can coincide in a crafted record,
  // and two plan entries can name one row (a policy that repeats an attribute); then some other row is walked by nobody.  Otherwise: false, and
  // the walked elements of item j are walked_idx[walked_off[j] .. walked_off[j + 1]) (common.h: WalkedG2 tests the others stand-alone).
  bool every_row_walked(const Selection& s) {
    const size_t m_items = s.live.size();
    bool all = true;
    std::vector<uint8_t> seen;
    for (size_t j = 0; j < m_items && all; j++) {
      const uint32_t mj = s.entries(j), rows = s.row_off[j + 1] - s.row_off[j];
      all = s.standard[j] && mj == rows;
      if (!all) break;
      seen.assign(rows, 0);
      for (uint32_t e = 0; e < mj && all; e++) {
        const uint32_t row = s.sel_rec[s.sel_start[j] + e];
        all = row < rows && !seen[row];
        if (all) seen[row] = 1;
      }
    }
    if (all) return true;
    walked_off.push_back(0);
    for (size_t j = 0; j < m_items; j++) {
      for (uint32_t e = 0; e < s.entries(j); e++) walked_idx.push_back(s.row_off[j] + s.sel_rec[s.sel_start[j] + e]);
      walked_off.push_back((uint32_t)walked_idx.size());
    }
    return false;
  }
  // d_g2 = `total` rows in the selection's segments, its selected rows walking arguments of the decrypt's pairings (plus extra_walks arguments
  // per item that are no elements of it): verdicts from those walks where `walk`, from the stand-alone test of every row otherwise
  void check_g2(Engine& eng, bool walk, const Selection& s, size_t total, const uint32_t* dev_row_off, uint32_t extra_walks = 0) {
    if (walk) {
      const bool all = every_row_walked(s);
      walked.reset(new WalkedG2(eng, *mc, d_g2.ptr(), total, dev_row_off, s.row_off, 1, all ? nullptr : &walked_idx, all ? nullptr : &walked_off, extra_walks));
    } else {
      k_alone = mc->add_count();
      mc->add(2, d_g2.ptr(), total, dev_row_off, s.live.size());
    }
  }
  // before the open: a live item that any of mc's checks `ks` refused fails with `msg` (k_alone counts where it exists); an earlier call's
  // message stays, so the calls go in the decoder's order
  void fail(const std::vector<size_t>& live, std::initializer_list<size_t> ks, const char* msg, std::vector<std::string>* errors) const {
    for (size_t k : ks) {
      if (k == (size_t)-1) continue;
      const auto& ok = mc->ok(k);
      for (size_t j = 0; j < live.size(); j++) if (!ok[j] && (*errors)[live[j]].empty()) (*errors)[live[j]] = msg;
    }
  }
  // a decaps has no open to queue behind the pairings: the walk's verdicts are read before the keys are derived, like every other verdict
  void fail_walked(const std::vector<size_t>& live, const char* msg, std::vector<std::string>* errors) {
    if (!walked) return;
    std::vector<uint8_t> ok;
    walked->finish(&ok);
    for (size_t j = 0; j < live.size(); j++) if (!ok[j]) (*errors)[live[j]] = msg;
  }
  // after the open: the items whose walk refused an element
  void retract(const std::vector<size_t>& live, const char* msg, int32_t* status, uint8_t* pt_buf, const uint64_t* pt_off, std::vector<std::string>* errors) {
    if (!walked) return;
    std::vector<uint8_t> ok;
    walked->finish(&ok);
    for (size_t j = 0; j < live.size(); j++) if (!ok[j]) retract_item(live[j], msg, status, pt_buf, pt_off, errors);
  }
};

// One live record of a BlobGather (records.h): records that share `key` (null: this record alone) share a shape; fill(parts) lists the
// parts of a shape nobody registered yet
template <class FILL>
void gather_record(BlobGather& gather, uint64_t rec_off, const void* key, FILL fill) {
  int shape = key ? gather.find(key) : -1;
  if (shape < 0) {
    std::vector<RecordLayout::Part> parts;
    fill(parts);
    shape = (int)gather.add_shape(key, std::move(parts));
  }
  gather.item(rec_off, (uint32_t)shape);
}

// where an item's sealed plaintext sits in the caller's blob (opened on the device: records.h, open_sealed_records)
struct Sealed { const uint8_t* p = nullptr; uint32_t len = 0; };

}  // namespace

// ================================================================================================================= AC17 keygen
namespace ac17 {
namespace {
struct MskTables { rhip_g1_table* g = nullptr; rhip_g2_table* h = nullptr; };
void* make_msk_tables(Engine& eng, const void* arg) {
  const Ac17MasterKey& msk = *(const Ac17MasterKey*)arg;
  std::unique_ptr<MskTables> t(new MskTables());
  eng.check(rhip_g1_table_create(eng.ctx(), (const rhip_g1*)msk.g.data(), &t->g), "rhip_g1_table_create");
  int32_t rc = rhip_g1_table_add_w16(eng.ctx(), t->g);
  if (!rc) rc = rhip_g2_table_create(eng.ctx(), (const rhip_g2*)msk.h.data(), &t->h);
  if (!rc) rc = rhip_g2_table_add_w16(eng.ctx(), t->h);
  if (rc) { rhip_g1_table_destroy(t->g); if (t->h) rhip_g2_table_destroy(t->h); eng.check(rc, "master-key tables"); }
  return t.release();
}
void destroy_msk_tables(void* h) {
  MskTables* t = (MskTables*)h;
  rhip_g1_table_destroy(t->g);
  rhip_g2_table_destroy(t->h);
  delete t;
}
}  // namespace
// window tables of a master key's g and h, built on first use and kept (cp_keygen, cp_keygen_packed)
void msk_tables(Engine& eng, const Ac17MasterKey& msk, rhip_g1_table** g, rhip_g2_table** h) {
  std::string key((const char*)msk.g.data(), 64);
  key.append((const char*)msk.h.data(), 128);
  const MskTables* tb = (const MskTables*)eng.aux("ac17_msk_tables", key, make_msk_tables, &msk, destroy_msk_tables, 4);
  *g = tb->g;
  *h = tb->h;
}

// n calls of ac17::cp_keygen (ac17/mod.rs:191-264) under one master key -- a key authority issuing keys in bulk.  Item i gets the
// attribute list sets[item_set[i]]; draw order per item as in the reference: r0, r1, sigma per attribute (list order), sigma'.
// Record = Ac17CpSecretKey: attribute strings, k_0[3], rows (name, k[3]), k_p[3].  Items that share a list run as one launch of the
// Level B kernels (the label hashes of a list are computed once); the window tables of the master key's g and h are kept across calls.
bool cp_keygen_packed(Engine& eng, Rng& rng, const Ac17MasterKey& msk, const std::vector<std::vector<std::string>>& sets, size_t n,
                      const uint32_t* item_set, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm("ac17::cp_keygen_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // master-key-derived scalars pass through the staging buffers
  if (msk.a.size() != 2 || msk.b.size() != 2 || msk.g_k.size() != 3) throw RabeError("malformed Ac17MasterKey: a, b must have 2 and g_k 3 elements");
  if (n && (!item_set || !out_off)) throw RabeError("cp_keygen_packed: null input");
  std::vector<size_t> fixed(sets.size());
  for (size_t s = 0; s < sets.size(); s++) {
    if (sets[s].empty()) throw RabeError("empty attributes!");
    fixed[s] = 4 + 4 + 384 + 4 + 4 + 192;
    for (const auto& a : sets[s]) fixed[s] += (4 + a.size()) + (4 + a.size() + 4 + 192);
  }
  if (!record_offsets("cp_keygen_packed", "item_set", n, item_set, sets.size(), fixed, nullptr, out_buf, out_cap, out_off)) return false;
  if (!n) return true;
  // items grouped by attribute list (stable: the order inside a group is the item order)
  std::vector<std::vector<size_t>> members(sets.size());
  for (size_t i = 0; i < n; i++) members[item_set[i]].push_back(i);
  std::vector<size_t> slot(n), sig_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) sig_off[i + 1] = sig_off[i] + sets[item_set[i]].size();
  // randomness, item after item: r0, r1, sigma_y ..., sigma'
  uint8_t* h_r = eng.pinned(0, n * 96 + sig_off[n] * 32 + 32);
  uint8_t* h_sp = h_r + n * 64;
  uint8_t* h_sig = h_sp + n * 32;
  draw_items(rng, n, [&](Rng& r, size_t i) {
    Fr r0 = r.next_fr(), r1 = r.next_fr();
    memcpy(h_r + 64 * i, r0.l, 32);
    memcpy(h_r + 64 * i + 32, r1.l, 32);
    for (size_t y = sig_off[i]; y < sig_off[i + 1]; y++) { Fr sg = r.next_fr(); memcpy(h_sig + 32 * y, sg.l, 32); }
    Fr sp = r.next_fr();
    memcpy(h_sp + 32 * i, sp.l, 32);
  });
  tm.lap("draws");
  MskTables tables;
  msk_tables(eng, msk, &tables.g, &tables.h);
  const MskTables* tb = &tables;
  std::vector<Fr> H01;
  for (int l = 0; l < 3; l++)
    for (int t = 0; t < 2; t++) H01.push_back(sha3_hash_fr(std::string("01") + std::to_string(l) + std::to_string(t)));
  std::vector<Fr> a_inv(2);
  for (int t = 0; t < 2; t++)
    if (!fr_inv(msk.a[t], &a_inv[t])) throw std::runtime_error("called `Option::unwrap()` on a `None` value (Fr::inverse of zero)");
  DBuf dgk = up_bytes(eng, flatten(msk.g_k)), da = up_bytes(eng, flatten_fr(a_inv)), db = up_bytes(eng, flatten_fr(msk.b)), dH01 = up_bytes(eng, flatten_fr(H01));
  rhip_ctx* cx = eng.ctx();
  // per group: gather its items' randomness into contiguous staging, launch, fetch
  struct Group { size_t first_out; size_t cnt; size_t n_attr; };
  std::vector<Group> groups(sets.size());
  size_t tot_items = 0, tot_rows = 0;
  for (size_t s = 0; s < sets.size(); s++) { groups[s] = {tot_items, members[s].size(), sets[s].size()}; tot_items += members[s].size(); tot_rows += members[s].size() * sets[s].size(); }
  uint8_t* g_r = eng.pinned(1, tot_items * 96 + tot_rows * 32 + 32);              // r | sigma' | sigma, group-major
  uint8_t* g_sp = g_r + tot_items * 64;
  uint8_t* g_sig = g_sp + tot_items * 32;
  std::vector<size_t> grp_row0(sets.size() + 1, 0);
  for (size_t s = 0; s < sets.size(); s++) grp_row0[s + 1] = grp_row0[s] + members[s].size() * sets[s].size();
  for (size_t s = 0; s < sets.size(); s++)
    parallel_for(members[s].size(), [&](size_t q) {
      const size_t i = members[s][q], o = groups[s].first_out + q;
      slot[i] = o;
      memcpy(g_r + 64 * o, h_r + 64 * i, 64);
      memcpy(g_sp + 32 * o, h_sp + 32 * i, 32);
      memcpy(g_sig + 32 * (grp_row0[s] + q * sets[s].size()), h_sig + 32 * sig_off[i], 32 * sets[s].size());
    });
  DBuf d_r(&eng, tot_items * 64), d_sp(&eng, tot_items * 32), d_sig(&eng, tot_rows * 32 + 4), d_k0(&eng, tot_items * 384), d_k(&eng, tot_rows * 192 + 4),
      d_kp(&eng, tot_items * 192);
  eng.check(rhip_upload_async(cx, d_r.ptr(), g_r, tot_items * 64), "upload");
  eng.check(rhip_upload_async(cx, d_sp.ptr(), g_sp, tot_items * 32), "upload");
  eng.check(rhip_upload_async(cx, d_sig.ptr(), g_sig, tot_rows * 32), "upload");
  std::vector<DBuf> dH;
  for (size_t s = 0; s < sets.size(); s++) {
    if (members[s].empty()) { dH.emplace_back(); continue; }
    std::vector<Fr> H;
    for (const auto& attr : sets[s])
      for (int l = 0; l < 3; l++)
        for (int t = 0; t < 2; t++) H.push_back(sha3_hash_fr(attr + std::to_string(l) + std::to_string(t)));
    dH.push_back(up_bytes(eng, flatten_fr(H)));
    const Group& g = groups[s];
    eng.check(rhip_ac17_cp_keygen_batch(cx, tb->g, tb->h, dgk.as<rhip_g1>(), da.as<rhip_fr>(), db.as<rhip_fr>(), g.cnt, g.n_attr, dH.back().as<rhip_fr>(),
                                        dH01.as<rhip_fr>(), (const rhip_fr*)(d_r.as<uint8_t>() + 64 * g.first_out),
                                        (const rhip_fr*)(d_sig.as<uint8_t>() + 32 * grp_row0[s]), (const rhip_fr*)(d_sp.as<uint8_t>() + 32 * g.first_out),
                                        (rhip_g2*)(d_k0.as<uint8_t>() + 384 * g.first_out), (rhip_g1*)(d_k.as<uint8_t>() + 192 * grp_row0[s]),
                                        (rhip_g1*)(d_kp.as<uint8_t>() + 192 * g.first_out)), "rhip_ac17_cp_keygen_batch");
  }
  uint8_t* h_k = eng.pinned(2, tot_rows * 192 + tot_items * (384 + 192) + 4);
  uint8_t* h_k0 = h_k + tot_rows * 192;
  uint8_t* h_kp = h_k0 + tot_items * 384;
  eng.check(rhip_download_async(cx, h_k, d_k.ptr(), tot_rows * 192), "download");
  eng.check(rhip_download_async(cx, h_k0, d_k0.ptr(), tot_items * 384), "download");
  eng.check(rhip_download_async(cx, h_kp, d_kp.ptr(), tot_items * 192), "download");
  eng.check(rhip_sync(cx), "rhip_sync");
  tm.lap("device + copies");
  parallel_for(n, [&](size_t i) {
    const size_t s = item_set[i], o = slot[i], q = o - groups[s].first_out;
    const auto& attrs = sets[s];
    uint8_t* w = out_buf + out_off[i];
    put_u32(w, (uint32_t)attrs.size()); w += 4;
    for (const auto& a : attrs) { put_u32(w, (uint32_t)a.size()); w += 4; memcpy(w, a.data(), a.size()); w += a.size(); }
    put_u32(w, 3); w += 4;
    memcpy(w, h_k0 + 384 * o, 384); w += 384;
    put_u32(w, (uint32_t)attrs.size()); w += 4;
    const uint8_t* rows = h_k + 192 * (grp_row0[s] + q * attrs.size());
    for (size_t y = 0; y < attrs.size(); y++) {
      put_u32(w, (uint32_t)attrs[y].size()); w += 4;
      memcpy(w, attrs[y].data(), attrs[y].size()); w += attrs[y].size();
      put_u32(w, 3); w += 4;
      memcpy(w, rows + 192 * y, 192); w += 192;
    }
    put_u32(w, 3); w += 4;
    memcpy(w, h_kp + 192 * o, 192);
  });
  tm.lap("assembly");
  return true;
}

// n calls of ac17::kp_keygen (:439-547) under one master key: item i's policy = policies[item_policy[i]].  Draw order per item as above.
// The Fr half runs on all host cores; the group half is ONE fixed-base launch per group (window tables of msk.g / msk.h, kept across
// calls), one batched addition for the rows whose first MSP column is +/-1 (+/- g_k), and the records are written on the device.
// Record = Ac17KpSecretKey: policy text, language, k_0 (3 G2), rows (name, 3 G1), an empty k_p.  Buffers as cp_keygen_packed.
bool kp_keygen_packed(Engine& eng, Rng& rng, const Ac17MasterKey& msk, const std::vector<std::string>& policies, PolicyLanguage lang, size_t n,
                      const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm("ac17::kp_keygen_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // master-key-derived scalars pass through the staging buffers
  if (msk.a.size() != 2 || msk.b.size() != 2 || msk.g_k.size() != 3) throw RabeError("malformed Ac17MasterKey: a, b must have 2 and g_k 3 elements");
  if (n && (!item_policy || !out_off)) throw RabeError("kp_keygen_packed: null input");
  std::vector<KpPolicy> kps;
  std::vector<RecordLayout> layouts(policies.size());
  for (size_t p_ = 0; p_ < policies.size(); p_++) {
    kps.push_back(kp_policy(policies[p_], lang));
    RecordLayout& L = layouts[p_];
    const AbePolicy& msp = kps.back().msp;
    policy_header(L, policies[p_], lang);
    L.u32(3);
    L.src(0, 0, 384);
    L.u32((uint32_t)msp.m.size());
    for (size_t r = 0; r < msp.m.size(); r++) { L.str(msp.pi[r]); L.u32(3); L.src(1, (uint32_t)(192 * r), 192); }
    L.u32(0);                                   // k_p: empty for a KP key
  }
  if (!record_offsets("kp_keygen_packed", "item_policy", n, item_policy, policies.size(), [&](size_t i) { return layouts[item_policy[i]].bytes(); }, nullptr,
                      out_buf, out_cap, out_off)) return false;
  if (!n) return true;
  std::vector<uint32_t> row_off(n + 1, 0), draw_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    const AbePolicy& msp = kps[item_policy[i]].msp;
    row_off[i + 1] = row_off[i] + (uint32_t)msp.m.size();
    draw_off[i + 1] = draw_off[i] + 2 + (uint32_t)(msp.m[0].size() - 1) + (uint32_t)msp.m.size();
  }
  const size_t total_rows = row_off[n];
  std::vector<Fr> draws(draw_off[n] + 1);
  draw_items(rng, n, 1024, 256, [&](Rng& r, size_t i) { for (uint32_t d = draw_off[i]; d < draw_off[i + 1]; d++) draws[d] = r.next_fr(); });
  tm.lap("policies + draws");
  Fr a_inv[2] = {must_inv(msk.a[0]), must_inv(msk.a[1])};
  uint8_t* h_scal = eng.pinned(0, total_rows * 96 + n * 96 + 32);          // row scalars | br
  uint8_t* h_br = h_scal + total_rows * 96;
  uint8_t* h_add = eng.pinned(1, total_rows * 192 + 4);                     // +/- g_k[t] per row element, the point at infinity where nothing is added
  G1 neg_gk[3];
  {
    std::vector<G1> ng = eng.g1_mul(msk.g_k, std::vector<Fr>(3, fr_neg(fr_one())));
    for (int t = 0; t < 3; t++) neg_gk[t] = ng[t];
  }
  parallel_for(n, [&](size_t i) {
    const KpPolicy& kp = kps[item_policy[i]];
    const size_t cols = kp.msp.m[0].size(), rows = kp.msp.m.size();
    const Fr* d = draws.data() + draw_off[i];
    std::vector<Fr> scal(3 * rows);
    Fr br[3];
    kp_keygen_scalars(msk, kp, a_inv, d[0], d[1], d + 2, d + 2 + (cols - 1), scal.data(), br);
    memcpy(h_scal + 96 * (size_t)row_off[i], scal.data(), 96 * rows);
    memcpy(h_br + 96 * i, br, 96);
    uint8_t* ad = h_add + 192 * (size_t)row_off[i];
    for (size_t r = 0; r < rows; r++)
      for (int t = 0; t < 3; t++) {
        const int8_t c = kp.msp.m[r][0];
        if (c == 0) memset(ad + 192 * r + 64 * t, 0, 64);
        else memcpy(ad + 192 * r + 64 * t, (c == 1 ? msk.g_k[t] : neg_gk[t]).data(), 64);
      }
  });
  tm.lap("scalars");
  rhip_g1_table* gt = nullptr;
  rhip_g2_table* ht = nullptr;
  msk_tables(eng, msk, &gt, &ht);
  rhip_ctx* cx = eng.ctx();
  DBuf d_scal(&eng, total_rows * 96 + n * 96), d_add(&eng, total_rows * 192 + 4), d_pts(&eng, total_rows * 192 + 4), d_k(&eng, total_rows * 192 + 4),
      d_k0(&eng, n * 384);
  eng.check(rhip_upload_async(cx, d_scal.ptr(), h_scal, total_rows * 96 + n * 96), "upload");
  eng.check(rhip_upload_async(cx, d_add.ptr(), h_add, total_rows * 192), "upload");
  eng.check(rhip_g1_table_mul(cx, gt, 3 * total_rows, d_scal.as<rhip_fr>(), d_pts.as<rhip_g1>()), "rhip_g1_table_mul");
  eng.check(rhip_g1_add(cx, 3 * total_rows, d_pts.as<rhip_g1>(), d_add.as<rhip_g1>(), d_k.as<rhip_g1>()), "rhip_g1_add");
  eng.check(rhip_g2_table_mul(cx, ht, 3 * n, (const rhip_fr*)(d_scal.as<uint8_t>() + total_rows * 96), d_k0.as<rhip_g2>()), "rhip_g2_table_mul");
  emit_plain_records(eng, layouts, n, item_policy, RecordSources(n).by_item(d_k0.ptr(), 384).by_rows(d_k.ptr(), 192, row_off), out_off, out_buf);
  tm.lap("device: fixed-base multiplications, records; one copy out");
  return true;
}

// ---------------------------------------------------------------------------------------------- packed batches
// The same two functions with packed input and output (no per-item objects on either side of the C ABI): n ciphertexts are
// one blob of canonical records (the byte form of rabe_obj_serialize for Ac17CpCiphertext) with an offset array.  Everything
// per item that is not group arithmetic -- record assembly, KDF, AES-GCM, parsing, pruning -- runs on all host cores; the
// group arithmetic is one launch set; PCIe copies go through pinned staging buffers.
// parse + MSP + Fr table of a policy text, cached across calls (a server encrypts under the same few policies again and again)
struct EncPolicy { AbePolicy msp; std::vector<Fr> tab; size_t fixed_bytes; };
static std::shared_ptr<const EncPolicy> enc_policy(const std::string& pol, PolicyLanguage language) {
  static std::mutex mu;
  static std::map<std::pair<int, std::string>, std::shared_ptr<const EncPolicy>> cache;
  const auto key = std::make_pair((int)language, pol);
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  auto e = std::make_shared<EncPolicy>();
  e->msp = calculate_msp(parse_or_error(pol, language));
  e->tab = policy_table(e->msp);
  e->fixed_bytes = 4 + pol.size() + 1 + 4 + 3 * 128 + 4 + 384 + 4;      // record size without the sealed plaintext
  for (const auto& name : e->msp.pi) e->fixed_bytes += 4 + name.size() + 4 + 3 * 64;
  std::lock_guard<std::mutex> g(mu);
  if (cache.size() >= 1024) cache.clear();
  cache[key] = e;
  return e;
}
// out_buf / out_cap: caller-allocated (reusable) output; out_off: n + 1 caller-allocated entries, always filled.  Returns false
// -- before any randomness is drawn or work is done -- when out_cap < out_off[n], the size the records need.
// KP-ABE's encrypt (:556-616) is the same arithmetic with a table of plain label hashes: rows = the attribute list, no MSP columns.  The
// record differs only in its head (the attribute strings instead of policy text + language).
static std::shared_ptr<const EncPolicy> enc_attr_set(const std::vector<std::string>& attrs) {
  auto e = std::make_shared<EncPolicy>();
  e->msp.pi = attrs;
  e->msp.m.assign(attrs.size(), std::vector<int8_t>{0});
  for (const auto& a : attrs)
    for (int l = 0; l < 3; l++)
      for (int t = 0; t < 2; t++) e->tab.push_back(sha3_hash_fr(a + std::to_string(l) + std::to_string(t)));
  e->fixed_bytes = 4 + 4 + 3 * 128 + 4 + 384 + 4;
  for (const auto& a : attrs) e->fixed_bytes += (4 + a.size()) + (4 + a.size() + 4 + 3 * 64);
  return e;
}
static bool encrypt_packed_core(Engine& eng, Rng& rng, const Ac17PublicKey& pk, const std::vector<std::shared_ptr<const EncPolicy>>& pols,
                                const std::vector<std::string>* policies /* CP: the texts; KP: nullptr */, PolicyLanguage language, size_t n,
                                const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off,
                                uint8_t* key_buf = nullptr /* encaps: no plaintexts, no sealing; 32 bytes of content key per item */);
bool cp_encrypt_packed(Engine& eng, Rng& rng, const Ac17PublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                       const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  std::vector<std::shared_ptr<const EncPolicy>> pols;
  for (const auto& pol : policies) pols.push_back(enc_policy(pol, language));
  return encrypt_packed_core(eng, rng, pk, pols, &policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off);
}
// Key encapsulation (include/rabe_host.h: rabe_ac17_cp_encaps_packed): cp_encrypt_packed's records with a sealed part of length zero and,
// per item, the content key SHA3-256(bytes(msg)) instead of a payload sealed under it.  Draws: cp_encrypt_packed's without the nonce.
bool cp_encaps_packed(Engine& eng, Rng& rng, const Ac17PublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                      const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  if (n && !key_buf) throw RabeError("cp_encaps_packed: null input");
  if (!n) { out_off[0] = 0; return true; }
  std::vector<std::shared_ptr<const EncPolicy>> pols;
  for (const auto& pol : policies) pols.push_back(enc_policy(pol, language));
  return encrypt_packed_core(eng, rng, pk, pols, &policies, language, n, item_policy, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}
// n calls of ac17::kp_encrypt: item i is encrypted under the attribute list sets[item_set[i]]; records = Ac17KpCiphertext
bool kp_encrypt_packed(Engine& eng, Rng& rng, const Ac17PublicKey& pk, const std::vector<std::vector<std::string>>& sets, size_t n, const uint32_t* item_set,
                       const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  std::vector<std::shared_ptr<const EncPolicy>> pols;
  for (const auto& a : sets) pols.push_back(enc_attr_set(a));
  return encrypt_packed_core(eng, rng, pk, pols, nullptr, PolicyLanguage::JsonPolicy, n, item_set, pt_blob, pt_off, out_buf, out_cap, out_off);
}
// Key encapsulation over the KP pair (include/rabe_host.h: rabe_ac17_kp_encaps_packed): kp_encrypt_packed's records with a sealed part of length
// zero and the content keys, as cp_encaps_packed
bool kp_encaps_packed(Engine& eng, Rng& rng, const Ac17PublicKey& pk, const std::vector<std::vector<std::string>>& sets, size_t n, const uint32_t* item_set,
                      uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  if (n && !key_buf) throw RabeError("kp_encaps_packed: null input");
  if (!n) { out_off[0] = 0; return true; }
  std::vector<std::shared_ptr<const EncPolicy>> pols;
  for (const auto& a : sets) pols.push_back(enc_attr_set(a));
  return encrypt_packed_core(eng, rng, pk, pols, nullptr, PolicyLanguage::JsonPolicy, n, item_set, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}
static bool encrypt_packed_core(Engine& eng, Rng& rng, const Ac17PublicKey& pk, const std::vector<std::shared_ptr<const EncPolicy>>& pols,
                                const std::vector<std::string>* policies, PolicyLanguage language, size_t n,
                                const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off,
                                uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? (policies ? "ac17::cp_encaps_packed" : "ac17::kp_encaps_packed") : policies ? "ac17::cp_encrypt_packed" : "ac17::kp_encrypt_packed");
  Engine::ArenaScope arena(eng);
  if (pk.h_a.size() != 3 || pk.e_gh_ka.size() != 2) throw RabeError("malformed Ac17PublicKey");
  std::vector<uint32_t> a_off{0};
  std::vector<Fr> A;
  for (const auto& e : pols) {
    A.insert(A.end(), e->tab.begin(), e->tab.end());
    a_off.push_back(a_off.back() + (uint32_t)e->msp.m.size());
  }
  if (!record_offsets("encrypt_packed", "item_policy", n, item_policy, pols.size(), [&](size_t i) { return pols[item_policy[i]]->fixed_bytes; },
                      kem ? nullptr : pt_off, out_buf, out_cap, out_off)) return false;
  tm.lap("policies");
  // randomness in the reference's per-call draw order: s0, s1, msg, nonce -- item after item (encaps: no nonce)
  uint8_t* h_s = eng.pinned(0, n * (64 + 32));
  uint8_t* h_rho = h_s + n * 64;
  std::vector<std::array<uint8_t, 12>> nonces(n);
  draw_items(rng, n, 1024, 256, [&](Rng& r, size_t i) {
    Fr s0 = r.next_fr(), s1 = r.next_fr(), rho = r.next_fr();
    memcpy(h_s + 64 * i, s0.l, 32);
    memcpy(h_s + 64 * i + 32, s1.l, 32);
    memcpy(h_rho + 32 * i, rho.l, 32);
    if (!kem) r.fill(nonces[i].data(), 12);
  });
  std::vector<uint32_t> item_a_off(n), row_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    item_a_off[i] = a_off[item_policy[i]];
    row_off[i + 1] = row_off[i] + (uint32_t)pols[item_policy[i]]->msp.m.size();
  }
  const size_t total_rows = row_off[n];
  tm.lap("draws");
  rhip_ac17_pk* dpk = eng.ac17_pk(pk.g, pk.h_a, pk.e_gh_ka);
  rhip_gt_table* egt = eng.gt_generator_table();
  auto fA = flatten_fr(A);
  DBuf dA(&eng, fA.data(), fA.size()), dio(&eng, item_a_off.data(), n * 4), ds(&eng, n * 64), drho(&eng, n * 32),
      dm(&eng, n * 384), dc0(&eng, n * 3 * 128), dc(&eng, total_rows * 3 * 64 + 4), dcp(&eng, n * 384);
  rhip_ctx* cx = eng.ctx();
  eng.check(rhip_upload_async(cx, ds.ptr(), h_s, n * 64), "upload");
  eng.check(rhip_upload_async(cx, drho.ptr(), h_rho, n * 32), "upload");
  // records and sealing on the device (records.h): per policy a template of the literal bytes with the elements dropped in
  std::vector<RecordLayout> layouts(pols.size());
  for (size_t p_ = 0; p_ < pols.size(); p_++) {
    RecordLayout& L = layouts[p_];
    const AbePolicy& msp = pols[p_]->msp;
    if (policies) {                               // Ac17CpCiphertext: policy text + language
      policy_header(L, (*policies)[p_], language);
    } else {                                      // Ac17KpCiphertext: the attribute strings
      L.u32((uint32_t)msp.pi.size());
      for (const auto& a : msp.pi) L.str(a);
    }
    L.u32(3);
    L.src(0, 0, 384);
    L.u32((uint32_t)msp.m.size());
    for (size_t r = 0; r < msp.m.size(); r++) {
      L.str(msp.pi[r]);
      L.u32(3);
      L.src(1, (uint32_t)(192 * r), 192);
    }
    L.src(2, 0, 384);
    if (close_ciphertext(L, kem) != pols[p_]->fixed_bytes) throw RabeError("ac17 encrypt_packed: record layout and size disagree");
  }
  // The batch can go through the device in PARTS of >= 16 384 items, a part's records copied out (10.4 KB per item at 50 rows, 15 ms per
  // 65 536 items) on the side stream while the next part's group arithmetic runs; randomness was drawn above for the whole batch, item
  // after item, so the bytes do not depend on the cut (tests/test_gpu_packed.py).  OFF by default (RABE_AC17_ENC_PARTS=4 turns it on):
  // measured no faster -- 37.2 against 36.9 ms at 65 536 items -- because the runtime's D2H copy of such a block is a blit kernel that
  // covers the chip: k_table_pow_gt of the next part takes 5.3 instead of 1.3 ms under it.
  static const size_t max_parts = [] { const char* e = getenv("RABE_AC17_ENC_PARTS"); const long v = e ? atol(e) : 1; return (size_t)(v > 0 ? v : 1); }();
  const size_t parts = kem ? 1 : std::max<size_t>(1, std::min<size_t>(max_parts, n / 16384));
  std::vector<PendingCopy> pending(parts);
  if (parts > 1) eng.pinned_reserve((size_t)out_off[n] + parts * ((size_t)8 << 20) + 300 * n);          // staging of every part + their parameter packs: no growth inside the loop
  // every part's row offsets (relative to the part's first row), uploaded once and asynchronously: nothing inside the loop may wait for
  // the stream, or the host would queue part k + 1 only after part k has finished
  std::vector<uint32_t> ro_all(n + parts);
  std::vector<size_t> ro_at(parts);
  for (size_t part = 0, at = 0; part < parts; part++) {
    const size_t lo = n * part / parts, hi = n * (part + 1) / parts;
    ro_at[part] = at;
    for (size_t i = lo; i <= hi; i++) ro_all[at++] = row_off[i] - row_off[lo];
  }
  uint8_t* const h_ro = eng.pinned_bump(ro_all.size() * 4);
  memcpy(h_ro, ro_all.data(), ro_all.size() * 4);
  DBuf d_ro_all(&eng, ro_all.size() * 4);
  eng.check(rhip_upload_async(cx, d_ro_all.ptr(), h_ro, ro_all.size() * 4), "upload");
  for (size_t part = 0; part < parts; part++) {
    const size_t lo = n * part / parts, hi = n * (part + 1) / parts, np = hi - lo;
    const uint32_t* const ro = ro_all.data() + ro_at[part];
    const uint32_t* const dro_p = d_ro_all.as<uint32_t>() + ro_at[part];
    const size_t rows_p = ro[np];
    rhip_g1* const dc_p = (rhip_g1*)(dc.as<uint8_t>() + 192ull * row_off[lo]);
    eng.check(rhip_gt_table_pow(cx, egt, np, drho.as<rhip_fr>() + lo, dm.as<rhip_gt>() + lo), "rhip_gt_table_pow");
    eng.check(rhip_ac17_cp_encrypt_batch(cx, dpk, np, dA.as<rhip_fr>(), dio.as<uint32_t>() + lo, dro_p, rows_p, ds.as<rhip_fr>() + 2 * lo,
                                         dm.as<rhip_gt>() + lo, dc0.as<rhip_g2>() + 3 * lo, dc_p, dcp.as<rhip_gt>() + lo), "rhip_ac17_cp_encrypt_batch");
    // the part's sources: base pointers shifted to its first item, row offsets relative to its first row.  An encaps is one part (lo = 0)
    RecordSources src(np);
    src.by_item(dc0.as<uint8_t>() + 384ull * lo, 384).by_rows(dc_p, 192, ro, np + 1).by_item(dcp.as<uint8_t>() + 384ull * lo, 384);
    finish_encrypt(eng, nullptr, layouts, np, item_policy + lo, src, dm.as<uint8_t>() + 384ull * lo, (const uint8_t*)nonces.data() + 12 * lo, pt_blob,
                   kem ? nullptr : pt_off + lo, out_off + lo, out_buf, key_buf, parts > 1 ? &pending[part] : nullptr);
  }
  for (auto& pc : pending) pc.wait(eng);
  tm.lap(kem ? "device: group arithmetic, headers, keys; two copies out" : "device: group arithmetic, records, sealing; copies out beside the next part");
  return true;
}

static void* make_ac17_sk_lines(Engine& eng, const void* arg) {
  const std::string& k0 = *(const std::string*)arg;
  DBuf d(&eng, k0.data(), k0.size());
  rhip_ac17_sk_lines* lines = nullptr;
  eng.check(rhip_ac17_sk_prepare(eng.ctx(), 1, d.as<rhip_g2>(), &lines), "rhip_ac17_sk_prepare");
  return lines;
}
static void destroy_ac17_sk_lines(void* h) { rhip_ac17_sk_lines_destroy((rhip_ac17_sk_lines*)h); }
// status[i]: 0 ok, -1 the key does not satisfy the policy / malformed record / authentication failure (errors[i] says which).
// pt_buf / pt_cap: caller-allocated; a capacity of ct_off[n] bytes always suffices (a plaintext is 28 bytes shorter than its sealed
// form).  Returns false, before any work, when pt_cap is smaller than that.
//
// The records come from outside: the offsets are validated against ct_len before anything is read (monotone, inside the blob -- an
// item whose own bounds are bad fails alone), and unless `trusted` is set every decoded element goes through one batched membership
// pass on the GPU (coordinates < p, rows on the G1 curve, c_0 in the r-torsion of the twist, c_p in the order-r subgroup of Fq12:
// what rabe-bn's decoding establishes, FieldError::NotMember) -- the Gt arithmetic downstream (cyclotomic squarings, conjugate as
// inverse) is only valid inside the subgroup.  `trusted` is for ciphertexts this process produced itself.
// KP-ABE's decrypt (:625-675) is the same product of pairings with the roles of the two sides' names swapped: the policy is the KEY's, the
// attribute list the ciphertext's (its record starts with the attribute strings instead of policy text + language); k_p is absent.
// plans of the packed decrypt, kept across calls: one bucket per key fingerprint (attributes or policy + row names), inside it one plan
// per policy text.  A bucket that has grown past its cap is REPLACED (calls that still hold the old one finish on it).
struct Ac17PolPlan {
  std::string err; PrunedList lst; std::vector<uint32_t> sk_sel;
  std::mutex mu; std::atomic<bool> have_rows{false}; std::vector<std::string> row_names; std::vector<uint32_t> ct_sel;
  // the name-matching loop of ac17/mod.rs:403-408 as an index list
  void select(const std::vector<Name>& names, std::vector<uint32_t>* out) const {
    for (const auto& cur : lst)
      for (uint32_t r = 0; r < names.size(); r++) if (same(names[r], cur.first)) out->push_back(r);
  }
  // The first record seen with this plan defines its row names and ct_sel (under mu, once; read-only from then on).  Does a record with
  // these names have that layout -- may it use ct_sel?  Any other record selects on its own.
  bool shares_layout(const std::vector<Name>& names) {
    if (!have_rows.load(std::memory_order_acquire)) {
      std::lock_guard<std::mutex> g(mu);
      if (!have_rows.load(std::memory_order_relaxed)) {
        for (const Name& nm : names) row_names.emplace_back(nm.first, nm.second);
        select(names, &ct_sel);
        have_rows.store(true, std::memory_order_release);
      }
    }
    if (row_names.size() != names.size()) return false;
    for (size_t r = 0; r < names.size(); r++) if (!same(names[r], row_names[r])) return false;
    return true;
  }
};
struct Ac17PlanBucket { PlanCache<Ac17PolPlan> plans; };
struct Ac17PlanCache {
  static std::shared_ptr<Ac17PlanBucket> get(const std::string& fingerprint) {
    static std::mutex mu;
    static std::unordered_map<std::string, std::shared_ptr<Ac17PlanBucket>> m;
    std::lock_guard<std::mutex> g(mu);
    if (m.size() > 64) m.clear();                                     // keys come and go: bounded
    auto& b = m[fingerprint];
    if (!b || b->plans.size() > 4096) b = std::make_shared<Ac17PlanBucket>();       // policies come and go as well
    return b;
  }
};
struct DecKey {
  const Ac17SecretKey& sk;
  const std::vector<std::string>* cp_attrs;      // CP: the key's attributes; the policy comes with every ciphertext
  const PolicyRef* kp_policy;                    // KP: the key's policy; the attributes come with every ciphertext
};
// The plan of one key text: the verdict for this key, the pruned list and the key-side selection.  CP: `text` is a record's policy.  KP:
// `text` is a record's head as the reader accepted it -- u32 count, then (u32 length, bytes) per attribute -- and kp_tree the key's parsed policy.
static void make_plan(Ac17PolPlan& pl, const std::string& text, PolicyLanguage lang, const DecKey& key, const PolicyNode* kp_tree) {
  if (kp_tree) {
    std::vector<std::string> attrs;
    Cursor c{(const uint8_t*)text.data(), (const uint8_t*)text.data() + text.size()};
    for (uint32_t k = 0, cnt = c.u32(); k < cnt; k++) { const Name a = c.str(); attrs.emplace_back(a.first, a.second); }
    if (!traverse_policy(attrs, *kp_tree)) throw RabeError("Error in kp_decrypt: attributes in ct do not match policy in sk.");
    if (!calc_pruned(attrs, *kp_tree, &pl.lst)) throw RabeError("Error in kp_decrypt: pruned attributes in sk do not match policy in ct.");
  } else {
    PolicyNode tree = parse_or_error(text, lang);
    if (!traverse_policy(*key.cp_attrs, tree)) throw RabeError("Error in cp_decrypt: attributes in SK do not match policy in CT.");
    if (!calc_pruned(*key.cp_attrs, tree, &pl.lst)) throw RabeError("Error: attributes in sk do not match policy in ct.");
  }
  for (const auto& cur : pl.lst)
    for (size_t r = 0; r < key.sk.k.size(); r++) if (key.sk.k[r].first == cur.first) pl.sk_sel.push_back((uint32_t)r);
}
static bool decrypt_packed_core(Engine& eng, const DecKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                                int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors,
                                uint8_t* key_buf = nullptr /* decaps: keys instead of plaintexts; pt_buf / pt_cap / pt_off unused */);
bool cp_decrypt_packed(Engine& eng, const Ac17CpSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                       int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  if (sk.sk.k_p.size() != 3) throw RabeError("malformed Ac17CpSecretKey");
  return decrypt_packed_core(eng, DecKey{sk.sk, &sk.attr, nullptr}, n, ct_blob, ct_len, ct_off, trusted, status, pt_buf, pt_cap, pt_off, errors);
}
// Key decapsulation (include/rabe_host.h: rabe_ac17_cp_decaps_packed): cp_decrypt_packed up to the final Gt, then the KDF behind the verdict
// mask (records.h: derive_keys) instead of gather + open.  The sealed part of a record is skipped by its length field and never read.
void cp_decaps_packed(Engine& eng, const Ac17CpSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                      int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  if (sk.sk.k_p.size() != 3) throw RabeError("malformed Ac17CpSecretKey");
  if (n && (!status || !key_buf)) throw RabeError("cp_decaps_packed: null input");
  uint8_t none = 0;          // n = 0: nothing is written
  decrypt_packed_core(eng, DecKey{sk.sk, &sk.attr, nullptr}, n, ct_blob, ct_len, ct_off, trusted, status, nullptr, 0, nullptr, errors, key_buf ? key_buf : &none);
}
bool kp_decrypt_packed(Engine& eng, const Ac17KpSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                       int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  if (!(sk.sk.k_p.empty() || sk.sk.k_p.size() == 3)) throw RabeError("malformed Ac17KpSecretKey");
  return decrypt_packed_core(eng, DecKey{sk.sk, nullptr, &sk.policy}, n, ct_blob, ct_len, ct_off, trusted, status, pt_buf, pt_cap, pt_off, errors);
}
// Key decapsulation over the KP pair (include/rabe_host.h: rabe_ac17_kp_decaps_packed), as cp_decaps_packed: kp_decrypt_packed up to the final Gt
void kp_decaps_packed(Engine& eng, const Ac17KpSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                      int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  if (!(sk.sk.k_p.empty() || sk.sk.k_p.size() == 3)) throw RabeError("malformed Ac17KpSecretKey");
  if (n && (!status || !key_buf)) throw RabeError("kp_decaps_packed: null input");
  uint8_t none = 0;          // n = 0: nothing is written
  decrypt_packed_core(eng, DecKey{sk.sk, nullptr, &sk.policy}, n, ct_blob, ct_len, ct_off, trusted, status, nullptr, 0, nullptr, errors, key_buf ? key_buf : &none);
}
static const char* const C0_NOT_MEMBER = "deserialize: c_0 element is not a member of G2 (FieldError::NotMember)";
static bool decrypt_packed_core(Engine& eng, const DecKey& key, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                                int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors, uint8_t* key_buf) {
  const bool kp = key.kp_policy != nullptr, kem = key_buf != nullptr;
  const Ac17SecretKey& core = key.sk;
  StageTimer tm(kem ? (kp ? "ac17::kp_decaps_packed" : "ac17::cp_decaps_packed") : kp ? "ac17::kp_decrypt_packed" : "ac17::cp_decrypt_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || (n && !ct_blob)) throw RabeError("cp_decrypt_packed: null input");
  // ---- bounds first: everything below trusts [ct_off[i], ct_off[i+1]) to lie inside the blob
  const uint64_t span = check_offsets(n, ct_off, ct_len, errors);
  if (!kem && (!pt_buf || pt_cap < span)) return false;
  // ---- the key
  if (core.k_0.size() != 3) throw RabeError("malformed AC17 secret key");
  for (const auto& row : core.k) if (row.second.size() != 3) throw RabeError("malformed AC17 secret key: a row does not have 3 elements");
  PolicyNode kp_tree;                            // KP: the key's policy, parsed once (a policy that does not parse fails the call like kp_decrypt)
  if (kp) kp_tree = parse_or_error(key.kp_policy->first, key.kp_policy->second);
  // ---- parse + plan.  Per distinct policy text (items of a batch repeat a few): the verdict for this key, the key-side selection and -- for
  // the row layout the first item with that policy shows -- the ciphertext-side selection.  The plans are a pure function of (key attributes /
  // key policy, key row names, policy text): they are kept ACROSS calls (Ac17PlanCache above) -- a queue batch of a few dozen requests spent
  // 1.5 of its 6 ms re-parsing and re-pruning the same sixteen policies.
  std::string fp(kp ? "K" : "C");
  if (kp) { fp += key.kp_policy->first; fp.push_back((char)('0' + (int)key.kp_policy->second)); }
  else for (const auto& a : *key.cp_attrs) { fp += a; fp.push_back('\x1f'); }
  fp.push_back('\x1e');
  for (const auto& row : core.k) { fp += row.first; fp.push_back('\x1f'); }
  const std::shared_ptr<Ac17PlanBucket> bucket = Ac17PlanCache::get(fp);          // holds every plan the items below point to
  BlobGather gather(eng, ct_blob, ct_len);          // the blob starts for the device now, beside the parsing below (records.h)
  struct Item { View rec; Ac17PolPlan* plan = nullptr; bool shared = false; std::vector<uint32_t> own_sel;
                const std::vector<uint32_t>& ct_sel() const { return shared ? plan->ct_sel : own_sel; } };
  std::vector<Item> v(n);
  const auto plan_for_key = [&](Ac17PolPlan& pl, const std::string& text, PolicyLanguage l) { make_plan(pl, text, l, key, kp ? &kp_tree : nullptr); };
  for_each_record(n, errors, [&](size_t i) {
    static thread_local std::vector<Name> names;      // per-thread scratch: no allocation per item
    Item& it = v[i];
    read_record(ct_blob + ct_off[i], ct_blob + ct_off[i + 1], kp, names, &it.rec);
    const PolicyLanguage lang = it.rec.human ? PolicyLanguage::HumanPolicy : PolicyLanguage::JsonPolicy;
    it.plan = bucket->plans.get_kept((const char*)it.rec.key, it.rec.key_len, lang, plan_for_key);          // `bucket` keeps it alive
    if (!it.plan->err.empty()) throw RabeError(it.plan->err);
    it.shared = it.plan->shares_layout(names);
    if (!it.shared) it.plan->select(names, &it.own_sel);
  });
  tm.lap("parse + plan");
  std::vector<size_t> live;
  for (size_t i = 0; i < n; i++) if ((*errors)[i].empty()) live.push_back(i);
  const size_t m = live.size();
  // ---- selection lists: offsets first (a scan), then the lists copied into place on all cores (65 536 items x ~30 entries x 2: 6 ms when
  // serial), straight into pinned staging (65 536 items: 2 x 8 MB), and uploaded from there.  Two plain index lists without weights: not a
  // `Selection`, which is serial and shaped for (record row, key row, z) entries (docs/tried.md).
  std::vector<uint32_t> ct_row_off(m + 1, 0), ct_sel_off(m + 1, 0), sk_sel_off(m + 1, 0);
  for (size_t j = 0; j < m; j++) {
    const Item& w = v[live[j]];
    ct_row_off[j + 1] = ct_row_off[j] + w.rec.rows;
    ct_sel_off[j + 1] = ct_sel_off[j] + (uint32_t)w.ct_sel().size();
    sk_sel_off[j + 1] = sk_sel_off[j] + (uint32_t)w.plan->sk_sel.size();
  }
  const size_t n_ct_sel = ct_sel_off[m], n_sk_sel = sk_sel_off[m];
  uint32_t* const ct_sel = (uint32_t*)eng.pinned_bump((n_ct_sel + n_sk_sel + 2) * 4);
  uint32_t* const sk_sel = ct_sel + n_ct_sel + 1;
  {
    const size_t per = 1024, blocks = (m + per - 1) / per;
    parallel_for(blocks, [&](size_t b) {
      for (size_t j = b * per; j < m && j < (b + 1) * per; j++) {
        const Item& w = v[live[j]];
        const std::vector<uint32_t>&cs = w.ct_sel(), &ss = w.plan->sk_sel;
        if (!cs.empty()) memcpy(ct_sel + ct_sel_off[j], cs.data(), cs.size() * 4);
        if (!ss.empty()) memcpy(sk_sel + sk_sel_off[j], ss.data(), ss.size() * 4);
      }
    });
  }
  // uploaded at once: a later take from the same pinned block may move the block (Engine::pinned_bump waits for the stream first)
  DBuf d_sel(&eng, (n_ct_sel + n_sk_sel + 2) * 4);
  eng.check(rhip_upload_async(eng.ctx(), d_sel.ptr(), ct_sel, (n_ct_sel + n_sk_sel + 2) * 4), "upload (selection lists)");
  const uint32_t* const d_ct_sel = d_sel.as<uint32_t>();
  const uint32_t* const d_sk_sel = d_ct_sel + n_ct_sel + 1;
  if (!m) {
    if (kem) { for (size_t i = 0; i < n; i++) status[i] = -1; if (n) memset(key_buf, 0, n * 32); return true; }
    pt_off[0] = 0;
    for (size_t i = 0; i < n; i++) { pt_off[i + 1] = 0; status[i] = -1; }
    return true;
  }
  const size_t total_rows = ct_row_off[m];
  rhip_ctx* cx = eng.ctx();
  // ---- shapes: the elements are gathered out of the device copy of the blob.  Records on their plan's shared layout share one part list,
  // keyed by the plan; any other record brings its own.  Sharing needs no comparison of offsets: one plan means equal key text (CP: the
  // policy text, behind it ONE language byte whatever its value; KP: the whole attribute head), so c_0 starts at the same offset, and the
  // shared layout means the same number of rows with equal names, which fixes every later offset of the skeleton up to and including c_p.
  std::vector<uint64_t> sealed_off(m);
  std::vector<uint32_t> sealed_len(m);
  for (size_t j = 0; j < m; j++) {
    const Item& w = v[live[j]];
    const uint8_t* rec = ct_blob + ct_off[live[j]];
    sealed_off[j] = (uint64_t)(w.rec.sealed - ct_blob);
    sealed_len[j] = w.rec.sealed_len;
    gather_record(gather, ct_off[live[j]], w.shared ? w.plan : nullptr, [&](std::vector<RecordLayout::Part>& parts) {
      parts.push_back({(uint32_t)(w.rec.c0 - rec), 384, 0, 0});
      for (uint32_t r = 0; r < w.rec.rows; r++) parts.push_back({(uint32_t)(w.rec.row_ptr[r] - rec), 192, 1, 192 * r});
      parts.push_back({(uint32_t)(w.rec.cp - rec), 384, 2, 0});
    });
  }
  // ---- buffers
  std::vector<uint8_t> k0 = flatten(core.k_0), kp_bytes = core.k_p.size() == 3 ? flatten(core.k_p) : std::vector<uint8_t>(3 * 64, 0), kk;   // KP: prod_h starts from G1::zero()
  for (const auto& row : core.k) for (const auto& x : row.second) kk.insert(kk.end(), x.begin(), x.end());
  if (kk.empty()) kk.assign(64, 0);
  std::vector<uint32_t> sk_row_off{0, (uint32_t)core.k.size()}, sk_idx(m, 0);
  DBuf d1(&eng, m * 384), d2(&eng, total_rows * 192 + 4), d4(&eng, m * 384), dout(&eng, m * 384);
  std::vector<uint64_t> dst_off(3 * m);
  for (size_t j = 0; j < m; j++) { dst_off[j] = 384ull * j; dst_off[m + j] = 192ull * ct_row_off[j]; dst_off[2 * m + j] = 384ull * j; }
  std::vector<uint32_t> seg(m + 1);          // c_0: three elements per item
  for (size_t j = 0; j <= m; j++) seg[j] = (uint32_t)j;
  ParamPack pp(eng);
  const size_t h3 = pp.add(ct_row_off), h6 = pp.add(kk), h7 = pp.add(sk_row_off), h8 = pp.add(kp_bytes), h9 = pp.add(sk_idx),
               h11 = pp.add(ct_sel_off), h13 = pp.add(sk_sel_off), h_seg = trusted ? 0 : pp.add(seg);
  pp.upload();
  tm.lap("selection tables");
  gather.run({d1.ptr(), d2.ptr(), d4.ptr()}, dst_off);
  const uint32_t* d3 = pp.dev<uint32_t>(h3);
  // ---- checks: decoding checks over the gathered elements, on the side context beside the decrypt kernels; a non-member fails its item only
  // (the batch still runs: the kernels terminate on any input, the item's result is discarded below).  mc's checks: 0 rows, 1 c_p, and
  // without walk verdicts 2 = c_0 stand-alone, segmented like the rows -- an item's verdict is the AND of its three elements' on either path.
  // c_0's segment offsets (item j = elements 3 j .. 3 j + 2) went up with the call's parameter pack: `pp`, declared before `ws`, outlives
  // the walk's late verdicts, and MemberChecks' side context waits for everything queued before it, the pack's upload included.  WalkScope
  // owns the checks and the walk; its d_g2 is not needed here -- c_0 is d1, which lives as long as the call.
  WalkScope ws;
  if (!trusted) {
    ws.mc.reset(new MemberChecks(eng));
    ws.mc->add(1, d2.ptr(), 3 * total_rows, d3, m, 3);
    ws.mc->add(3, d4.ptr(), m);
    // c_0: the decrypt walks all three elements of every ciphertext -- their subgroup membership comes out of its Miller loops
    if (walk_checks()) ws.walked.reset(new WalkedG2(eng, *ws.mc, d1.ptr(), 3 * m, pp.dev<uint32_t>(h_seg), seg, 3));
    else { ws.k_alone = ws.mc->add_count(); ws.mc->add(2, d1.ptr(), 3 * m, pp.dev<uint32_t>(h_seg), m, 3); }
  }
  // ---- launch.  The key's prepared k_0 lines are a function of the key alone: kept across calls (a server decrypts with the same key again and again)
  std::string k0_key((const char*)k0.data(), k0.size());
  rhip_ac17_sk_lines* lines = (rhip_ac17_sk_lines*)eng.aux("ac17_sk_lines", k0_key, make_ac17_sk_lines, &k0_key, destroy_ac17_sk_lines, 4);
  if (ws.walked) ws.walked->arm();
  eng.check(rhip_ac17_cp_decrypt_batch_prepared(cx, m, d1.as<rhip_g2>(), d2.as<rhip_g1>(), d3, d4.as<rhip_gt>(), lines, pp.dev<rhip_g1>(h6),
                                                pp.dev<uint32_t>(h7), pp.dev<rhip_g1>(h8), pp.dev<uint32_t>(h9), d_ct_sel,
                                                pp.dev<uint32_t>(h11), d_sk_sel, pp.dev<uint32_t>(h13), dout.as<rhip_gt>()),
            "rhip_ac17_cp_decrypt_batch_prepared");
  // ---- verdicts, in the decoder's order: c_0, rows, c_p
  if (ws.mc) {
    ws.mc->collect();
    ws.fail(live, {ws.k_alone}, C0_NOT_MEMBER, errors);
    ws.fail(live, {0}, "deserialize: a row element is not a point of G1 (FieldError::NotMember)", errors);
    ws.fail(live, {1}, "deserialize: c_p is not a member of Gt (FieldError::NotMember)", errors);
  }
  // ---- ending
  if (kem) {          // every verdict first (there is no open to queue behind the pairings), then the KDF behind their mask: 32 n bytes come back
    ws.fail_walked(live, C0_NOT_MEMBER, errors);
    derive_keys(eng, n, live, dout.ptr(), status, key_buf, *errors);
    tm.lap(trusted ? "device: gather, pairings, keys" : "device: gather, pairings, keys; membership beside");
    return true;
  }
  // KDF + AES-GCM open on the device: the decrypted Gt never leaves HBM; plaintext bytes come back in one copy
  open_sealed_records(eng, n, live, dout.ptr(), gather.dev_blob(), sealed_off, sealed_len, status, pt_buf, pt_off, errors);
  ws.retract(live, C0_NOT_MEMBER, status, pt_buf, pt_off, errors);          // read AFTER the open was queued behind the pairings (records.h: retract_item)
  tm.lap(trusted ? "device: gather, pairings, open" : "device: gather, pairings, open; membership beside");
  return true;
}
}  // namespace ac17

// ================================================================================================================= BSW
namespace bsw {
namespace {
void* make_pk(Engine& eng, const void* arg) {
  const CpAbePublicKey& pk = *(const CpAbePublicKey*)arg;
  rhip_bsw_pk* d = nullptr;
  eng.check(rhip_bsw_pk_create(eng.ctx(), (const rhip_g1*)pk.g1.data(), (const rhip_g2*)pk.g2.data(), (const rhip_g1*)pk.h.data(),
                               (const rhip_gt*)pk.e_gg_alpha.data(), &d), "rhip_bsw_pk_create");
  return d;
}
void destroy_pk(void* h) { rhip_bsw_pk_destroy((rhip_bsw_pk*)h); }
void* make_sk_lines(Engine& eng, const void* arg) {          // arg: d | d_j[0].g2 | d_j[1].g2 ... (128 B each)
  const std::string& pts = *(const std::string*)arg;
  DBuf d(&eng, pts.data(), pts.size());
  rhip_bsw_sk_lines* lines = nullptr;
  eng.check(rhip_bsw_sk_prepare(eng.ctx(), 1, pts.size() / 128 - 1, d.as<rhip_g2>(), (const rhip_g2*)(d.as<uint8_t>() + 128), &lines), "rhip_bsw_sk_prepare");
  return lines;
}
void destroy_sk_lines(void* h) { rhip_bsw_sk_lines_destroy((rhip_bsw_sk_lines*)h); }
struct GenTables { rhip_g1_table* g1 = nullptr; rhip_g2_table* g2 = nullptr; };
void* make_gen_tables(Engine& eng, const void* arg) {
  const CpAbePublicKey& pk = *(const CpAbePublicKey*)arg;
  std::unique_ptr<GenTables> t(new GenTables());
  eng.check(rhip_g1_table_create(eng.ctx(), (const rhip_g1*)pk.g1.data(), &t->g1), "rhip_g1_table_create");
  int32_t rc = rhip_g1_table_add_w16(eng.ctx(), t->g1);
  if (!rc) rc = rhip_g2_table_create(eng.ctx(), (const rhip_g2*)pk.g2.data(), &t->g2);
  if (!rc) rc = rhip_g2_table_add_w16(eng.ctx(), t->g2);
  if (rc) { rhip_g1_table_destroy(t->g1); if (t->g2) rhip_g2_table_destroy(t->g2); eng.check(rc, "generator tables"); }
  return t.release();
}
void destroy_gen_tables(void* h) {
  GenTables* t = (GenTables*)h;
  rhip_g1_table_destroy(t->g1);
  rhip_g2_table_destroy(t->g2);
  delete t;
}
}  // namespace

// n calls of bsw::keygen (bsw/mod.rs:125-152) under one master key -- a key authority issuing keys in bulk.  Item i gets the attribute list
// sets[item_set[i]]; draw order per item: r (:130), then r_j per attribute (:142).  Record = CpAbeSecretKey: d, rows (name, g1*r_j,
// g2*r + (g2*h(j))*r_j).  Every element is a fixed-base multiple of a generator: d = g2_alpha/beta + g2*(r/beta) (the first term is
// computed once per call), D_j.g1 = g1*r_j, D_j.g2 = g2*(r + h(j) r_j) -- three window-table launches for the whole batch.
bool keygen_packed(Engine& eng, Rng& rng, const CpAbePublicKey& pk, const CpAbeMasterKey& msk, const std::vector<std::vector<std::string>>& sets, size_t n,
                   const uint32_t* item_set, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm("bsw::keygen_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // master-key-derived scalars pass through the staging buffers
  if (n && (!item_set || !out_off)) throw RabeError("bsw::keygen_packed: null input");
  std::vector<size_t> fixed(sets.size());
  std::vector<std::vector<Fr>> hashes(sets.size());
  for (size_t s = 0; s < sets.size(); s++) {
    if (sets[s].empty()) throw RabeError("bsw::keygen_packed: an empty attribute list (bsw::keygen returns None for it)");
    fixed[s] = 128 + 4;
    for (const auto& a : sets[s]) { fixed[s] += 4 + a.size() + 64 + 128; hashes[s].push_back(sha3_hash_fr(a)); }
  }
  if (!record_offsets("bsw::keygen_packed", "item_set", n, item_set, sets.size(), fixed, nullptr, out_buf, out_cap, out_off)) return false;
  if (!n) return true;
  Fr beta_inv;
  if (!fr_inv(msk.beta, &beta_inv)) throw std::runtime_error("called `Option::unwrap()` on a `None` value (Fr::inverse of zero)");
  std::vector<size_t> row_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) row_off[i + 1] = row_off[i] + sets[item_set[i]].size();
  const size_t total = row_off[n];
  uint8_t* h_k = eng.pinned(0, (n + 2 * total) * 32 + 32);          // r/beta per key | r_j per row | r + h(j) r_j per row
  uint8_t* h_kd = h_k;
  uint8_t* h_k1 = h_k + n * 32;
  uint8_t* h_k2 = h_k1 + total * 32;
  draw_items(rng, n, [&](Rng& r, size_t i) {
    const Fr ri = r.next_fr();
    const Fr kd = fr_mul(ri, beta_inv);
    memcpy(h_kd + 32 * i, kd.l, 32);
    const auto& hs = hashes[item_set[i]];
    for (size_t y = 0; y < hs.size(); y++) {
      const Fr rj = r.next_fr();
      const Fr k2 = fr_add(ri, fr_mul(hs[y], rj));
      memcpy(h_k1 + 32 * (row_off[i] + y), rj.l, 32);
      memcpy(h_k2 + 32 * (row_off[i] + y), k2.l, 32);
    }
  });
  tm.lap("draws + scalars");
  const GenTables* tb;
  {
    std::string key((const char*)pk.g1.data(), 64);
    key.append((const char*)pk.g2.data(), 128);
    tb = (const GenTables*)eng.aux("bsw_gen_tables", key, make_gen_tables, &pk, destroy_gen_tables, 4);
  }
  const G2 a_const = eng.g2_mul({msk.g2_alpha}, {beta_inv})[0];          // g2_alpha / beta, once per call
  std::vector<uint8_t> a_rep(n * 128);
  for (size_t i = 0; i < n; i++) memcpy(a_rep.data() + 128 * i, a_const.data(), 128);
  rhip_ctx* cx = eng.ctx();
  DBuf d_kd(&eng, n * 32), d_k1(&eng, total * 32 + 4), d_k2(&eng, total * 32 + 4), d_a = up_bytes(eng, a_rep), d_dp(&eng, n * 128), d_d(&eng, n * 128),
      d_g1(&eng, total * 64 + 4), d_g2(&eng, total * 128 + 4);
  eng.check(rhip_upload_async(cx, d_kd.ptr(), h_kd, n * 32), "upload");
  eng.check(rhip_upload_async(cx, d_k1.ptr(), h_k1, total * 32), "upload");
  eng.check(rhip_upload_async(cx, d_k2.ptr(), h_k2, total * 32), "upload");
  eng.check(rhip_g2_table_mul(cx, tb->g2, n, d_kd.as<rhip_fr>(), d_dp.as<rhip_g2>()), "rhip_g2_table_mul");
  eng.check(rhip_g2_add(cx, n, d_a.as<rhip_g2>(), d_dp.as<rhip_g2>(), d_d.as<rhip_g2>()), "rhip_g2_add");
  eng.check(rhip_g1_table_mul(cx, tb->g1, total, d_k1.as<rhip_fr>(), d_g1.as<rhip_g1>()), "rhip_g1_table_mul");
  eng.check(rhip_g2_table_mul(cx, tb->g2, total, d_k2.as<rhip_fr>(), d_g2.as<rhip_g2>()), "rhip_g2_table_mul");
  uint8_t* h_o = eng.pinned(1, n * 128 + total * 192 + 4);
  uint8_t* h_g1 = h_o + n * 128;
  uint8_t* h_g2 = h_g1 + total * 64;
  eng.check(rhip_download_async(cx, h_o, d_d.ptr(), n * 128), "download");
  eng.check(rhip_download_async(cx, h_g1, d_g1.ptr(), total * 64), "download");
  eng.check(rhip_download_async(cx, h_g2, d_g2.ptr(), total * 128), "download");
  eng.check(rhip_sync(cx), "rhip_sync");
  tm.lap("device + copies");
  parallel_for(n, [&](size_t i) {
    const auto& attrs = sets[item_set[i]];
    uint8_t* w = out_buf + out_off[i];
    memcpy(w, h_o + 128 * i, 128); w += 128;
    put_u32(w, (uint32_t)attrs.size()); w += 4;
    for (size_t y = 0; y < attrs.size(); y++) {
      put_u32(w, (uint32_t)attrs[y].size()); w += 4;
      memcpy(w, attrs[y].data(), attrs[y].size()); w += attrs[y].size();
      memcpy(w, h_g1 + 64 * (row_off[i] + y), 64); w += 64;
      memcpy(w, h_g2 + 128 * (row_off[i] + y), 128); w += 128;
    }
  });
  tm.lap("assembly");
  return true;
}

// n calls of bsw::delegate (bsw/mod.rs:162-206) on ONE key: item i delegates `sk` to subsets[item_subset[i]].  Draw order per item: r
// (:178), then r_j per attribute of the subset in its order (:183).  d' = d + f * r; per attribute (D_j.g1 + g1 * r_j,
// D_j.g2 + g2 * (h(j) r_j + r)): three window-table launches (f's table is built on first use and kept) and three batched additions;
// records = CpAbeSecretKey, written on the device.  A subset that is empty or not contained in the key's attributes (is_subset,
// tools/mod.rs:24-28 -- delegate returns None) fails the call.
namespace {
void* make_f_table(Engine& eng, const void* arg) {
  rhip_g2_table* t = nullptr;
  eng.check(rhip_g2_table_create(eng.ctx(), (const rhip_g2*)((const G2*)arg)->data(), &t), "rhip_g2_table_create");
  int32_t rc = rhip_g2_table_add_w16(eng.ctx(), t);
  if (rc) { rhip_g2_table_destroy(t); eng.check(rc, "rhip_g2_table_add_w16"); }
  return t;
}
void destroy_f_table(void* h) { rhip_g2_table_destroy((rhip_g2_table*)h); }
}  // namespace
bool delegate_packed(Engine& eng, Rng& rng, const CpAbePublicKey& pk, const CpAbeSecretKey& sk, const std::vector<std::vector<std::string>>& subsets, size_t n,
                     const uint32_t* item_subset, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm("bsw::delegate_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // the key's elements pass through the staging buffers
  if (n && (!item_subset || !out_off)) throw RabeError("bsw::delegate_packed: null input");
  std::vector<std::vector<uint32_t>> row_of(subsets.size());          // subset attribute -> the key's row
  std::vector<std::vector<Fr>> hashes(subsets.size());
  std::vector<RecordLayout> layouts(subsets.size());
  for (size_t s_ = 0; s_ < subsets.size(); s_++) {
    if (subsets[s_].empty()) throw RabeError("bsw::delegate_packed: an empty subset (bsw::delegate returns None for it)");
    RecordLayout& L = layouts[s_];
    L.src(0, 0, 128);
    L.u32((uint32_t)subsets[s_].size());
    for (size_t y = 0; y < subsets[s_].size(); y++) {
      const std::string& a = subsets[s_][y];
      uint32_t r = 0;
      while (r < sk.d_j.size() && sk.d_j[r].string != a) r++;
      if (r == sk.d_j.size()) throw RabeError("bsw::delegate_packed: the subset is not contained in the key's attributes (bsw::delegate returns None)");
      row_of[s_].push_back(r);
      hashes[s_].push_back(sha3_hash_fr(a));
      L.str(a);
      L.src(1, (uint32_t)(64 * y), 64);
      L.src(2, (uint32_t)(128 * y), 128);
    }
  }
  if (!record_offsets("bsw::delegate_packed", "item_subset", n, item_subset, subsets.size(), [&](size_t i) { return layouts[item_subset[i]].bytes(); }, nullptr,
                      out_buf, out_cap, out_off)) return false;
  if (!n) return true;
  std::vector<size_t> row_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) row_off[i + 1] = row_off[i] + subsets[item_subset[i]].size();
  const size_t total = row_off[n];
  uint8_t* h_k = eng.pinned(0, (n + 2 * total) * 32 + 32);          // r per item | r_j per row | h(j) r_j + r per row
  uint8_t* h_kr = h_k;
  uint8_t* h_k1 = h_k + n * 32;
  uint8_t* h_k2 = h_k1 + total * 32;
  uint8_t* h_old = eng.pinned(1, n * 128 + total * 192 + 4);         // d per item | D_j.g1 per row | D_j.g2 per row
  uint8_t* h_o1 = h_old + n * 128;
  uint8_t* h_o2 = h_o1 + total * 64;
  draw_items(rng, n, [&](Rng& r, size_t i) {
    const Fr ri = r.next_fr();
    memcpy(h_kr + 32 * i, ri.l, 32);
    memcpy(h_old + 128 * i, sk.d.data(), 128);
    const size_t s_ = item_subset[i];
    for (size_t y = 0; y < hashes[s_].size(); y++) {
      const Fr rj = r.next_fr();
      const Fr k2 = fr_add(fr_mul(hashes[s_][y], rj), ri);
      memcpy(h_k1 + 32 * (row_off[i] + y), rj.l, 32);
      memcpy(h_k2 + 32 * (row_off[i] + y), k2.l, 32);
      memcpy(h_o1 + 64 * (row_off[i] + y), sk.d_j[row_of[s_][y]].g1.data(), 64);
      memcpy(h_o2 + 128 * (row_off[i] + y), sk.d_j[row_of[s_][y]].g2.data(), 128);
    }
  });
  tm.lap("draws + scalars");
  const GenTables* tb;
  {
    std::string key((const char*)pk.g1.data(), 64);
    key.append((const char*)pk.g2.data(), 128);
    tb = (const GenTables*)eng.aux("bsw_gen_tables", key, make_gen_tables, &pk, destroy_gen_tables, 4);
  }
  rhip_g2_table* ft = (rhip_g2_table*)eng.aux("bsw_f_table", std::string((const char*)pk.f.data(), 128), make_f_table, &pk.f, destroy_f_table, 4);
  rhip_ctx* cx = eng.ctx();
  DBuf d_k(&eng, (n + 2 * total) * 32 + 32), d_old(&eng, n * 128 + total * 192 + 4), d_fr(&eng, n * 128), d_m1(&eng, total * 64 + 4), d_m2(&eng, total * 128 + 4),
      d_d(&eng, n * 128), d_g1(&eng, total * 64 + 4), d_g2(&eng, total * 128 + 4);
  eng.check(rhip_upload_async(cx, d_k.ptr(), h_k, (n + 2 * total) * 32), "upload");
  eng.check(rhip_upload_async(cx, d_old.ptr(), h_old, n * 128 + total * 192), "upload");
  const rhip_fr* kr = d_k.as<rhip_fr>();
  const uint8_t* old = d_old.as<uint8_t>();
  eng.check(rhip_g2_table_mul(cx, ft, n, kr, d_fr.as<rhip_g2>()), "rhip_g2_table_mul");
  eng.check(rhip_g2_add(cx, n, (const rhip_g2*)old, d_fr.as<rhip_g2>(), d_d.as<rhip_g2>()), "rhip_g2_add");
  eng.check(rhip_g1_table_mul(cx, tb->g1, total, kr + n, d_m1.as<rhip_g1>()), "rhip_g1_table_mul");
  eng.check(rhip_g1_add(cx, total, (const rhip_g1*)(old + n * 128), d_m1.as<rhip_g1>(), d_g1.as<rhip_g1>()), "rhip_g1_add");
  eng.check(rhip_g2_table_mul(cx, tb->g2, total, kr + n + total, d_m2.as<rhip_g2>()), "rhip_g2_table_mul");
  eng.check(rhip_g2_add(cx, total, (const rhip_g2*)(old + n * 128 + total * 64), d_m2.as<rhip_g2>(), d_g2.as<rhip_g2>()), "rhip_g2_add");
  emit_plain_records(eng, layouts, n, item_subset, RecordSources(n).by_item(d_d.ptr(), 128).by_rows(d_g1.ptr(), 64, row_off).by_rows(d_g2.ptr(), 128, row_off),
                     out_off, out_buf);
  tm.lap("device: fixed-base multiplications, additions, records; one copy out");
  return true;
}

// n calls of bsw::encrypt (bsw/mod.rs:217-251).  Draw order per item: secret (:228), msg (:229), the gate coefficients of
// gen_shares_policy (secretsharing/mod.rs:128-134), the AES nonce (aes/mod.rs:17).  Record = CpAbeCiphertext:
//   policy text, language, c, c_p, leaf count, per leaf (name_col, g1 * q_y, (g2 * h(name)) * q_y), sealed plaintext.
// key_buf != nullptr is the key encapsulation (encaps_packed below): no plaintexts, no nonce draw, records that end in the length field of an
// empty sealed part, and per item the content key SHA3-256(bytes(msg)) instead of a payload sealed under it.
static bool encrypt_core(Engine& eng, Rng& rng, const CpAbePublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                         const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off,
                         uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? "bsw::encaps_packed" : "bsw::encrypt_packed");
  Engine::ArenaScope arena(eng);
  ShareTrees st;
  for (const auto& p : policies) st.add(p, language);
  const auto& pols = st.pols;
  // records and sealing on the device (records.h); a record's size is its layout's
  std::vector<size_t> fixed(policies.size());
  std::vector<RecordLayout> layouts(policies.size());
  for (size_t p_ = 0; p_ < policies.size(); p_++) {
    RecordLayout& L = layouts[p_];
    const FlatPolicy& f = *pols[p_];
    policy_header(L, policies[p_], language);
    L.src(0, 0, 64);
    L.src(1, 0, 384);
    L.u32((uint32_t)f.leaf_name.size());
    for (size_t y = 0; y < f.leaf_name.size(); y++) {
      L.str(f.leaf_name_col[y]);
      L.src(2, (uint32_t)(64 * y), 64);
      L.src(3, (uint32_t)(128 * y), 128);
    }
    fixed[p_] = close_ciphertext(L, kem);
  }
  if (!record_offsets("bsw::encrypt_packed", "item_policy", n, item_policy, policies.size(), fixed, kem ? nullptr : pt_off, out_buf, out_cap, out_off)) return false;
  st.place(n, item_policy, 1);
  const std::vector<uint32_t>&leaf_off = st.leaf_off, &coef_off = st.coef_off;
  const size_t total = st.total, total_coef = st.total_coef;
  tm.lap("policies");
  uint8_t* h_in = eng.pinned(0, n * 64 + (total_coef + 1) * 32);          // secret | msg exponent | coefficients
  uint8_t* h_sec = h_in;
  uint8_t* h_rho = h_in + n * 32;
  uint8_t* h_coef = h_in + n * 64;
  std::vector<std::array<uint8_t, 12>> nonces(n);
  draw_items(rng, n, [&](Rng& r, size_t i) {
    Fr s = r.next_fr(), rho = r.next_fr();
    memcpy(h_sec + 32 * i, s.l, 32);
    memcpy(h_rho + 32 * i, rho.l, 32);
    for (uint32_t c = coef_off[i]; c < coef_off[i + 1]; c++) { Fr a = r.next_fr(); memcpy(h_coef + 32 * (size_t)c, a.l, 32); }
    if (!kem) r.fill(nonces[i].data(), 12);
  });
  tm.lap("draws");
  rhip_ctx* cx = eng.ctx();
  std::string key((const char*)pk.g1.data(), 64);
  key.append((const char*)pk.g2.data(), 128).append((const char*)pk.h.data(), 64).append((const char*)pk.e_gg_alpha.data(), 384);
  rhip_bsw_pk* dpk = (rhip_bsw_pk*)eng.aux("bsw_pk", key, make_pk, &pk, destroy_pk);
  st.upload(eng);
  DBuf d_in(&eng, n * 64 + (total_coef + 1) * 32), d_msg(&eng, n * 384), d_c(&eng, n * 64), d_cp(&eng, n * 384), d_g1(&eng, total * 64), d_g2(&eng, total * 128);
  eng.check(rhip_upload_async(cx, d_in.ptr(), h_in, n * 64 + total_coef * 32), "upload");
  const rhip_fr* dsec = d_in.as<rhip_fr>();
  eng.check(rhip_gt_table_pow(cx, eng.gt_generator_table(), n, dsec + n, d_msg.as<rhip_gt>()), "rhip_gt_table_pow");
  eng.check(rhip_bsw_encrypt_batch(cx, dpk, n, total,
                                   st.d_leaf_off, st.d_tree_leaf, st.d_tree_gate, st.d_path_off, st.d_path_gate, st.d_path_x, st.d_gate_k, st.d_gate_coef_off, st.d_leaf_hash,
                                   dsec, dsec + 2 * n, st.d_coef_off, d_msg.as<rhip_gt>(), d_c.as<rhip_g1>(), d_cp.as<rhip_gt>(), d_g1.as<rhip_g1>(),
                                   d_g2.as<rhip_g2>()), "rhip_bsw_encrypt_batch");
  RecordSources src(n);
  src.by_item(d_c.ptr(), 64).by_item(d_cp.ptr(), 384).by_rows(d_g1.ptr(), 64, leaf_off).by_rows(d_g2.ptr(), 128, leaf_off);
  finish_encrypt(eng, &tm, layouts, n, item_policy, src, d_msg.ptr(), (const uint8_t*)nonces.data(), pt_blob, pt_off, out_off, out_buf, key_buf);
  return true;
}
bool encrypt_packed(Engine& eng, Rng& rng, const CpAbePublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                    const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  return encrypt_core(eng, rng, pk, policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off, nullptr);
}
bool encaps_packed(Engine& eng, Rng& rng, const CpAbePublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                   const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  if (n && !key_buf) throw RabeError("bsw::encaps_packed: null input");
  if (!n) { out_off[0] = 0; return true; }
  return encrypt_core(eng, rng, pk, policies, language, n, item_policy, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}

// n calls of bsw::decrypt (bsw/mod.rs:260-318) with one key.  Per distinct policy text: traverse_policy, calc_pruned and the
// coefficients, turned into the selection entries the device path takes -- entry = (ciphertext leaf row, key attribute row, z):
// for every pruned (name, name_col) the FIRST ciphertext row named name_col, the FIRST key row named name, and one entry per
// coefficient named name_col (:283-299 as index lists).  status / errors / buffers as ac17::cp_decrypt_packed.
// key_buf != nullptr is the key decapsulation (decaps_packed below): the same launch set up to the final Gt, then the KDF behind the verdict mask
// (records.h: derive_keys) instead of the open; pt_buf / pt_cap / pt_off are unused, the sealed part is skipped by its length field and never read.
static bool decrypt_core(Engine& eng, const CpAbeSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                         int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors, uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? "bsw::decaps_packed" : "bsw::decrypt_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || (n && !ct_blob)) throw RabeError("bsw::decrypt_packed: null input");
  const uint64_t span = check_offsets(n, ct_off, ct_len, errors);
  if (!kem && (!pt_buf || pt_cap < span)) return false;
  BlobGather gather(eng, ct_blob, ct_len);          // the blob starts for the device now, beside the parsing below (records.h)
  std::vector<std::string> attr;
  for (const auto& v : sk.d_j) attr.push_back(v.string);
  struct Plan {
    std::shared_ptr<const FlatPolicy> flat; std::string err;
    struct E { std::string name_col; uint32_t sk_row; Fr z; uint32_t std_ct_row; };
    std::vector<E> ent;
  };
  PlanCache<Plan> plans;
  auto make_plan = [&](Plan& pl, const std::string& text, PolicyLanguage lang) {
    pl.flat = flat_policy(text, lang);
    const PolicyNode& tree = pl.flat->tree;
    if (!traverse_policy(attr, tree)) throw RabeError("Error in bsw/encrypt: attributes do not match policy.");
    PrunedList pruned;
    if (!calc_pruned(attr, tree, &pruned)) throw RabeError("Error in bsw/encrypt: attributes do not match policy.");
    for (const auto& pr : pruned) {
      size_t dj = 0;
      while (dj < sk.d_j.size() && sk.d_j[dj].string != pr.first) dj++;
      if (dj == sk.d_j.size()) continue;
      size_t std_row = 0;
      while (std_row < pl.flat->leaf_name_col.size() && pl.flat->leaf_name_col[std_row] != pr.second) std_row++;
      for (size_t y = 0; y < pl.flat->leaf_name_col.size(); y++)
        if (pl.flat->leaf_name_col[y] == pr.second) pl.ent.push_back({pr.second, (uint32_t)dj, pl.flat->leaf_coeff[y], (uint32_t)std_row});
    }
  };
  struct View { const uint8_t* c; const uint8_t* cp; uint32_t rows; std::vector<const uint8_t*> g1, g2; std::shared_ptr<Plan> plan;
                std::vector<uint32_t> ct_row; bool standard; };
  std::vector<View> v(n);
  std::vector<Sealed> sealed(n);
  for_each_record(n, errors, [&](size_t i) {
    Cursor r{ct_blob + ct_off[i], ct_blob + ct_off[i + 1]};
    auto pol = r.str();
    const PolicyLanguage lang = *r.raw(1) ? PolicyLanguage::HumanPolicy : PolicyLanguage::JsonPolicy;
    v[i].c = r.raw(64);
    v[i].cp = r.raw(384);
    const uint32_t rows = r.u32();
    if ((size_t)rows * 196 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
    v[i].rows = rows;
    v[i].g1.resize(rows);
    v[i].g2.resize(rows);
    std::vector<std::pair<const char*, uint32_t>> names(rows);
    for (uint32_t y = 0; y < rows; y++) { names[y] = r.str(); v[i].g1[y] = r.raw(64); v[i].g2[y] = r.raw(128); }
    sealed[i].len = r.u32();
    sealed[i].p = r.raw(sealed[i].len);
    auto pl = plans.get(pol.first, pol.second, lang, make_plan);
    if (!pl->err.empty()) throw RabeError(pl->err);
    v[i].plan = pl;
    const auto& std_names = pl->flat->leaf_name_col;
    bool standard = rows == std_names.size();
    for (uint32_t y = 0; y < rows && standard; y++) standard = same(names[y], std_names[y]);
    v[i].standard = standard;
    if (!standard) {                              // rows in another order / other names: the name-matching loop itself (:283-287)
      for (const auto& e : pl->ent) {
        uint32_t y = 0;
        while (y < rows && !same(names[y], e.name_col)) y++;
        v[i].ct_row.push_back(y);               // y == rows: no such row -> the entry is skipped below
      }
    }
  });
  tm.lap("parse + plan");
  Selection sel(2, 1);          // m entries: 2 m + 1 pairs
  for (size_t i = 0; i < n; i++) {
    if (!(*errors)[i].empty()) continue;
    const View& w = v[i];
    sel.add(i, w.rows, w.plan.get(), w.standard, [&](auto emit) {
      const auto& ent = w.plan->ent;
      for (size_t e = 0; e < ent.size(); e++) {
        if (w.standard) emit(ent[e].std_ct_row, ent[e].sk_row, ent[e].z);
        else if (w.ct_row[e] < w.rows) emit(w.ct_row[e], ent[e].sk_row, ent[e].z);
      }
    });
  }
  const std::vector<size_t>& live = sel.live;
  const std::vector<uint32_t>& leaf_off = sel.row_off;
  const size_t m_items = live.size();
  std::vector<uint64_t> sealed_off(m_items);
  std::vector<uint32_t> sealed_len(m_items);
  DBuf d_out(&eng, m_items * 384 + 4);
  WalkScope ws;          // the decoding checks run on the side context, beside the decrypt kernels (common.h)
  if (m_items) {
    const size_t total = leaf_off[m_items];
    DBuf d_c(&eng, m_items * 64), d_cp(&eng, m_items * 384), d_g1(&eng, total * 64 + 4);
    DBuf& d_g2 = ws.d_g2 = DBuf(&eng, total * 128 + 4);
    std::vector<uint64_t> dst_off(4 * m_items);
    for (size_t j = 0; j < m_items; j++) {
      const View& w = v[live[j]];
      const uint8_t* rec = ct_blob + ct_off[live[j]];
      sealed_off[j] = (uint64_t)(sealed[live[j]].p - ct_blob);
      sealed_len[j] = sealed[live[j]].len;
      dst_off[j] = 64ull * j; dst_off[m_items + j] = 384ull * j; dst_off[2 * m_items + j] = 64ull * leaf_off[j]; dst_off[3 * m_items + j] = 128ull * leaf_off[j];
      // standard layout: policy text and names as encrypt writes them -> one skeleton
      gather_record(gather, ct_off[live[j]], w.standard ? w.plan.get() : nullptr, [&](std::vector<RecordLayout::Part>& parts) {
        parts.push_back({(uint32_t)(w.c - rec), 64, 0, 0});
        parts.push_back({(uint32_t)(w.cp - rec), 384, 1, 0});
        for (uint32_t y = 0; y < w.rows; y++) {
          parts.push_back({(uint32_t)(w.g1[y] - rec), 64, 2, 64 * y});
          parts.push_back({(uint32_t)(w.g2[y] - rec), 128, 3, 128 * y});
        }
      });
    }
    tm.lap("shapes");
    rhip_ctx* cx = eng.ctx();
    std::vector<uint8_t> kg1, kg2;
    for (const auto& a : sk.d_j) { kg1.insert(kg1.end(), a.g1.begin(), a.g1.end()); kg2.insert(kg2.end(), a.g2.begin(), a.g2.end()); }
    std::vector<uint32_t> sk_attr_off{0, (uint32_t)sk.d_j.size()};
    auto fz = flatten_fr(sel.sel_z);
    DBuf d_leaf_off = up32(eng, leaf_off),
        d_pair_off = up32(eng, sel.pair_off), d_sel_start = up32(eng, sel.sel_start), d_sel_ct = up32(eng, sel.sel_rec), d_sel_sk = up32(eng, sel.sel_one),
        d_sel_z = up_bytes(eng, fz), d_skd(&eng, sk.d.data(), 128), d_kg1 = up_bytes(eng, kg1), d_kg2 = up_bytes(eng, kg2),
        d_sk_attr_off = up32(eng, sk_attr_off);
    gather.run({d_c.ptr(), d_cp.ptr(), d_g1.ptr(), d_g2.ptr()}, dst_off);
    // the key's prepared lines (d and every d_j.g2: 17 KB per point) are a function of the key alone: kept across calls
    rhip_bsw_sk_lines* lines = nullptr;
    if (!sk.d_j.empty()) {
      std::string key((const char*)sk.d.data(), 128);
      for (const auto& a : sk.d_j) key.append((const char*)a.g2.data(), 128);
      lines = (rhip_bsw_sk_lines*)eng.aux("bsw_sk_lines", key, make_sk_lines, &key, destroy_sk_lines, 4);
    }
    if (!trusted) {
      ws.mc.reset(new MemberChecks(eng));
      ws.mc->add(1, d_c.ptr(), m_items); ws.mc->add(1, d_g1.ptr(), total, d_leaf_off.as<uint32_t>(), m_items);
      ws.mc->add(3, d_cp.ptr(), m_items);
      // Cy.g2 of every selected leaf is the walking argument of a pairing (the key's side replays prepared lines): the decrypt's own
      // Miller loops say whether it is a member of G2; leaves the policy did not select get the stand-alone test (common.h: WalkedG2)
      ws.check_g2(eng, walk_checks() && lines, sel, total, d_leaf_off.as<uint32_t>());
    }
    // one key for all ciphertexts: its scaled Dj.g1 are computed once per selection entry (ciphertexts that share a policy share them)
    if (ws.walked) ws.walked->arm();
    int32_t rc = rhip_bsw_decrypt_batch_one_sk(cx, m_items, sel.max_pairs, sel.pair_off[m_items], sel.sel_rec.size(), d_pair_off.as<uint32_t>(),
                                               d_sel_start.as<uint32_t>(), d_sel_ct.as<uint32_t>(), d_sel_sk.as<uint32_t>(), d_sel_z.as<rhip_fr>(), d_c.as<rhip_g1>(),
                                               d_cp.as<rhip_gt>(), d_g1.as<rhip_g1>(), d_g2.as<rhip_g2>(), d_leaf_off.as<uint32_t>(), d_skd.as<rhip_g2>(),
                                               d_kg1.as<rhip_g1>(), d_kg2.as<rhip_g2>(), d_sk_attr_off.as<uint32_t>(), lines, d_out.as<rhip_gt>());
    eng.check(rc, "rhip_bsw_decrypt_batch");
    if (ws.mc) {
      ws.mc->collect();
      ws.fail(live, {0}, "deserialize: c is not a point of G1 (FieldError::NotMember)", errors);
      ws.fail(live, {2}, "deserialize: c_p is not a member of Gt (FieldError::NotMember)", errors);
      ws.fail(live, {1, ws.k_alone}, "deserialize: a leaf element is not a group member (FieldError::NotMember)", errors);
    }
  }
  if (kem) {
    ws.fail_walked(live, "deserialize: a leaf element is not a group member (FieldError::NotMember)", errors);
    derive_keys(eng, n, live, d_out.ptr(), status, key_buf, *errors);
    tm.lap(trusted ? "device: gather, pairings, keys" : "device: gather, pairings, keys; membership beside");
    return true;
  }
  // KDF + AES-GCM open on the device: the decrypted Gt never leaves HBM; plaintext bytes come back in one copy
  open_sealed_records(eng, n, live, d_out.ptr(), gather.dev_blob(), sealed_off, sealed_len, status, pt_buf, pt_off, errors);
  ws.retract(live, "deserialize: a leaf element is not a group member (FieldError::NotMember)", status, pt_buf, pt_off, errors);
  tm.lap(trusted ? "device: gather, pairings, open" : "device: gather, pairings, open; membership beside");
  return true;
}
bool decrypt_packed(Engine& eng, const CpAbeSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                    int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  return decrypt_core(eng, sk, n, ct_blob, ct_len, ct_off, trusted, status, pt_buf, pt_cap, pt_off, errors, nullptr);
}
void decaps_packed(Engine& eng, const CpAbeSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                   int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  if (n && (!status || !key_buf)) throw RabeError("bsw::decaps_packed: null input");
  uint8_t none = 0;          // n = 0: nothing is written
  decrypt_core(eng, sk, n, ct_blob, ct_len, ct_off, trusted, status, nullptr, 0, nullptr, errors, key_buf ? key_buf : &none);
}
}  // namespace bsw


// ================================================================================================================= LSW
namespace lsw {
namespace {
void* make_pk(Engine& eng, const void* arg) {
  const KpAbePublicKey& pk = *(const KpAbePublicKey*)arg;
  rhip_lsw_pk* d = nullptr;
  eng.check(rhip_lsw_pk_create(eng.ctx(), (const rhip_g1*)pk.g1.data(), (const rhip_g2*)pk.g2.data(), &d), "rhip_lsw_pk_create");
  return d;
}
void destroy_pk(void* h) { rhip_lsw_pk_destroy((rhip_lsw_pk*)h); }
void* make_e2_lines(Engine& eng, const void* arg) {
  const std::string& pt = *(const std::string*)arg;
  DBuf d(&eng, pt.data(), pt.size());
  rhip_g2_lines* lines = nullptr;
  eng.check(rhip_g2_lines_prepare(eng.ctx(), 1, d.as<rhip_g2>(), &lines), "rhip_g2_lines_prepare");
  return lines;
}
void destroy_e2_lines(void* h) { rhip_g2_lines_destroy((rhip_g2_lines*)h); }
}  // namespace

namespace {
struct EncTables { rhip_g1_table* g1 = nullptr; rhip_g1_table* g1_b = nullptr; rhip_g1_table* g1_b2 = nullptr; rhip_g1_table* h_b = nullptr;
                   rhip_g2_table* g2 = nullptr; rhip_gt_table* egg = nullptr; };
void destroy_enc_tables(void* h) {
  EncTables* t = (EncTables*)h;
  if (t->g1) rhip_g1_table_destroy(t->g1);
  if (t->g1_b) rhip_g1_table_destroy(t->g1_b);
  if (t->g1_b2) rhip_g1_table_destroy(t->g1_b2);
  if (t->h_b) rhip_g1_table_destroy(t->h_b);
  if (t->g2) rhip_g2_table_destroy(t->g2);
  if (t->egg) rhip_gt_table_destroy(t->egg);
  delete t;
}
void* make_enc_tables(Engine& eng, const void* arg) {
  const KpAbePublicKey& pk = *(const KpAbePublicKey*)arg;
  EncTables* t = new EncTables();
  rhip_ctx* cx = eng.ctx();
  int32_t rc = rhip_g1_table_create(cx, (const rhip_g1*)pk.g1.data(), &t->g1);
  if (!rc) rc = rhip_g1_table_add_w16(cx, t->g1);
  if (!rc) rc = rhip_g1_table_create(cx, (const rhip_g1*)pk.g1_b.data(), &t->g1_b);
  if (!rc) rc = rhip_g1_table_add_w16(cx, t->g1_b);
  if (!rc) rc = rhip_g1_table_create(cx, (const rhip_g1*)pk.g1_b2.data(), &t->g1_b2);
  if (!rc) rc = rhip_g1_table_add_w16(cx, t->g1_b2);
  if (!rc) rc = rhip_g1_table_create(cx, (const rhip_g1*)pk.h_b.data(), &t->h_b);
  if (!rc) rc = rhip_g1_table_add_w16(cx, t->h_b);
  if (!rc) rc = rhip_g2_table_create(cx, (const rhip_g2*)pk.g2.data(), &t->g2);
  if (!rc) rc = rhip_g2_table_add_w16(cx, t->g2);
  if (!rc) rc = rhip_gt_table_create(cx, (const rhip_gt*)pk.e_gg_alpha.data(), &t->egg);
  if (!rc) rc = rhip_gt_table_add_w16(cx, t->egg);
  if (rc) { destroy_enc_tables(t); eng.check(rc, "lsw public-key tables"); }
  return t;
}
}  // namespace
// The rows of the ciphertexts, two ways.  Both read the call's scalar block d_k (per item secret | msg exponent, then what the draw loop stored
// per row) and leave the sources of the three row elements in `src`.  heads() uploads d_k and queues msg, e1 and e2: a stage calls it once it
// has its buffers, so that the fused stage's small blocking uploads go before anything is queued, not behind it.
namespace {
// encrypt: the host stored h*secret | sx | sx*h per row; four table walks and an addition write e3, e4, e5 as three arrays of 64-byte rows
void rows_by_tables(Engine& eng, const EncTables* tb, size_t n, size_t total, const DBuf& d_k, const std::vector<uint32_t>& row_off,
                    const std::function<void()>& heads, std::vector<DBuf>& keep, RecordSources& src) {
  rhip_ctx* cx = eng.ctx();
  const rhip_fr* k_a = d_k.as<rhip_fr>() + 2 * n;
  const rhip_fr* k_b = k_a + total;
  const rhip_fr* k_c = k_b + total;
  DBuf d_r1(&eng, total * 64 + 4), d_r2(&eng, total * 64 + 4), d_t1(&eng, total * 64 + 4), d_t2(&eng, total * 64 + 4), d_r3(&eng, total * 64 + 4);
  heads();
  eng.check(rhip_g1_table_mul(cx, tb->g1, total, k_a, d_r1.as<rhip_g1>()), "rhip_g1_table_mul");
  eng.check(rhip_g1_table_mul(cx, tb->g1_b, total, k_b, d_r2.as<rhip_g1>()), "rhip_g1_table_mul");
  eng.check(rhip_g1_table_mul(cx, tb->g1_b2, total, k_c, d_t1.as<rhip_g1>()), "rhip_g1_table_mul");
  eng.check(rhip_g1_table_mul(cx, tb->h_b, total, k_b, d_t2.as<rhip_g1>()), "rhip_g1_table_mul");
  eng.check(rhip_g1_add(cx, total, d_t1.as<rhip_g1>(), d_t2.as<rhip_g1>(), d_r3.as<rhip_g1>()), "rhip_g1_add");
  src.by_rows(d_r1.ptr(), 64, row_off).by_rows(d_r2.ptr(), 64, row_off).by_rows(d_r3.ptr(), 64, row_off);
  for (DBuf* d : {&d_r1, &d_r2, &d_t1, &d_t2, &d_r3}) keep.push_back(std::move(*d));
}
// encaps: the host stored sx alone; one lane per row (k_lsw_enc_rows) forms h secret and sx h on the device from one hash per (list, position),
// takes e5 as two walks on one accumulator and shares one inversion among a row's three conversions: one array of 192-byte rows
void rows_fused(Engine& eng, const EncTables* tb, size_t n, size_t total, const DBuf& d_k, const std::vector<uint32_t>& row_off,
                const std::vector<uint32_t>& hash_off, const std::vector<Fr>& hashes, const std::function<void()>& heads, std::vector<DBuf>& keep,
                RecordSources& src) {
  DBuf d_rows(&eng, total * 192 + 4), d_row_off = up32(eng, row_off), d_hash_off = up32(eng, hash_off), d_hash = up_bytes(eng, flatten_fr(hashes));
  const rhip_fr* k_sec = d_k.as<rhip_fr>();
  heads();
  eng.check(rhip_lsw_encrypt_rows(eng.ctx(), tb->g1, tb->g1_b, tb->g1_b2, tb->h_b, n, total, d_row_off.as<uint32_t>(), d_hash_off.as<uint32_t>(),
                                  d_hash.as<rhip_fr>(), k_sec, k_sec + 2 * n, d_rows.as<rhip_g1>()), "rhip_lsw_encrypt_rows");
  src.by_rows(d_rows.ptr(), 192, row_off);
  for (DBuf* d : {&d_rows, &d_row_off, &d_hash_off, &d_hash}) keep.push_back(std::move(*d));
}
}  // namespace

// n calls of lsw::encrypt (lsw/mod.rs:180-219): item i under the attribute list sets[item_set[i]].  Draw order per item: secret (:188), one
// sx per attribute (:196-200, with the reference's index quirk: sx[0] loses sx[i], not the new element), the message exponent, the nonce.
// Record = KpAbeCiphertext: e1 = e_gg_alpha^secret * msg, e2 = g2*secret, rows (name, g1*(h(a) secret), g1_b*sx_i, g1_b2*(sx_i h(a)) + h_b*sx_i),
// sealed plaintext.  Every element is a fixed-base multiple of a public-key element: window-table launches for the whole batch.
// key_buf != nullptr is the key encapsulation (encaps_packed below): no plaintexts, no nonce draw, records that end in the length field of an
// empty sealed part, per item the content key SHA3-256(bytes(msg)) -- and the rows from the fused kernel (rows_fused), which writes the
// three elements of a row side by side: the kem flag forks what the draw loop stores, the row stage and with it the row source, nothing else.
static bool encrypt_core(Engine& eng, Rng& rng, const KpAbePublicKey& pk, const std::vector<std::vector<std::string>>& sets, size_t n, const uint32_t* item_set,
                         const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  const char* const what = kem ? "lsw::encaps_packed" : "lsw::encrypt_packed";
  StageTimer tm(what);
  Engine::ArenaScope arena(eng);
  std::vector<size_t> fixed(sets.size());
  std::vector<uint32_t> set_hash_off(sets.size() + 1, 0);
  std::vector<Fr> hashes;
  std::vector<RecordLayout> layouts(sets.size());          // layout = attribute set; a record's size is its layout's
  for (size_t s = 0; s < sets.size(); s++) {
    if (sets[s].empty()) throw RabeError("attributes or data empty");
    RecordLayout& L = layouts[s];
    L.src(0, 0, 384);
    L.src(1, 0, 128);
    L.u32((uint32_t)sets[s].size());
    for (size_t y = 0; y < sets[s].size(); y++) {
      hashes.push_back(sha3_hash_fr(sets[s][y]));
      L.str(sets[s][y]);
      if (kem) L.src(2, (uint32_t)(192 * y), 192);
      else for (uint32_t k = 2; k < 5; k++) L.src(k, (uint32_t)(64 * y), 64);
    }
    set_hash_off[s + 1] = (uint32_t)hashes.size();
    fixed[s] = close_ciphertext(L, kem);
  }
  // the first bad item decides the message: an empty payload counts up to the first index out of range, which record_offsets reports
  if (!kem) for (size_t i = 0; i < n && item_set[i] < sets.size(); i++) if (pt_off[i + 1] <= pt_off[i]) throw RabeError("attributes or data empty");
  if (!record_offsets(what, "item_set", n, item_set, sets.size(), fixed, pt_off, out_buf, out_cap, out_off)) return false;
  if (!n) return true;
  std::vector<uint32_t> row_off(n + 1, 0), hash_off(n);
  for (size_t i = 0; i < n; i++) {
    row_off[i + 1] = row_off[i] + (uint32_t)sets[item_set[i]].size();
    hash_off[i] = set_hash_off[item_set[i]];
  }
  const size_t total = row_off[n], per_row = kem ? 1 : 3;
  // scalars: per item secret | msg exponent; per row sx (encaps), or h*secret | sx_i | sx_i*h as three arrays (encrypt)
  const size_t k_bytes = (2 * n + per_row * total) * 32;
  uint8_t* h_k = eng.pinned(0, k_bytes + 32);
  uint8_t* h_sec = h_k;
  uint8_t* h_rho = h_sec + n * 32;
  uint8_t* h_row = h_rho + n * 32;
  std::vector<std::array<uint8_t, 12>> nonces(n);
  draw_items(rng, n, [&](Rng& r, size_t i) {
    const Fr secret = r.next_fr();
    const Fr* hs = hashes.data() + hash_off[i];
    const size_t rows = row_off[i + 1] - row_off[i];
    std::vector<Fr> sx{secret};
    for (size_t y = 0; y < rows; y++) {
      sx.push_back(r.next_fr());
      sx[0] = fr_sub(sx[0], sx[y]);                 // :197-200 as it is written
    }
    for (size_t y = 0; y < rows; y++) {
      uint8_t* at = h_row + 32 * (row_off[i] + y);
      if (kem) { memcpy(at, sx[y].l, 32); continue; }
      const Fr a = fr_mul(hs[y], secret), c = fr_mul(sx[y], hs[y]);
      memcpy(at, a.l, 32);
      memcpy(at + 32 * total, sx[y].l, 32);
      memcpy(at + 64 * total, c.l, 32);
    }
    const Fr rho = r.next_fr();
    memcpy(h_sec + 32 * i, secret.l, 32);
    memcpy(h_rho + 32 * i, rho.l, 32);
    if (!kem) r.fill(nonces[i].data(), 12);
  });
  tm.lap("draws + scalars");
  const EncTables* tb;
  {
    std::string key((const char*)pk.g1.data(), 64);
    key.append((const char*)pk.g2.data(), 128).append((const char*)pk.g1_b.data(), 64).append((const char*)pk.g1_b2.data(), 64).append((const char*)pk.h_b.data(), 64);
    key.append((const char*)pk.e_gg_alpha.data(), 384);
    tb = (const EncTables*)eng.aux("lsw_enc_tables", key, make_enc_tables, &pk, destroy_enc_tables, 2);
  }
  rhip_gt_table* gen = eng.gt_generator_table();
  rhip_ctx* cx = eng.ctx();
  DBuf d_k(&eng, k_bytes + 4), d_msg(&eng, n * 384), d_pw(&eng, n * 384), d_e1(&eng, n * 384), d_e2(&eng, n * 128);
  const auto heads = [&] {
    eng.check(rhip_upload_async(cx, d_k.ptr(), h_k, k_bytes), "upload");
    const rhip_fr* k_sec = d_k.as<rhip_fr>();
    const rhip_fr* k_rho = k_sec + n;
    eng.check(rhip_gt_table_pow(cx, gen, n, k_rho, d_msg.as<rhip_gt>()), "rhip_gt_table_pow");                 // rng.gen::<Gt>() = e(g1, g2)^rho
    eng.check(rhip_gt_table_pow(cx, tb->egg, n, k_sec, d_pw.as<rhip_gt>()), "rhip_gt_table_pow");
    eng.check(rhip_gt_mul(cx, n, d_pw.as<rhip_gt>(), d_msg.as<rhip_gt>(), d_e1.as<rhip_gt>()), "rhip_gt_mul");
    eng.check(rhip_g2_table_mul(cx, tb->g2, n, k_sec, d_e2.as<rhip_g2>()), "rhip_g2_table_mul");
  };
  RecordSources src(n);
  src.by_item(d_e1.ptr(), 384).by_item(d_e2.ptr(), 128);
  std::vector<DBuf> d_rows;
  if (kem) rows_fused(eng, tb, n, total, d_k, row_off, hash_off, hashes, heads, d_rows, src);
  else rows_by_tables(eng, tb, n, total, d_k, row_off, heads, d_rows, src);
  finish_encrypt(eng, &tm, layouts, n, item_set, src, d_msg.ptr(), (const uint8_t*)nonces.data(), pt_blob, pt_off, out_off, out_buf, key_buf);
  return true;
}
bool encrypt_packed(Engine& eng, Rng& rng, const KpAbePublicKey& pk, const std::vector<std::vector<std::string>>& sets, size_t n, const uint32_t* item_set,
                    const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  if (n && (!item_set || !pt_off || !out_off)) throw RabeError("lsw::encrypt_packed: null input");
  return encrypt_core(eng, rng, pk, sets, n, item_set, pt_blob, pt_off, out_buf, out_cap, out_off, nullptr);
}
// n key encapsulations (include/rabe_host.h: rabe_lsw_encaps_packed): record i is the KpAbeCiphertext header encrypt_packed writes for the same
// draws with a sealed part of length zero, key_buf + 32 i = SHA3-256(bytes(msg_i)).  Draw order per item: encrypt_packed's without the nonce.
// e1 and e2 keep their table calls.  No AES kernel.
bool encaps_packed(Engine& eng, Rng& rng, const KpAbePublicKey& pk, const std::vector<std::vector<std::string>>& sets, size_t n, const uint32_t* item_set,
                   uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  if (n && (!item_set || !key_buf)) throw RabeError("lsw::encaps_packed: null input");
  if (!out_off) throw RabeError("lsw::encaps_packed: null input");
  return encrypt_core(eng, rng, pk, sets, n, item_set, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}

// n calls of lsw::keygen (lsw/mod.rs:121-170).  Draw order per item: the gate coefficients of gen_shares_policy(alpha1), then one
// `random` per share (:136).  Record = KpAbeSecretKey: policy text, language, leaf count, per leaf (name, d1, d2, d3, d4, d5) with
// d3..d5 the identity for positive leaves and d1, d2 the identity for negative ones ("!x", :137-146: rhip_lsw_keygen_batch_signed).
bool keygen_packed(Engine& eng, Rng& rng, const KpAbePublicKey& pk, const KpAbeMasterKey& msk, const std::vector<std::string>& policies,
                   PolicyLanguage language, size_t n, const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm("lsw::keygen_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // master-key-derived scalars pass through the staging buffers
  ShareTrees st;
  std::vector<std::vector<std::string>> striped(policies.size());
  std::vector<size_t> fixed(policies.size());
  bool any_negative = false;
  for (size_t p = 0; p < policies.size(); p++) {
    const FlatPolicy& f = st.add(policies[p], language);
    any_negative = any_negative || f.has_negative;
    fixed[p] = 4 + policies[p].size() + 1 + 4;
    for (const auto& nc : f.leaf_name_col) { striped[p].push_back(remove_index(nc)); fixed[p] += 4 + striped[p].back().size() + 64 + 128 + 3 * 64; }
  }
  if (!record_offsets("lsw::keygen_packed", "item_policy", n, item_policy, policies.size(), fixed, nullptr, out_buf, out_cap, out_off)) return false;
  st.place(n, item_policy, 1);
  const std::vector<uint32_t>&leaf_off = st.leaf_off, &coef_off = st.coef_off;
  const size_t total = st.total, total_coef = st.total_coef;
  uint8_t* h_in = eng.pinned(0, 64 + (total_coef + total + 1) * 32);        // alpha1 | alpha2 | coefficients | randoms
  memcpy(h_in, msk.alpha1.l, 32);
  memcpy(h_in + 32, msk.alpha2.l, 32);
  uint8_t* h_coef = h_in + 64;
  uint8_t* h_rand = h_coef + total_coef * 32;
  draw_items(rng, n, [&](Rng& r, size_t i) {
    for (uint32_t c = coef_off[i]; c < coef_off[i + 1]; c++) { Fr a = r.next_fr(); memcpy(h_coef + 32 * (size_t)c, a.l, 32); }
    for (uint32_t y = leaf_off[i]; y < leaf_off[i + 1]; y++) { Fr a = r.next_fr(); memcpy(h_rand + 32 * (size_t)y, a.l, 32); }
  });
  tm.lap("policies + draws");
  rhip_ctx* cx = eng.ctx();
  std::string key((const char*)pk.g1.data(), 64);
  key.append((const char*)pk.g2.data(), 128);
  rhip_lsw_pk* dpk = (rhip_lsw_pk*)eng.aux("lsw_pk", key, make_pk, &pk, destroy_pk);
  st.upload(eng);
  DBuf d_in(&eng, 64 + (total_coef + total + 1) * 32), d_d1(&eng, total * 64 + 4), d_d2(&eng, total * 128 + 4);
  eng.check(rhip_upload_async(cx, d_in.ptr(), h_in, 64 + (total_coef + total) * 32), "upload");
  const rhip_fr* din = d_in.as<rhip_fr>();
  DBuf d_d345;
  if (!any_negative) {
    eng.check(rhip_lsw_keygen_batch(cx, dpk, n, total,
                                    st.d_leaf_off, st.d_tree_leaf, st.d_tree_gate, st.d_path_off, st.d_path_gate, st.d_path_x, st.d_gate_k, st.d_gate_coef_off, st.d_leaf_hash,
                                    din, din + 2, st.d_coef_off, din + 2 + total_coef, d_d1.as<rhip_g1>(), d_d2.as<rhip_g2>()), "rhip_lsw_keygen_batch");
  } else {                                   // negative leaves (lsw/mod.rs:137-146): d3, d4, d5 from the share, b and the master key's h_g1
    std::vector<uint32_t> leaf_neg;
    for (const auto& f : st.pols) for (const auto& nm : f->leaf_name) leaf_neg.push_back(is_negative(nm) ? 1u : 0u);
    DBuf d_neg = up32(eng, leaf_neg), d_b(&eng, msk.b.l, 32);
    d_d345 = DBuf(&eng, total * 192 + 4);
    rhip_g1* d3 = d_d345.as<rhip_g1>();
    eng.check(rhip_lsw_keygen_batch_signed(cx, dpk, n, total,
                                           st.d_leaf_off, st.d_tree_leaf, st.d_tree_gate, st.d_path_off, st.d_path_gate, st.d_path_x, st.d_gate_k, st.d_gate_coef_off,
                                           st.d_leaf_hash, d_neg.as<uint32_t>(), din, d_b.as<rhip_fr>(), (const rhip_g1*)msk.h_g1.data(), din + 2, st.d_coef_off,
                                           din + 2 + total_coef, d_d1.as<rhip_g1>(), d_d2.as<rhip_g2>(), d3, d3 + total, d3 + 2 * total), "rhip_lsw_keygen_batch_signed");
  }
  // the records are written on the device (records.h): policy text, leaf names and counts from the policy's template, the elements dropped
  // in (d3 .. d5 are the point at infinity -- zeros -- for a policy without negative leaves)
  std::vector<RecordLayout> layouts(policies.size());
  for (size_t p_ = 0; p_ < policies.size(); p_++) {
    RecordLayout& L = layouts[p_];
    policy_header(L, policies[p_], language);
    L.u32((uint32_t)striped[p_].size());
    for (size_t y = 0; y < striped[p_].size(); y++) {
      L.str(striped[p_][y]);
      L.src(0, (uint32_t)(64 * y), 64);
      L.src(1, (uint32_t)(128 * y), 128);
      if (any_negative) { L.src(2, (uint32_t)(64 * y), 64); L.src(3, (uint32_t)(64 * y), 64); L.src(4, (uint32_t)(64 * y), 64); }
      else { const uint8_t zeros[192] = {0}; L.lit(zeros, 192); }
    }
  }
  RecordSources src(n);
  src.by_rows(d_d1.ptr(), 64, leaf_off).by_rows(d_d2.ptr(), 128, leaf_off);
  if (any_negative) for (size_t k = 0; k < 3; k++) src.by_rows(d_d345.as<uint8_t>() + k * total * 64, 64, leaf_off);
  emit_plain_records(eng, layouts, n, item_policy, src, out_off, out_buf);
  tm.lap("device: shares, fixed-base multiplications, records; one copy out");
  return true;
}

// n calls of lsw::decrypt (lsw/mod.rs:228-290): n keys (a blob of KpAbeSecretKey records) against ONE ciphertext (BASELINE config 4:
// a pre-made ciphertext, a fresh key per item).  Per distinct key policy: calc_pruned over the ciphertext's attributes and, for every
// pruned (name, name_col), the FIRST key row and the FIRST ciphertext row named `name` and the FIRST coefficient named name_col
// (:249-263).  A pruned negative attribute (the reference's TODO branch, :265-278) fails the item here: the object API reproduces it.
bool decrypt_packed(Engine& eng, const KpAbeCiphertext& ct, size_t n, const uint8_t* sk_blob, size_t sk_len, const uint64_t* sk_off, bool trusted,
                    int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  StageTimer tm("lsw::decrypt_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!sk_off || (n && !sk_blob)) throw RabeError("lsw::decrypt_packed: null input");
  (void)check_offsets(n, sk_off, sk_len, errors);
  const size_t pt_each = ct.ct.size() >= 28 ? ct.ct.size() - 28 : 0;
  if (!pt_buf || pt_cap < n * pt_each) return false;
  BlobGather gather(eng, sk_blob, sk_len);          // the blob starts for the device now, beside the parsing below (records.h)
  std::vector<std::string> attr;
  for (const auto& a : ct.ej) attr.push_back(a.name);
  struct Plan {
    std::shared_ptr<const FlatPolicy> flat; std::string err; std::vector<std::string> std_names;
    struct E { std::string name; uint32_t ct_row; Fr c; uint32_t std_sk_row; };
    std::vector<E> ent;
  };
  PlanCache<Plan> plans;
  auto make_plan = [&](Plan& pl, const std::string& text, PolicyLanguage lang) {
    pl.flat = flat_policy(text, lang);
    for (const auto& nc : pl.flat->leaf_name_col) pl.std_names.push_back(remove_index(nc));
    PrunedList list;
    if (!calc_pruned(attr, pl.flat->tree, &list)) throw RabeError("Error in lsw/decrypt: attributes do not match policy.");
    for (const auto& a : list) {
      if (is_negative(a.first)) throw RabeError("lsw::decrypt_packed: a negative attribute is selected; rabe_lsw_decrypt reproduces the reference's branch");
      size_t cr = 0, sr = 0, co = 0;
      while (cr < ct.ej.size() && ct.ej[cr].name != a.first) cr++;
      while (sr < pl.std_names.size() && pl.std_names[sr] != a.first) sr++;
      while (co < pl.flat->leaf_name_col.size() && pl.flat->leaf_name_col[co] != a.second) co++;
      if (cr == ct.ej.size() || co == pl.flat->leaf_name_col.size()) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
      pl.ent.push_back({a.first, (uint32_t)cr, pl.flat->leaf_coeff[co], (uint32_t)sr});
    }
  };
  struct View { uint32_t rows; std::vector<const uint8_t*> d1, d2; std::shared_ptr<Plan> plan; std::vector<uint32_t> sk_row; bool standard; };
  std::vector<View> v(n);
  for_each_record(n, errors, [&](size_t i) {
    Cursor r{sk_blob + sk_off[i], sk_blob + sk_off[i + 1]};
    auto pol = r.str();
    const PolicyLanguage lang = *r.raw(1) ? PolicyLanguage::HumanPolicy : PolicyLanguage::JsonPolicy;
    const uint32_t rows = r.u32();
    if ((size_t)rows * 388 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
    v[i].rows = rows;
    v[i].d1.resize(rows);
    v[i].d2.resize(rows);
    std::vector<std::pair<const char*, uint32_t>> names(rows);
    for (uint32_t y = 0; y < rows; y++) { names[y] = r.str(); v[i].d1[y] = r.raw(64); v[i].d2[y] = r.raw(128); (void)r.raw(192); }
    auto pl = plans.get(pol.first, pol.second, lang, make_plan);
    if (!pl->err.empty()) throw RabeError(pl->err);
    v[i].plan = pl;
    bool standard = rows == pl->std_names.size();
    for (uint32_t y = 0; y < rows && standard; y++) standard = same(names[y], pl->std_names[y]);
    v[i].standard = standard;
    if (!standard) {
      for (const auto& e : pl->ent) {
        uint32_t y = 0;
        while (y < rows && !same(names[y], e.name)) y++;
        if (y == rows) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
        v[i].sk_row.push_back(y);
      }
    } else {
      for (const auto& e : pl->ent) if (e.std_sk_row >= rows) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
    }
  });
  tm.lap("parse + plan");
  Selection sel(1, 1);          // m entries: m + 1 pairs
  for (size_t i = 0; i < n; i++) {
    if (!(*errors)[i].empty()) continue;
    const View& w = v[i];
    sel.add(i, w.rows, w.plan.get(), w.standard, [&](auto emit) {
      const auto& ent = w.plan->ent;
      for (size_t e = 0; e < ent.size(); e++) emit(w.standard ? ent[e].std_sk_row : w.sk_row[e], ent[e].ct_row, ent[e].c);
    });
  }
  const std::vector<size_t>& live = sel.live;
  const std::vector<uint32_t>& leaf_off = sel.row_off;
  const size_t m_items = live.size();
  DBuf d_out(&eng, m_items * 384 + 4);
  WalkScope ws;
  if (m_items) {
    const size_t total = leaf_off[m_items];
    DBuf d_d1(&eng, total * 64 + 4);
    DBuf& d_d2 = ws.d_g2 = DBuf(&eng, total * 128 + 4);
    std::vector<uint64_t> dst_off(2 * m_items);
    for (size_t j = 0; j < m_items; j++) {
      const View& w = v[live[j]];
      const uint8_t* rec = sk_blob + sk_off[live[j]];
      dst_off[j] = 64ull * leaf_off[j]; dst_off[m_items + j] = 128ull * leaf_off[j];
      gather_record(gather, sk_off[live[j]], w.standard ? w.plan.get() : nullptr, [&](std::vector<RecordLayout::Part>& parts) {
        for (uint32_t y = 0; y < w.rows; y++) {
          parts.push_back({(uint32_t)(w.d1[y] - rec), 64, 0, 64 * y});
          parts.push_back({(uint32_t)(w.d2[y] - rec), 128, 1, 128 * y});
        }
      });
    }
    tm.lap("shapes");
    rhip_ctx* cx = eng.ctx();
    std::vector<uint8_t> e1j, e1rep(m_items * 384);
    for (const auto& a : ct.ej) e1j.insert(e1j.end(), a.e1.begin(), a.e1.end());
    for (size_t j = 0; j < m_items; j++) memcpy(e1rep.data() + 384 * j, ct.e1.data(), 384);

    DBuf d_leaf_off = up32(eng, leaf_off), d_pair_off = up32(eng, sel.pair_off),
        d_sel_start = up32(eng, sel.sel_start), d_sel_sk = up32(eng, sel.sel_rec), d_sel_ct = up32(eng, sel.sel_one), d_sel_z = up_bytes(eng, flatten_fr(sel.sel_z)),
        d_e1 = up_bytes(eng, e1rep), d_e2(&eng, ct.e2.data(), 128), d_e1j = up_bytes(eng, e1j);
    gather.run({d_d1.ptr(), d_d2.ptr()}, dst_off);
    std::string e2_key((const char*)ct.e2.data(), 128);         // the ciphertext's prepared e2 lines: kept across calls
    rhip_g2_lines* lines = (rhip_g2_lines*)eng.aux("lsw_e2_lines", e2_key, make_e2_lines, &e2_key, destroy_e2_lines, 4);
    if (!trusted) {
      ws.mc.reset(new MemberChecks(eng));
      ws.mc->add(1, d_d1.ptr(), total, d_leaf_off.as<uint32_t>(), m_items);
      // D2 of every selected key leaf is the walking argument of a pairing (e2 replays prepared lines): membership out of the decrypt's
      // own Miller loops, the stand-alone test for the leaves the selection left out (common.h: WalkedG2)
      ws.check_g2(eng, walk_checks() && lines, sel, total, d_leaf_off.as<uint32_t>());
    }
    if (ws.walked) ws.walked->arm();
    // one ciphertext for all keys: the scaled ciphertext rows are computed once per selection entry (keys that share a policy share them)
    int32_t rc = rhip_lsw_decrypt_batch_one_ct(cx, m_items, sel.max_pairs, sel.pair_off[m_items], sel.sel_rec.size(), d_pair_off.as<uint32_t>(),
                                               d_sel_start.as<uint32_t>(), d_sel_sk.as<uint32_t>(), d_sel_ct.as<uint32_t>(), d_sel_z.as<rhip_fr>(), d_e1.as<rhip_gt>(),
                                               d_e2.as<rhip_g2>(), d_e1j.as<rhip_g1>(), d_d1.as<rhip_g1>(), d_d2.as<rhip_g2>(), d_leaf_off.as<uint32_t>(),
                                               (const uint32_t*)nullptr, lines, d_out.as<rhip_gt>());
    eng.check(rc, "rhip_lsw_decrypt_batch");
    if (ws.mc) {
      ws.mc->collect();
      ws.fail(live, {0, ws.k_alone}, "deserialize: a key element is not a group member (FieldError::NotMember)", errors);
    }
  }
  // the ONE ciphertext's sealed data, opened under every key's Gt on the device (KDF + AES-GCM; the Gt never leaves HBM)
  DBuf d_sealed(&eng, ct.ct.data(), ct.ct.size());
  std::vector<uint64_t> sealed_off(m_items, 0);
  std::vector<uint32_t> sealed_len(m_items, (uint32_t)ct.ct.size());
  open_sealed_records(eng, n, live, d_out.ptr(), d_sealed.as<uint8_t>(), sealed_off, sealed_len, status, pt_buf, pt_off, errors);
  ws.retract(live, "deserialize: a key element is not a group member (FieldError::NotMember)", status, pt_buf, pt_off, errors);
  tm.lap(trusted ? "device: gather, pairings, open" : "device: gather, pairings, open; membership beside");
  return true;
}

namespace {
void* make_sk_d2_lines(Engine& eng, const void* arg) {          // arg: d2 of every key row (128 B each)
  const std::string& pts = *(const std::string*)arg;
  DBuf d(&eng, pts.data(), pts.size());
  rhip_g2_lines* lines = nullptr;
  eng.check(rhip_g2_lines_prepare(eng.ctx(), pts.size() / 128, d.as<rhip_g2>(), &lines), "rhip_g2_lines_prepare");
  return lines;
}
}  // namespace

// n calls of lsw::decrypt (lsw/mod.rs:228-290) with ONE key: n ciphertexts (a blob of KpAbeCiphertext records) from outside, the shape of a
// KP-ABE key holder.  The key's policy is parsed once; per distinct list of row names (the bytes of the names, in the record's order):
// calc_pruned over those names and, for every pruned (name, name_col), the FIRST key row and the FIRST ciphertext row named `name` and the
// FIRST coefficient named name_col (:249-263).  Records with the same list share their selection entries -- one selection GROUP of
// rhip_lsw_decrypt_batch_one_sk; the same names in another order, or a duplicated name, are another list with entries of its own.  A
// pruned negative attribute fails the item as in decrypt_packed.  Every D2 is the key's (prepared lines, kept per engine); the one walked
// G2 argument of an item is its own e2, whose walk gives its membership verdict.  The whole rows (e1, e2, e3 of every attribute) are gathered
// and checked as a decoder would; row r's E1 is element 3 r of that array.  pt_cap below the sealed lengths of the well-formed records:
// returns false with that size in pt_off[n].
// key_buf != nullptr is the key decapsulation (decaps_packed below): the same launch set up to the final Gt, then the KDF behind the verdict mask
// (records.h: derive_keys) instead of the open; pt_buf / pt_cap / pt_off are unused, the sealed part is skipped by its length field and never read.
static bool decrypt_one_sk_core(Engine& eng, const KpAbeSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                                int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors, uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? "lsw::decaps_packed" : "lsw::decrypt_one_sk_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || (!kem && !pt_off) || (n && !ct_blob)) throw RabeError("lsw::decrypt_one_sk_packed: null input");
  (void)check_offsets(n, ct_off, ct_len, errors);
  BlobGather gather(eng, ct_blob, ct_len);          // the blob starts for the device now, beside the parsing below (records.h)
  const std::shared_ptr<const FlatPolicy> flat = flat_policy(sk.policy.first, sk.policy.second);
  struct Plan {
    std::string err;
    struct E { uint32_t ct_row, sk_row; Fr c; };
    std::vector<E> ent;
  };
  PlanCache<Plan> plans;          // keyed on the bytes of the row names; the language is no part of that key
  auto make_plan = [&](Plan& pl, const std::string& names, PolicyLanguage) {          // names: (u32 length, bytes) per row, as the record holds them
    std::vector<std::string> attr;
    for (size_t at = 0; at < names.size();) {
      const uint32_t l = get_u32((const uint8_t*)names.data() + at);
      attr.push_back(names.substr(at + 4, l));
      at += 4 + (size_t)l;
    }
    PrunedList list;
    if (!calc_pruned(attr, flat->tree, &list)) throw RabeError("Error in lsw/decrypt: attributes do not match policy.");
    for (const auto& a : list) {
      if (is_negative(a.first)) throw RabeError("lsw::decrypt_packed: a negative attribute is selected; rabe_lsw_decrypt reproduces the reference's branch");
      size_t cr = 0, sr = 0, co = 0;
      while (cr < attr.size() && attr[cr] != a.first) cr++;
      while (sr < sk.dj.size() && sk.dj[sr].name != a.first) sr++;
      while (co < flat->leaf_name_col.size() && flat->leaf_name_col[co] != a.second) co++;
      if (cr == attr.size() || sr == sk.dj.size() || co == flat->leaf_name_col.size()) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
      pl.ent.push_back({(uint32_t)cr, (uint32_t)sr, flat->leaf_coeff[co]});
    }
    if (pl.ent.empty()) throw RabeError("Error in lsw/decrypt: attributes do not match policy.");
  };
  struct View { const uint8_t* e1; const uint8_t* e2; const uint8_t* first_row; uint32_t rows; std::shared_ptr<Plan> plan; };
  std::vector<View> v(n);
  std::vector<Sealed> sealed(n);
  std::vector<uint8_t> parsed(n, 0);
  for_each_record(n, errors, [&](size_t i) {
    Cursor r{ct_blob + ct_off[i], ct_blob + ct_off[i + 1]};
    v[i].e1 = r.raw(384);
    v[i].e2 = r.raw(128);
    const uint32_t rows = r.u32();
    if ((size_t)rows * 196 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
    v[i].rows = rows;
    v[i].first_row = r.p;
    std::string names;
    for (uint32_t y = 0; y < rows; y++) {
      const auto nm = r.str();
      names.append(nm.first - 4, (size_t)nm.second + 4);
      (void)r.raw(192);
    }
    sealed[i].len = r.u32();
    sealed[i].p = r.raw(sealed[i].len);
    parsed[i] = 1;
    auto pl = plans.get(names.data(), names.size(), PolicyLanguage::JsonPolicy, make_plan);
    if (!pl->err.empty()) throw RabeError(pl->err);
    v[i].plan = pl;
  });
  tm.lap("parse + plan");
  uint64_t need = 0;
  for (size_t i = 0; i < n; i++) if (parsed[i]) need += sealed[i].len;
  if (!kem && (!pt_buf || pt_cap < need)) { pt_off[n] = need; return false; }
  // every record is in the standard layout of ITS list of names; the records of one list are one selection group of the kernel
  Selection sel(1, 1);
  std::vector<uint32_t> attr_off{0}, group_off{0}, item_group;
  std::map<const Plan*, uint32_t> group_of;
  for (size_t i = 0; i < n; i++) {
    if (!(*errors)[i].empty()) continue;
    const Plan& pl = *v[i].plan;
    sel.add(i, v[i].rows, &pl, true, [&](auto emit) { for (const auto& e : pl.ent) emit(3 * e.ct_row, e.sk_row, e.c); });
    attr_off.push_back(3 * sel.row_off.back());
    if (sel.sel_start.back() == group_off.back()) {          // its entries were appended just now: a new group
      group_of[&pl] = (uint32_t)group_off.size() - 1;
      group_off.push_back((uint32_t)sel.sel_rec.size());
    }
    item_group.push_back(group_of[&pl]);
  }
  const std::vector<size_t>& live = sel.live;
  const std::vector<uint32_t>& row_off = sel.row_off;
  const size_t m_items = live.size();
  std::vector<uint64_t> sealed_off(m_items);
  std::vector<uint32_t> sealed_len(m_items);
  DBuf d_out(&eng, m_items * 384 + 4);
  WalkScope ws;
  if (m_items) {
    const size_t total = row_off[m_items];
    DBuf d_e1(&eng, m_items * 384), d_rows(&eng, total * 192 + 4);
    DBuf& d_e2 = ws.d_g2 = DBuf(&eng, m_items * 128);
    std::vector<uint64_t> dst_off(3 * m_items);
    for (size_t j = 0; j < m_items; j++) {
      const View& w = v[live[j]];
      const uint8_t* rec = ct_blob + ct_off[live[j]];
      sealed_off[j] = (uint64_t)(sealed[live[j]].p - ct_blob);
      sealed_len[j] = sealed[live[j]].len;
      dst_off[j] = 384ull * j; dst_off[m_items + j] = 128ull * j; dst_off[2 * m_items + j] = 192ull * row_off[j];
      // the same list of names: the same skeleton
      gather_record(gather, ct_off[live[j]], w.plan.get(), [&](std::vector<RecordLayout::Part>& parts) {
        parts.push_back({(uint32_t)(w.e1 - rec), 384, 0, 0});
        parts.push_back({(uint32_t)(w.e2 - rec), 128, 1, 0});
        Cursor r{w.first_row, ct_blob + ct_off[live[j] + 1]};
        for (uint32_t y = 0; y < w.rows; y++) { (void)r.str(); parts.push_back({(uint32_t)(r.raw(192) - rec), 192, 2, 192 * y}); }
      });
    }
    tm.lap("shapes");
    rhip_ctx* cx = eng.ctx();
    std::vector<uint8_t> kd1;
    std::string kd2;
    for (const auto& d : sk.dj) { kd1.insert(kd1.end(), d.d1.begin(), d.d1.end()); kd2.append((const char*)d.d2.data(), 128); }
    std::vector<uint32_t> e2_off;
    for (size_t j = 0; j <= m_items; j++) e2_off.push_back((uint32_t)j);
    DBuf d_row_off = up32(eng, row_off), d_attr_off = up32(eng, attr_off), d_pair_off = up32(eng, sel.pair_off), d_sel_start = up32(eng, sel.sel_start),
         d_sel_sk = up32(eng, sel.sel_one), d_sel_ct = up32(eng, sel.sel_rec), d_sel_z = up_bytes(eng, flatten_fr(sel.sel_z)), d_group_off = up32(eng, group_off),
         d_item_group = up32(eng, item_group), d_kd1 = up_bytes(eng, kd1), d_e2_off = up32(eng, e2_off);
    gather.run({d_e1.ptr(), d_e2.ptr(), d_rows.ptr()}, dst_off);
    // the key's prepared lines (every D2: 17 KB per row) are a function of the key alone: kept across calls
    rhip_g2_lines* lines = (rhip_g2_lines*)eng.aux("lsw_sk_d2_lines", kd2, make_sk_d2_lines, &kd2, destroy_e2_lines, 4);
    if (!trusted) {
      ws.mc.reset(new MemberChecks(eng));
      ws.mc->add(1, d_rows.ptr(), total * 3, d_row_off.as<uint32_t>(), m_items, 3);
      ws.mc->add(3, d_e1.ptr(), m_items);
      // e2 is the one walking argument of an item (the key's side replays prepared lines): membership out of the decrypt's own Miller
      // loop; an item whose last pair was skipped gets the stand-alone test (common.h: WalkedG2)
      if (walk_checks()) ws.walked.reset(new WalkedG2(eng, *ws.mc, d_e2.ptr(), m_items, d_e2_off.as<uint32_t>(), e2_off, 1));
      else { ws.k_alone = ws.mc->add_count(); ws.mc->add(2, d_e2.ptr(), m_items); }
    }
    if (ws.walked) ws.walked->arm();
    int32_t rc = rhip_lsw_decrypt_batch_one_sk(cx, m_items, sel.max_pairs, sel.pair_off[m_items], sel.sel_rec.size(), d_pair_off.as<uint32_t>(),
                                               d_sel_start.as<uint32_t>(), d_sel_sk.as<uint32_t>(), d_sel_ct.as<uint32_t>(), d_sel_z.as<rhip_fr>(), group_off.size() - 1,
                                               d_group_off.as<uint32_t>(), d_item_group.as<uint32_t>(), d_e1.as<rhip_gt>(), d_e2.as<rhip_g2>(),
                                               d_rows.as<rhip_g1>(), d_attr_off.as<uint32_t>(), d_kd1.as<rhip_g1>(), lines, d_out.as<rhip_gt>());
    eng.check(rc, "rhip_lsw_decrypt_batch_one_sk");
    if (ws.mc) {
      ws.mc->collect();
      ws.fail(live, {1}, "deserialize: e1 is not a member of Gt (FieldError::NotMember)", errors);
      ws.fail(live, {0}, "deserialize: a row element is not a point of G1 (FieldError::NotMember)", errors);
      ws.fail(live, {ws.k_alone}, "deserialize: e2 is not a member of G2 (FieldError::NotMember)", errors);
    }
  }
  if (kem) {
    ws.fail_walked(live, "deserialize: e2 is not a member of G2 (FieldError::NotMember)", errors);
    derive_keys(eng, n, live, d_out.ptr(), status, key_buf, *errors);
    tm.lap(trusted ? "device: gather, pairings, keys" : "device: gather, pairings, keys; membership beside");
    return true;
  }
  // KDF + AES-GCM open on the device: the decrypted Gt never leaves HBM; plaintext bytes come back in one copy
  open_sealed_records(eng, n, live, d_out.ptr(), gather.dev_blob(), sealed_off, sealed_len, status, pt_buf, pt_off, errors);
  ws.retract(live, "deserialize: e2 is not a member of G2 (FieldError::NotMember)", status, pt_buf, pt_off, errors);
  tm.lap(trusted ? "device: gather, pairings, open" : "device: gather, pairings, open; membership beside");
  return true;
}
bool decrypt_one_sk_packed(Engine& eng, const KpAbeSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                           int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  return decrypt_one_sk_core(eng, sk, n, ct_blob, ct_len, ct_off, trusted, status, pt_buf, pt_cap, pt_off, errors, nullptr);
}
// n key decapsulations under ONE key (include/rabe_host.h: rabe_lsw_decaps_packed): key_buf + 32 i = SHA3-256(bytes(Gt)) of what decrypt_gt
// returns for record i; input may be headers or full records
void decaps_packed(Engine& eng, const KpAbeSecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                   int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  if (n && (!status || !key_buf)) throw RabeError("lsw::decaps_packed: null input");
  uint8_t none = 0;          // n = 0: nothing is written
  decrypt_one_sk_core(eng, sk, n, ct_blob, ct_len, ct_off, trusted, status, nullptr, 0, nullptr, errors, key_buf ? key_buf : &none);
}
}  // namespace lsw

// ================================================================================================================= AW11
namespace aw11 {
namespace {
std::string upper(const std::string& s) {
  std::string o = s;
  for (auto& c : o) if (c >= 'a' && c <= 'z') c = (char)(c - 'a' + 'A');
  return o;
}
struct PkArg { const Aw11GlobalKey* gk; std::vector<const Aw11PkAttr*> attrs; };
void* make_pk(Engine& eng, const void* arg) {
  const PkArg& a = *(const PkArg*)arg;
  std::vector<uint8_t> egg, g2y;
  for (const auto* t : a.attrs) { egg.insert(egg.end(), t->egg_alpha.begin(), t->egg_alpha.end()); g2y.insert(g2y.end(), t->g2_y.begin(), t->g2_y.end()); }
  rhip_aw11_pk* d = nullptr;
  eng.check(rhip_aw11_pk_create(eng.ctx(), (const rhip_g1*)a.gk->g1.data(), (const rhip_g2*)a.gk->g2.data(), a.attrs.size(), (const rhip_gt*)egg.data(),
                                (const rhip_g2*)g2y.data(), &d), "rhip_aw11_pk_create");
  return d;
}
void destroy_pk(void* h) { rhip_aw11_pk_destroy((rhip_aw11_pk*)h); }
}  // namespace

// n calls of aw11::encrypt (aw11/mod.rs:241-289) under the same authority keys.  Draw order per item: s (:257), the gate
// coefficients of the s-shares then of the 0-shares (:259-260), msg (:262), one r_x per share (:267), the nonce.  Record =
// Aw11Ciphertext: policy, c_0, row count, per row (NAME_COL upper-cased, c1, c2, c3), sealed data.  A leaf whose attribute no
// authority key lists is silently dropped by the reference (:269-271); here it is an error (use rabe_aw11_encrypt for that case).
// key_buf != nullptr is the key encapsulation (encaps_packed below): no plaintexts, no nonce draw, records that end in the length field of an
// empty sealed part, and per item the content key SHA3-256(bytes(msg)) instead of a payload sealed under it.
static bool encrypt_core(Engine& eng, Rng& rng, const Aw11GlobalKey& gk, const std::vector<const Aw11PublicKey*>& pks, const std::vector<std::string>& policies,
                         PolicyLanguage language, size_t n, const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf,
                         size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? "aw11::encaps_packed" : "aw11::encrypt_packed");
  Engine::ArenaScope arena(eng);
  PkArg arg{&gk, {}};
  std::string key((const char*)gk.g1.data(), 64);
  key.append((const char*)gk.g2.data(), 128);
  for (const auto* pk : pks) for (const auto& t : pk->attr) { arg.attrs.push_back(&t); key.append((const char*)t.egg_alpha.data(), 384).append((const char*)t.g2_y.data(), 128); }
  if (arg.attrs.empty()) throw RabeError("aw11::encrypt_packed: no authority attributes");
  ShareTrees st;
  std::vector<uint32_t> leaf_attr;
  std::vector<size_t> fixed(policies.size());
  std::vector<RecordLayout> layouts(policies.size());          // records and sealing on the device (records.h); a record's size is its layout's
  for (size_t p = 0; p < policies.size(); p++) {
    const FlatPolicy& f = st.add(policies[p], language);
    (void)calculate_msp(f.tree);                           // built and unused in the reference (:253-255) -- but it must not panic
    RecordLayout& L = layouts[p];
    policy_header(L, policies[p], language);
    L.src(0, 0, 384);
    L.u32((uint32_t)f.leaf_name_col.size());
    for (uint32_t y = 0; y < f.leaf_name_col.size(); y++) {
      const std::string up = upper(f.leaf_name_col[y]), want = remove_index(up);
      size_t a = 0;
      while (a < arg.attrs.size() && arg.attrs[a]->name != want) a++;
      if (a == arg.attrs.size()) throw RabeError("aw11::encrypt_packed: attribute " + want + " is in no authority key (rabe_aw11_encrypt drops such rows like the reference)");
      leaf_attr.push_back((uint32_t)a);
      L.str(up);
      L.src(1, 384 * y, 384);
      L.src(2, 128 * y, 128);
      L.src(3, 128 * y, 128);
    }
    fixed[p] = close_ciphertext(L, kem);
  }
  if (!record_offsets("aw11::encrypt_packed", "item_policy", n, item_policy, policies.size(), fixed, kem ? nullptr : pt_off, out_buf, out_cap, out_off)) return false;
  st.place(n, item_policy, 2);          // the s-shares' coefficients, then the 0-shares'
  std::vector<uint32_t> n_coef(n);
  for (size_t i = 0; i < n; i++) n_coef[i] = st.pols[item_policy[i]]->n_coef;
  const std::vector<uint32_t>&row_off = st.leaf_off, &coef_off = st.coef_off;
  const size_t total = st.total, total_coef = st.total_coef;
  uint8_t* h_in = eng.pinned(0, (2 * n + total_coef + total + 1) * 32);      // s | msg exponent | coefficients | r_x
  uint8_t* h_s = h_in;
  uint8_t* h_rho = h_in + n * 32;
  uint8_t* h_coef = h_in + 2 * n * 32;
  uint8_t* h_rand = h_coef + total_coef * 32;
  std::vector<std::array<uint8_t, 12>> nonces(n);
  draw_items(rng, n, [&](Rng& r, size_t i) {
    Fr s = r.next_fr();
    memcpy(h_s + 32 * i, s.l, 32);
    for (uint32_t c = coef_off[i]; c < coef_off[i + 1]; c++) { Fr a = r.next_fr(); memcpy(h_coef + 32 * (size_t)c, a.l, 32); }
    Fr rho = r.next_fr();
    memcpy(h_rho + 32 * i, rho.l, 32);
    for (uint32_t y = row_off[i]; y < row_off[i + 1]; y++) { Fr a = r.next_fr(); memcpy(h_rand + 32 * (size_t)y, a.l, 32); }
    if (!kem) r.fill(nonces[i].data(), 12);
  });
  tm.lap("policies + draws");
  rhip_ctx* cx = eng.ctx();
  rhip_aw11_pk* dpk = (rhip_aw11_pk*)eng.aux("aw11_pk", key, make_pk, &arg, destroy_pk, 2);
  st.upload(eng);
  DBuf d_nc = up32(eng, n_coef), d_leaf_attr = up32(eng, leaf_attr), d_in(&eng, (2 * n + total_coef + total + 1) * 32), d_msg(&eng, n * 384), d_c0(&eng, n * 384),
       d_c1(&eng, total * 384 + 4), d_c2(&eng, total * 128 + 4), d_c3(&eng, total * 128 + 4);
  eng.check(rhip_upload_async(cx, d_in.ptr(), h_in, (2 * n + total_coef + total) * 32), "upload");
  const rhip_fr* din = d_in.as<rhip_fr>();
  eng.check(rhip_gt_table_pow(cx, eng.gt_generator_table(), n, din + n, d_msg.as<rhip_gt>()), "rhip_gt_table_pow");
  eng.check(rhip_aw11_encrypt_batch(cx, dpk, n, total,
                                    st.d_leaf_off, st.d_tree_leaf, st.d_tree_gate, d_nc.as<uint32_t>(), st.d_path_off, st.d_path_gate, st.d_path_x, st.d_gate_k, st.d_gate_coef_off,
                                    d_leaf_attr.as<uint32_t>(), din, din + 2 * n, st.d_coef_off, din + 2 * n + total_coef, d_msg.as<rhip_gt>(), d_c0.as<rhip_gt>(),
                                    d_c1.as<rhip_gt>(), d_c2.as<rhip_g2>(), d_c3.as<rhip_g2>()), "rhip_aw11_encrypt_batch");
  RecordSources src(n);
  src.by_item(d_c0.ptr(), 384).by_rows(d_c1.ptr(), 384, row_off).by_rows(d_c2.ptr(), 128, row_off).by_rows(d_c3.ptr(), 128, row_off);
  finish_encrypt(eng, &tm, layouts, n, item_policy, src, d_msg.ptr(), (const uint8_t*)nonces.data(), pt_blob, pt_off, out_off, out_buf, key_buf);
  return true;
}
bool encrypt_packed(Engine& eng, Rng& rng, const Aw11GlobalKey& gk, const std::vector<const Aw11PublicKey*>& pks, const std::vector<std::string>& policies,
                    PolicyLanguage language, size_t n, const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf,
                    size_t out_cap, uint64_t* out_off) {
  return encrypt_core(eng, rng, gk, pks, policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off, nullptr);
}
// n key encapsulations (include/rabe_host.h: rabe_aw11_encaps_packed): header i is the Aw11Ciphertext record encrypt_packed writes for the same
// draws with a sealed part of length zero, key_buf + 32 i = SHA3-256(bytes(msg_i)).  Draw order: encrypt_packed's minus the nonce.
bool encaps_packed(Engine& eng, Rng& rng, const Aw11GlobalKey& gk, const std::vector<const Aw11PublicKey*>& pks, const std::vector<std::string>& policies,
                   PolicyLanguage language, size_t n, const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  if (n && !key_buf) throw RabeError("aw11::encaps_packed: null input");
  if (!n) { out_off[0] = 0; return true; }
  return encrypt_core(eng, rng, gk, pks, policies, language, n, item_policy, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}

namespace {
void* make_g1_table(Engine& eng, const void* arg) {
  const G1& g1 = *(const G1*)arg;
  rhip_g1_table* t = nullptr;
  eng.check(rhip_g1_table_create(eng.ctx(), (const rhip_g1*)g1.data(), &t), "rhip_g1_table_create");
  const int32_t rc = rhip_g1_table_add_w16(eng.ctx(), t);
  if (rc) { rhip_g1_table_destroy(t); eng.check(rc, "rhip_g1_table_add_w16"); }
  return t;
}
void destroy_g1_table(void* h) { rhip_g1_table_destroy((rhip_g1_table*)h); }
}  // namespace
// n calls of aw11::keygen (aw11/mod.rs:165-231) by ONE authority: user i (gids[i]) gets the attribute list sets[item_set[i]].  No randomness:
// K_x = g1*alpha_x + H(gid)*y_x with H(gid) = g1*h(gid) is g1*(alpha_x + h(gid) y_x) -- one window-table launch for the whole batch.
// Record = Aw11SecretKey: gid, rows (upper-cased attribute name, K_x).  An attribute the authority does not own is the reference's
// unwrap panic (:213); an empty gid or list its RabeError.
bool keygen_packed(Engine& eng, const Aw11GlobalKey& gk, const Aw11MasterKey& msk, const std::vector<std::string>& gids,
                   const std::vector<std::vector<std::string>>& sets, size_t n, const uint32_t* item_set, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm("aw11::keygen_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // master-key-derived scalars pass through the staging buffers
  if (n && (!item_set || !out_off)) throw RabeError("aw11::keygen_packed: null input");
  if (gids.size() != n) throw RabeError("aw11::keygen_packed: one gid per item");
  std::vector<std::vector<const Aw11MkAttr*>> auth(sets.size());
  std::vector<std::vector<std::string>> names(sets.size());
  std::vector<size_t> fixed(sets.size());
  for (size_t s = 0; s < sets.size(); s++) {
    if (sets[s].empty()) throw RabeError("empty _attributes");
    fixed[s] = 4 + 4;
    for (const auto& a : sets[s]) {
      if (a.empty()) throw RabeError("empty _attributes");
      const Aw11MkAttr* hit = nullptr;
      for (const auto& m : msk.attr) if (m.name == a) { hit = &m; break; }
      if (!hit) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
      auth[s].push_back(hit);
      names[s].push_back(upper(hit->name));
      fixed[s] += 4 + names[s].back().size() + 64;
    }
  }
  // the first bad item decides the message: an empty gid counts up to the first index out of range, which record_offsets reports
  for (size_t i = 0; i < n && item_set[i] < sets.size(); i++) if (gids[i].empty()) throw RabeError("empty _name");
  if (!record_offsets("aw11::keygen_packed", "item_set", n, item_set, sets.size(), [&](size_t i) { return fixed[item_set[i]] + gids[i].size(); }, nullptr,
                      out_buf, out_cap, out_off)) return false;
  if (!n) return true;
  std::vector<size_t> row_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) row_off[i + 1] = row_off[i] + sets[item_set[i]].size();
  const size_t total = row_off[n];
  uint8_t* h_k = eng.pinned(0, total * 32 + 32);
  parallel_for(n, [&](size_t i) {
    const Fr hg = sha3_hash_fr(gids[i]);
    const auto& au = auth[item_set[i]];
    for (size_t y = 0; y < au.size(); y++) {
      const Fr k = fr_add(au[y]->alpha, fr_mul(hg, au[y]->y));
      memcpy(h_k + 32 * (row_off[i] + y), k.l, 32);
    }
  });
  tm.lap("scalars");
  const rhip_g1_table* tb = (const rhip_g1_table*)eng.aux("aw11_g1_table", std::string((const char*)gk.g1.data(), 64), make_g1_table, &gk.g1, destroy_g1_table, 4);
  rhip_ctx* cx = eng.ctx();
  DBuf d_k(&eng, total * 32 + 4), d_out(&eng, total * 64 + 4);
  eng.check(rhip_upload_async(cx, d_k.ptr(), h_k, total * 32), "upload");
  eng.check(rhip_g1_table_mul(cx, tb, total, d_k.as<rhip_fr>(), d_out.as<rhip_g1>()), "rhip_g1_table_mul");
  uint8_t* h_o = eng.pinned(1, total * 64 + 4);
  eng.check(rhip_download_async(cx, h_o, d_out.ptr(), total * 64), "download");
  eng.check(rhip_sync(cx), "rhip_sync");
  tm.lap("device + copies");
  parallel_for(n, [&](size_t i) {
    const auto& nm = names[item_set[i]];
    uint8_t* w = out_buf + out_off[i];
    put_u32(w, (uint32_t)gids[i].size()); w += 4;
    memcpy(w, gids[i].data(), gids[i].size()); w += gids[i].size();
    put_u32(w, (uint32_t)nm.size()); w += 4;
    for (size_t y = 0; y < nm.size(); y++) {
      put_u32(w, (uint32_t)nm[y].size()); w += 4;
      memcpy(w, nm[y].data(), nm[y].size()); w += nm[y].size();
      memcpy(w, h_o + 64 * (row_off[i] + y), 64); w += 64;
    }
  });
  tm.lap("assembly");
  return true;
}

// n calls of aw11::decrypt (aw11/mod.rs:298-366) with one key.  Per distinct policy: traverse_policy, calc_pruned, and per pruned
// (name, name_col) the FIRST key attribute named `name`, the FIRST ciphertext row named name_col (literal spelling, :325-333) and the
// FIRST coefficient named name_col.
// key_buf != nullptr is the key decapsulation (decaps_packed below): the same launch set up to the final Gt, then the KDF behind the verdict
// mask (records.h: derive_keys) instead of the open; pt_buf / pt_cap / pt_off are unused, the sealed part is skipped by its length field and never read.
static bool decrypt_core(Engine& eng, const Aw11GlobalKey& gk, const Aw11SecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off,
                         bool trusted, int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors, uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? "aw11::decaps_packed" : "aw11::decrypt_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || (n && !ct_blob)) throw RabeError("aw11::decrypt_packed: null input");
  const uint64_t span = check_offsets(n, ct_off, ct_len, errors);
  if (!kem && (!pt_buf || pt_cap < span)) return false;
  BlobGather gather(eng, ct_blob, ct_len);          // the blob starts for the device now, beside the parsing below (records.h)
  std::vector<std::string> str_attr;
  for (const auto& a : sk.attr) str_attr.push_back(a.first);
  struct Plan {
    std::shared_ptr<const FlatPolicy> flat; std::string err; std::vector<std::string> std_names;
    struct E { std::string name_col; uint32_t sk_row; Fr c; uint32_t std_ct_row; };
    std::vector<E> ent;
  };
  PlanCache<Plan> plans;
  auto make_plan = [&](Plan& pl, const std::string& text, PolicyLanguage lang) {
    pl.flat = flat_policy(text, lang);
    for (const auto& nc : pl.flat->leaf_name_col) pl.std_names.push_back(upper(nc));
    if (!traverse_policy(str_attr, pl.flat->tree)) throw RabeError("Error: attributes in sk do not match policy in ct.");
    PrunedList list;
    if (!calc_pruned(str_attr, pl.flat->tree, &list)) throw RabeError("Error in aw11/decrypt: attributes in sk do not match policy in ct.");
    for (const auto& cur : list) {
      size_t sr = 0, co = 0, cr = 0;
      while (sr < sk.attr.size() && sk.attr[sr].first != cur.first) sr++;
      while (co < pl.flat->leaf_name_col.size() && pl.flat->leaf_name_col[co] != cur.second) co++;
      while (cr < pl.std_names.size() && pl.std_names[cr] != cur.second) cr++;
      if (sr == sk.attr.size() || co == pl.flat->leaf_name_col.size()) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
      pl.ent.push_back({cur.second, (uint32_t)sr, pl.flat->leaf_coeff[co], (uint32_t)cr});
    }
  };
  struct View { const uint8_t* c0; uint32_t rows; std::vector<const uint8_t*> c1, c2, c3; std::shared_ptr<Plan> plan; std::vector<uint32_t> ct_row; bool standard; };
  std::vector<View> v(n);
  std::vector<Sealed> sealed(n);
  for_each_record(n, errors, [&](size_t i) {
    Cursor r{ct_blob + ct_off[i], ct_blob + ct_off[i + 1]};
    auto pol = r.str();
    const PolicyLanguage lang = *r.raw(1) ? PolicyLanguage::HumanPolicy : PolicyLanguage::JsonPolicy;
    v[i].c0 = r.raw(384);
    const uint32_t rows = r.u32();
    if ((size_t)rows * 644 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
    v[i].rows = rows;
    v[i].c1.resize(rows); v[i].c2.resize(rows); v[i].c3.resize(rows);
    std::vector<std::pair<const char*, uint32_t>> names(rows);
    for (uint32_t y = 0; y < rows; y++) { names[y] = r.str(); v[i].c1[y] = r.raw(384); v[i].c2[y] = r.raw(128); v[i].c3[y] = r.raw(128); }
    sealed[i].len = r.u32();
    sealed[i].p = r.raw(sealed[i].len);
    auto pl = plans.get(pol.first, pol.second, lang, make_plan);
    if (!pl->err.empty()) throw RabeError(pl->err);
    v[i].plan = pl;
    bool standard = rows == pl->std_names.size();
    for (uint32_t y = 0; y < rows && standard; y++) standard = same(names[y], pl->std_names[y]);
    v[i].standard = standard;
    for (size_t e = 0; e < pl->ent.size(); e++) {
      uint32_t y = standard ? pl->ent[e].std_ct_row : 0;
      if (!standard) while (y < rows && !same(names[y], pl->ent[e].name_col)) y++;
      if (y >= rows) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
      if (!standard) v[i].ct_row.push_back(y);
    }
  });
  tm.lap("parse + plan");
  Selection sel(1, 1);          // m entries: m + 1 pairs
  for (size_t i = 0; i < n; i++) {
    if (!(*errors)[i].empty()) continue;
    const View& w = v[i];
    sel.add(i, w.rows, w.plan.get(), w.standard, [&](auto emit) {
      const auto& ent = w.plan->ent;
      for (size_t e = 0; e < ent.size(); e++) emit(w.standard ? ent[e].std_ct_row : w.ct_row[e], ent[e].sk_row, ent[e].c);
    });
  }
  const std::vector<size_t>& live = sel.live;
  const std::vector<uint32_t>& row_off = sel.row_off;
  const size_t m_items = live.size();
  std::vector<uint64_t> sealed_off(m_items);
  std::vector<uint32_t> sealed_len(m_items);
  DBuf d_out(&eng, m_items * 384 + 4);
  WalkScope ws;
  if (m_items) {
    const size_t total = row_off[m_items];
    DBuf d_c0(&eng, m_items * 384), d_c1(&eng, total * 384 + 4), d_c3(&eng, total * 128 + 4);
    DBuf& d_c2 = ws.d_g2 = DBuf(&eng, total * 128 + 4);
    std::vector<uint64_t> dst_off(4 * m_items);
    for (size_t j = 0; j < m_items; j++) {
      const View& w = v[live[j]];
      const uint8_t* rec = ct_blob + ct_off[live[j]];
      sealed_off[j] = (uint64_t)(sealed[live[j]].p - ct_blob);
      sealed_len[j] = sealed[live[j]].len;
      dst_off[j] = 384ull * j; dst_off[m_items + j] = 384ull * row_off[j]; dst_off[2 * m_items + j] = dst_off[3 * m_items + j] = 128ull * row_off[j];
      gather_record(gather, ct_off[live[j]], w.standard ? w.plan.get() : nullptr, [&](std::vector<RecordLayout::Part>& parts) {
        parts.push_back({(uint32_t)(w.c0 - rec), 384, 0, 0});
        for (uint32_t y = 0; y < w.rows; y++) {
          parts.push_back({(uint32_t)(w.c1[y] - rec), 384, 1, 384 * y});
          parts.push_back({(uint32_t)(w.c2[y] - rec), 128, 2, 128 * y});
          parts.push_back({(uint32_t)(w.c3[y] - rec), 128, 3, 128 * y});
        }
      });
    }
    tm.lap("shapes");
    rhip_ctx* cx = eng.ctx();
    G1 hash = eng.g1_mul({gk.g1}, {sha3_hash_fr(sk.gid)})[0];            // H(gid) = g1 * h(gid), hashed inside decrypt (:318)
    std::vector<uint8_t> kk;
    for (const auto& a : sk.attr) kk.insert(kk.end(), a.second.begin(), a.second.end());
    std::vector<uint32_t> sk_attr_off{0, (uint32_t)sk.attr.size()}, sk_idx(m_items, 0);
    DBuf d_row_off = up32(eng, row_off),
        d_pair_off = up32(eng, sel.pair_off), d_sel_start = up32(eng, sel.sel_start), d_sel_ct = up32(eng, sel.sel_rec), d_sel_sk = up32(eng, sel.sel_one),
        d_sel_z = up_bytes(eng, flatten_fr(sel.sel_z)), d_hash(&eng, hash.data(), 64), d_kk = up_bytes(eng, kk), d_sk_attr_off = up32(eng, sk_attr_off),
        d_sk_idx = up32(eng, sk_idx);
    gather.run({d_c0.ptr(), d_c1.ptr(), d_c2.ptr(), d_c3.ptr()}, dst_off);
    if (!trusted) {
      ws.mc.reset(new MemberChecks(eng));
      ws.mc->add(3, d_c0.ptr(), m_items); ws.mc->add(3, d_c1.ptr(), total, d_row_off.as<uint32_t>(), m_items);
      ws.mc->add(2, d_c3.ptr(), total, d_row_off.as<uint32_t>(), m_items);          // C3 enters its pairing as a SUM: every term keeps the stand-alone test
      // C2 of every selected row is the walking argument of a pairing; one more argument walks per item (the sum of the C3 terms)
      ws.check_g2(eng, walk_checks(), sel, total, d_row_off.as<uint32_t>(), 1);
    }
    if (ws.walked) ws.walked->arm();
    // measured (docs/tried.md): the windowed leading factor loses to the NAF walk on this scheme's coefficients, so the decaps keeps the
    // decrypt's kernels; RABE_AW11_LEAD_W4=1 puts the windowed routine in its place (tools/bench_aw11_kem.py alternates the two)
    const bool lead_w4 = kem && getenv("RABE_AW11_LEAD_W4") != nullptr;
    int32_t rc = (lead_w4 ? rhip_aw11_decrypt_batch_w4 : rhip_aw11_decrypt_batch)(cx, m_items, sel.max_pairs, sel.pair_off[m_items], sel.sel_rec.size(), d_pair_off.as<uint32_t>(), d_sel_start.as<uint32_t>(),
                                         d_sel_ct.as<uint32_t>(), d_sel_sk.as<uint32_t>(), d_sel_z.as<rhip_fr>(), d_c0.as<rhip_gt>(), d_c1.as<rhip_gt>(),
                                         d_c2.as<rhip_g2>(), d_c3.as<rhip_g2>(), d_row_off.as<uint32_t>(), d_hash.as<rhip_g1>(), d_kk.as<rhip_g1>(),
                                         d_sk_attr_off.as<uint32_t>(), d_sk_idx.as<uint32_t>(), d_out.as<rhip_gt>());
    eng.check(rc, "rhip_aw11_decrypt_batch");
    if (ws.mc) {
      ws.mc->collect();
      ws.fail(live, {0, 1, 2, ws.k_alone}, "deserialize: a ciphertext element is not a group member (FieldError::NotMember)", errors);
    }
  }
  if (kem) {
    ws.fail_walked(live, "deserialize: a ciphertext element is not a group member (FieldError::NotMember)", errors);
    derive_keys(eng, n, live, d_out.ptr(), status, key_buf, *errors);
    tm.lap(trusted ? "device: gather, pairings, keys" : "device: gather, pairings, keys; membership beside");
    return true;
  }
  // KDF + AES-GCM open on the device: the decrypted Gt never leaves HBM; plaintext bytes come back in one copy
  open_sealed_records(eng, n, live, d_out.ptr(), gather.dev_blob(), sealed_off, sealed_len, status, pt_buf, pt_off, errors);
  ws.retract(live, "deserialize: a ciphertext element is not a group member (FieldError::NotMember)", status, pt_buf, pt_off, errors);
  tm.lap(trusted ? "device: gather, pairings, open" : "device: gather, pairings, open; membership beside");
  return true;
}
bool decrypt_packed(Engine& eng, const Aw11GlobalKey& gk, const Aw11SecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off,
                    bool trusted, int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  return decrypt_core(eng, gk, sk, n, ct_blob, ct_len, ct_off, trusted, status, pt_buf, pt_cap, pt_off, errors, nullptr);
}
// n key decapsulations under ONE key (include/rabe_host.h: rabe_aw11_decaps_packed): key_buf + 32 i = SHA3-256(bytes(Gt)) of what decrypt_gt
// returns for record i; input may be headers or full records
void decaps_packed(Engine& eng, const Aw11GlobalKey& gk, const Aw11SecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off,
                   bool trusted, int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  if (n && (!status || !key_buf)) throw RabeError("aw11::decaps_packed: null input");
  uint8_t none = 0;          // n = 0: nothing is written
  decrypt_core(eng, gk, sk, n, ct_blob, ct_len, ct_off, trusted, status, nullptr, 0, nullptr, errors, key_buf ? key_buf : &none);
}
}  // namespace aw11

// ================================================================================================================= GHW11
namespace ghw11 {
namespace {
void* make_tk_lines(Engine& eng, const void* arg) {          // arg: k_z | l_z | k_x[0] | k_x[1] ... (128 B each)
  const std::string& pts = *(const std::string*)arg;
  DBuf d(&eng, pts.data(), pts.size());
  rhip_g2_lines* lines = nullptr;
  eng.check(rhip_g2_lines_prepare(eng.ctx(), pts.size() / 128, d.as<rhip_g2>(), &lines), "rhip_g2_lines_prepare");
  return lines;
}
void destroy_tk_lines(void* h) { rhip_g2_lines_destroy((rhip_g2_lines*)h); }
void* make_pk(Engine& eng, const void* arg) {
  const Ghw11PublicKey& pk = *(const Ghw11PublicKey*)arg;
  rhip_ghw11_pk* d = nullptr;
  eng.check(rhip_ghw11_pk_create(eng.ctx(), (const rhip_g1*)pk.g1.data(), (const rhip_g1*)pk.g1_a.data(), (const rhip_gt*)pk.e_gg_alpha.data(), &d),
            "rhip_ghw11_pk_create");
  return d;
}
void destroy_pk(void* h) { rhip_ghw11_pk_destroy((rhip_ghw11_pk*)h); }
struct KeysArg { const Ghw11PublicKey* pk; const Ghw11MasterKey* msk; };
void* make_keys(Engine& eng, const void* arg) {
  const KeysArg& a = *(const KeysArg*)arg;
  rhip_ghw11_keys* d = nullptr;
  eng.check(rhip_ghw11_keys_create(eng.ctx(), (const rhip_g2*)a.pk->g2.data(), (const rhip_g2*)a.pk->g2_a.data(), (const rhip_g2*)a.msk->g2_alpha.data(), &d),
            "rhip_ghw11_keys_create");
  return d;
}
void destroy_keys(void* h) { rhip_ghw11_keys_destroy((rhip_ghw11_keys*)h); }
}  // namespace

// n calls of ghw11::encrypt (ghw11/mod.rs:189-225).  Draw order per item: secret (:199), msg (:200), the gate coefficients of
// gen_shares_policy (secretsharing/mod.rs:128-134), one t_i per share in share order (:206), the AES nonce (aes/mod.rs:17).  Like the
// reference (:195-197) and the object API, an empty plaintext is encrypted.  Record = Ghw11Ciphertext:
//   policy text, language, c, c1, row count, per row (name_col, C_i = g1_a * share - (g1 * h(name)) * t_i, D_i = g1 * t_i), sealed data.
// The rows are one lane each (k_ghw11_enc_rows): share, both walks of C on one accumulator, D, one inversion per block.
// key_buf != nullptr is the key encapsulation (encaps_packed below): no plaintexts, no nonce draw, records that end in the length field of an
// empty sealed part, and per item the content key SHA3-256(bytes(msg)) instead of a payload sealed under it.
static bool encrypt_core(Engine& eng, Rng& rng, const Ghw11PublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                         const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off,
                         uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? "ghw11::encaps_packed" : "ghw11::encrypt_packed");
  Engine::ArenaScope arena(eng);
  ShareTrees st;
  for (const auto& p : policies) st.add(p, language);
  const auto& pols = st.pols;
  // records and sealing on the device (records.h); a record's size is its layout's
  std::vector<size_t> fixed(policies.size());
  std::vector<RecordLayout> layouts(policies.size());
  for (size_t p_ = 0; p_ < policies.size(); p_++) {
    RecordLayout& L = layouts[p_];
    const FlatPolicy& f = *pols[p_];
    policy_header(L, policies[p_], language);
    L.src(0, 0, 384);
    L.src(1, 0, 64);
    L.u32((uint32_t)f.leaf_name.size());
    for (size_t y = 0; y < f.leaf_name.size(); y++) {
      L.str(f.leaf_name_col[y]);
      L.src(2, (uint32_t)(128 * y), 128);          // C | D, adjacent in the row kernel's output as in the record
    }
    fixed[p_] = close_ciphertext(L, kem);
  }
  if (!record_offsets("ghw11::encrypt_packed", "item_policy", n, item_policy, policies.size(), fixed, kem ? nullptr : pt_off, out_buf, out_cap, out_off)) return false;
  st.place(n, item_policy, 1);
  const std::vector<uint32_t>&leaf_off = st.leaf_off, &coef_off = st.coef_off;
  const size_t total = st.total, total_coef = st.total_coef;
  tm.lap("policies");
  const size_t in_bytes = (2 * n + total_coef + total) * 32;
  uint8_t* h_in = eng.pinned(0, in_bytes + 32);          // secret | msg exponent | coefficients | t per leaf row
  uint8_t* h_sec = h_in;
  uint8_t* h_rho = h_in + n * 32;
  uint8_t* h_coef = h_in + n * 64;
  uint8_t* h_t = h_coef + total_coef * 32;
  std::vector<std::array<uint8_t, 12>> nonces(n);
  draw_items(rng, n, [&](Rng& r, size_t i) {
    Fr s = r.next_fr(), rho = r.next_fr();
    memcpy(h_sec + 32 * i, s.l, 32);
    memcpy(h_rho + 32 * i, rho.l, 32);
    for (uint32_t c = coef_off[i]; c < coef_off[i + 1]; c++) { Fr a = r.next_fr(); memcpy(h_coef + 32 * (size_t)c, a.l, 32); }
    for (uint32_t y = leaf_off[i]; y < leaf_off[i + 1]; y++) { Fr t = r.next_fr(); memcpy(h_t + 32 * (size_t)y, t.l, 32); }
    if (!kem) r.fill(nonces[i].data(), 12);
  });
  tm.lap("draws");
  rhip_ctx* cx = eng.ctx();
  std::string key((const char*)pk.g1.data(), 64);
  key.append((const char*)pk.g1_a.data(), 64).append((const char*)pk.e_gg_alpha.data(), 384);
  rhip_ghw11_pk* dpk = (rhip_ghw11_pk*)eng.aux("ghw11_pk", key, make_pk, &pk, destroy_pk);
  st.upload(eng);
  DBuf d_in(&eng, in_bytes + 32), d_msg(&eng, n * 384), d_c(&eng, n * 384), d_c1(&eng, n * 64), d_cd(&eng, total * 128 + 4);
  eng.check(rhip_upload_async(cx, d_in.ptr(), h_in, in_bytes), "upload");
  const rhip_fr* dsec = d_in.as<rhip_fr>();
  eng.check(rhip_gt_table_pow(cx, eng.gt_generator_table(), n, dsec + n, d_msg.as<rhip_gt>()), "rhip_gt_table_pow");
  eng.check(rhip_ghw11_encrypt_batch(cx, dpk, n, total,
                                     st.d_leaf_off, st.d_tree_leaf, st.d_tree_gate, st.d_path_off, st.d_path_gate, st.d_path_x, st.d_gate_k, st.d_gate_coef_off, st.d_leaf_hash,
                                     dsec, dsec + 2 * n, st.d_coef_off, dsec + 2 * n + total_coef, d_msg.as<rhip_gt>(), d_c.as<rhip_gt>(), d_c1.as<rhip_g1>(),
                                     d_cd.as<rhip_g1>()), "rhip_ghw11_encrypt_batch");
  RecordSources src(n);
  src.by_item(d_c.ptr(), 384).by_item(d_c1.ptr(), 64).by_rows(d_cd.ptr(), 128, leaf_off);
  finish_encrypt(eng, &tm, layouts, n, item_policy, src, d_msg.ptr(), (const uint8_t*)nonces.data(), pt_blob, pt_off, out_off, out_buf, key_buf);
  return true;
}
bool encrypt_packed(Engine& eng, Rng& rng, const Ghw11PublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                    const uint32_t* item_policy, const uint8_t* pt_blob, const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  return encrypt_core(eng, rng, pk, policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off, nullptr);
}
// n key encapsulations: record i is the Ghw11Ciphertext header encrypt_packed writes for the same draws with an empty sealed part (its draws
// minus the AES nonce), key_buf + 32 i = SHA3-256(bytes(msg_i)).  Headers pass through transform_packed, which never reads the sealed part.
bool encaps_packed(Engine& eng, Rng& rng, const Ghw11PublicKey& pk, const std::vector<std::string>& policies, PolicyLanguage language, size_t n,
                   const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  if (n && !key_buf) throw RabeError("ghw11::encaps_packed: null input");
  if (!n) { out_off[0] = 0; return true; }
  return encrypt_core(eng, rng, pk, policies, language, n, item_policy, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}

// n calls of ghw11::decrypt_out (ghw11/mod.rs:297-305) under ONE retrieve key -- the client's half after transform_packed.  Item i: the
// Ghw11TransformCiphertext record c | t at tct + 768 i, and ciphertext record i of the blob, which carries the sealed data (the reference
// passes it beside the transformed ciphertext).  On the device: msg = c * t^(-z), KDF and AES-GCM open (records.h); only plaintexts come back.
// An item fails alone (status -1, empty plaintext slot): an all-zero tct record (transform_packed's failure mark), a malformed ciphertext
// record, c or t not in Gt (unless trusted), a tag that does not verify (a wrong rk, for one).
bool decrypt_out_packed(Engine& eng, const Ghw11RetrieveKey& rk, size_t n, const uint8_t* tct, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off,
                        bool trusted, int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  StageTimer tm("ghw11::decrypt_out_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || !pt_off || (n && (!ct_blob || !tct || !status))) throw RabeError("ghw11::decrypt_out_packed: null input");
  const uint64_t span = check_offsets(n, ct_off, ct_len, errors);
  if (!pt_buf || pt_cap < span) { pt_off[n] = span; return false; }
  std::vector<Sealed> sealed(n);
  for_each_record(n, errors, [&](size_t i) {
    const uint8_t* rec = tct + 768 * i;
    bool zero = true;
    for (size_t b = 0; b < 768 && zero; b++) zero = rec[b] == 0;
    if (zero) { (*errors)[i] = "ghw11::decrypt_out_packed: no transformed ciphertext for this item (transform failed)"; return; }
    Cursor r{ct_blob + ct_off[i], ct_blob + ct_off[i + 1]};
    (void)r.str();
    (void)r.raw(1 + 384 + 64);
    const uint32_t rows = r.u32();
    if ((size_t)rows * 132 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
    for (uint32_t y = 0; y < rows; y++) { (void)r.str(); (void)r.raw(128); }
    sealed[i].len = r.u32();
    sealed[i].p = r.raw(sealed[i].len);
    if (r.p != r.end) throw RabeError("deserialize: trailing bytes after the record");
  });
  tm.lap("parse");
  std::vector<size_t> live;
  for (size_t i = 0; i < n; i++) if ((*errors)[i].empty()) live.push_back(i);
  const size_t m = live.size();
  std::vector<uint64_t> sealed_off(m);
  std::vector<uint32_t> sealed_len(m);
  uint64_t sealed_total = 0;
  for (size_t j = 0; j < m; j++) { sealed_off[j] = sealed_total; sealed_len[j] = sealed[live[j]].len; sealed_total += sealed_len[j]; }
  DBuf d_msg(&eng, m * 384 + 4), d_sealed(&eng, sealed_total + 4);
  if (m) {
    eng.scrub_when_done();          // -z and the messages pass through the staging buffers
    rhip_ctx* cx = eng.ctx();
    // c | t of the live items, -z per item, the sealed parts: one staging block, three uploads
    uint8_t* h = eng.pinned(0, m * (768 + 32) + sealed_total + 4);
    uint8_t* h_c = h;
    uint8_t* h_t = h + m * 384;
    uint8_t* h_k = h + m * 768;
    uint8_t* h_s = h_k + m * 32;
    const Fr nz = fr_neg(rk.z);
    parallel_for(m, [&](size_t j) {
      const uint8_t* rec = tct + 768 * live[j];
      memcpy(h_c + 384 * j, rec, 384);
      memcpy(h_t + 384 * j, rec + 384, 384);
      memcpy(h_k + 32 * j, nz.l, 32);
      if (sealed_len[j]) memcpy(h_s + sealed_off[j], sealed[live[j]].p, sealed_len[j]);
    });
    tm.lap("pack");
    DBuf d_ct(&eng, m * 768), d_k(&eng, m * 32), d_p(&eng, m * 384);
    eng.check(rhip_upload_async(cx, d_ct.ptr(), h_c, m * 768), "upload");
    eng.check(rhip_upload_async(cx, d_k.ptr(), h_k, m * 32), "upload");
    if (sealed_total) eng.check(rhip_upload_async(cx, d_sealed.ptr(), h_s, sealed_total), "upload");
    const rhip_gt* d_c = d_ct.as<rhip_gt>();
    const rhip_gt* d_t = d_c + m;
    std::unique_ptr<MemberChecks> mc;
    if (!trusted) {
      mc.reset(new MemberChecks(eng));
      mc->add(3, d_c, m);
      mc->add(3, d_t, m);
    }
    eng.check(rhip_gt_pow(cx, m, d_t, d_k.as<rhip_fr>(), d_p.as<rhip_gt>()), "rhip_gt_pow");
    eng.check(rhip_gt_mul(cx, m, d_c, d_p.as<rhip_gt>(), d_msg.as<rhip_gt>()), "rhip_gt_mul");
    if (mc) {
      mc->collect();
      const auto &ok_c = mc->ok(0), &ok_t = mc->ok(1);
      for (size_t j = 0; j < m; j++) {
        if (!ok_c[j]) (*errors)[live[j]] = "deserialize: c is not a member of Gt (FieldError::NotMember)";
        else if (!ok_t[j]) (*errors)[live[j]] = "deserialize: t is not a member of Gt (FieldError::NotMember)";
      }
    }
  }
  // KDF + AES-GCM open on the device: the message never leaves HBM; plaintext bytes come back in one copy
  open_sealed_records(eng, n, live, d_msg.ptr(), d_sealed.as<uint8_t>(), sealed_off, sealed_len, status, pt_buf, pt_off, errors);
  tm.lap(trusted ? "device: powers, open" : "device: powers, open; membership beside");
  return true;
}

namespace {
// The host half that transform_packed and decrypt_packed share: bounds, the parse of every Ghw11Ciphertext record, the plan per distinct
// policy against the key's attribute names (a Ghw11SecretKey and a Ghw11TransformKey carry the same names in the same places -- only the G2
// elements whose lines are prepared differ), and the selection tables of rhip_ghw11_transform_batch, shared by the records in standard layout.
struct CtPlan {
  std::shared_ptr<const FlatPolicy> flat; std::string err;
  struct E { std::string name_col; uint32_t tk_attr; Fr w; uint32_t std_ct_row; };
  std::vector<E> ent;
};
struct CtView { const uint8_t* c; const uint8_t* c1; uint32_t rows; std::vector<const uint8_t*> ci, di; std::shared_ptr<CtPlan> plan;
                std::vector<uint32_t> ct_row; bool standard; };
struct CtBatch {
  std::vector<CtView> v;
  std::vector<Sealed> sealed;          // with_sealed: the data slice of every record whose fields decoded
  std::vector<uint8_t> parsed;         // with_sealed: 1 where the record's fields, the sealed slice included, decoded
  Selection sel{1, 2};                 // m entries: m + 2 pairs; sel_one = the key's attribute
  // with_sealed = false: the sealed data stays with the client (transform); true: it is kept, and the record has to end with it, as
  // decrypt_out_packed demands of the same record -- checked last, after everything the transform would have refused
  void parse(const std::vector<Ghw11Attribute>& key_attr, size_t n, const uint8_t* ct_blob, const uint64_t* ct_off, bool with_sealed,
             std::vector<std::string>* errors) {
    std::vector<std::vector<std::string>> one(1);
    for (const auto& a : key_attr) one[0].push_back(a.string);
    parse(one, nullptr, n, ct_blob, ct_off, with_sealed, errors);
  }
  // the records of a mixed queue: record i against the attribute names lists[item_list[i]] (item_list == nullptr: every record against
  // lists[0]).  One plan per pair of a list and a policy text -- a PlanCache per list, so keys that carry the same names share their plans.
  void parse(const std::vector<std::vector<std::string>>& lists, const uint32_t* item_list, size_t n, const uint8_t* ct_blob, const uint64_t* ct_off,
             bool with_sealed, std::vector<std::string>* errors);
  void select(size_t n, const std::vector<std::string>& errors);
};
void CtBatch::parse(const std::vector<std::vector<std::string>>& lists, const uint32_t* item_list, size_t n, const uint8_t* ct_blob, const uint64_t* ct_off,
                    bool with_sealed, std::vector<std::string>* errors) {
  std::unique_ptr<PlanCache<CtPlan>[]> plans(new PlanCache<CtPlan>[lists.size()]);
  auto make_plan = [](const std::vector<std::string>& attr, CtPlan& pl, const std::string& text, PolicyLanguage lang) {
    pl.flat = flat_policy(text, lang);
    const auto& names = pl.flat->leaf_name_col;
    if (!traverse_policy(attr, pl.flat->tree)) throw RabeError("Error: attributes in tk do not match policy in ct.");
    PrunedList list;
    if (!calc_pruned(attr, pl.flat->tree, &list)) throw RabeError("Error in Ghw11/decrypt: attributes in sk do not match policy in ct.");
    for (const auto& cur : list) {
      size_t a = 0, co = 0;
      while (a < attr.size() && attr[a] != cur.first) a++;
      while (co < names.size() && names[co] != cur.second) co++;
      if (a == attr.size() || co == names.size()) throw std::runtime_error("called `Option::unwrap()` on a `None` value");
      pl.ent.push_back({cur.second, (uint32_t)a, pl.flat->leaf_coeff[co], (uint32_t)co});
    }
  };
  v.resize(n);
  if (with_sealed) { sealed.resize(n); parsed.assign(n, 0); }
  for_each_record(n, errors, [&](size_t i) {
    Cursor r{ct_blob + ct_off[i], ct_blob + ct_off[i + 1]};
    auto pol = r.str();
    const PolicyLanguage lang = *r.raw(1) ? PolicyLanguage::HumanPolicy : PolicyLanguage::JsonPolicy;
    v[i].c = r.raw(384);
    v[i].c1 = r.raw(64);
    const uint32_t rows = r.u32();
    if ((size_t)rows * 132 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
    v[i].rows = rows;
    v[i].ci.resize(rows);
    v[i].di.resize(rows);
    std::vector<std::pair<const char*, uint32_t>> names(rows);
    for (uint32_t y = 0; y < rows; y++) { names[y] = r.str(); v[i].ci[y] = r.raw(64); v[i].di[y] = r.raw(64); }
    const uint32_t dl = r.u32();
    const uint8_t* data = r.raw(dl);                   // transform: the sealed data stays with the client (decrypt_out)
    if (with_sealed) { sealed[i].len = dl; sealed[i].p = data; parsed[i] = 1; }
    const std::vector<std::string>& attr = lists[item_list ? item_list[i] : 0];
    auto pl = plans[item_list ? item_list[i] : 0].get(pol.first, pol.second, lang,
                                                      [&](CtPlan& made, const std::string& text, PolicyLanguage l) { make_plan(attr, made, text, l); });
    if (!pl->err.empty()) throw RabeError(pl->err);
    v[i].plan = pl;
    const auto& std_names = pl->flat->leaf_name_col;
    bool standard = rows == std_names.size();
    for (uint32_t y = 0; y < rows && standard; y++) standard = same(names[y], std_names[y]);
    v[i].standard = standard;
    if (!standard) {
      for (const auto& e : pl->ent) {
        uint32_t y = 0;
        while (y < rows && !same(names[y], e.name_col)) y++;
        if (y == rows) throw RabeError("called `Option::unwrap()` on a `None` value");
        v[i].ct_row.push_back(y);
      }
    }
    if (with_sealed && r.p != r.end) throw RabeError("deserialize: trailing bytes after the record");
  });
}
void CtBatch::select(size_t n, const std::vector<std::string>& errors) {
  for (size_t i = 0; i < n; i++) {
    if (!errors[i].empty()) continue;
    const CtView& w = v[i];
    sel.add(i, w.rows, w.plan.get(), w.standard, [&](auto emit) {
      const auto& ent = w.plan->ent;
      for (size_t e = 0; e < ent.size(); e++) emit(w.standard ? ent[e].std_ct_row : w.ct_row[e], ent[e].tk_attr, ent[e].w);
    });
  }
}
// the prepared lines of a key's G2 elements in the order k, l, k_x[0], k_x[1], ... (kept per engine under `aux_name`, keyed on the bytes)
rhip_g2_lines* key_lines(Engine& eng, const char* aux_name, const G2& k, const G2& l, const std::vector<Ghw11Attribute>& attrs) {
  std::string key((const char*)k.data(), 128);
  key.append((const char*)l.data(), 128);
  for (const auto& a : attrs) key.append((const char*)a.k_x.data(), 128);
  return (rhip_g2_lines*)eng.aux(aux_name, key, make_tk_lines, &key, destroy_tk_lines, 4);
}
}  // namespace

// n calls of ghw11::transform (ghw11/mod.rs:227-295) under ONE transform key -- the outsourced half of a decryption, what a server
// holding users' transform keys runs.  Records in: Ghw11Ciphertext (policy, c, c1, rows (name, c_i, d_i), sealed
// data); records out: Ghw11TransformCiphertext = c | t, 768 bytes per item at out_buf + 768 i (zeros where status[i] = -1).
// Per distinct policy: traverse_policy, calc_pruned, and per pruned (name, name_col) the FIRST coefficient named name_col, the FIRST
// key attribute named `name`, the FIRST ciphertext row named name_col (:259-281); a missing one is the reference's unwrap panic.
// Every G2 argument is the key's: the batch replays prepared lines (kept across calls) and does no G2 arithmetic.
// The body is shared with transform_keyed (a mixed queue over a TkStore, below): `store` set = item i is served under key item_key[i] of the
// store -- its record is parsed against that key's attribute names, its pairs replay the store's lines from the key's base -- and `tk` is unused.
static bool transform_core(Engine& eng, const Ghw11TransformKey* tk, TkStore* store, const uint32_t* item_key, size_t n, const uint8_t* ct_blob, size_t ct_len,
                           const uint64_t* ct_off, bool trusted, int32_t* status, uint8_t* out_buf, size_t out_cap, std::vector<std::string>* errors) {
  StageTimer tm(store ? "ghw11::transform_keyed" : "ghw11::transform_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || (n && !ct_blob) || !status || (store && n && !item_key)) throw RabeError(store ? "ghw11::transform_keyed: null input" : "ghw11::transform_packed: null input");
  if (!out_buf || out_cap < n * 768) return false;
  (void)check_offsets(n, ct_off, ct_len, errors);
  CtBatch b;
  if (store) {
    std::vector<uint32_t> item_list(n, 0);
    for (size_t i = 0; i < n; i++) {
      const uint32_t u = item_key[i];
      if (u >= store->key_ok.size()) { if ((*errors)[i].empty()) (*errors)[i] = "ghw11::transform_keyed: item_key is out of the store's range"; }
      else if (!store->key_ok[u]) { if ((*errors)[i].empty()) (*errors)[i] = "ghw11::transform_keyed: the item's key failed when the store was built"; }
      else if (store->key_ok[u] != 1) { if ((*errors)[i].empty()) (*errors)[i] = "ghw11::transform_keyed: transform key revoked"; }          // never live: the device does not see the item
      else item_list[i] = store->key_list[u];
    }
    b.parse(store->lists, item_list.data(), n, ct_blob, ct_off, false, errors);
  } else {
    b.parse(tk->attr_key_z, n, ct_blob, ct_off, false, errors);
  }
  tm.lap("parse + plan");
  b.select(n, *errors);
  const Selection& sel = b.sel;
  const std::vector<size_t>& live = sel.live;
  const size_t m_items = live.size();
  uint8_t* h_out = nullptr;
  if (m_items) {
    const size_t total = sel.row_off[m_items];
    uint8_t* h_l = eng.pinned(1, total * 128 + 4);
    uint8_t* h_x = eng.pinned(2, m_items * (64 + 384 + 384));
    parallel_for(m_items, [&](size_t j) {
      const CtView& w = b.v[live[j]];
      memcpy(h_x + 64 * j, w.c1, 64);
      memcpy(h_x + m_items * 64 + 384 * j, w.c, 384);
      for (uint32_t y = 0; y < w.rows; y++) {
        memcpy(h_l + (size_t)(sel.row_off[j] + y) * 64, w.ci[y], 64);
        memcpy(h_l + total * 64 + (size_t)(sel.row_off[j] + y) * 64, w.di[y], 64);
      }
    });
    tm.lap("pack");
    rhip_ctx* cx = eng.ctx();
    rhip_g2_lines* lines = store ? store->lines_on(eng) : key_lines(eng, "ghw11_tk_lines", tk->k_z, tk->l_z, tk->attr_key_z);
    DBuf d_base;          // per live item: where its key's lines start in the store's handle
    if (store) {
      std::vector<uint32_t> line_base(m_items);
      for (size_t j = 0; j < m_items; j++) line_base[j] = store->key_base[item_key[live[j]]];
      d_base = up32(eng, line_base);
    }
    DBuf d_c1(&eng, m_items * 64), d_c(&eng, m_items * 384), d_ci(&eng, total * 64 + 4), d_di(&eng, total * 64 + 4), d_row_off = up32(eng, sel.row_off),
        d_pair_off = up32(eng, sel.pair_off), d_sel_start = up32(eng, sel.sel_start), d_sel_ct = up32(eng, sel.sel_rec), d_sel_tk = up32(eng, sel.sel_one),
        d_sel_w = up_bytes(eng, flatten_fr(sel.sel_z)), d_out(&eng, m_items * 384);
    eng.check(rhip_upload_async(cx, d_c1.ptr(), h_x, m_items * 64), "upload");
    eng.check(rhip_upload_async(cx, d_ci.ptr(), h_l, total * 64), "upload");
    eng.check(rhip_upload_async(cx, d_di.ptr(), h_l + total * 64, total * 64), "upload");
    std::unique_ptr<MemberChecks> mc;
    if (!trusted) {
      eng.check(rhip_upload_async(cx, d_c.ptr(), h_x + m_items * 64, m_items * 384), "upload");
      mc.reset(new MemberChecks(eng));
      mc->add(1, d_c1.ptr(), m_items); mc->add(1, d_ci.ptr(), total, d_row_off.as<uint32_t>(), m_items);
      mc->add(1, d_di.ptr(), total, d_row_off.as<uint32_t>(), m_items); mc->add(3, d_c.ptr(), m_items);
    }
    int32_t rc = store ? rhip_ghw11_transform_batch_keyed(cx, m_items, sel.max_pairs, sel.pair_off[m_items], sel.sel_rec.size(), d_pair_off.as<uint32_t>(),
                                                          d_sel_start.as<uint32_t>(), d_sel_ct.as<uint32_t>(), d_sel_tk.as<uint32_t>(), d_sel_w.as<rhip_fr>(),
                                                          d_c1.as<rhip_g1>(), d_ci.as<rhip_g1>(), d_di.as<rhip_g1>(), d_row_off.as<uint32_t>(),
                                                          d_base.as<uint32_t>(), nullptr, lines, d_out.as<rhip_gt>())          // a failed key's items are not live
                       : rhip_ghw11_transform_batch(cx, m_items, sel.max_pairs, sel.pair_off[m_items], sel.sel_rec.size(), d_pair_off.as<uint32_t>(), d_sel_start.as<uint32_t>(),
                                                    d_sel_ct.as<uint32_t>(), d_sel_tk.as<uint32_t>(), d_sel_w.as<rhip_fr>(), d_c1.as<rhip_g1>(), d_ci.as<rhip_g1>(),
                                                    d_di.as<rhip_g1>(), d_row_off.as<uint32_t>(), lines, d_out.as<rhip_gt>());
    h_out = h_x + m_items * 448;
    if (rc == RHIP_OK) rc = rhip_download_async(cx, h_out, d_out.ptr(), m_items * 384);
    if (rc == RHIP_OK) rc = rhip_sync(cx);
    eng.check(rc, store ? "rhip_ghw11_transform_batch_keyed" : "rhip_ghw11_transform_batch");
    if (mc) {
      mc->collect();
      const auto &ok_c1 = mc->ok(0), &ok_ci = mc->ok(1), &ok_di = mc->ok(2), &ok_c = mc->ok(3);
      for (size_t j = 0; j < m_items; j++)
        if (!ok_c1[j] || !ok_ci[j] || !ok_di[j] || !ok_c[j]) (*errors)[live[j]] = "deserialize: a ciphertext element is not a group member (FieldError::NotMember)";
    }
  }
  tm.lap(trusted ? "device + copies" : "device + copies, membership beside");
  std::vector<size_t> slot(n, (size_t)-1);
  for (size_t j = 0; j < m_items; j++) slot[live[j]] = j;
  parallel_for(n, [&](size_t i) {
    uint8_t* o = out_buf + 768 * i;
    if (!(*errors)[i].empty() || slot[i] == (size_t)-1) { memset(o, 0, 768); status[i] = -1; return; }
    memcpy(o, b.v[i].c, 384);
    memcpy(o + 384, h_out + 384 * slot[i], 384);
    status[i] = 0;
  });
  tm.lap("assembly");
  return true;
}
bool transform_packed(Engine& eng, const Ghw11TransformKey& tk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                      int32_t* status, uint8_t* out_buf, size_t out_cap, std::vector<std::string>* errors) {
  return transform_core(eng, &tk, nullptr, nullptr, n, ct_blob, ct_len, ct_off, trusted, status, out_buf, out_cap, errors);
}
bool transform_keyed(Engine& eng, TkStore& store, size_t n, const uint32_t* item_key, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off,
                     bool trusted, int32_t* status, uint8_t* out_buf, size_t out_cap, std::vector<std::string>* errors) {
  return transform_core(eng, nullptr, &store, item_key, n, ct_blob, ct_len, ct_off, trusted, status, out_buf, out_cap, errors);
}

// ---- the device-resident key store of a proxy (schemes.h: TkStore)
namespace {
void wipe(std::string& s) { if (!s.empty()) explicit_bzero(&s[0], s.size()); }
// the record of a transform key (k_z, l_z, u32 rows, rows of (name, k_x_z)) read with tkgen_packed's conventions: the names, or a throw
void tk_record_names(const uint8_t* rec, const uint8_t* end, std::vector<std::string>* names) {
  Cursor r{rec, end};
  (void)r.raw(256);
  const uint32_t cnt = r.u32();
  if ((size_t)cnt * 132 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
  for (uint32_t y = 0; y < cnt; y++) { auto nm = r.str(); names->emplace_back(nm.first, nm.second); (void)r.raw(128); }
  if (r.p != r.end) throw RabeError("deserialize: trailing bytes after the record");
}
}  // namespace
TkStore::TkStore(uint64_t capacity_blocks) : ranges(capacity_blocks) {
  if (capacity_blocks >= 0xFFFFFFF0ull) throw RabeError("ghw11::tk_store_create: more than 2^32 key elements in one store");
  points.assign((size_t)capacity_blocks * 128, '\0');
}
rhip_g2_lines* TkStore::lines_on(Engine& eng) {
  std::lock_guard<std::mutex> g(mu_);          // an engine's first use prepares; the others of a group wait their turn behind it
  return replica_locked(eng);
}
rhip_g2_lines* TkStore::replica_locked(Engine& eng) {
  for (const auto& r : replicas_) if (r.first == &eng) return r.second;
  if (points.empty()) throw RabeError("ghw11 key store: no key of the store is usable");
  rhip_g2_lines* lines = nullptr;
  eng.check(rhip_g2_lines_reserve(eng.ctx(), ranges.capacity(), &lines), "rhip_g2_lines_reserve");
  std::unique_ptr<rhip_g2_lines, void (*)(rhip_g2_lines*)> hold(lines, rhip_g2_lines_destroy);
  const auto used = ranges.used_ranges();          // the store as it is NOW; empty ranges stay reserved and empty
  if (!used.empty()) {
    DBuf d(&eng, points.data(), points.size());
    for (const auto& u : used)
      eng.check(rhip_g2_lines_prepare_range(eng.ctx(), lines, (size_t)u.first, (size_t)u.second, d.as<rhip_g2>() + u.first), "rhip_g2_lines_prepare_range");
  }
  replicas_.push_back({&eng, hold.release()});
  return lines;
}
void TkStore::stat(uint64_t out[4]) {
  std::lock_guard<std::mutex> g(mu_);
  out[0] = live_keys; out[1] = ranges.capacity(); out[2] = ranges.in_use(); out[3] = ranges.largest_free();
}
// scrubbed on every replica before anything on the host forgets where the key was
void TkStore::drop_key_locked(uint32_t id, uint8_t state) {
  const size_t first = key_base[id], n = key_blocks[id];
  for (const auto& r : replicas_) r.first->check(rhip_g2_lines_scrub_range(r.first->ctx(), r.second, first, n), "rhip_g2_lines_scrub_range");
  explicit_bzero(&points[first * 128], n * 128);
  if (key_ok[id] == 1) {
    live_keys--;
    const uint32_t li = key_list[id];
    if (--list_refs_[li] == 0) {
      list_of_.erase(lists[li]);
      for (auto& name : lists[li]) wipe(name);
      lists[li].clear();
      list_free_.push_back(li);
    }
  }
  if (!ranges.release(first, n)) throw RabeError("ghw11 key store: a key's range is not in use");
  key_ok[id] = state;
  key_list[id] = 0; key_base[id] = 0; key_blocks[id] = 0;
}
bool TkStore::add(Engine& eng, size_t n_keys, const uint8_t* tk_blob, size_t tk_len, const uint64_t* tk_off, bool trusted, bool index_ids, int32_t* key_status,
                  uint32_t* key_id, std::vector<std::string>* errors) {
  const char* who = index_ids ? "ghw11::tk_store_create" : "ghw11::tk_store_add";
  StageTimer tm(who);
  Engine::ArenaScope arena(eng);
  errors->assign(n_keys, "");
  if (!tk_off || (n_keys && (!tk_blob || !key_status || (!index_ids && !key_id)))) throw RabeError(std::string(who) + ": null input");
  (void)check_offsets(n_keys, tk_off, tk_len, errors);
  std::vector<std::vector<std::string>> names(n_keys);
  for_each_record(n_keys, errors, [&](size_t u) { tk_record_names(tk_blob + tk_off[u], tk_blob + tk_off[u + 1], &names[u]); });
  tm.lap("parse");
  std::lock_guard<std::mutex> g(mu_);
  if ((uint64_t)key_ok.size() + n_keys >= 0xFFFFFFFFull) throw RabeError(std::string(who) + ": the store has issued 2^32 key ids");
  if (ranges.capacity()) (void)replica_locked(eng);          // the caller's engine holds a replica of the store as it is before the call
  // every well-formed key gets its range, or none does
  std::vector<size_t> fresh;          // the well-formed records, in order
  std::vector<uint32_t> base, row_off{0};
  {
    host::BlockRanges trial = ranges;
    for (size_t u = 0; u < n_keys; u++) {
      if (!(*errors)[u].empty()) continue;
      uint64_t first = 0;
      if (!trial.alloc(2 + names[u].size(), &first)) return false;
      fresh.push_back(u);
      base.push_back((uint32_t)first);
      row_off.push_back(row_off.back() + (uint32_t)(2 + names[u].size()));          // below the capacity, which is below 2^32
    }
    ranges = trial;
  }
  const size_t m = fresh.size(), total = row_off[m];
  std::vector<uint8_t> member(m, 1);
  std::string elems(total * 128, '\0');          // the new elements only, key after key: what goes to the device
  parallel_for(m, [&](size_t j) {
    const uint8_t* rec = tk_blob + tk_off[fresh[j]];
    uint8_t* o = (uint8_t*)&elems[128 * (size_t)row_off[j]];
    memcpy(o, rec, 256);
    const uint8_t* q = rec + 260;
    for (uint32_t y = 2; y < row_off[j + 1] - row_off[j]; y++) {
      q += 4 + get_u32(q);
      memcpy(o + 128 * (size_t)y, q, 128);
      q += 128;
    }
    memcpy(&points[128 * (size_t)base[j]], o, 128 * (size_t)(row_off[j + 1] - row_off[j]));
  });
  tm.lap("pack");
  // from here on the ranges are taken: a key that does not make it gives its range back (drop), whatever the reason
  const size_t id0 = key_ok.size();
  std::vector<uint32_t> id_of(m);
  for (size_t j = 0; j < m; j++) {
    id_of[j] = (uint32_t)(index_ids ? id0 + fresh[j] : id0 + j);          // provisional for add: closed up below when a key fails membership
  }
  const size_t slots = index_ids ? n_keys : m;
  key_list.resize(id0 + slots, 0); key_base.resize(id0 + slots, 0); key_blocks.resize(id0 + slots, 0); key_ok.resize(id0 + slots, 0);
  for (size_t j = 0; j < m; j++) { key_base[id_of[j]] = base[j]; key_blocks[id_of[j]] = row_off[j + 1] - row_off[j]; key_ok[id_of[j]] = 3; }          // 3: placed, not yet judged
  auto undo = [&]() {          // an exception on the way: nothing of this call stays
    for (size_t j = 0; j < m; j++) if (key_ok[id_of[j]] == 3) { try { drop_key_locked(id_of[j], 0); } catch (...) {} }
    key_list.resize(id0); key_base.resize(id0); key_blocks.resize(id0); key_ok.resize(id0);
  };
  try {
    if (m) {
      // runs of keys whose ranges are adjacent, in the order of the upload: one rhip_g2_lines_prepare_range each
      struct Run { size_t first, n, src; };
      std::vector<Run> runs;
      for (size_t j = 0; j < m; j++) {
        const size_t n = row_off[j + 1] - row_off[j];
        if (!runs.empty() && runs.back().first + runs.back().n == base[j]) runs.back().n += n;
        else runs.push_back({base[j], n, row_off[j]});
      }
      DBuf d_p(&eng, elems.data(), elems.size()), d_row_off = up32(eng, row_off);
      std::unique_ptr<MemberChecks> mc;
      if (!trusted) {
        mc.reset(new MemberChecks(eng));
        mc->add(2, d_p.ptr(), total, d_row_off.as<uint32_t>(), m);
      }
      for (const auto& r : replicas_) {          // one replica at a time; each call returns when its range is complete
        Engine& e = *r.first;
        DBuf d_other;
        if (&e != &eng) d_other = DBuf(&e, elems.data(), elems.size());
        const rhip_g2* src = &e == &eng ? d_p.as<rhip_g2>() : d_other.as<rhip_g2>();
        for (const auto& run : runs) e.check(rhip_g2_lines_prepare_range(e.ctx(), r.second, run.first, run.n, src + run.src), "rhip_g2_lines_prepare_range");
      }
      if (mc) {
        mc->collect();
        const auto& ok = mc->ok(0);
        for (size_t j = 0; j < m; j++)
          if (!ok[j]) { member[j] = 0; (*errors)[fresh[j]] = "deserialize: a key element is not a member of G2 (FieldError::NotMember)"; }
      }
    }
    tm.lap(trusted ? "device: upload, lines" : "device: upload, lines; membership beside");
    // a non-member leaves nothing behind: its blocks are scrubbed and free again
    for (size_t j = 0; j < m; j++) if (!member[j]) drop_key_locked(id_of[j], 0);
  } catch (...) {
    undo();
    wipe(elems);
    throw;
  }
  wipe(elems);
  if (!index_ids) {          // ids count the successful additions: close the numbering up over the keys that failed membership
    size_t next = id0;
    for (size_t j = 0; j < m; j++) {
      if (!member[j]) continue;
      const uint32_t from = id_of[j], to = (uint32_t)next++;
      if (from != to) { key_base[to] = key_base[from]; key_blocks[to] = key_blocks[from]; }
      id_of[j] = to;
    }
    key_list.resize(next); key_base.resize(next); key_blocks.resize(next); key_ok.resize(next);
  }
  for (size_t u = 0; u < n_keys; u++) { key_status[u] = -1; if (key_id) key_id[u] = 0xFFFFFFFFu; }
  for (size_t j = 0; j < m; j++) {
    if (!member[j]) continue;
    const size_t u = fresh[j];
    auto it = list_of_.find(names[u]);
    if (it == list_of_.end()) {
      uint32_t li;
      if (!list_free_.empty()) { li = list_free_.back(); list_free_.pop_back(); lists[li] = names[u]; }
      else { li = (uint32_t)lists.size(); lists.push_back(names[u]); list_refs_.push_back(0); }
      it = list_of_.insert({names[u], li}).first;
    }
    list_refs_[it->second]++;
    key_list[id_of[j]] = it->second;
    key_ok[id_of[j]] = 1;
    live_keys++;
    key_status[u] = 0;
    if (key_id) key_id[u] = id_of[j];
  }
  return true;
}
void TkStore::revoke(Engine& eng, size_t n, const uint32_t* key_id, int32_t* status, std::vector<std::string>* errors) {
  (void)eng;
  errors->assign(n, "");
  if (n && (!key_id || !status)) throw RabeError("ghw11::tk_store_revoke: null input");
  std::lock_guard<std::mutex> g(mu_);
  for (size_t j = 0; j < n; j++) {
    const uint32_t id = key_id[j];
    status[j] = -1;
    if (id >= key_ok.size()) (*errors)[j] = "ghw11::tk_store_revoke: key id was never issued";
    else if (key_ok[id] == 0) (*errors)[j] = "ghw11::tk_store_revoke: the key failed when it was added";
    else if (key_ok[id] != 1) (*errors)[j] = "ghw11::tk_store_revoke: transform key revoked already";
    else { drop_key_locked(id, 2); status[j] = 0; }
  }
}
uint64_t TkStore::device_bytes() {
  std::lock_guard<std::mutex> g(mu_);
  uint64_t total = 0;
  for (const auto& r : replicas_) total += rhip_g2_lines_bytes(r.second);
  return total;
}
TkStore::~TkStore() {
  for (const auto& r : replicas_) r.first->release(r.second, destroy_tk_lines);
}
std::unique_ptr<TkStore> tk_store_open(Engine& eng, uint64_t capacity_blocks) {
  std::unique_ptr<TkStore> st(new TkStore(capacity_blocks));
  if (capacity_blocks) (void)st->lines_on(eng);          // reserved, every block empty
  return st;
}
// Records as tkgen_packed writes them, read with its conventions (TkStore::add).  The store is opened with exactly the blocks of the records
// that parse and filled by one add: a key that fails keeps its slot in the numbering (key_ok = 0), and the blocks of a key that failed the
// membership pass are free -- the only room such a store has until a key is revoked.
std::unique_ptr<TkStore> tk_store_create(Engine& eng, size_t n_keys, const uint8_t* tk_blob, size_t tk_len, const uint64_t* tk_off, bool trusted,
                                         int32_t* key_status, std::vector<std::string>* errors) {
  errors->assign(n_keys, "");
  if (!tk_off || (n_keys && (!tk_blob || !key_status))) throw RabeError("ghw11::tk_store_create: null input");
  std::vector<std::string> sizing(n_keys, "");
  (void)check_offsets(n_keys, tk_off, tk_len, &sizing);
  std::vector<uint64_t> blocks(n_keys, 0);
  for_each_record(n_keys, &sizing, [&](size_t u) {
    std::vector<std::string> names;
    tk_record_names(tk_blob + tk_off[u], tk_blob + tk_off[u + 1], &names);
    blocks[u] = 2 + names.size();
  });
  uint64_t capacity = 0;
  for (size_t u = 0; u < n_keys; u++) if (sizing[u].empty()) capacity += blocks[u];
  std::unique_ptr<TkStore> st = tk_store_open(eng, capacity);
  if (!st->add(eng, n_keys, tk_blob, tk_len, tk_off, trusted, true, key_status, nullptr, errors))
    throw RabeError("ghw11::tk_store_create: the keys do not fit the store sized for them");
  return st;
}
// ghw11 for a key holder WITHOUT a proxy: n ciphertext records under ONE secret key.  By definition the plaintexts of tkgen -> transform_packed
// -> decrypt_out_packed for any z: with k_z = k / z, l_z = l / z, k_x_z = k_x / z the transform returns t_z = t_1^(1/z), t_1 = its own
// expression on the secret key's elements (ghw11/mod.rs:252-282), and decrypt_out computes c * (t_z^z)^-1 = c * t_1^-1 (:302).  So z, the m + 2
// G2 multiplications of tkgen, the Gt power of decrypt_out, the second parse and the 768 bytes per item between the two calls are skipped:
// the records are parsed once (CtBatch, transform_packed's own half), the blob goes to the device once and the elements are gathered out of
// it there, rhip_ghw11_decrypt_batch replays the SECRET key's prepared lines (kept under "ghw11_sk_lines", keyed on the key's bytes) and
// leaves msg = c * t_1^-1 in HBM, and the KDF + AES-GCM open reads the sealed data from the device copy of the blob.  Only plaintexts and
// verdicts come back.  Failures stay with their item, with transform_packed's error texts (bounds, a malformed record, a policy the key does
// not satisfy, a missing row name, a non-member unless trusted) or decrypt_out_packed's (trailing bytes, a tag that does not verify): status
// -1 and an EMPTY plaintext slot.  pt_cap below the sealed lengths of the well-formed records: returns false with that size in pt_off[n].
// key_buf != nullptr is the key decapsulation (decaps_packed below): the same launch set up to msg = c * t_1^-1, then the KDF behind the verdict
// mask (records.h: derive_keys) instead of the open; pt_buf / pt_cap / pt_off are unused, the sealed part is skipped by its length field and never
// read -- headers (an empty sealed part) and full records give the same key.
static bool decrypt_core(Engine& eng, const Ghw11SecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                         int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors, uint8_t* key_buf) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? "ghw11::decaps_packed" : "ghw11::decrypt_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || (!kem && !pt_off) || (n && (!ct_blob || !status))) throw RabeError("ghw11::decrypt_packed: null input");
  if (!n) { if (!kem) pt_off[0] = 0; return true; }
  (void)check_offsets(n, ct_off, ct_len, errors);
  BlobGather gather(eng, ct_blob, ct_len);          // the blob starts for the device now, beside the parsing below (records.h)
  CtBatch b;
  b.parse(sk.attr_key, n, ct_blob, ct_off, true, errors);
  tm.lap("parse + plan");
  uint64_t need = 0;
  for (size_t i = 0; i < n; i++) if (b.parsed[i]) need += b.sealed[i].len;
  if (!kem && (!pt_buf || pt_cap < need)) { pt_off[n] = need; return false; }
  b.select(n, *errors);
  const Selection& sel = b.sel;
  const std::vector<size_t>& live = sel.live;
  const size_t m_items = live.size();
  std::vector<uint64_t> sealed_off(m_items);
  std::vector<uint32_t> sealed_len(m_items);
  DBuf d_msg(&eng, m_items * 384 + 4);
  if (m_items) {
    const size_t total = sel.row_off[m_items];
    DBuf d_c(&eng, m_items * 384), d_c1(&eng, m_items * 64), d_ci(&eng, total * 64 + 4), d_di(&eng, total * 64 + 4);
    std::vector<uint64_t> dst_off(4 * m_items);
    for (size_t j = 0; j < m_items; j++) {
      const CtView& w = b.v[live[j]];
      const uint8_t* rec = ct_blob + ct_off[live[j]];
      sealed_off[j] = (uint64_t)(b.sealed[live[j]].p - ct_blob);
      sealed_len[j] = b.sealed[live[j]].len;
      dst_off[j] = 384ull * j; dst_off[m_items + j] = 64ull * j; dst_off[2 * m_items + j] = dst_off[3 * m_items + j] = 64ull * sel.row_off[j];
      // the same policy text and row names: the same skeleton
      gather_record(gather, ct_off[live[j]], w.standard ? w.plan.get() : nullptr, [&](std::vector<RecordLayout::Part>& parts) {
        parts.push_back({(uint32_t)(w.c - rec), 384, 0, 0});
        parts.push_back({(uint32_t)(w.c1 - rec), 64, 1, 0});
        for (uint32_t y = 0; y < w.rows; y++) {
          parts.push_back({(uint32_t)(w.ci[y] - rec), 64, 2, 64 * y});
          parts.push_back({(uint32_t)(w.di[y] - rec), 64, 3, 64 * y});
        }
      });
    }
    tm.lap("shapes");
    rhip_ctx* cx = eng.ctx();
    rhip_g2_lines* lines = key_lines(eng, "ghw11_sk_lines", sk.k, sk.l, sk.attr_key);
    DBuf d_row_off = up32(eng, sel.row_off), d_pair_off = up32(eng, sel.pair_off), d_sel_start = up32(eng, sel.sel_start), d_sel_ct = up32(eng, sel.sel_rec),
         d_sel_sk = up32(eng, sel.sel_one), d_sel_w = up_bytes(eng, flatten_fr(sel.sel_z));
    gather.run({d_c.ptr(), d_c1.ptr(), d_ci.ptr(), d_di.ptr()}, dst_off);
    std::unique_ptr<MemberChecks> mc;
    if (!trusted) {          // transform_packed's checks; every G2 argument is the key's own, so no walk verdicts
      mc.reset(new MemberChecks(eng));
      mc->add(1, d_c1.ptr(), m_items); mc->add(1, d_ci.ptr(), total, d_row_off.as<uint32_t>(), m_items);
      mc->add(1, d_di.ptr(), total, d_row_off.as<uint32_t>(), m_items); mc->add(3, d_c.ptr(), m_items);
    }
    eng.check(rhip_ghw11_decrypt_batch(cx, m_items, sel.max_pairs, sel.pair_off[m_items], sel.sel_rec.size(), d_pair_off.as<uint32_t>(), d_sel_start.as<uint32_t>(),
                                       d_sel_ct.as<uint32_t>(), d_sel_sk.as<uint32_t>(), d_sel_w.as<rhip_fr>(), d_c1.as<rhip_g1>(), d_ci.as<rhip_g1>(),
                                       d_di.as<rhip_g1>(), d_row_off.as<uint32_t>(), lines, d_c.as<rhip_gt>(), d_msg.as<rhip_gt>()),
              "rhip_ghw11_decrypt_batch");
    if (mc) {
      mc->collect();
      const auto &ok_c1 = mc->ok(0), &ok_ci = mc->ok(1), &ok_di = mc->ok(2), &ok_c = mc->ok(3);
      for (size_t j = 0; j < m_items; j++)
        if (!ok_c1[j] || !ok_ci[j] || !ok_di[j] || !ok_c[j]) (*errors)[live[j]] = "deserialize: a ciphertext element is not a group member (FieldError::NotMember)";
    }
  }
  if (kem) {
    derive_keys(eng, n, live, d_msg.ptr(), status, key_buf, *errors);
    tm.lap(trusted ? "device: gather, pairings, keys" : "device: gather, pairings, keys; membership beside");
    return true;
  }
  // KDF + AES-GCM open on the device: msg never leaves HBM; plaintext bytes come back in one copy
  open_sealed_records(eng, n, live, d_msg.ptr(), gather.dev_blob(), sealed_off, sealed_len, status, pt_buf, pt_off, errors);
  // a tag that did not verify leaves a zeroed slot behind: close it up, so that every failed item has an empty one
  bool holes = false;
  for (size_t i = 0; i < n && !holes; i++) holes = status[i] != 0 && pt_off[i + 1] != pt_off[i];
  if (holes) {
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
      const uint64_t lo = pt_off[i], len = status[i] == 0 ? pt_off[i + 1] - lo : 0;
      if (len && at != lo) memmove(pt_buf + at, pt_buf + lo, (size_t)len);
      pt_off[i] = at;
      at += len;
    }
    pt_off[n] = at;
  }
  tm.lap(trusted ? "device: gather, pairings, open" : "device: gather, pairings, open; membership beside");
  return true;
}
bool decrypt_packed(Engine& eng, const Ghw11SecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                    int32_t* status, uint8_t* pt_buf, size_t pt_cap, uint64_t* pt_off, std::vector<std::string>* errors) {
  return decrypt_core(eng, sk, n, ct_blob, ct_len, ct_off, trusted, status, pt_buf, pt_cap, pt_off, errors, nullptr);
}
void decaps_packed(Engine& eng, const Ghw11SecretKey& sk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                   int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  if (n && (!status || !key_buf)) throw RabeError("ghw11::decaps_packed: null input");
  uint8_t none = 0;          // n = 0: nothing is written
  decrypt_core(eng, sk, n, ct_blob, ct_len, ct_off, trusted, status, nullptr, 0, nullptr, errors, key_buf ? key_buf : &none);
}
// n key decapsulations of a thin client under ONE retrieve key: item i is the Ghw11TransformCiphertext record c | t at tct + 768 i and nothing
// else -- no ciphertext blob.  key_buf + 32 i = SHA3-256(bytes(c_i * t_i^-z)), the KDF of what decrypt_out_gt returns.  On the device: ONE
// rhip_gt_pow_rows call over the live records (one item, every row under the one z uploaded once, mul = c, the inverse a conjugation), then
// the KDF behind the verdict mask.  An item fails alone (status -1, 32 zero bytes): an all-zero tct record (transform_packed's failure mark);
// c or t not in Gt unless trusted -- with trusted a non-member's key is unspecified (the power's split assumes the order-r subgroup).
void decaps_out_packed(Engine& eng, const Ghw11RetrieveKey& rk, size_t n, const uint8_t* tct, bool trusted, int32_t* status, uint8_t* key_buf,
                       std::vector<std::string>* errors) {
  StageTimer tm("ghw11::decaps_out_packed");
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (n && (!tct || !status || !key_buf)) throw RabeError("ghw11::decaps_out_packed: null input");
  if (!n) return;
  std::vector<size_t> live;
  for (size_t i = 0; i < n; i++) {
    const uint8_t* rec = tct + 768 * i;
    bool zero = true;
    for (size_t b = 0; b < 768 && zero; b++) zero = rec[b] == 0;
    if (zero) (*errors)[i] = "ghw11::decaps_out_packed: no transformed ciphertext for this item (transform failed)";
    else live.push_back(i);
  }
  const size_t m = live.size();
  if (m > 0xFFFFFFF0ull) throw RabeError("ghw11::decaps_out_packed: more than 2^32 records in one call");
  DBuf d_msg(&eng, m * 384 + 4);
  if (m) {
    eng.scrub_when_done();          // z and the messages pass through the staging buffers
    rhip_ctx* cx = eng.ctx();
    uint8_t* h = eng.pinned(0, m * 768 + 32);          // c of the live items | t of the live items | z
    uint8_t* h_t = h + m * 384;
    uint8_t* h_k = h + m * 768;
    parallel_for(m, [&](size_t j) {
      const uint8_t* rec = tct + 768 * live[j];
      memcpy(h + 384 * j, rec, 384);
      memcpy(h_t + 384 * j, rec + 384, 384);
    });
    memcpy(h_k, rk.z.l, 32);
    tm.lap("pack");
    const std::vector<uint32_t> row_off{0, (uint32_t)m};          // one item: every record under the one z
    DBuf d_ct(&eng, m * 768), d_k(&eng, 32), d_off = up32(eng, row_off);
    eng.check(rhip_upload_async(cx, d_ct.ptr(), h, m * 768), "upload");
    eng.check(rhip_upload_async(cx, d_k.ptr(), h_k, 32), "upload");
    const rhip_gt* d_c = d_ct.as<rhip_gt>();
    const rhip_gt* d_t = d_c + m;
    std::unique_ptr<MemberChecks> mc;
    if (!trusted) {
      mc.reset(new MemberChecks(eng));
      mc->add(3, d_c, m);
      mc->add(3, d_t, m);
    }
    eng.check(rhip_gt_pow_rows(cx, m, d_off.as<uint32_t>(), d_t, 1, d_k.as<rhip_fr>(), d_c, RHIP_GT_POW_INVERT, d_msg.as<rhip_gt>()), "rhip_gt_pow_rows");
    if (mc) {
      mc->collect();
      const auto &ok_c = mc->ok(0), &ok_t = mc->ok(1);
      for (size_t j = 0; j < m; j++) {
        if (!ok_c[j]) (*errors)[live[j]] = "deserialize: c is not a member of Gt (FieldError::NotMember)";
        else if (!ok_t[j]) (*errors)[live[j]] = "deserialize: t is not a member of Gt (FieldError::NotMember)";
      }
    }
  }
  derive_keys(eng, n, live, d_msg.ptr(), status, key_buf, *errors);
  tm.lap(trusted ? "device: power, keys" : "device: power, keys; membership beside");
}
// n calls of ghw11::keygen (ghw11/mod.rs:123-152) under one master key.  Item i gets the attribute list sets[item_set[i]]; draw order: one r
// per item, in item order (:130).  Record = Ghw11SecretKey: k, l, rows (name, k_x).  Every element is a fixed-base multiple (the hash to G2
// is g2 * h(x)): L = g2 * r, K = g2_alpha + g2_a * r, K_x = g2 * (h(x) r) -- one lane per element over the 16-bit window tables of g2 and
// g2_a (k_ghw11_keygen_rows; tables built once per key pair and kept), records written on the device from one template per list.
bool keygen_packed(Engine& eng, Rng& rng, const Ghw11PublicKey& pk, const Ghw11MasterKey& msk, const std::vector<std::vector<std::string>>& sets, size_t n,
                   const uint32_t* item_set, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm("ghw11::keygen_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // the keys' r pass through the staging buffers
  if (!out_off || (n && !item_set)) throw RabeError("ghw11::keygen_packed: null input");
  check_index("ghw11::keygen_packed", "item_set", n, item_set, sets.size());          // before the empty-list check, as ever
  std::vector<size_t> fixed(sets.size());
  std::vector<uint32_t> hash_off(sets.size() + 1, 0);
  std::vector<Fr> hashes;
  for (size_t s = 0; s < sets.size(); s++) {
    if (sets[s].empty()) throw RabeError("ghw11::keygen_packed: an empty attribute list (ghw11::keygen returns None for it)");
    fixed[s] = 128 + 128 + 4;
    for (const auto& a : sets[s]) { fixed[s] += 4 + a.size() + 128; hashes.push_back(sha3_hash_fr(a)); }
    hash_off[s + 1] = (uint32_t)hashes.size();
  }
  if (!record_offsets("ghw11::keygen_packed", "item_set", n, item_set, sets.size(), fixed, nullptr, out_buf, out_cap, out_off) && n) return false;
  if (!n) return true;
  std::vector<uint32_t> row_off(n + 1, 0), item_hash(n);
  for (size_t i = 0; i < n; i++) {
    const uint64_t next = (uint64_t)row_off[i] + 2 + sets[item_set[i]].size();
    if (next > 0xFFFFFFF0ull) throw RabeError("ghw11::keygen_packed: more than 2^32 key elements in one call");
    row_off[i + 1] = (uint32_t)next;
    item_hash[i] = hash_off[item_set[i]];
  }
  const size_t total = row_off[n];
  uint8_t* h_r = eng.pinned(0, n * 32 + 32);
  draw_items(rng, n, [&](Rng& r, size_t i) { const Fr ri = r.next_fr(); memcpy(h_r + 32 * i, ri.l, 32); });
  tm.lap("draws");
  std::string key((const char*)pk.g2.data(), 128);
  key.append((const char*)pk.g2_a.data(), 128).append((const char*)msk.g2_alpha.data(), 128);
  const KeysArg ka{&pk, &msk};
  const rhip_ghw11_keys* keys = (const rhip_ghw11_keys*)eng.aux("ghw11_keys", key, make_keys, &ka, destroy_keys, 4);
  rhip_ctx* cx = eng.ctx();
  DBuf d_r(&eng, n * 32), d_row_off = up32(eng, row_off), d_item_hash = up32(eng, item_hash), d_hash = up_bytes(eng, flatten_fr(hashes)),
      d_out(&eng, total * 128 + 4);
  eng.check(rhip_upload_async(cx, d_r.ptr(), h_r, n * 32), "upload");
  eng.check(rhip_ghw11_keygen_batch(cx, keys, n, total, d_row_off.as<uint32_t>(), d_item_hash.as<uint32_t>(), d_hash.as<rhip_fr>(), d_r.as<rhip_fr>(),
                                    d_out.as<rhip_g2>()), "rhip_ghw11_keygen_batch");
  std::vector<RecordLayout> layouts(sets.size());
  for (size_t s = 0; s < sets.size(); s++) {
    RecordLayout& L = layouts[s];
    L.src(0, 128, 128);          // k: row 1
    L.src(0, 0, 128);            // l: row 0
    L.u32((uint32_t)sets[s].size());
    for (size_t y = 0; y < sets[s].size(); y++) { L.str(sets[s][y]); L.src(0, (uint32_t)(128 * (2 + y)), 128); }
    if (L.bytes() != fixed[s]) throw RabeError("ghw11::keygen_packed: record layout and size disagree");
  }
  emit_plain_records(eng, layouts, n, item_set, RecordSources(n).by_rows(d_out.ptr(), 128, row_off), out_off, out_buf);
  tm.lap("device: rows, records; one copy out");
  return true;
}

// n calls of ghw11::tkgen (ghw11/mod.rs:156-178), one per Ghw11SecretKey record of an UNTRUSTED blob.  An item whose bounds are bad or whose
// record does not parse fails alone (status -1, empty tk slot, zero rk) and draws nothing; every other item draws one z, in item order --
// the membership verdicts of the decoded elements (unless trusted: canonical coordinates, on the twist, in the r-torsion; one batched pass
// beside the multiplication) arrive later and do not change what is drawn: a non-member fails its item like a malformed record, its z is
// spent.  z = 0 fails the call as tkgen's inverse().unwrap() does.  Every element times z^-1 is one row of rhip_g2_mul_rows (a four-way
// split of z^-1 per item, one joint chain per row); tk record = the sk record with every element replaced, rk = z.
bool tkgen_packed(Engine& eng, Rng& rng, size_t n, const uint8_t* sk_blob, size_t sk_len, const uint64_t* sk_off, bool trusted, int32_t* status,
                  uint8_t* tk_buf, size_t tk_cap, uint64_t* tk_off, uint8_t* rk_buf, std::vector<std::string>* errors) {
  StageTimer tm("ghw11::tkgen_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // z and z^-1 (the retrieve keys) pass through the staging buffers
  errors->assign(n, "");
  if (!sk_off || !tk_off || (n && (!sk_blob || !status || !rk_buf))) throw RabeError("ghw11::tkgen_packed: null input");
  (void)check_offsets(n, sk_off, sk_len, errors);
  std::vector<uint32_t> rows(n, 0);
  for_each_record(n, errors, [&](size_t i) {
    Cursor r{sk_blob + sk_off[i], sk_blob + sk_off[i + 1]};
    (void)r.raw(256);
    const uint32_t cnt = r.u32();
    if ((size_t)cnt * 132 > (size_t)(r.end - r.p)) throw RabeError("deserialize: truncated input");
    for (uint32_t y = 0; y < cnt; y++) { (void)r.str(); (void)r.raw(128); }
    if (r.p != r.end) throw RabeError("deserialize: trailing bytes after the record");
    rows[i] = 2 + cnt;
  });
  tm.lap("parse");
  std::vector<size_t> live;
  std::vector<uint32_t> row_off{0};
  uint64_t span = 0;
  for (size_t i = 0; i < n; i++) {
    if (!(*errors)[i].empty()) continue;
    live.push_back(i);
    const uint64_t next = (uint64_t)row_off.back() + rows[i];
    if (next > 0xFFFFFFF0ull) throw RabeError("ghw11::tkgen_packed: more than 2^32 key elements in one call");
    row_off.push_back((uint32_t)next);
    span += sk_off[i + 1] - sk_off[i];
  }
  if (span && (!tk_buf || tk_cap < span)) {          // nothing drawn
    tk_off[0] = 0;
    for (size_t i = 0; i < n; i++) tk_off[i + 1] = tk_off[i] + ((*errors)[i].empty() ? sk_off[i + 1] - sk_off[i] : 0);
    return false;
  }
  const size_t m = live.size(), total = row_off[m];
  std::vector<uint8_t> good(m, 1);
  uint8_t* h_out = nullptr;
  std::vector<Fr> zs(m);
  if (m) {
    uint8_t* h_k = eng.pinned(0, m * 32 + 32);
    {
      struct Turn { Rng& r; explicit Turn(Rng& x) : r(x) { r.begin_draws(); } ~Turn() { r.end_draws(); } } turn(rng);
      for (size_t j = 0; j < m; j++) {
        zs[j] = rng.next_fr();
        Fr zi;
        if (!fr_inv(zs[j], &zi)) throw std::runtime_error("called `Option::unwrap()` on a `None` value (Fr::inverse of zero)");
        memcpy(h_k + 32 * j, zi.l, 32);
      }
    }
    tm.lap("draws + inversions");
    uint8_t* h_p = eng.pinned(1, total * 128 + 4);
    parallel_for(m, [&](size_t j) {
      const uint8_t* rec = sk_blob + sk_off[live[j]];
      uint8_t* o = h_p + 128 * (size_t)row_off[j];
      memcpy(o, rec, 256);
      const uint8_t* q = rec + 260;
      for (uint32_t y = 2; y < rows[live[j]]; y++) {
        q += 4 + get_u32(q);
        memcpy(o + 128 * (size_t)y, q, 128);
        q += 128;
      }
    });
    tm.lap("pack");
    rhip_ctx* cx = eng.ctx();
    DBuf d_p(&eng, total * 128 + 4), d_k(&eng, m * 32), d_row_off = up32(eng, row_off), d_out(&eng, total * 128 + 4);
    eng.check(rhip_upload_async(cx, d_p.ptr(), h_p, total * 128), "upload");
    eng.check(rhip_upload_async(cx, d_k.ptr(), h_k, m * 32), "upload");
    std::unique_ptr<MemberChecks> mc;
    if (!trusted) {
      mc.reset(new MemberChecks(eng));
      mc->add(2, d_p.ptr(), total, d_row_off.as<uint32_t>(), m);
    }
    eng.check(rhip_g2_mul_rows(cx, total, d_row_off.as<uint32_t>(), d_p.as<rhip_g2>(), m, d_k.as<rhip_fr>(), d_out.as<rhip_g2>()), "rhip_g2_mul_rows");
    h_out = eng.pinned(2, total * 128 + 4);
    eng.check(rhip_download_async(cx, h_out, d_out.ptr(), total * 128), "download");
    eng.check(rhip_sync(cx), "rhip_sync");
    if (mc) {
      mc->collect();
      const auto& ok = mc->ok(0);
      for (size_t j = 0; j < m; j++)
        if (!ok[j]) { good[j] = 0; (*errors)[live[j]] = "deserialize: a key element is not a member of G2 (FieldError::NotMember)"; }
    }
    tm.lap(trusted ? "device + copies" : "device + copies, membership beside");
  }
  std::vector<size_t> slot(n, (size_t)-1);
  for (size_t j = 0; j < m; j++) if (good[j]) slot[live[j]] = j;
  tk_off[0] = 0;
  for (size_t i = 0; i < n; i++) tk_off[i + 1] = tk_off[i] + (slot[i] != (size_t)-1 ? sk_off[i + 1] - sk_off[i] : 0);
  parallel_for(n, [&](size_t i) {
    uint8_t* rk = rk_buf + 32 * i;
    if (slot[i] == (size_t)-1) { memset(rk, 0, 32); status[i] = -1; return; }
    const size_t j = slot[i];
    const uint8_t* rec = sk_blob + sk_off[i];
    const uint8_t* src = h_out + 128 * (size_t)row_off[j];
    uint8_t* w = tk_buf + tk_off[i];
    memcpy(w, src, 256);
    memcpy(w + 256, rec + 256, 4);
    size_t at = 260;
    for (uint32_t y = 2; y < rows[i]; y++) {
      const size_t name = 4 + (size_t)get_u32(rec + at);
      memcpy(w + at, rec + at, name);
      at += name;
      memcpy(w + at, src + 128 * (size_t)y, 128);
      at += 128;
    }
    memcpy(rk, zs[j].l, 32);
    status[i] = 0;
  });
  for (auto& z : zs) memset(z.l, 0, sizeof(z.l));
  tm.lap("assembly");
  return true;
}

// keygen_packed followed by tkgen_packed on its output, for an authority that issues both and so knows r and z: every transform-key element
// is a fixed-base multiple as well -- L_z = g2 * (r z^-1), K_z = g2_alpha * z^-1 + g2_a * (r z^-1), K_x_z = g2 * (h(x) r z^-1) -- so there
// is no parse, no membership pass and no variable-base chain, and z^-1, r z^-1 are formed on the device (rhip_ghw11_provision_batch).  Draw
// order: r_0 .. r_{n-1}, then z_0 .. z_{n-1} (the two calls back to back).  Both record sets are written on the device from one template per
// list (the transform key has the secret key's layout); rk = z.  sk_off == nullptr: no secret-key rows, the same draws.  z = 0 fails the call
// before any record is written.
bool provision_packed(Engine& eng, Rng& rng, const Ghw11PublicKey& pk, const Ghw11MasterKey& msk, const std::vector<std::vector<std::string>>& sets,
                      size_t n, const uint32_t* item_set, uint8_t* sk_buf, size_t sk_cap, uint64_t* sk_off, uint8_t* tk_buf, size_t tk_cap,
                      uint64_t* tk_off, uint8_t* rk_buf) {
  StageTimer tm("ghw11::provision_packed");
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // r, z, z^-1 and r z^-1 pass through the staging buffers
  const bool want_sk = sk_off != nullptr;
  if (!tk_off || (n && (!item_set || !rk_buf))) throw RabeError("ghw11::provision_packed: null input");
  check_index("ghw11::provision_packed", "item_set", n, item_set, sets.size());          // before the empty-list check, as ever
  std::vector<size_t> fixed(sets.size());
  std::vector<uint32_t> hash_off(sets.size() + 1, 0);
  std::vector<Fr> hashes;
  for (size_t s = 0; s < sets.size(); s++) {
    if (sets[s].empty()) throw RabeError("ghw11::provision_packed: an empty attribute list (ghw11::keygen returns None for it)");
    fixed[s] = 128 + 128 + 4;
    for (const auto& a : sets[s]) { fixed[s] += 4 + a.size() + 128; hashes.push_back(sha3_hash_fr(a)); }
    hash_off[s + 1] = (uint32_t)hashes.size();
  }
  const bool tk_fits = record_offsets("ghw11::provision_packed", "item_set", n, item_set, sets.size(), fixed, nullptr, tk_buf, tk_cap, tk_off);
  if (want_sk) memcpy(sk_off, tk_off, (n + 1) * sizeof(uint64_t));
  if (n && (!tk_fits || (want_sk && (!sk_buf || sk_cap < sk_off[n])))) return false;
  if (!n) return true;
  std::vector<uint32_t> row_off(n + 1, 0), item_hash(n);
  for (size_t i = 0; i < n; i++) {
    const uint64_t next = (uint64_t)row_off[i] + 2 + sets[item_set[i]].size();
    if (next > 0xFFFFFFF0ull) throw RabeError("ghw11::provision_packed: more than 2^32 key elements in one call");
    row_off[i + 1] = (uint32_t)next;
    item_hash[i] = hash_off[item_set[i]];
  }
  const size_t total = row_off[n];
  uint8_t* h_rz = eng.pinned(0, 2 * n * 32 + n * 4 + 32);          // r | z | the flags coming back
  draw_items(rng, 2 * n, [&](Rng& r, size_t i) { const Fr v = r.next_fr(); memcpy(h_rz + 32 * i, v.l, 32); });
  tm.lap("draws");
  std::string key((const char*)pk.g2.data(), 128);
  key.append((const char*)pk.g2_a.data(), 128).append((const char*)msk.g2_alpha.data(), 128);
  const KeysArg ka{&pk, &msk};
  rhip_ghw11_keys* keys = (rhip_ghw11_keys*)eng.aux("ghw11_keys", key, make_keys, &ka, destroy_keys, 4);
  rhip_ctx* cx = eng.ctx();
  DBuf d_rz(&eng, 2 * n * 32), d_flags(&eng, n * 4), d_row_off = up32(eng, row_off), d_item_hash = up32(eng, item_hash),
      d_hash = up_bytes(eng, flatten_fr(hashes)), d_tk(&eng, total * 128 + 4), d_sk;
  if (want_sk) d_sk = DBuf(&eng, total * 128 + 4);
  eng.check(rhip_upload_async(cx, d_rz.ptr(), h_rz, 2 * n * 32), "upload");
  eng.check(rhip_ghw11_provision_batch(cx, keys, n, total, d_row_off.as<uint32_t>(), d_item_hash.as<uint32_t>(), d_hash.as<rhip_fr>(), d_rz.as<rhip_fr>(),
                                       d_rz.as<rhip_fr>() + n, want_sk ? d_sk.as<rhip_g2>() : nullptr, d_tk.as<rhip_g2>(), d_flags.as<uint32_t>()),
            "rhip_ghw11_provision_batch");
  uint8_t* h_flags = h_rz + 2 * n * 32;
  eng.check(rhip_download_async(cx, h_flags, d_flags.ptr(), n * 4), "download");
  std::vector<RecordLayout> layouts(sets.size());
  for (size_t s = 0; s < sets.size(); s++) {
    RecordLayout& L = layouts[s];
    L.src(0, 128, 128);          // k / k_z: row 1
    L.src(0, 0, 128);            // l / l_z: row 0
    L.u32((uint32_t)sets[s].size());
    for (size_t y = 0; y < sets[s].size(); y++) { L.str(sets[s][y]); L.src(0, (uint32_t)(128 * (2 + y)), 128); }
    if (L.bytes() != fixed[s]) throw RabeError("ghw11::provision_packed: record layout and size disagree");
  }
  eng.check(rhip_sync(cx), "rhip_sync");
  for (size_t i = 0; i < n; i++)
    if (get_u32(h_flags + 4 * i)) throw std::runtime_error("called `Option::unwrap()` on a `None` value (Fr::inverse of zero)");
  tm.lap("device: scalars, rows");
  if (want_sk) emit_plain_records(eng, layouts, n, item_set, RecordSources(n).by_rows(d_sk.ptr(), 128, row_off), sk_off, sk_buf);
  emit_plain_records(eng, layouts, n, item_set, RecordSources(n).by_rows(d_tk.ptr(), 128, row_off), tk_off, tk_buf);
  memcpy(rk_buf, h_rz + n * 32, n * 32);
  tm.lap("device: records; copies out");
  return true;
}
}  // namespace ghw11

// ================================================================================================ BDABE / MKE08 packed encrypt
namespace dnfabe {
namespace {
// a public attribute key as the packed encrypt reads it: name, G1 and G2 parts, the n_gt Gt parts (BDABE a3; MKE08 gt1, gt2)
struct DnfKey { const std::string* attr; const G1* g1; const G2* g2; const Gt* gt[2]; };
struct DnfScheme {
  const char* timer;               // "bdabe::encrypt_packed"
  const char* kem_timer;           // "bdabe::encaps_packed"
  const char* terms_kind;          // cache of the term tables (Engine::aux)
  const char* not_dnf;             // the object API's message for a policy that is not in DNF
  uint32_t n_gt;
};
// Term tables are cached per engine under the BYTES of the attribute keys each term folds (the same policy text under other keys
// is another entry).  At most TERMS_CACHE policies of at most TERMS_CACHE_MAX_TERMS terms are kept: 16 x 32 x 7.8 MB = 4.0 GB of HBM
// for MKE08 (2.4 GB for BDABE) per engine.  A policy with more terms gets tables for the call alone.
const size_t TERMS_CACHE = 16, TERMS_CACHE_MAX_TERMS = 32;
struct TermsArg {
  const std::vector<DnfTerm>* terms;
  const std::vector<G1>* k1;
  const std::vector<G2>* k2;
  const std::vector<std::vector<Gt>>* kt;
};
void* make_terms(Engine& eng, const void* arg) {
  const TermsArg& a = *(const TermsArg*)arg;
  std::vector<G1> t1;
  std::vector<G2> t2;
  std::vector<std::vector<Gt>> tgt;
  fold_term_bases(eng, *a.terms, *a.k1, *a.k2, *a.kt, &t1, &t2, &tgt);
  std::vector<Gt> flat;
  for (const auto& v : tgt) flat.insert(flat.end(), v.begin(), v.end());
  rhip_dnf_terms* d = nullptr;
  eng.check(rhip_dnf_terms_create(eng.ctx(), t1.size(), (uint32_t)tgt.size(), (const rhip_g1*)t1.data(), (const rhip_g2*)t2.data(),
                                  (const rhip_gt*)flat.data(), &d), "rhip_dnf_terms_create");
  return d;
}
void destroy_terms(void* h) { rhip_dnf_terms_destroy((rhip_dnf_terms*)h); }
struct PkArg { const G1* p1; const G2* p2; };
void* make_pk(Engine& eng, const void* arg) {
  const PkArg& a = *(const PkArg*)arg;
  rhip_dnf_pk* d = nullptr;
  eng.check(rhip_dnf_pk_create(eng.ctx(), (const rhip_g1*)a.p1->data(), (const rhip_g2*)a.p2->data(), &d), "rhip_dnf_pk_create");
  return d;
}
void destroy_pk(void* h) { rhip_dnf_pk_destroy((rhip_dnf_pk*)h); }
// rethrown with the index of the policy it is about, in the class the object API throws
[[noreturn]] void policy_error(const std::exception& e, bool panic, size_t p) {
  const std::string msg = std::string(e.what()) + " (policies[" + std::to_string(p) + "])";
  if (panic) throw std::runtime_error(msg);
  throw RabeError(msg);
}

// n calls of bdabe::encrypt (bdabe/mod.rs:317-358) or mke08::encrypt (mke08/mod.rs:290-334).  Draw order per item: the message's
// a, b (BDABE msg = e(G1::one(), G2::one())^(ab); MKE08 also c: msg1 = gen^(ab), msg2 = gen^(abc), the data is sealed under
// msg1 msg2 = gen^(ab(1+c))), one r_j per DNF term in json_to_dnf's order, the AES nonce.  Per distinct policy: parse, DNF check,
// json_to_dnf against the names of attr_pks, term tables (folded once, cached).  One row per (item, term) on the device
// (rhip_dnf_encrypt_batch); records assembled and sealed there (records.h).
// key_buf != nullptr is the key encapsulation (include/rabe_host.h: rabe_{bdabe,mke08}_kem_encaps): no plaintexts, no nonce draw, records that end
// in the length field of an empty sealed part, and per item the content key SHA3-256(bytes(msg)) -- of the element the data would be sealed
// under -- instead of a payload.  Call-level errors keep encrypt_packed's texts.
bool encrypt_packed(Engine& eng, Rng& rng, const DnfScheme& sc, const G1& p1, const G2& p2, const std::vector<DnfKey>& keys,
                    const std::vector<std::string>& policies, PolicyLanguage language, size_t n, const uint32_t* item_policy, const uint8_t* pt_blob,
                    const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf = nullptr) {
  const bool kem = key_buf != nullptr;
  StageTimer tm(kem ? sc.kem_timer : sc.timer);
  Engine::ArenaScope arena(eng);
  Engine::Busy working(eng);          // a term set evicted by a later policy of this call lives until the call is done
  const size_t P = policies.size(), n_gt = sc.n_gt;
  std::vector<std::string> names;
  for (const auto& k : keys) names.push_back(*k.attr);
  std::vector<std::vector<DnfTerm>> terms(P);
  std::vector<RecordLayout> layouts(P);
  std::vector<size_t> fixed(P);
  for (size_t p = 0; p < P; p++) {
    PolicyNode tree;
    try {
      tree = parse_or_error(policies[p], language);
    } catch (const std::exception& e) {
      policy_error(e, false, p);
    }
    if (!policy_in_dnf(tree)) policy_error(RabeError(sc.not_dnf), false, p);
    if (!json_to_dnf(tree, names, &terms[p]))
      policy_error(std::runtime_error("called `Result::unwrap()` on an `Err` value: Error in json_to_dnf: could not parse policy as DNF"), true, p);
    // the record (host_abi.cpp: ser): policy, language, term count, per term its attribute names, Gt part(s), p1 r, p2 r, T1 r, T2 r
    RecordLayout& L = layouts[p];
    policy_header(L, policies[p], language);
    L.u32((uint32_t)terms[p].size());
    for (size_t y = 0; y < terms[p].size(); y++) {
      L.u32((uint32_t)terms[p][y].attrs.size());
      for (const auto& a : terms[p][y].attrs) L.str(a);
      L.src(0, (uint32_t)(384 * n_gt * y), (uint32_t)(384 * n_gt));
      L.src(1, (uint32_t)(128 * y), 64);
      L.src(2, (uint32_t)(256 * y), 128);
      L.src(1, (uint32_t)(128 * y + 64), 64);
      L.src(2, (uint32_t)(256 * y + 128), 128);
    }
    fixed[p] = close_ciphertext(L, kem);
  }
  if (!record_offsets(sc.timer, "item_policy", n, item_policy, P, fixed, kem ? nullptr : pt_off, out_buf, out_cap, out_off)) return false;
  if (!n) return true;
  std::vector<uint32_t> row_off(n + 1, 0);
  for (size_t i = 0; i < n; i++) row_off[i + 1] = row_off[i] + (uint32_t)terms[item_policy[i]].size();
  const size_t rows = row_off[n], n_exp = n_gt == 1 ? 1 : 3;
  tm.lap("policies");
  // the tables -- the key's (cached) and one term set per policy some item uses -- before the staging block is filled: a cache miss
  // runs the fold through the engine
  const PkArg pka{&p1, &p2};
  rhip_dnf_pk* dpk = (rhip_dnf_pk*)eng.aux("dnf_pk", std::string((const char*)p1.data(), 64) + std::string((const char*)p2.data(), 128), make_pk, &pka,
                                           destroy_pk);
  std::vector<G1> k1;
  std::vector<G2> k2;
  std::vector<std::vector<Gt>> kt(n_gt);
  for (const auto& k : keys) {
    k1.push_back(*k.g1);
    k2.push_back(*k.g2);
    for (size_t g = 0; g < n_gt; g++) kt[g].push_back(*k.gt[g]);
  }
  std::vector<bool> used(P, false);
  for (size_t i = 0; i < n; i++) used[item_policy[i]] = true;
  std::vector<const rhip_dnf_terms*> sets;
  std::vector<std::unique_ptr<rhip_dnf_terms, void (*)(rhip_dnf_terms*)>> own;
  std::vector<uint32_t> term_base(P, 0);
  uint32_t n_terms = 0;
  for (size_t p = 0; p < P; p++) {
    if (!used[p] || terms[p].empty()) continue;
    const TermsArg ta{&terms[p], &k1, &k2, &kt};
    const rhip_dnf_terms* s;
    if (terms[p].size() <= TERMS_CACHE_MAX_TERMS) {
      std::string key;
      for (const auto& t : terms[p]) {
        key.append(4, '\0');
        put_u32((uint8_t*)&key[key.size() - 4], (uint32_t)t.keys.size());
        for (size_t k : t.keys) {
          key.append((const char*)k1[k].data(), 64).append((const char*)k2[k].data(), 128);
          for (size_t g = 0; g < n_gt; g++) key.append((const char*)kt[g][k].data(), 384);
        }
      }
      s = (const rhip_dnf_terms*)eng.aux(sc.terms_kind, key, make_terms, &ta, destroy_terms, TERMS_CACHE);
    } else {
      own.emplace_back((rhip_dnf_terms*)make_terms(eng, &ta), rhip_dnf_terms_destroy);
      s = own.back().get();
    }
    sets.push_back(s);
    term_base[p] = n_terms;
    n_terms += (uint32_t)terms[p].size();
  }
  tm.lap("tables");
  const size_t in_bytes = (n_exp * n + rows) * 32;
  uint8_t* h_in = eng.pinned(0, in_bytes + 32);          // message exponents [n_exp][n] | r per row
  uint8_t* h_r = h_in + n_exp * n * 32;
  std::vector<std::array<uint8_t, 12>> nonces(n);
  draw_items(rng, n, [&](Rng& r, size_t i) {
    const Fr a = r.next_fr(), b = r.next_fr(), ab = fr_mul(a, b);
    memcpy(h_in + 32 * i, ab.l, 32);
    if (n_gt == 2) {
      const Fr c = r.next_fr(), abc = fr_mul(ab, c), msg = fr_mul(ab, fr_add(fr_one(), c));
      memcpy(h_in + 32 * (n + i), abc.l, 32);
      memcpy(h_in + 32 * (2 * n + i), msg.l, 32);
    }
    for (uint32_t y = row_off[i]; y < row_off[i + 1]; y++) { const Fr rj = r.next_fr(); memcpy(h_r + 32 * (size_t)y, rj.l, 32); }
    if (!kem) r.fill(nonces[i].data(), 12);
  });
  tm.lap("draws");
  rhip_ctx* cx = eng.ctx();
  DBuf d_in(&eng, in_bytes + 32), d_msg(&eng, n_exp * n * 384);
  eng.check(rhip_upload_async(cx, d_in.ptr(), h_in, in_bytes), "upload");
  eng.check(rhip_gt_table_pow(cx, eng.gt_generator_table(), n_exp * n, d_in.as<rhip_fr>(), d_msg.as<rhip_gt>()), "rhip_gt_table_pow");
  std::vector<uint32_t> row_term(rows), row_item(rows);
  for (size_t i = 0; i < n; i++)
    for (uint32_t y = row_off[i]; y < row_off[i + 1]; y++) { row_term[y] = term_base[item_policy[i]] + (y - row_off[i]); row_item[y] = (uint32_t)i; }
  DBuf d_rt = up32(eng, row_term), d_ri = up32(eng, row_item), d_gt(&eng, rows * 384 * n_gt + 4), d_g1(&eng, rows * 128 + 4), d_g2(&eng, rows * 256 + 4);
  eng.check(rhip_dnf_encrypt_batch(cx, dpk, sets.size(), sets.data(), n, rows, d_rt.as<uint32_t>(), d_ri.as<uint32_t>(), d_in.as<rhip_fr>() + n_exp * n,
                                   d_msg.as<rhip_gt>(), d_gt.as<rhip_gt>(), d_g1.as<rhip_g1>(), d_g2.as<rhip_g2>()), "rhip_dnf_encrypt_batch");
  // records and sealing on the device (records.h); the data is sealed under msg (BDABE) / msg1 msg2 (MKE08)
  RecordSources src(n);
  src.by_rows(d_gt.ptr(), 384 * n_gt, row_off).by_rows(d_g1.ptr(), 128, row_off).by_rows(d_g2.ptr(), 256, row_off);
  finish_encrypt(eng, &tm, layouts, n, item_policy, src, d_msg.as<rhip_gt>() + (n_exp - 1) * n, (const uint8_t*)nonces.data(), pt_blob, pt_off, out_off, out_buf,
                 key_buf);
  return true;
}

// ------------------------------------------------------------------------------------------------ BDABE / MKE08 bulk key issuing
struct KeysArg { const G1* p1; const G1* g1; const G2* p2; const G2* g2; const G1* a1; const G2* a2; };
void* make_keys(Engine& eng, const void* arg) {
  const KeysArg& a = *(const KeysArg*)arg;
  rhip_dnf_keys* d = nullptr;
  eng.check(rhip_dnf_keys_create(eng.ctx(), (const rhip_g1*)a.p1->data(), (const rhip_g1*)a.g1->data(), (const rhip_g2*)a.p2->data(),
                                 (const rhip_g2*)a.g2->data(), (const rhip_g1*)a.a1->data(), (const rhip_g2*)a.a2->data(), &d), "rhip_dnf_keys_create");
  return d;
}
void destroy_keys(void* h) { rhip_dnf_keys_destroy((rhip_dnf_keys*)h); }

// n calls of bdabe::keygen (bdabe/mod.rs:201-222) or mke08::keygen (mke08/mod.rs:185-206) under one authority key (a1, a2; MKE08: the master
// key's g1, g2).  Draw order: one r_u per item, in item order.  Record = the user key with an empty sk_a: sk.u1 | sk.u2 | name | pk.u1 | pk.u2 |
// u32 0.  Every element is a fixed-base multiple (a1 + p1 r, a2 + p2 r, g1 r, g2 r): one lane per element over the 16-bit window tables of
// p1, g1, p2, g2 (k_dnf_keygen_g1 / _g2; tables built once per key and kept), records written on the device -- the names are a device
// source of their own, one layout per distinct name length.
bool keygen_packed(Engine& eng, Rng& rng, const char* what, const G1& p1, const G1& g1, const G2& p2, const G2& g2, const G1& a1, const G2& a2,
                   const std::vector<std::string>& names, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  StageTimer tm(what);
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // the keys' r_u pass through the staging buffers
  const size_t n = names.size();
  if (!out_off) throw RabeError(std::string(what) + ": null input");
  std::map<size_t, uint32_t> layout_of;          // name length -> layout
  std::vector<uint32_t> item_layout(n);
  std::vector<uint64_t> name_off(n);
  std::vector<uint8_t> name_bytes;
  out_off[0] = 0;
  for (size_t i = 0; i < n; i++) {
    const size_t len = names[i].size();
    if (len >= ((size_t)1 << 24)) throw RabeError(std::string(what) + ": a user name of 2^24 bytes or more");
    auto it = layout_of.find(len);
    if (it == layout_of.end()) it = layout_of.emplace(len, (uint32_t)layout_of.size()).first;
    item_layout[i] = it->second;
    name_off[i] = name_bytes.size();
    name_bytes.insert(name_bytes.end(), names[i].begin(), names[i].end());
    out_off[i + 1] = out_off[i] + 64 + 128 + 4 + len + 64 + 128 + 4;
  }
  if (n && (!out_buf || out_cap < out_off[n])) return false;
  if (!n) return true;
  std::vector<RecordLayout> layouts(layout_of.size());
  for (const auto& kv : layout_of) {
    RecordLayout& L = layouts[kv.second];
    L.src(0, 0, 64);             // sk.u1: G1 row 0
    L.src(1, 0, 128);            // sk.u2: G2 row 0
    L.u32((uint32_t)kv.first);
    if (kv.first) L.src(2, 0, (uint32_t)kv.first);
    L.src(0, 64, 64);            // pk.u1: G1 row 1
    L.src(1, 128, 128);          // pk.u2: G2 row 1
    L.u32(0);                    // sk_a: empty
  }
  uint8_t* h_r = eng.pinned(0, n * 32 + 32);
  draw_items(rng, n, [&](Rng& r, size_t i) { const Fr ri = r.next_fr(); memcpy(h_r + 32 * i, ri.l, 32); });
  tm.lap("draws");
  std::string key((const char*)p1.data(), 64);
  key.append((const char*)g1.data(), 64).append((const char*)p2.data(), 128).append((const char*)g2.data(), 128).append((const char*)a1.data(), 64)
      .append((const char*)a2.data(), 128);
  const KeysArg ka{&p1, &g1, &p2, &g2, &a1, &a2};
  const rhip_dnf_keys* keys = (const rhip_dnf_keys*)eng.aux("dnf_keys", key, make_keys, &ka, destroy_keys, 4);
  tm.lap("tables");
  rhip_ctx* cx = eng.ctx();
  DBuf d_r(&eng, n * 32), d_g1(&eng, n * 128 + 4), d_g2(&eng, n * 256 + 4), d_names = up_bytes(eng, name_bytes);
  eng.check(rhip_upload_async(cx, d_r.ptr(), h_r, n * 32), "upload");
  eng.check(rhip_dnf_keygen_batch(cx, keys, n, d_r.as<rhip_fr>(), d_g1.as<rhip_g1>(), d_g2.as<rhip_g2>()), "rhip_dnf_keygen_batch");
  emit_plain_records(eng, layouts, n, item_layout.data(), RecordSources(n).by_item(d_g1.ptr(), 128).by_item(d_g2.ptr(), 256).at_bytes(d_names.ptr(), name_off),
                     out_off, out_buf);
  tm.lap("device: rows, records; one copy out");
  return true;
}

// For every public user key record (name | u1 | u2) of an UNTRUSTED blob the secret attribute keys (attribute, u1 * exp, u2 * exp) of the list
// sets[item_set[i]], exp = h(attribute) h(authority) secret (bdabe/mod.rs:275-305, mke08/mod.rs:248-278).  Nothing is drawn.  An attribute
// that is not this authority's fails the call before any work, as does an item_set out of range; an item with bad bounds, a malformed
// record or (unless trusted) a u1 off the curve / a u2 outside G2 fails alone.  Record = u32 count + rows (attribute, au1, au2): the sk_a
// tail of the user-key record.  The multiplications run scalar-major -- one scalar per (list, position), its rows = the users of that
// list (rhip_g1_mul_rows_at, rhip_g2_mul_rows_at) -- and write item-major through the row index, where the record writer reads them.
bool request_sk_packed(Engine& eng, const char* what, const std::string& authority, const Fr& secret, const std::vector<std::vector<std::string>>& sets,
                       size_t n, const uint32_t* item_set, const uint8_t* blob, size_t blob_len, const uint64_t* in_off, bool trusted, int32_t* status,
                       uint8_t* out_buf, size_t out_cap, uint64_t* out_off, std::vector<std::string>* errors) {
  StageTimer tm(what);
  Engine::ArenaScope arena(eng);
  eng.scrub_when_done();          // the attribute exponents pass through the staging buffers
  errors->assign(n, "");
  if (!in_off || !out_off || (n && (!item_set || !status || !blob))) throw RabeError(std::string(what) + ": null input");
  for (size_t s = 0; s < sets.size(); s++)
    for (const auto& a : sets[s])
      if (!from_authority(a, authority))
        throw RabeError("attribute " + a + " is not from_authority() or !is_eligible() (attribute list " + std::to_string(s) + ")");
  // the first bad item decides the message: the rows count up to the first index out of range, which check_index reports -- before the parse
  uint64_t all_rows = 0;
  for (size_t i = 0; i < n && item_set[i] < sets.size(); i++) {
    all_rows += sets[item_set[i]].size();
    if (all_rows > 0xFFFFFFF0ull) throw RabeError(std::string(what) + ": more than 2^32 key elements in one call");
  }
  check_index(what, "item_set", n, item_set, sets.size());
  std::vector<size_t> fixed(sets.size());
  std::vector<uint32_t> scal_base(sets.size() + 1, 0);
  for (size_t s = 0; s < sets.size(); s++) {
    fixed[s] = 4;
    for (const auto& a : sets[s]) fixed[s] += 4 + a.size() + 64 + 128;
    scal_base[s + 1] = scal_base[s] + (uint32_t)sets[s].size();
  }
  (void)check_offsets(n, in_off, blob_len, errors);
  for_each_record(n, errors, [&](size_t i) {
    Cursor r{blob + in_off[i], blob + in_off[i + 1]};
    (void)r.str();
    (void)r.raw(64 + 128);
    if (r.p != r.end) throw RabeError("deserialize: trailing bytes after the record");
  });
  tm.lap("parse");
  std::vector<size_t> live;
  for (size_t i = 0; i < n; i++) if ((*errors)[i].empty()) live.push_back(i);
  // a failed item's slot is empty
  if (!record_offsets(what, "item_set", n, item_set, sets.size(), [&](size_t i) { return (*errors)[i].empty() ? fixed[item_set[i]] : 0; }, nullptr, out_buf,
                      out_cap, out_off) && out_off[n]) return false;
  const size_t m = live.size();
  std::vector<uint8_t> good(m, 1);
  if (m) {
    // rows, scalar-major: scalar j = (list s, position y) owns the live items of list s, in item order
    std::vector<std::vector<uint32_t>> users(sets.size());
    std::vector<uint32_t> item_row(m + 1, 0);
    for (size_t j = 0; j < m; j++) {
      const uint32_t s = item_set[live[j]];
      users[s].push_back((uint32_t)j);
      item_row[j + 1] = item_row[j] + (uint32_t)sets[s].size();
    }
    const size_t total = item_row[m], n_scal = scal_base[sets.size()];
    std::vector<uint32_t> scal_row(n_scal + 1, 0), row_src(total), row_dst(total);
    for (size_t s = 0; s < sets.size(); s++)
      for (size_t y = 0; y < sets[s].size(); y++) {
        const size_t k = scal_base[s] + y;
        uint32_t t = scal_row[k];
        for (uint32_t j : users[s]) { row_src[t] = j; row_dst[t] = item_row[j] + (uint32_t)y; t++; }
        scal_row[k + 1] = t;
      }
    uint8_t* h_k = eng.pinned(0, n_scal * 32 + 32);
    {
      const Fr ha = sha3_hash_fr(authority);
      for (size_t s = 0; s < sets.size(); s++)
        for (size_t y = 0; y < sets[s].size(); y++) {
          Fr e = fr_mul(fr_mul(sha3_hash_fr(sets[s][y]), ha), secret);
          memcpy(h_k + 32 * (size_t)(scal_base[s] + y), e.l, 32);
          memset(e.l, 0, sizeof(e.l));
        }
    }
    tm.lap("rows + exponents");
    uint8_t* h_u1 = eng.pinned(1, m * 64 + 4);
    uint8_t* h_u2 = eng.pinned(2, m * 128 + 4);
    parallel_for(m, [&](size_t j) {
      const uint8_t* end = blob + in_off[live[j] + 1];
      memcpy(h_u1 + 64 * j, end - 192, 64);
      memcpy(h_u2 + 128 * j, end - 128, 128);
    });
    tm.lap("pack");
    rhip_ctx* cx = eng.ctx();
    DBuf d_u1(&eng, m * 64 + 4), d_u2(&eng, m * 128 + 4), d_a1(&eng, total * 64 + 4), d_a2(&eng, total * 128 + 4);
    eng.check(rhip_upload_async(cx, d_u1.ptr(), h_u1, m * 64), "upload");
    eng.check(rhip_upload_async(cx, d_u2.ptr(), h_u2, m * 128), "upload");
    std::unique_ptr<MemberChecks> mc;
    if (!trusted) {
      mc.reset(new MemberChecks(eng));
      mc->add(1, d_u1.ptr(), m);
      mc->add(2, d_u2.ptr(), m);
    }
    if (total) {
      DBuf d_k(&eng, n_scal * 32), d_scal_row = up32(eng, scal_row), d_src = up32(eng, row_src), d_dst = up32(eng, row_dst);
      eng.check(rhip_upload_async(cx, d_k.ptr(), h_k, n_scal * 32), "upload");
      eng.check(rhip_g1_mul_rows_at(cx, total, d_scal_row.as<uint32_t>(), d_u1.as<rhip_g1>(), d_src.as<uint32_t>(), n_scal, d_k.as<rhip_fr>(),
                                    d_dst.as<uint32_t>(), d_a1.as<rhip_g1>()), "rhip_g1_mul_rows_at");
      eng.check(rhip_g2_mul_rows_at(cx, total, d_scal_row.as<uint32_t>(), d_u2.as<rhip_g2>(), d_src.as<uint32_t>(), n_scal, d_k.as<rhip_fr>(),
                                    d_dst.as<uint32_t>(), d_a2.as<rhip_g2>()), "rhip_g2_mul_rows_at");
    }
    if (mc) {
      mc->collect();
      const auto &ok1 = mc->ok(0), &ok2 = mc->ok(1);
      for (size_t j = 0; j < m; j++) {
        if (ok1[j] && ok2[j]) continue;
        good[j] = 0;
        (*errors)[live[j]] = !ok1[j] ? "deserialize: u1 is not a point of G1 with canonical coordinates (FieldError::NotMember)"
                                     : "deserialize: u2 is not a member of G2 (FieldError::NotMember)";
      }
    }
    // the records of the items that passed: a failed item's slot is empty, so the live records stay back to back
    std::vector<RecordLayout> layouts(sets.size());
    for (size_t s = 0; s < sets.size(); s++) {
      RecordLayout& L = layouts[s];
      L.u32((uint32_t)sets[s].size());
      for (size_t y = 0; y < sets[s].size(); y++) { L.str(sets[s][y]); L.src(0, (uint32_t)(64 * y), 64); L.src(1, (uint32_t)(128 * y), 128); }
      if (L.bytes() != fixed[s]) throw RabeError(std::string(what) + ": record layout and size disagree");
    }
    std::vector<uint32_t> lay;
    std::vector<uint64_t> off1, off2, rec_off;
    size_t at = 0;
    for (size_t i = 0, j = 0; i < n; i++) {
      const bool is_live = j < m && live[j] == i;
      const bool ok = is_live && good[j];
      out_off[i] = at;
      if (ok) {
        lay.push_back(item_set[i]);
        off1.push_back(64ull * item_row[j]);
        off2.push_back(128ull * item_row[j]);
        rec_off.push_back(at);
        at += fixed[item_set[i]];
      }
      if (is_live) j++;
    }
    out_off[n] = at;
    rec_off.push_back(at);
    emit_plain_records(eng, layouts, lay.size(), lay.data(), RecordSources(lay.size()).at_bytes(d_a1.ptr(), off1).at_bytes(d_a2.ptr(), off2), rec_off.data(),
                       out_buf);
    if (lay.empty()) eng.check(rhip_sync(cx), "rhip_sync");
    tm.lap(trusted ? "device: rows, records; one copy out" : "device: rows, records, membership beside; one copy out");
  }
  for (size_t i = 0; i < n; i++) status[i] = (*errors)[i].empty() ? 0 : -1;
  return true;
}

// ------------------------------------------------------------------------------------------------ BDABE / MKE08 key decapsulation
// n calls of bdabe::decrypt (bdabe/mod.rs:367-399) / mke08::decrypt (mke08/mod.rs:343-380) up to the Gt, with ONE user key against n records
// (include/rabe_host.h: rabe_{bdabe,mke08}_kem_decaps), then the KDF behind the verdict mask.  Record = policy, language, conjunction count, per
// conjunction (name count, names, n_gt Gt, G1, G2, G1, G2), sealed length, sealed bytes (skipped, never read).  Three caches of the call:
//   policies  by (language, text): parse + traverse_policy against the key's attribute names -- the reference's first verdict;
//   classes   by the bytes of ONE conjunction's name list as the record states it: is_satisfiable and, name by name, the FIRST key row (find());
//   skeletons by (policy length, the name lists of all conjunctions): the first satisfiable conjunction and its class -- records of one skeleton
//             have every element at the same offset, so they also share their gather shape.
// Per class S1 = sum au1, S2 = sum au2 in list order on the device (rounds of rhip_g1_add / rhip_g2_add over the classes that still have a
// term: classes are numbered by falling length, so a round is a prefix), one rhip_g2_lines_prepare over [u2, S2 of every class], then
// rhip_dnf_decrypt_batch_one_uk: four Miller loops per item.  Untrusted input: every element of every conjunction is gathered a second time into
// whole-record arrays for the decoder's checks (curve, Gt membership, G2 subgroup -- the chosen conjunction's two G2 elements out of their own
// walks); the pairings read the chosen conjunction's copy.
struct DnfUserRow { const std::string* attr; const G1* g1; const G2* g2; };
struct DnfDecScheme {
  const char* timer;               // "bdabe::decaps_packed"
  const char* no_match;            // the object API's message where traverse_policy fails
  uint32_t n_gt;
};
void decaps_packed(Engine& eng, const DnfDecScheme& sc, const G1& u1, const G2& u2, const std::vector<DnfUserRow>& rows, size_t n, const uint8_t* ct_blob,
                   size_t ct_len, const uint64_t* ct_off, bool trusted, int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  StageTimer tm(sc.timer);
  Engine::ArenaScope arena(eng);
  errors->assign(n, "");
  if (!ct_off || (n && (!ct_blob || !status || !key_buf))) throw RabeError(std::string(sc.timer) + ": null input");
  if (!n) return;
  (void)check_offsets(n, ct_off, ct_len, errors);
  BlobGather gather(eng, ct_blob, ct_len);          // the blob starts for the device now, beside the parsing below (records.h)
  const size_t n_gt = sc.n_gt, conj_bytes = 384 * n_gt + 384;
  std::vector<std::string> key_names;
  for (const auto& r : rows) key_names.push_back(*r.attr);
  struct PolPlan { std::string err; };
  struct ClassPlan { std::string err; bool sat = true; std::vector<uint32_t> key_row; uint32_t id = 0xFFFFFFFFu; };
  struct SkelPlan { std::string err; uint32_t chosen = 0, n_conj = 0; std::shared_ptr<ClassPlan> cls; };
  PlanCache<PolPlan> pols;
  PlanCache<ClassPlan> classes;          // keyed on bytes, like the skeletons: the language is no part of those keys
  PlanCache<SkelPlan> skels;
  auto make_pol = [&](PolPlan&, const std::string& text, PolicyLanguage lang) {
    if (!traverse_policy(key_names, parse_or_error(text, lang))) throw RabeError(sc.no_match);
  };
  auto make_class = [&](ClassPlan& c, const std::string& names, PolicyLanguage) {          // names: u32 count, then (u32 length, bytes) per name
    for (size_t at = 4; at < names.size();) {
      const uint32_t l = get_u32((const uint8_t*)names.data() + at);
      size_t k = 0;
      while (k < rows.size() && !(rows[k].attr->size() == l && memcmp(rows[k].attr->data(), names.data() + at + 4, l) == 0)) k++;
      if (k == rows.size()) { c.sat = false; c.key_row.clear(); return; }
      c.key_row.push_back((uint32_t)k);
      at += 4 + (size_t)l;
    }
  };
  auto make_skel = [&](SkelPlan& s, const std::string& key, PolicyLanguage) {          // key: u32 policy length, u32 conjunctions, their name lists
    const uint8_t* p = (const uint8_t*)key.data() + 4;
    s.n_conj = get_u32(p);
    p += 4;
    for (uint32_t y = 0; y < s.n_conj; y++) {
      const uint8_t* first = p;
      const uint32_t na = get_u32(p);
      p += 4;
      for (uint32_t k = 0; k < na; k++) p += 4 + (size_t)get_u32(p);
      auto c = classes.get((const char*)first, (size_t)(p - first), PolicyLanguage::JsonPolicy, make_class);
      if (!c->sat) continue;
      s.chosen = y;
      s.cls = c;
      return;
    }
    throw RabeError(std::string(sc.timer) + ": the key satisfies the record's policy but none of its conjunction lists (decrypt_gt returns Gt::one() there)");
  };
  struct View { std::shared_ptr<SkelPlan> skel; uint32_t first_conj = 0; };          // first_conj: offset of the first conjunction in the record
  std::vector<View> v(n);
  for_each_record(n, errors, [&](size_t i) {
    const uint8_t* rec = ct_blob + ct_off[i];
    Cursor r{rec, ct_blob + ct_off[i + 1]};
    const auto text = r.str();
    const PolicyLanguage lang = *r.raw(1) ? PolicyLanguage::HumanPolicy : PolicyLanguage::JsonPolicy;
    static thread_local std::string key;          // per-thread scratch: no allocation per record once it has grown
    key.assign(8, '\0');
    put_u32((uint8_t*)&key[0], text.second);
    const uint32_t n_conj = r.u32();
    if ((size_t)n_conj * (4 + conj_bytes) > (size_t)(r.end - r.p)) throw_truncated();          // before anything is sized by it
    put_u32((uint8_t*)&key[4], n_conj);
    v[i].first_conj = (uint32_t)(r.p - rec);
    for (uint32_t y = 0; y < n_conj; y++) {
      const uint8_t* first = r.p;
      const uint32_t na = r.u32();
      if ((size_t)na * 4 > (size_t)(r.end - r.p)) throw_truncated();
      for (uint32_t k = 0; k < na; k++) (void)r.str();
      key.append((const char*)first, (size_t)(r.p - first));
      (void)r.raw(conj_bytes);
    }
    (void)r.raw(r.u32());          // the sealed part: skipped by its length field
    if (r.p != r.end) throw RabeError("deserialize: trailing bytes after the record");
    auto pl = pols.get(text.first, text.second, lang, make_pol);
    if (!pl->err.empty()) throw RabeError(pl->err);
    auto sk = skels.get(key.data(), key.size(), PolicyLanguage::JsonPolicy, make_skel);
    if (!sk->err.empty()) throw RabeError(sk->err);
    v[i].skel = sk;
  });
  tm.lap("parse + plan");
  // ---- live items, their rows (one per conjunction of the record) and the classes they name, numbered by falling length
  std::vector<size_t> live;
  std::vector<uint32_t> row_off{0};
  std::vector<ClassPlan*> cls;
  for (size_t i = 0; i < n; i++) {
    if (!(*errors)[i].empty()) continue;
    live.push_back(i);
    row_off.push_back(row_off.back() + v[i].skel->n_conj);
    ClassPlan* c = v[i].skel->cls.get();
    if (c->id == 0xFFFFFFFFu) { c->id = 0; cls.push_back(c); }
  }
  const size_t m = live.size(), total = row_off[m], n_classes = cls.size();
  if (!m) {
    for (size_t i = 0; i < n; i++) status[i] = -1;
    memset(key_buf, 0, n * 32);
    return;
  }
  std::stable_sort(cls.begin(), cls.end(), [](const ClassPlan* a, const ClassPlan* b) { return a->key_row.size() > b->key_row.size(); });
  for (size_t c = 0; c < n_classes; c++) cls[c]->id = (uint32_t)c;
  rhip_ctx* cx = eng.ctx();
  // ---- S1, S2 per class: the first terms from the host, then one round of additions per further term over the classes that have one
  const size_t longest = cls[0]->key_row.size();
  std::vector<uint8_t> h_s1(n_classes * 64, 0), h_q((1 + n_classes) * 128, 0), b1, b2;
  std::vector<uint8_t> skip(n_classes, 0);
  memcpy(h_q.data(), u2.data(), 128);
  std::vector<size_t> round_n;
  for (size_t c = 0; c < n_classes; c++) {
    if (cls[c]->key_row.empty()) { skip[c] = 3; continue; }          // an empty conjunction: both sums are the identity
    const DnfUserRow& k = rows[cls[c]->key_row[0]];
    memcpy(h_s1.data() + 64 * c, k.g1->data(), 64);
    memcpy(h_q.data() + 128 * (1 + c), k.g2->data(), 128);
  }
  for (size_t r = 1; r < longest; r++) {
    size_t k_r = 0;
    while (k_r < n_classes && cls[k_r]->key_row.size() > r) k_r++;
    round_n.push_back(k_r);
    for (size_t c = 0; c < k_r; c++) {
      const DnfUserRow& k = rows[cls[c]->key_row[r]];
      b1.insert(b1.end(), k.g1->begin(), k.g1->end());
      b2.insert(b2.end(), k.g2->begin(), k.g2->end());
    }
  }
  eng.scrub_session_when_done();          // the key's elements and their sums pass through the arena
  DBuf d_s1 = up_bytes(eng, h_s1), d_q = up_bytes(eng, h_q), d_b1 = up_bytes(eng, b1.empty() ? std::vector<uint8_t>(64, 0) : b1),
       d_b2 = up_bytes(eng, b2.empty() ? std::vector<uint8_t>(128, 0) : b2);
  {
    size_t at = 0;
    for (size_t k_r : round_n) {
      eng.check(rhip_g1_add(cx, k_r, d_s1.as<rhip_g1>(), d_b1.as<rhip_g1>() + at, d_s1.as<rhip_g1>()), "rhip_g1_add");
      eng.check(rhip_g2_add(cx, k_r, d_q.as<rhip_g2>() + 1, d_b2.as<rhip_g2>() + at, d_q.as<rhip_g2>() + 1), "rhip_g2_add");
      at += k_r;
    }
  }
  if (longest > 1) {          // a sum may be the identity (key rows that cancel): the skip bits are read off the sums themselves
    eng.check(rhip_download(cx, h_s1.data(), d_s1.ptr(), h_s1.size()), "download (S1)");
    eng.check(rhip_download(cx, h_q.data(), d_q.ptr(), h_q.size()), "download (S2)");
  }
  auto all_zero = [](const uint8_t* p, size_t k) { for (size_t i = 0; i < k; i++) if (p[i]) return false; return true; };
  for (size_t c = 0; c < n_classes; c++)
    skip[c] |= (all_zero(h_s1.data() + 64 * c, 64) ? 1 : 0) | (all_zero(h_q.data() + 128 * (1 + c), 128) ? 2 : 0);
  std::unique_ptr<rhip_g2_lines, void (*)(rhip_g2_lines*)> lines(nullptr, rhip_g2_lines_destroy);
  {
    rhip_g2_lines* l = nullptr;
    eng.check(rhip_g2_lines_prepare(cx, 1 + n_classes, d_q.as<rhip_g2>(), &l), "rhip_g2_lines_prepare");
    lines.reset(l);
  }
  DBuf d_u1 = up_bytes(eng, std::vector<uint8_t>(u1.begin(), u1.end())), d_nu1(&eng, 64), d_skip = up_bytes(eng, skip);
  eng.check(rhip_g1_neg(cx, 1, d_u1.as<rhip_g1>(), d_nu1.as<rhip_g1>()), "rhip_g1_neg");
  tm.lap("classes: sums, lines");
  // ---- shapes: destinations 0 / 1 the chosen conjunction's Gt element(s), 2 its (e2, e4), 3 its (e3, e5); untrusted input also 4 / 5 / 6:
  // every conjunction's Gt, G1 and G2 elements, for the decoder's checks
  std::vector<uint32_t> item_class(m), walked_idx, walked_off{0};
  const size_t n_dst = trusted ? 4 : 7;
  std::vector<uint64_t> dst_off(n_dst * m);
  for (size_t j = 0; j < m; j++) {
    const View& w = v[live[j]];
    const SkelPlan& s = *w.skel;
    item_class[j] = s.cls->id;
    dst_off[j] = dst_off[m + j] = 384ull * j;
    dst_off[2 * m + j] = 128ull * j;
    dst_off[3 * m + j] = 256ull * j;
    if (!trusted) {
      dst_off[4 * m + j] = 384ull * n_gt * row_off[j];
      dst_off[5 * m + j] = 128ull * row_off[j];
      dst_off[6 * m + j] = 256ull * row_off[j];
      walked_idx.push_back(2 * (row_off[j] + s.chosen));
      walked_idx.push_back(2 * (row_off[j] + s.chosen) + 1);
      walked_off.push_back((uint32_t)walked_idx.size());
    }
    gather_record(gather, ct_off[live[j]], &s, [&](std::vector<RecordLayout::Part>& parts) {
      const uint8_t* rec = ct_blob + ct_off[live[j]];
      Cursor r{rec + w.first_conj, ct_blob + ct_off[live[j] + 1]};
      for (uint32_t y = 0; y < s.n_conj; y++) {
        const uint32_t na = r.u32();
        for (uint32_t k = 0; k < na; k++) (void)r.str();
        const uint32_t at = (uint32_t)(r.raw(conj_bytes) - rec), g = at + (uint32_t)(384 * n_gt);          // Gt element(s) | G1 G2 G1 G2
        if (y == s.chosen) {
          for (uint32_t t = 0; t < n_gt; t++) parts.push_back({at + 384 * t, 384, t, 0});
          parts.push_back({g, 64, 2, 0});
          parts.push_back({g + 64, 128, 3, 0});
          parts.push_back({g + 192, 64, 2, 64});
          parts.push_back({g + 256, 128, 3, 128});
        }
        if (trusted) continue;
        parts.push_back({at, (uint32_t)(384 * n_gt), 4, (uint32_t)(384 * n_gt * y)});
        parts.push_back({g, 64, 5, 128 * y});
        parts.push_back({g + 64, 128, 6, 256 * y});
        parts.push_back({g + 192, 64, 5, 128 * y + 64});
        parts.push_back({g + 256, 128, 6, 256 * y + 128});
      }
    });
  }
  tm.lap("shapes");
  DBuf d_class = up32(eng, item_class), d_row_off = up32(eng, row_off), d_j1(&eng, m * 384), d_j2(&eng, n_gt == 2 ? m * 384 : 4), d_g1(&eng, m * 128),
       d_g2(&eng, m * 256), d_out(&eng, m * 384 + 4), d_all_gt(&eng, trusted ? 4 : total * 384 * n_gt + 4), d_all_g1(&eng, trusted ? 4 : total * 128 + 4);
  WalkScope ws;
  ws.d_g2 = DBuf(&eng, trusted ? 4 : total * 256 + 4);
  std::vector<void*> dst{d_j1.ptr(), d_j2.ptr(), d_g1.ptr(), d_g2.ptr()};
  if (!trusted) { dst.push_back(d_all_gt.ptr()); dst.push_back(d_all_g1.ptr()); dst.push_back(ws.d_g2.ptr()); }
  gather.run(dst, dst_off);
  if (!trusted) {
    ws.mc.reset(new MemberChecks(eng));
    ws.mc->add(1, d_all_g1.ptr(), total * 2, d_row_off.as<uint32_t>(), m, 2);
    ws.mc->add(3, d_all_gt.ptr(), total * n_gt, d_row_off.as<uint32_t>(), m, (uint32_t)n_gt);
    // e3 and e5 of the chosen conjunction are the two walking arguments of an item: their membership comes out of the decrypt's own Miller
    // loops; the G2 elements of the other conjunctions, and those of an item with a skipped pair, get the stand-alone test (common.h: WalkedG2)
    if (walk_checks()) ws.walked.reset(new WalkedG2(eng, *ws.mc, ws.d_g2.ptr(), total * 2, d_row_off.as<uint32_t>(), row_off, 2, &walked_idx, &walked_off));
    else { ws.k_alone = ws.mc->add_count(); ws.mc->add(2, ws.d_g2.ptr(), total * 2, d_row_off.as<uint32_t>(), m, 2); }
  }
  if (n_gt == 2) eng.check(rhip_gt_mul(cx, m, d_j1.as<rhip_gt>(), d_j2.as<rhip_gt>(), d_j1.as<rhip_gt>()), "rhip_gt_mul");          // MKE08: the lead is j1 j2
  if (ws.walked) ws.walked->arm();
  eng.check(rhip_dnf_decrypt_batch_one_uk(cx, m, n_classes, d_class.as<uint32_t>(), d_s1.as<rhip_g1>(), d_skip.as<uint8_t>(), d_nu1.as<rhip_g1>(), lines.get(),
                                          d_g1.as<rhip_g1>(), d_g2.as<rhip_g2>(), d_j1.as<rhip_gt>(), d_out.as<rhip_gt>()),
            "rhip_dnf_decrypt_batch_one_uk");
  static const char* const G2_NOT_MEMBER = "deserialize: a G2 element is not a group member (FieldError::NotMember)";
  if (ws.mc) {
    ws.mc->collect();
    ws.fail(live, {0}, "deserialize: a G1 element is not a group member (FieldError::NotMember)", errors);
    ws.fail(live, {ws.k_alone}, G2_NOT_MEMBER, errors);
    ws.fail(live, {1}, "deserialize: a Gt element is not a group member (FieldError::NotMember)", errors);
  }
  ws.fail_walked(live, G2_NOT_MEMBER, errors);          // every verdict first: there is no open to queue behind the pairings
  derive_keys(eng, n, live, d_out.ptr(), status, key_buf, *errors);
  tm.lap(trusted ? "device: gather, pairings, keys" : "device: gather, pairings, keys; membership beside");
}
}  // namespace
}  // namespace dnfabe

namespace bdabe {
static bool encrypt_core(Engine& eng, Rng& rng, const BdabePublicKey& pk, const std::vector<const BdabePublicAttributeKey*>& attr_pks,
                         const std::vector<std::string>& policies, PolicyLanguage language, size_t n, const uint32_t* item_policy, const uint8_t* pt_blob,
                         const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  static const dnfabe::DnfScheme sc{"bdabe::encrypt_packed", "bdabe::encaps_packed", "bdabe_terms", "Error in bdabe/encrypt: Policy not in DNF.", 1};
  std::vector<dnfabe::DnfKey> keys;
  for (const auto* k : attr_pks) keys.push_back({&k->attr, &k->a1, &k->a2, {&k->a3, nullptr}});
  return dnfabe::encrypt_packed(eng, rng, sc, pk.p1, pk.p2, keys, policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off, key_buf);
}
bool encrypt_packed(Engine& eng, Rng& rng, const BdabePublicKey& pk, const std::vector<const BdabePublicAttributeKey*>& attr_pks,
                    const std::vector<std::string>& policies, PolicyLanguage language, size_t n, const uint32_t* item_policy, const uint8_t* pt_blob,
                    const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  return encrypt_core(eng, rng, pk, attr_pks, policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off, nullptr);
}
// n key encapsulations (include/rabe_host.h: rabe_bdabe_kem_encaps): header i is the BdabeCiphertext record encrypt_packed writes for the same draws
// with a sealed part of length zero, key_buf + 32 i = SHA3-256(bytes(msg_i)).  Draw order: encrypt_packed's minus the nonce.
bool encaps_packed(Engine& eng, Rng& rng, const BdabePublicKey& pk, const std::vector<const BdabePublicAttributeKey*>& attr_pks,
                   const std::vector<std::string>& policies, PolicyLanguage language, size_t n, const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap,
                   uint64_t* out_off, uint8_t* key_buf) {
  if (n && !key_buf) throw RabeError("bdabe::encaps_packed: null input");
  if (!n) { out_off[0] = 0; return true; }
  return encrypt_core(eng, rng, pk, attr_pks, policies, language, n, item_policy, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}
// n key decapsulations under ONE user key (include/rabe_host.h: rabe_bdabe_kem_decaps): key_buf + 32 i = SHA3-256(bytes(Gt)) of what decrypt_gt
// returns for record i; input may be headers or full records
void decaps_packed(Engine& eng, const BdabeUserKey& uk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                   int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  static const dnfabe::DnfDecScheme sc{"bdabe::decaps_packed", "Error in bdabe/decrypt: attributes in sk do not match policy in ct.", 1};
  std::vector<dnfabe::DnfUserRow> rows;
  for (const auto& k : uk.sk_a) rows.push_back({&k.attr, &k.au1, &k.au2});
  dnfabe::decaps_packed(eng, sc, uk.sk.u1, uk.sk.u2, rows, n, ct_blob, ct_len, ct_off, trusted, status, key_buf, errors);
}
bool keygen_packed(Engine& eng, Rng& rng, const BdabePublicKey& pk, const BdabeSecretAuthorityKey& ska, const std::vector<std::string>& names,
                   uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  return dnfabe::keygen_packed(eng, rng, "bdabe::keygen_packed", pk.p1, pk.g1, pk.p2, pk.g2, ska.a1, ska.a2, names, out_buf, out_cap, out_off);
}
bool request_attribute_sk_packed(Engine& eng, const BdabeSecretAuthorityKey& ska, const std::vector<std::vector<std::string>>& sets, size_t n,
                                 const uint32_t* item_set, const uint8_t* upk_blob, size_t upk_len, const uint64_t* upk_off, bool trusted, int32_t* status,
                                 uint8_t* out_buf, size_t out_cap, uint64_t* out_off, std::vector<std::string>* errors) {
  return dnfabe::request_sk_packed(eng, "bdabe::request_attribute_sk_packed", ska.name, ska.a3, sets, n, item_set, upk_blob, upk_len, upk_off, trusted,
                                   status, out_buf, out_cap, out_off, errors);
}
}  // namespace bdabe

namespace mke08 {
static bool encrypt_core(Engine& eng, Rng& rng, const Mke08PublicKey& pk, const std::vector<const Mke08PublicAttributeKey*>& attr_pks,
                         const std::vector<std::string>& policies, PolicyLanguage language, size_t n, const uint32_t* item_policy, const uint8_t* pt_blob,
                         const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off, uint8_t* key_buf) {
  static const dnfabe::DnfScheme sc{"mke08::encrypt_packed", "mke08::encaps_packed", "mke08_terms", "Error in mke08/encrypt: policy is not in dnf", 2};
  std::vector<dnfabe::DnfKey> keys;
  for (const auto* k : attr_pks) keys.push_back({&k->attr, &k->g1, &k->g2, {&k->gt1, &k->gt2}});
  return dnfabe::encrypt_packed(eng, rng, sc, pk.p1, pk.p2, keys, policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off, key_buf);
}
bool encrypt_packed(Engine& eng, Rng& rng, const Mke08PublicKey& pk, const std::vector<const Mke08PublicAttributeKey*>& attr_pks,
                    const std::vector<std::string>& policies, PolicyLanguage language, size_t n, const uint32_t* item_policy, const uint8_t* pt_blob,
                    const uint64_t* pt_off, uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  return encrypt_core(eng, rng, pk, attr_pks, policies, language, n, item_policy, pt_blob, pt_off, out_buf, out_cap, out_off, nullptr);
}
// the key encapsulation pair, as bdabe's: the key is the KDF of msg1 * msg2, the element encrypt_packed seals under
bool encaps_packed(Engine& eng, Rng& rng, const Mke08PublicKey& pk, const std::vector<const Mke08PublicAttributeKey*>& attr_pks,
                   const std::vector<std::string>& policies, PolicyLanguage language, size_t n, const uint32_t* item_policy, uint8_t* out_buf, size_t out_cap,
                   uint64_t* out_off, uint8_t* key_buf) {
  if (n && !key_buf) throw RabeError("mke08::encaps_packed: null input");
  if (!n) { out_off[0] = 0; return true; }
  return encrypt_core(eng, rng, pk, attr_pks, policies, language, n, item_policy, nullptr, nullptr, out_buf, out_cap, out_off, key_buf);
}
void decaps_packed(Engine& eng, const Mke08UserKey& uk, size_t n, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off, bool trusted,
                   int32_t* status, uint8_t* key_buf, std::vector<std::string>* errors) {
  static const dnfabe::DnfDecScheme sc{"mke08::decaps_packed", "Error in mke08/decrypt: attributes in sk do not match policy in ct.", 2};
  std::vector<dnfabe::DnfUserRow> rows;
  for (const auto& k : uk.sk_a) rows.push_back({&k.attr, &k.g1, &k.g2});
  dnfabe::decaps_packed(eng, sc, uk.sk.g1, uk.sk.g2, rows, n, ct_blob, ct_len, ct_off, trusted, status, key_buf, errors);
}
bool keygen_packed(Engine& eng, Rng& rng, const Mke08PublicKey& pk, const Mke08MasterKey& msk, const std::vector<std::string>& names, uint8_t* out_buf,
                   size_t out_cap, uint64_t* out_off) {
  return dnfabe::keygen_packed(eng, rng, "mke08::keygen_packed", pk.p1, pk.g1, pk.p2, pk.g2, msk.g1, msk.g2, names, out_buf, out_cap, out_off);
}
bool request_authority_sk_packed(Engine& eng, const Mke08SecretAuthorityKey& ska, const std::vector<std::vector<std::string>>& sets, size_t n,
                                 const uint32_t* item_set, const uint8_t* upk_blob, size_t upk_len, const uint64_t* upk_off, bool trusted, int32_t* status,
                                 uint8_t* out_buf, size_t out_cap, uint64_t* out_off, std::vector<std::string>* errors) {
  return dnfabe::request_sk_packed(eng, "mke08::request_authority_sk_packed", ska.name, ska.r, sets, n, item_set, upk_blob, upk_len, upk_off, trusted,
                                   status, out_buf, out_cap, out_off, errors);
}
}  // namespace mke08

}  // namespace schemes
}  // namespace rabe
