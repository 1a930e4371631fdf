// planner.cpp -- see planner.hpp
#include "planner.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <queue>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

namespace allwave {
namespace planner {

// ---- SipHash (Aumasson & Bernstein); Rust's DefaultHasher is SipHash-1-3 with k0 = k1 = 0 ----
static inline uint64_t rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

uint64_t siphash(const uint8_t* data, size_t n, uint64_t k0, uint64_t k1, int c_rounds, int d_rounds) {
  uint64_t v0 = 0x736f6d6570736575ULL ^ k0, v1 = 0x646f72616e646f6dULL ^ k1;
  uint64_t v2 = 0x6c7967656e657261ULL ^ k0, v3 = 0x7465646279746573ULL ^ k1;
  auto round = [&]() {
    v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
    v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
    v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
  };
  const size_t full = n / 8;
  for (size_t i = 0; i < full; ++i) {
    uint64_t m;
    memcpy(&m, data + 8 * i, 8);
    v3 ^= m;
    for (int r = 0; r < c_rounds; ++r) round();
    v0 ^= m;
  }
  uint64_t b = (uint64_t)n << 56;
  for (size_t i = 0; i < (n & 7); ++i) b |= (uint64_t)data[8 * full + i] << (8 * i);
  v3 ^= b;
  for (int r = 0; r < c_rounds; ++r) round();
  v0 ^= b;
  v2 ^= 0xff;
  for (int r = 0; r < d_rounds; ++r) round();
  return v0 ^ v1 ^ v2 ^ v3;
}

uint64_t default_hash_bytes(const uint8_t* p, size_t n) {
  // <[u8] as Hash>::hash: write_length_prefix(len) (a usize = u64 LE) then the bytes
  uint8_t buf[8 + 64];
  std::vector<uint8_t> big;
  uint8_t* b = buf;
  if (n > 64) { big.resize(n + 8); b = big.data(); }
  const uint64_t len = (uint64_t)n;
  memcpy(b, &len, 8);
  if (n) memcpy(b + 8, p, n);
  return siphash(b, n + 8, 0, 0, 1, 3);
}

uint64_t default_hash_str(const std::string& s) {
  // <str as Hash>::hash: the bytes followed by 0xFF
  std::vector<uint8_t> b(s.size() + 1);
  if (!s.empty()) memcpy(b.data(), s.data(), s.size());
  b[s.size()] = 0xFF;
  return siphash(b.data(), b.size(), 0, 0, 1, 3);
}

static inline bool is_dna_base(uint8_t b) {  // alignment.rs:151-154, mash.rs:116-119
  const uint8_t u = (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b;
  return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

template <bool CANONICAL>
static std::vector<uint64_t> sketch_impl(const std::vector<uint8_t>& seq, size_t k, size_t sketch_size) {
  std::vector<uint64_t> hashes;
  if (seq.size() < k || k == 0) return hashes;
  hashes.reserve(seq.size() - k + 1);
  // positions of the last non-ACGT byte seen, to skip k-mers containing one in O(1)
  size_t bad_until = 0;  // k-mers starting before this index contain a non-base
  for (size_t i = 0; i < k - 1 && i < seq.size(); ++i)
    if (!is_dna_base(seq[i])) bad_until = i + 1;
  std::vector<uint8_t> rc(k);
  for (size_t i = 0; i + k <= seq.size(); ++i) {
    if (!is_dna_base(seq[i + k - 1])) bad_until = i + k;
    if (i < bad_until) continue;
    uint64_t h = default_hash_bytes(seq.data() + i, k);
    if (CANONICAL) {  // mash.rs:121-133: upper-cases while complementing
      for (size_t j = 0; j < k; ++j) {
        const uint8_t b = seq[i + k - 1 - j];
        const uint8_t u = (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b;
        rc[j] = u == 'A' ? 'T' : u == 'T' ? 'A' : u == 'C' ? 'G' : u == 'G' ? 'C' : b;
      }
      h = std::min(h, default_hash_bytes(rc.data(), k));
    }
    hashes.push_back(h);
  }
  std::sort(hashes.begin(), hashes.end());
  if (hashes.size() > sketch_size) hashes.resize(sketch_size);  // truncate BEFORE deduplicating
  hashes.erase(std::unique(hashes.begin(), hashes.end()), hashes.end());
  return hashes;
}

std::vector<uint64_t> sketch_sequence_stranded(const std::vector<uint8_t>& seq, size_t k, size_t sketch_size) {
  return sketch_impl<false>(seq, k, sketch_size);
}
std::vector<uint64_t> sketch_sequence_canonical(const std::vector<uint8_t>& seq, size_t k, size_t sketch_size) {
  return sketch_impl<true>(seq, k, sketch_size);
}

double jaccard(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {  // alignment.rs:125-139
  size_t i = 0, j = 0, inter = 0;
  while (i < a.size() && j < b.size()) {
    if (a[i] == b[j]) { ++inter; ++i; ++j; }
    else if (a[i] < b[j]) ++i;
    else ++j;
  }
  const size_t uni = a.size() + b.size() - inter;
  return uni == 0 ? 0.0 : (double)inter / (double)uni;
}

double mash_distance(double j, size_t k) {  // mash.rs:59-74
  if (j <= 0.0) return 1.0;
  const double ratio = (2.0 * j) / (1.0 + j);
  if (ratio <= 0.0) return 1.0;
  return (-1.0 / (double)k) * std::log(ratio);
}

template <typename F>
static void parallel_for(size_t n, int threads, F f) {
  const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), n));
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back([=]() { for (size_t i = n * t / T; i < n * (t + 1) / T; ++i) f(i); });
  for (auto& x : th) x.join();
}

std::vector<uint8_t> orient_pairs_mash(const std::vector<Sequence>& seqs, const std::pair<size_t, size_t>* pairs, size_t npairs,
                                       int threads) {
  constexpr size_t K = 15, S = 1000;  // alignment.rs:70-75
  std::vector<std::vector<uint64_t>> fwd(seqs.size()), rev(seqs.size());
  parallel_for(seqs.size(), threads, [&](size_t i) {
    fwd[i] = sketch_sequence_stranded(seqs[i].seq, K, S);
    rev[i] = sketch_sequence_stranded(reverse_complement(seqs[i].seq), K, S);
  });
  std::vector<uint8_t> is_rev(npairs, 0);
  parallel_for(npairs, threads, [&](size_t p) {
    const size_t q = pairs[p].first, t = pairs[p].second;
    const double jf = jaccard(fwd[q], fwd[t]), jr = jaccard(rev[q], fwd[t]);
    is_rev[p] = jf >= jr ? 0 : 1;  // forward wins ties (alignment.rs:89)
  });
  return is_rev;
}

static std::atomic<int> g_host_threads{8};
void set_host_threads(int threads) { g_host_threads.store(std::max(1, threads)); }
int host_threads() { return g_host_threads.load(); }

std::vector<std::vector<double>> compute_distance_matrix(const std::vector<Sequence>& seqs, size_t k, size_t sketch_size) {
  const size_t n = seqs.size();
  std::vector<std::vector<uint64_t>> sk(n);
  parallel_for(n, host_threads(), [&](size_t i) { sk[i] = sketch_sequence_canonical(seqs[i].seq, k, sketch_size); });
  std::vector<std::vector<double>> m(n, std::vector<double>(n, 0.0));
  for (size_t i = 0; i < n; ++i)
    for (size_t j = i + 1; j < n; ++j) m[i][j] = m[j][i] = mash_distance(jaccard(sk[i], sk[j]), k);
  return m;
}

static std::string matrix_header(const std::vector<Sequence>& seqs) {
  std::string out = "sequence";  // mash.rs:168-184
  for (const auto& s : seqs) { out += "\t"; out += s.id; }
  out += "\n";
  return out;
}
static void append_matrix_row(std::string& out, const std::string& id, const double* d, size_t n) {
  char buf[64];
  out += id;
  for (size_t j = 0; j < n; ++j) { snprintf(buf, sizeof(buf), "\t%.6f", d[j]); out += buf; }
  out += "\n";
}

std::string format_distance_matrix(const std::vector<Sequence>& seqs, const std::vector<std::vector<double>>& m) {
  std::string out = matrix_header(seqs);
  for (size_t i = 0; i < m.size(); ++i) append_matrix_row(out, seqs[i].id, m[i].data(), m[i].size());
  return out;
}

double compute_connectivity_probability(size_t n, double connectivity_prob) {  // iterator.rs:300-334
  if (n <= 1) return 1.0;
  const double x = std::min(std::max(connectivity_prob, 0.001), 0.999);
  if (n <= 10) return n == 2 ? 1.0 : n == 3 ? 0.8 : n == 4 ? 0.7 : n == 5 ? 0.6 : 0.5;
  const double nf = (double)n;
  const double c = -std::log(-std::log(x));
  const double p = (std::log(nf) + c) / nf;
  return std::min(std::max(p, 0.001), 1.0);
}

static inline bool keep_pair(const std::string& a, const std::string& b, double fraction) {  // iterator.rs:261-281
  const uint64_t h = default_hash_str(a + ":" + b);
  return (double)h / (double)UINT64_MAX < fraction;
}

std::vector<std::pair<size_t, size_t>> apply_random_sparsification(std::vector<std::pair<size_t, size_t>> pairs,
                                                                   double keep_fraction, const std::vector<Sequence>& seqs) {
  std::vector<std::pair<size_t, size_t>> out;
  for (const auto& p : pairs)
    if (keep_pair(seqs[p.first].id, seqs[p.second].id, keep_fraction)) out.push_back(p);
  return out;
}

std::vector<std::pair<size_t, size_t>> build_knn_graph(const std::vector<std::vector<double>>& d, size_t k, bool farthest) {
  const size_t n = d.size();  // knn_graph.rs:112-143 (Rust's sort_by is stable)
  std::vector<std::pair<size_t, size_t>> pairs;
  for (size_t i = 0; i < n; ++i) {
    std::vector<std::pair<double, size_t>> nb;
    for (size_t j = 0; j < n; ++j)
      if (j != i) nb.emplace_back(d[i][j], j);
    if (farthest) std::stable_sort(nb.begin(), nb.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    else std::stable_sort(nb.begin(), nb.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (size_t t = 0; t < std::min(k, nb.size()); ++t) pairs.emplace_back(i, nb[t].second);
  }
  return pairs;
}

std::vector<std::pair<size_t, size_t>> extract_tree_pairs(const std::vector<Sequence>& seqs, size_t k_nearest,
                                                          size_t k_farthest, double random_fraction, size_t kmer_size) {
  std::vector<std::pair<size_t, size_t>> all;  // knn_graph.rs:12-52
  if (seqs.size() < 2) return all;
  const auto dm = compute_distance_matrix(seqs, kmer_size, 1000);
  if (k_nearest > 0) { auto p = build_knn_graph(dm, k_nearest, false); all.insert(all.end(), p.begin(), p.end()); }
  if (k_farthest > 0) { auto p = build_knn_graph(dm, k_farthest, true); all.insert(all.end(), p.begin(), p.end()); }
  if (random_fraction > 0.0)
    for (size_t i = 0; i < seqs.size(); ++i)
      for (size_t j = 0; j < seqs.size(); ++j)
        if (i != j && keep_pair(seqs[i].id, seqs[j].id, random_fraction)) all.emplace_back(i, j);
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  return all;
}


// ---- device planning ------------------------------------------------------------------------------------------------------
namespace {
// one engine on the planning device for the duration of a call (no alignment arenas: it only sketches and hashes)
struct PlanEngine {
  awv_engine* e = nullptr;
  explicit PlanEngine(int device) {
    awv_engine_config cfg{};
    cfg.device = device;
    if (awv_engine_create(&cfg, &e) != AWV_OK)
      throw AlignmentError("plan device " + std::to_string(device) + ": " + awv_last_error());
  }
  ~PlanEngine() { awv_engine_destroy(e); }
  PlanEngine(const PlanEngine&) = delete;
  PlanEngine& operator=(const PlanEngine&) = delete;
  static void check(int rc, const char* what) {
    if (rc != AWV_OK) throw AlignmentError(std::string(what) + ": " + awv_last_error());
  }
  void upload(const std::vector<Sequence>& seqs) {
    if (seqs.size() > (size_t)INT32_MAX) throw AlignmentError("device planning: more than 2^31 - 1 sequences");
    std::vector<uint64_t> offs(seqs.size() + 1, 0);
    for (size_t i = 0; i < seqs.size(); ++i) offs[i + 1] = offs[i] + seqs[i].seq.size();
    std::vector<uint8_t> cat(offs.back() + 1);
    for (size_t i = 0; i < seqs.size(); ++i)
      if (!seqs[i].seq.empty()) memcpy(cat.data() + offs[i], seqs[i].seq.data(), seqs[i].seq.size());
    check(awv_engine_set_sequences(e, (int32_t)seqs.size(), cat.data(), offs.data()), "awv_engine_set_sequences");
  }
  std::vector<uint32_t> sketch(SketchKind kind, size_t k, size_t s, size_t n) {
    std::vector<uint32_t> sizes(n);
    check(awv_sketch(e, (int32_t)kind, (int32_t)k, (int32_t)s, sizes.data()), "awv_sketch");
    return sizes;
  }
  // bitmap rows of `words` 32-bit words: bit (i, j) set when the pair passes keep_pair(fraction)
  void keep_bits(const std::vector<Sequence>& seqs, double fraction, bool include_diag, std::vector<uint32_t>& bitmap) {
    std::vector<uint64_t> offs(seqs.size() + 1, 0);
    std::string ids;
    for (size_t i = 0; i < seqs.size(); ++i) { ids += seqs[i].id; offs[i + 1] = ids.size(); }
    bool all = false;
    const uint64_t t = keep_threshold(fraction, &all);
    check(awv_keep_pairs(e, (int32_t)seqs.size(), (const uint8_t*)ids.data(), offs.data(), t, all ? 1 : 0, include_diag ? 1 : 0,
                         bitmap.data()),
          "awv_keep_pairs");
  }
};

inline double jaccard_counts(size_t inter, size_t a, size_t b) {  // jaccard() from the counts (the same arithmetic)
  const size_t uni = a + b - inter;
  return uni == 0 ? 0.0 : (double)inter / (double)uni;
}
inline bool device_sketch_ok(size_t k, size_t s) { return k >= 1 && k <= AWV_PLAN_MAX_K && s >= 1 && s <= AWV_PLAN_MAX_S; }

// rows of counts at a time: at most 16 M entries (32 MiB) per block
inline size_t row_block(size_t n) { return std::max<size_t>(1, std::min<size_t>(n, ((size_t)16 << 20) / std::max<size_t>(n, 1))); }

// the set bits of an n x n bitmap, row-major
std::vector<std::pair<size_t, size_t>> bitmap_pairs(const std::vector<uint32_t>& bitmap, size_t n) {
  const size_t words = (n + 31) / 32;
  size_t total = 0;
  for (uint32_t w : bitmap) total += (size_t)__builtin_popcount(w);
  std::vector<std::pair<size_t, size_t>> out;
  out.reserve(total);
  for (size_t i = 0; i < n; ++i)
    for (size_t w = 0; w < words; ++w)
      for (uint32_t x = bitmap[i * words + w]; x; x &= x - 1) out.emplace_back(i, 32 * w + (size_t)__builtin_ctz(x));
  return out;
}
}  // namespace

std::vector<std::vector<uint64_t>> sketch_all(const std::vector<Sequence>& seqs, SketchKind kind, size_t k, size_t sketch_size,
                                              int device) {
  const size_t n = seqs.size();
  std::vector<std::vector<uint64_t>> out(n);
  auto host = [&]() {
    parallel_for(n, host_threads(), [&](size_t i) {
      out[i] = kind == SketchKind::Canonical ? sketch_sequence_canonical(seqs[i].seq, k, sketch_size)
               : kind == SketchKind::Forward ? sketch_sequence_stranded(seqs[i].seq, k, sketch_size)
                                             : sketch_sequence_stranded(reverse_complement(seqs[i].seq), k, sketch_size);
    });
    return out;
  };
  if (device < 0) return host();
  PlanEngine pe(device);
  if (!device_sketch_ok(k, sketch_size)) return host();
  if (n == 0) return out;
  pe.upload(seqs);
  pe.sketch(kind, k, sketch_size, n);
  std::vector<uint64_t> offs(n + 1);
  PlanEngine::check(awv_sketch_copy(pe.e, (int32_t)kind, offs.data(), nullptr), "awv_sketch_copy");
  std::vector<uint64_t> all(offs[n] + 1);
  PlanEngine::check(awv_sketch_copy(pe.e, (int32_t)kind, nullptr, all.data()), "awv_sketch_copy");
  for (size_t i = 0; i < n; ++i) out[i].assign(all.begin() + (ptrdiff_t)offs[i], all.begin() + (ptrdiff_t)offs[i + 1]);
  return out;
}

uint64_t keep_threshold(double fraction, bool* keep_all) {
  // keep_pair's predicate, the same expression: monotone in h, so {h : kept} = [0, T) for the least h it rejects
  auto kept = [&](uint64_t h) { return (double)h / (double)UINT64_MAX < fraction; };
  *keep_all = kept(UINT64_MAX);
  if (*keep_all) return UINT64_MAX;
  uint64_t lo = 0, hi = UINT64_MAX;  // kept(hi) is false
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (kept(mid)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

static void distance_rows(PlanEngine& pe, const std::vector<uint32_t>& sz, size_t k, size_t n,
                          const std::function<void(size_t row0, size_t nrows, const std::vector<double>& d)>& take) {
  const size_t R = row_block(n);
  std::vector<uint16_t> inter(R * n);
  std::vector<double> d(R * n);
  for (size_t r0 = 0; r0 < n; r0 += R) {
    const size_t nr = std::min(R, n - r0);
    PlanEngine::check(awv_sketch_rows(pe.e, AWV_SK_CANONICAL, (int32_t)r0, (int32_t)nr, inter.data()), "awv_sketch_rows");
    for (size_t r = 0; r < nr; ++r) {
      const size_t i = r0 + r;
      for (size_t j = 0; j < n; ++j)
        d[r * n + j] = j == i ? 0.0 : mash_distance(jaccard_counts(inter[r * n + j], sz[i], sz[j]), k);
    }
    take(r0, nr, d);
  }
}

std::vector<std::vector<double>> compute_distance_matrix(const std::vector<Sequence>& seqs, size_t k, size_t sketch_size, int device) {
  if (device < 0) return compute_distance_matrix(seqs, k, sketch_size);
  PlanEngine pe(device);
  if (!device_sketch_ok(k, sketch_size)) return compute_distance_matrix(seqs, k, sketch_size);
  const size_t n = seqs.size();
  std::vector<std::vector<double>> m(n, std::vector<double>(n, 0.0));
  if (n == 0) return m;
  pe.upload(seqs);
  const std::vector<uint32_t> sz = pe.sketch(SketchKind::Canonical, k, sketch_size, n);
  distance_rows(pe, sz, k, n, [&](size_t r0, size_t nr, const std::vector<double>& d) {
    for (size_t r = 0; r < nr; ++r) std::copy(d.begin() + (ptrdiff_t)(r * n), d.begin() + (ptrdiff_t)((r + 1) * n), m[r0 + r].begin());
  });
  return m;
}

void write_distance_matrix(const std::vector<Sequence>& seqs, size_t k, size_t sketch_size, int device,
                           const std::function<void(const std::string&)>& sink) {
  if (device < 0) { sink(format_distance_matrix(seqs, compute_distance_matrix(seqs, k, sketch_size))); return; }
  PlanEngine pe(device);
  if (!device_sketch_ok(k, sketch_size)) { sink(format_distance_matrix(seqs, compute_distance_matrix(seqs, k, sketch_size))); return; }
  const size_t n = seqs.size();
  sink(matrix_header(seqs));
  if (n == 0) return;
  pe.upload(seqs);
  const std::vector<uint32_t> sz = pe.sketch(SketchKind::Canonical, k, sketch_size, n);
  std::vector<std::string> text;
  distance_rows(pe, sz, k, n, [&](size_t r0, size_t nr, const std::vector<double>& d) {
    text.assign(nr, std::string());  // (formatting is most of the host's work: spread over the host threads)
    parallel_for(nr, host_threads(), [&](size_t r) { append_matrix_row(text[r], seqs[r0 + r].id, d.data() + r * n, n); });
    std::string block;
    for (const std::string& t : text) block += t;
    sink(block);
  });
}

std::vector<std::pair<size_t, size_t>> apply_random_sparsification(const std::vector<Sequence>& seqs, double keep_fraction,
                                                                   bool exclude_self, int device) {
  const size_t n = seqs.size();
  if (device < 0) {
    std::vector<std::pair<size_t, size_t>> all;
    for (size_t i = 0; i < n; ++i)
      for (size_t j = 0; j < n; ++j)
        if (!exclude_self || i != j) all.emplace_back(i, j);
    return apply_random_sparsification(std::move(all), keep_fraction, seqs);
  }
  PlanEngine pe(device);
  if (n == 0) return {};
  std::vector<uint32_t> bitmap(n * ((n + 31) / 32), 0);
  pe.keep_bits(seqs, keep_fraction, !exclude_self, bitmap);
  return bitmap_pairs(bitmap, n);
}

std::vector<std::pair<size_t, size_t>> extract_tree_pairs(const std::vector<Sequence>& seqs, size_t k_nearest, size_t k_farthest,
                                                          double random_fraction, size_t kmer_size, int device) {
  if (device < 0) return extract_tree_pairs(seqs, k_nearest, k_farthest, random_fraction, kmer_size);
  PlanEngine pe(device);
  const size_t n = seqs.size();
  if (n < 2) return {};
  // the integer ranking puts J = 0 (distance 1.0) behind every J > 0: it equals the host's order when the smallest
  // positive Jaccard of two sketches of <= 1,000 hashes, 1 / 1,999, is still nearer than 1.0 (k >= 7)
  const bool ranked_ok = device_sketch_ok(kmer_size, 1000) && mash_distance(1.0 / 1999.0, kmer_size) < 1.0;
  if (k_nearest > AWV_PLAN_MAX_KNN || k_farthest > AWV_PLAN_MAX_KNN || ((k_nearest || k_farthest) && !ranked_ok))
    return extract_tree_pairs(seqs, k_nearest, k_farthest, random_fraction, kmer_size);
  const size_t words = (n + 31) / 32;
  std::vector<uint32_t> bitmap(n * words, 0);
  if (random_fraction > 0.0) pe.keep_bits(seqs, random_fraction, false, bitmap);
  if (k_nearest > 0 || k_farthest > 0) {
    pe.upload(seqs);
    pe.sketch(SketchKind::Canonical, kmer_size, 1000, n);
    std::vector<int32_t> nearest(n * k_nearest + 1), farthest(n * k_farthest + 1);
    PlanEngine::check(awv_sketch_knn(pe.e, AWV_SK_CANONICAL, (int32_t)k_nearest, (int32_t)k_farthest, nearest.data(), farthest.data()),
                      "awv_sketch_knn");
    auto mark = [&](const std::vector<int32_t>& v, size_t k) {
      for (size_t i = 0; i < n; ++i)
        for (size_t t = 0; t < k; ++t) {
          const int32_t j = v[i * k + t];
          if (j >= 0 && (size_t)j < n) bitmap[i * words + (size_t)j / 32] |= 1u << (j & 31);
        }
    };
    mark(nearest, k_nearest);
    mark(farthest, k_farthest);
  }
  return bitmap_pairs(bitmap, n);
}

std::vector<uint8_t> orient_pairs_mash(const std::vector<Sequence>& seqs, const std::pair<size_t, size_t>* pairs, size_t npairs,
                                       int threads, int device) {
  if (device < 0) return orient_pairs_mash(seqs, pairs, npairs, threads);
  constexpr size_t K = 15, S = 1000;  // alignment.rs:70-75
  PlanEngine pe(device);
  std::vector<uint8_t> is_rev(npairs, 0);
  if (npairs == 0) return is_rev;
  const size_t n = seqs.size();
  std::vector<int32_t> q(npairs), t(npairs);
  for (size_t p = 0; p < npairs; ++p) {
    if (pairs[p].first >= n || pairs[p].second >= n) throw AlignmentError("orient_pairs_mash: sequence index out of range");
    q[p] = (int32_t)pairs[p].first;
    t[p] = (int32_t)pairs[p].second;
  }
  pe.upload(seqs);
  const std::vector<uint32_t> sf = pe.sketch(SketchKind::Forward, K, S, n), sr = pe.sketch(SketchKind::RevComp, K, S, n);
  std::vector<uint16_t> cf(npairs), cr(npairs);
  PlanEngine::check(awv_sketch_pair_counts(pe.e, AWV_SK_FORWARD, AWV_SK_FORWARD, q.data(), t.data(), (int64_t)npairs, cf.data()),
                    "awv_sketch_pair_counts");
  PlanEngine::check(awv_sketch_pair_counts(pe.e, AWV_SK_REVCOMP, AWV_SK_FORWARD, q.data(), t.data(), (int64_t)npairs, cr.data()),
                    "awv_sketch_pair_counts");
  parallel_for(npairs, threads, [&](size_t p) {
    const double jf = jaccard_counts(cf[p], sf[q[p]], sf[t[p]]), jr = jaccard_counts(cr[p], sr[q[p]], sf[t[p]]);
    is_rev[p] = jf >= jr ? 0 : 1;  // forward wins ties (alignment.rs:89)
  });
  return is_rev;
}

double predicted_pair_cost(size_t qlen, size_t tlen, const AlignmentParams& params) {
  const double lo = (double)std::min(qlen, tlen), g = (double)(qlen > tlen ? qlen - tlen : tlen - qlen);
  double gap = 0;
  if (g > 0) {
    gap = params.gap_open + g * params.gap_extend;
    if (params.gap2_open && params.gap2_extend) gap = std::min(gap, (double)*params.gap2_open + g * (double)*params.gap2_extend);
  }
  const double s = 0.06 * params.mismatch_penalty * lo + gap + 16.0;  // ~6 % of the bases pay a mismatch's worth
  return s * s;
}

std::vector<uint32_t> assign_shards_lpt(const std::vector<double>& cost, size_t world) {
  const size_t n = cost.size();
  std::vector<uint32_t> shard(n, 0);
  if (world <= 1 || n == 0) return shard;
  bool uniform = true;
  for (size_t i = 1; i < n && uniform; ++i) uniform = cost[i] == cost[0];
  if (uniform) {  // LPT on equal costs is the strided shard
    for (size_t i = 0; i < n; ++i) shard[i] = (uint32_t)(i % world);
    return shard;
  }
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
  // min-heap of (load, rank)
  typedef std::pair<double, uint32_t> LR;
  std::priority_queue<LR, std::vector<LR>, std::greater<LR>> heap;
  for (size_t r = 0; r < world; ++r) heap.push(LR(0.0, (uint32_t)r));
  for (size_t k = 0; k < n; ++k) {
    LR top = heap.top();
    heap.pop();
    shard[order[k]] = top.second;
    top.first += cost[order[k]];
    heap.push(top);
  }
  return shard;
}

std::vector<std::vector<size_t>> device_batches(const std::vector<double>& cost, size_t slots, size_t min_batch_pairs) {
  const size_t n = cost.size(), m = std::max<size_t>(1, min_batch_pairs);
  const size_t nb = std::max<size_t>(1, std::min(4 * std::max<size_t>(1, slots), (n + m - 1) / m));
  const std::vector<uint32_t> batch = assign_shards_lpt(cost, nb);
  std::vector<std::vector<size_t>> out(nb);
  for (size_t i = 0; i < n; ++i) out[batch[i]].push_back(i);
  return out;
}

}  // namespace planner
}  // namespace allwave
