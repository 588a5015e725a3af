// gaml_oracle.hpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// CPU restatement of the GAML assembly-likelihood hot path, written from the
// reference's algorithm (not its text), single-threaded like the reference.
// Every function cites the reference file:line (relative to /root/reference)
// whose behaviour it restates.
//
// PARITY PINNING STATUS
//   * logdouble arithmetic  : PINNED  -- oracle/_ref builds a driver that includes the
//     reference's own logdouble.hpp / utility.h in place (they need only libm) and
//     tests/test_oracle_ref.py checks this restatement against it bit for bit.
//   * graph.cc scoring/alignment stages : PARITY UNPINNED.  graph.cc / graph.h /
//     prob_calculator.h include Boost (graph.h:5, graph.cc:6-12), Boost is absent
//     from this image and a stand-in Boost is not allowed, so the reference
//     translation units cannot be built here; the reference ships no tests,
//     golden vectors or fixtures for this path.  What pins
//     this file is therefore (a) line-by-line review against the cited reference
//     lines, (b) the committed golden fixtures under tests/golden produced by THIS
//     oracle (regression pins, not reference pins), (c) agreement with the
//     independently structured product host logic + HIP kernels, (d) for the paired
//     term alone: exact arithmetic at 60 digits on hand-made records
//     (tests/test_crafted_records_host.py; orc_put_window_records files them).
//
// Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it.
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <fstream>
#include <limits>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

namespace orc {

// ---------------------------------------------------------------------------
// L1 numeric primitive: log-space double (logdouble.hpp:13-78)
// ---------------------------------------------------------------------------
struct LogD {
  double lv;                                              // logdouble.hpp:15
  LogD() : lv(-std::numeric_limits<double>::infinity()) {}  // :17 (zero probability)
  static LogD from_linear(double x) { LogD r; r.lv = std::log(x); return r; }  // :18
  static LogD from_log(double l) { LogD r; r.lv = l; return r; }
};
inline bool is_neg_inf(double v) { return std::isinf(v) && v < 0; }
// operator+ / operator+= (logdouble.hpp:20-30, 37-47): -inf short-circuits, else
// max + log1p(exp(min - max)).
inline LogD ld_add(const LogD& a, const LogD& b) {
  if (is_neg_inf(a.lv)) return b;
  if (is_neg_inf(b.lv)) return a;
  double hi = std::max(a.lv, b.lv), lo = std::min(a.lv, b.lv);
  return LogD::from_log(hi + std::log1p(std::exp(lo - hi)));
}
inline LogD ld_mul(const LogD& a, const LogD& b) { return LogD::from_log(a.lv + b.lv); }  // :49-53
inline LogD ld_pow(const LogD& a, double e) { return LogD::from_log(a.lv * e); }          // :55-59
inline LogD ld_div(const LogD& a, const LogD& b) { return LogD::from_log(a.lv - b.lv); }  // :61-65
inline bool ld_lt(const LogD& a, const LogD& b) { return a.lv < b.lv; }                   // :72-74

// utility.h:28-38 InvertPath: reverse order, flip strand bit of nodes, keep gaps.
inline std::vector<int> invert_walk(const std::vector<int>& w) {
  std::vector<int> r;
  for (int i = (int)w.size() - 1; i >= 0; i--) r.push_back(w[i] >= 0 ? (w[i] ^ 1) : w[i]);
  return r;
}

// hash of a node-id walk, same mixing as graph.h:21-45 (only iteration order of the
// hashed containers depends on it; no result does).
struct WalkHash {
  size_t operator()(const std::vector<int>& v) const {
    size_t seed = 0;
    for (int x : v) seed ^= std::hash<int>()(x) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
    return seed;
  }
};

// ---------------------------------------------------------------------------
// Graph model: only what the hot path reads (graph.h:74-80, 233-273; graph.cc:52-106)
// ---------------------------------------------------------------------------
struct Graph {
  std::vector<std::string> seq;          // nodes[i]->s ; twin of i is i^1
  std::vector<int> normalize_map;        // graph.h:247-266
  int len(int node) const { return (int)seq[node].size(); }
  void calc_normalize_map();
  void normalize_walk(std::vector<int>& w) const {  // graph.h:268-273
    for (auto& x : w) if (x >= 0) x = normalize_map[x];
  }
};
// Velvet LastGraph reader (graph.cc:52-106). Arcs are parsed and counted but the
// hot path never uses adjacency, so they are not stored.
bool load_lastgraph(const std::string& file, Graph& g, int* n_arcs = nullptr);

inline char comp_base(char a) {  // graph.h:58-64
  switch (a) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; }
  return a;
}
inline std::string revcomp(const std::string& s) {  // graph.h:66-72
  std::string r; r.reserve(s.size());
  for (int i = (int)s.size() - 1; i >= 0; i--) r += comp_base(s[i]);
  return r;
}

// Aligment record (graph.h:211-231): 4 x int32, ordered by (position, read_id).
struct Rec {
  int32_t pos, edit, read, orient;
  bool operator<(const Rec& o) const { return pos == o.pos ? read < o.read : pos < o.pos; }
};

constexpr int kWindowTail = 300;   // kMinSubpathLength graph.cc:27
constexpr int kSeedLen = 15;       // kIndexKmer graph.cc:33
constexpr double kCovEventMinProb = 1e-15;  // kThresholdProb2 graph.cc:25

// ---------------------------------------------------------------------------
// Max-hash read index (ReadIndexMinHash, graph.cc:1243-1348, graph.h:324-342)
// ---------------------------------------------------------------------------
struct MaxHashIndex {
  std::unordered_map<uint64_t, std::vector<int>> buckets;  // read_index_
  int read_len = 0;                                        // last added read's length (:1286)
  static int code(char c) {  // graph.h:326-331; other characters: the reference leaves
    switch (c) { case 'A': return 1; case 'T': return 2; case 'C': return 3; case 'G': return 0; }
    return 0;                // trans[] uninitialised -> treated as 0 here (documented)
  }
  static uint64_t mix(uint64_t x) { return x ^ 0x2204abcdULL; }  // :1243-1252
  static bool acgt_only(const std::string& s);                    // CheckRead :1271-1278
  static uint64_t max_hash(const std::string& s);                 // GetMinHashForSeq :1254-1269
  void add_read(const std::string& s, int id);                    // :1280-1287
  void window_hashes(const std::string& s, std::vector<std::pair<uint64_t, int>>& out) const;  // :1289-1323
  void candidates(const std::string& s, std::unordered_map<int, std::vector<int>>& out) const;  // :1325-1348
};

// seed extension by 0-1 BFS (ProcessHit, graph.cc:730-837). Returns errors (-1 = no
// alignment), 0-based first and last window index covered by the read.
struct HitResult { int errs, begin, end; };
HitResult extend_hit(int win_pos, int read_pos, const std::string& read, const std::string& win);

// ---------------------------------------------------------------------------
// Short-read set (ReadSet, graph.h:344-442)
// ---------------------------------------------------------------------------
struct ShortReadSet {
  double match_p = 0, mismatch_p = 0;           // match_prob_, mismatch_prob_
  std::vector<double> match_pow, mismatch_pow;  // match_probs_/mismatch_probs_ (:1448-1453)
  std::vector<std::string> reads;               // read_seqs_
  std::vector<int> lens;                        // read_lens_
  int max_len = 0;
  MaxHashIndex index;
  std::unordered_map<std::vector<int>, std::vector<Rec>, WalkHash> cache;  // aligment_cache_
  std::vector<std::vector<std::pair<int, std::pair<int, int>>>> positions;  // positions_ (single-end)
  std::vector<uint8_t> several;  // (not in the reference) add_positions met a second distinct alignment of the read
  long windows_aligned = 0;

  int n() const { return (int)reads.size(); }
  // FASTQ load = PreprocessReads (:1386-1415) + PrepareReadIndex (:1366-1384); reads get
  // ids in order of first appearance (graph.h:410-420). Names are not kept.
  bool load_fastq(const std::string& file);
  void set_reads(const std::vector<std::string>& r);
  void finalize();  // CalcMaxReadLen + index build

  std::string window_string(const Graph& g, const std::vector<int>& w, int* offset) const;  // :846-857
  void align_window(const Graph& g, const std::vector<int>& w);                // AlignSubpathInternal :839-899
  void align_windows(const Graph& g, const std::vector<std::vector<int>>& ws);  // PrecomputeAligmentForSubpaths :911-922
  void precompute_for_paths(const Graph& g, const std::vector<std::vector<int>>& paths);  // :447-493
  void missing_windows_of_contig(const Graph& g, const std::vector<int>& ctg,
                                 std::unordered_set<std::vector<int>, WalkHash>& out) const;  // GetSubpathsFromPath :495-533
  // GetPositionsOnlyPath (:535-598)
  void positions_only_path(const Graph& g, const std::vector<int>& ctg, int st,
                           std::unordered_map<int, std::vector<Rec>>& acc);
  // AddPositions (:600-649); cache miss = no alignments
  void add_positions(const Graph& g, const std::vector<int>& ctg, int& total_len, int st);
  void clear_positions();  // :316-321
  double base_prob(int read, int edit) const {  // m^e * M^(L-e), e.g. :1859-1860
    return mismatch_pow[edit] * match_pow[lens[read] - edit];
  }
};

double insert_prob(double len, double mean, double sd);  // GetInsertProbability :1593-1598

struct PairedState {  // ScoringState graph.h:612-619
  std::vector<std::vector<int>> old_paths;
  int bad_bases = 0;
  std::vector<double> probs;
};

struct PathScore {  // what CalcScoreForPathInc emits (:1794-1920)
  int bad_bases = 0;
  std::vector<std::pair<int, double>> changes;
};

void path_changes(const std::vector<std::vector<int>>& now, const std::vector<std::vector<int>>& old,
                  std::vector<std::vector<int>>& erased, std::vector<std::vector<int>>& added);  // GetChanges :1745-1764
int walk_len(const Graph& g, const std::vector<int>& w);                  // GetPathLen :1766-1773
int total_walk_len(const Graph& g, const std::vector<std::vector<int>>& p);  // GetTotalLen :1775-1781

void score_path_paired(const Graph& g, const std::vector<int>& path, ShortReadSet& r1, ShortReadSet& r2,
                       double ins_mean, double ins_sd, double cov_move, bool all_to_cov,
                       double floor_per_base, double floor_start, PathScore& out);  // :1794-1920
double total_prob_paired(const std::vector<double>& probs, int total_len, int& zero_reads,
                         double floor_per_base, double floor_start,
                         const ShortReadSet& r1, const ShortReadSet& r2);  // GetTotalProb :1495-1516
double total_prob_single(const std::vector<double>& probs, int total_len, int& zero_reads,
                         double floor_per_base, double floor_start, const ShortReadSet& r);  // :1518-1537

// CalcScoreForPathsNew (:1952-1989)
double score_paired(const Graph& g, const std::vector<std::vector<int>>& paths, ShortReadSet& r1,
                    ShortReadSet& r2, double ins_mean, double ins_sd, int& zero_reads, int& total_len,
                    PairedState& st, double penalty, double cov_move, bool all_to_cov,
                    double floor_per_base, double floor_start);
// the slow, non-incremental paired CalcScoreForPaths (:1991-2127; unreachable from gaml: a cross-check)
double score_paired_slow(const Graph& g, const std::vector<std::vector<int>>& paths, ShortReadSet& r1, ShortReadSet& r2,
                         double ins_mean, double ins_sd, int& zero_reads, int& total_len, double penalty, double cov_move,
                         bool all_to_cov, double floor_per_base, double floor_start, std::vector<double>* probs_out = nullptr,
                         int* bad_bases_out = nullptr, std::vector<uint8_t>* several_out = nullptr);
// CalcScoreForPaths single (:1650-1743)
double score_single(const Graph& g, const std::vector<std::vector<int>>& paths, ShortReadSet& r,
                    int& zero_reads, int& total_len, double penalty, double cov_move,
                    double floor_per_base, double floor_start, std::vector<double>* probs_out = nullptr,
                    int* bad_bases_out = nullptr);

// ---------------------------------------------------------------------------
// PacBio read set (PacbioReadSet graph.h:444-593), scoring side only
// ---------------------------------------------------------------------------
struct LongRec { int32_t pos, pos_end, read; LogD prob; };  // PacbioAligment graph.h:516-535

struct SamAlignment {  // PacbioAligmentData graph.h:499-514
  std::string name; int flags = 0, len = 0, posstart = 0, posend = 0, sstart = 0, send = 0, slen = 0,
      tstart = 0, tend = 0, edit_dist = 0;
  std::vector<std::pair<int, char>> cigar;
};

struct LongReadSet {
  LogD match_p, mismatch_p;        // logdouble(match_prob), logdouble(mismatch_prob) graph.h:446-449
  std::vector<int> lens;
  std::vector<std::string> reads;  // read_seq_ (only the banded DP needs bases)
  std::unordered_map<std::string, int> name_to_id;  // read_map_
  int max_len = 0;
  std::unordered_map<std::vector<int>, std::vector<LongRec>, WalkHash> cache;
  long cache_misses = 0;
  int n() const { return (int)lens.size(); }
  void set_params(double match, double mismatch) {
    match_p = LogD::from_linear(match); mismatch_p = LogD::from_linear(mismatch);
  }
  void finalize() { max_len = 0; for (int l : lens) max_len = std::max(max_len, l); }  // :1456-1461
  LogD min_read_prob(int i) const {  // GetMinReadProb graph.h:478-481
    return ld_mul(ld_pow(mismatch_p, lens[i] * 0.25), ld_pow(match_p, lens[i] * 0.75));
  }
  // GetReadProbabilities (:2410-2503); a sub-walk missing from the cache is where the
  // reference shells out to BLASR -- here it counts a miss and contributes nothing.
  void read_probabilities(const Graph& g, const std::vector<int>& path, int& total_len,
                          std::vector<std::vector<std::pair<std::pair<int, int>, LogD>>>& out);
  // ParseCigar (:3023-3038), ParseAligment (:2945-3021), AligmentProbability (:2129-2297)
  static std::vector<std::pair<int, char>> parse_cigar(const std::string& c);
  static SamAlignment parse_sam_line(const std::string& line, int total_len, bool do_reverse = true);
  LogD pair_match(char a, char b) const;  // MatchProbability graph.h:555-564
  // GetReadProbabilitiesSlow (graph.cc:2650-2795) from the point where BLASR's SAM output exists:
  // every SAM line -> banded alignment probability -> record filed under the sub-walk it spans.
  // Returns the number of records filed.
  int ingest_sam(const Graph& g, const std::vector<int>& path, const std::vector<std::string>& sam_lines);
  static std::vector<std::pair<int, int>> dp_cells(const SamAlignment& a, int band = 2);  // cell list graph.cc:2183-2221
  LogD alignment_probability(const std::string& s1, const std::string& s2, const SamAlignment& a,
                             int band = 2) const;
};

double total_prob_pacbio(const std::vector<LogD>& probs, int total_len, const LongReadSet& r,
                         int& zero_reads, double floor_per_base, double floor_start);  // :3062-3088
// CalcScoreForPacbio (:3171-3261)
double score_pacbio(const Graph& g, std::vector<std::vector<int>> paths, LongReadSet& r, int& zero_reads,
                    int& total_len, double penalty, double cov_move, double floor_per_base,
                    double floor_start, std::vector<double>* logprobs_out = nullptr,
                    int* bad_bases_out = nullptr);

// ---------------------------------------------------------------------------
// Read-set configs + aggregation (prob_calculator.h:7-124) and config files
// (gaml.cc:32-88, 737-872)
// ---------------------------------------------------------------------------
struct SingleCfg { double penalty_constant = 0, step = 50, min_prob_per_base = -0.7, min_prob_start = -10,
                   weight = 1; bool advice = false; };
struct PairedCfg { double penalty_constant = 0, step = 0, insert_mean = 0, insert_std = 0,
                   min_prob_per_base = -0.7, min_prob_start = -10, weight = 1; bool advice = false; };

struct Calculator {  // ProbCalculator prob_calculator.h:37-124
  Graph* g = nullptr;
  std::vector<std::pair<SingleCfg, ShortReadSet*>> single;
  std::vector<std::pair<PairedCfg, std::pair<ShortReadSet*, ShortReadSet*>>> paired;
  std::vector<std::pair<SingleCfg, LongReadSet*>> pacbio;
  std::vector<PairedState> paired_state;
  // fresh=true resets every PairedState first (= the reference evaluated with a fresh
  // ScoringState; this is the parity target of the HIP path).
  double calc_prob(const std::vector<std::vector<int>>& paths, std::vector<std::pair<int, int>>& zeros,
                   int& total_len, bool fresh);
};

using KV = std::unordered_map<std::string, std::string>;
bool load_config(const std::string& file, KV& global, std::unordered_map<std::string, KV>& sets);  // gaml.cc:748-780
struct ReadSetSpec {
  std::string name, type, file1, file2; double mismatch = 0.01, match = 0.96;
  SingleCfg scfg; PairedCfg pcfg;
};
// PrepareReadSetFromConfig (gaml.cc:783-872) minus file loading; keeps the quirks
// (min_prob_pre_base for paired sets, step = insert_mean - penalty_step, hash-order).
std::vector<ReadSetSpec> readsets_from_config(std::unordered_map<std::string, KV>& sets);

}  // namespace orc
