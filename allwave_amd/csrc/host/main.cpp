// main.cpp -- `allwave_hip`: command-line driver with the reference's flags (src/main.rs:30-80) over
// the MI355X engine.  FASTA in (plain, or .gz/BGZF through zlib), PAF out.  SURVEY.md 8f-1.
//   -i/--input  -o/--output  -s/--scores  -x/--preset  -t/--threads  -p/--sparsification
//   --no-progress  --mash-matrix  --wfa-orientation  -k/--keep-prefixes  -e/--exclude-prefixes
// Extensions: --device N (GPU ordinal), --devices LIST (several GPUs, or engines, in this one process),
// --shard R/N (this process's part of the pair list), --forward-only (skip orientation: all '+'),
// --wfa-orientation-full (WFA orientation by two full alignments per pair, the reference's method, instead of bounded scores),
// --score-only (penalties instead of PAF: WFA2's ComputeScore scope) with an optional --max-penalty N bound,
// --max-align-penalty N / --max-divergence D (full alignments under a bound: pairs above it are abandoned early and left out),
// --verify (check every alignment on the device before it is written; exit status 4 when one fails),
// --check-paf FILE [--check-optimal] [--partial] (check an existing PAF against the FASTA on the device; nothing is aligned),
// --align-paf FILE (align the interval pairs columns 1-9 of each line of FILE name, globally: mappings in, PAF with cg:Z: out).
// -t sets the host threads used for PAF formatting / sketching (alignment itself runs on the GPU).
#include <zlib.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "allwave.hpp"
#include "bed.hpp"
#include "planner.hpp"

using namespace allwave;

namespace {

struct Args {
  std::string input, output, scores = "0,5,8,2,24,1", preset, sparsification = "giant:0.99", keep, exclude;
  bool have_output = false, have_scores = false, have_preset = false, no_progress = false, mash_matrix = false;
  bool wfa_orientation = false, wfa_orientation_full = false, forward_only = false, have_keep = false, have_exclude = false;
  int threads = 1, device = 0;
  bool have_device = false;
  std::string devices;  // --devices LIST (empty: --device)
  bool have_devices = false;
  long shard_rank = 0, shard_world = 1;  // --shard R/N: this process aligns pairs R, R+N, ... (one process per GPU)
  bool score_only = false;  // --score-only: one line `qname qlen tname tlen strand penalty` per pair instead of PAF
  long max_penalty = -1;    // --max-penalty N (with --score-only): pairs whose penalty exceeds N are left out
  bool have_max_penalty = false;
  long max_align_penalty = -1;  // --max-align-penalty N: alignments whose penalty exceeds N are abandoned and left out
  double max_divergence = -1.0; // --max-divergence D: alignments with (#X + #I + #D) > D * columns are left out
  bool have_max_align_penalty = false, have_max_divergence = false;
  int plan_device = -1;     // --plan-device N: plan the pair list, the mash matrix and mash orientation on device N
  bool verify = false;      // --verify: awv_align_pairs_verified; `verified N pairs, F failed, K ms` on the summary line
  std::string check_paf;    // --check-paf FILE: check that PAF against the input instead of aligning
  bool have_check_paf = false, check_optimal = false;
  bool partial = false;     // --partial (with --check-paf): lines over a proper interval are checked as that interval pair
  std::string align_paf;    // --align-paf FILE: align the interval pairs that PAF names instead of a planned pair list
  bool have_align_paf = false, have_sparsification = false, have_shard = false;
  long clip = 0, clip_min_score = 1;  // --clip A: every alignment clipped to its best-scoring segment under the match bonus A
  bool have_clip = false, have_clip_min_score = false;
  long split = 0, split_min_score = 0;  // --split A --split-min-score S: every alignment split into all its segments that score at least S
  bool have_split = false, have_split_min_score = false;
  int normalize = AWV_NORM_OFF;  // --normalize left|right: every alignment's gap runs moved to their left- / right-normal place
  bool have_normalize = false;
  bool device_cigar = false;  // --device-cigar: the run-length text behind cg:Z: is made on the device
  int cs = 0;                 // --cs short|long: every line gains minimap2's cs:Z: tag, made on the device (0: off)
  std::string coverage;       // --coverage FILE: the per-base depth of what was aligned, accumulated on the device
  bool have_coverage = false;
  int coverage_of = AWV_COV_BOTH;  // --coverage-of target|query|both
  bool have_coverage_of = false;
  std::string variants;       // --variants FILE: the per-site allele table of what was aligned, tallied on the device
  bool have_variants = false;
  long variants_min_count = 1;  // --variants-min-count N: rows with a smaller count are not written
  bool have_variants_min_count = false;
  std::string liftover;       // --liftover BED: the regions lifted through what was aligned, on the device
  std::string liftover_out;   // --liftover-out FILE: one line per lifted region and alignment
  bool have_liftover = false, have_liftover_out = false, have_liftover_from = false;
  int liftover_from = AWV_LIFT_FROM_TARGET;  // --liftover-from target|query|both
  std::string msa;                        // --msa FILE: the targets' multiple alignments as aligned FASTA ({}: the target's index)
  std::vector<std::string> msa_targets;   // --msa-target NAME (repeatable), or all
  unsigned long long msa_max_bytes = 1ull << 30;  // --msa-max-bytes N
  bool have_msa = false, have_msa_max_bytes = false;
};

[[noreturn]] void die(const std::string& m, int code = 2) {
  std::cerr << "error: " << m << "\n";
  std::exit(code);
}

// parse_ani_preset (main.rs:83-124)
std::string parse_ani_preset(const std::string& preset) {
  double ani = 0;
  auto parse = [](const std::string& t, double& v) {
    size_t used = 0;
    try { v = std::stod(t, &used); } catch (...) { return false; }
    return used == t.size() && !t.empty();
  };
  if (preset.find('.') != std::string::npos) {
    double v;
    if (!parse(preset, v) || !(v > 0.0 && v <= 1.0)) die("Invalid ANI value: " + preset + ". Use 0.5-1.0 or 50%-100%");
    ani = v * 100.0;
  } else if (!preset.empty() && preset.back() == '%') {
    double v;
    if (!parse(preset.substr(0, preset.size() - 1), v) || !(v >= 50.0 && v <= 100.0)) die("Invalid ANI percentage: " + preset + ". Use 50%-100%");
    ani = v;
  } else {
    double v;
    if (!parse(preset, v) || !(v >= 50.0 && v <= 100.0)) die("Invalid ANI percentage: " + preset + ". Use 50%-100% or 50-100");
    ani = v;
  }
  if (ani >= 95.0) return "0,7,12,2,36,1";
  if (ani >= 85.0) return "0,5,8,2,24,1";
  if (ani >= 75.0) return "0,4,6,2,18,1";
  if (ani >= 65.0) return "0,3,4,1";
  return "0,1,1,1";
}

// FASTA: id = first word of the header, sequence bytes verbatim (no upper-casing), any line width
std::vector<Sequence> read_fasta(const std::string& path) {
  std::vector<Sequence> seqs;
  gzFile f = gzopen(path.c_str(), "rb");  // transparently reads plain files, gzip and BGZF
  if (!f) die("cannot open " + path, 1);
  gzbuffer(f, 1 << 20);
  std::string line;
  std::vector<char> buf(1 << 16);
  bool have = false;
  auto handle = [&](const std::string& l) {
    if (!l.empty() && l[0] == '>') {
      Sequence s;
      size_t e = l.find_first_of(" \t", 1);
      s.id = l.substr(1, e == std::string::npos ? std::string::npos : e - 1);
      seqs.push_back(std::move(s));
      have = true;
    } else if (have) {
      seqs.back().seq.insert(seqs.back().seq.end(), l.begin(), l.end());
    }
  };
  while (gzgets(f, buf.data(), (int)buf.size())) {
    const size_t n = strlen(buf.data());
    line.append(buf.data(), n);
    if (n && buf[n - 1] == '\n') {
      while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
      handle(line);
      line.clear();
    }
  }
  if (!line.empty()) handle(line);
  gzclose(f);
  return seqs;
}

std::vector<std::string> split_trim(const std::string& s) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string t;
  while (std::getline(ss, t, ',')) {
    size_t b = t.find_first_not_of(" \t"), e = t.find_last_not_of(" \t");
    out.push_back(b == std::string::npos ? "" : t.substr(b, e - b + 1));
  }
  return out;
}

// --devices LIST: comma-separated ordinals and ranges A-B (A <= B), e.g. 0,1,2 / 0-7 / 0,0; `all` = every visible device.
// Returns false with a message on a malformed list (before any device is opened).
bool parse_devices(const std::string& list, std::vector<int>& out, std::string& msg) {
  out.clear();
  if (list == "all") {
    try {
      const int n = std::min(256, visible_device_count());
      for (int d = 0; d < n; ++d) out.push_back(d);
    } catch (const std::exception& e) {
      msg = std::string("--devices all: ") + e.what();
      return false;
    }
    return true;
  }
  auto ordinal = [](const std::string& t, int& v) {
    if (t.empty() || t.size() > 6 || t.find_first_not_of("0123456789") != std::string::npos) return false;
    v = atoi(t.c_str());
    return true;
  };
  for (const std::string& tok : split_trim(list)) {
    const size_t dash = tok.find('-');
    int a = 0, b = 0;
    if (dash == std::string::npos ? !ordinal(tok, a) : !(ordinal(tok.substr(0, dash), a) && ordinal(tok.substr(dash + 1), b))) {
      msg = "--devices: '" + tok + "' is not a device ordinal or range A-B (LIST: e.g. 0,1,2 or 0-7 or 0,0 or all)";
      return false;
    }
    if (dash == std::string::npos) b = a;
    if (a > b) {
      msg = "--devices: empty range '" + tok + "' (A-B needs A <= B)";
      return false;
    }
    if (b - a >= 256 || out.size() + (size_t)(b - a) >= 256) {  // (one engine and one submitter thread per entry)
      msg = "--devices: more than 256 entries";
      return false;
    }
    for (int d = a; d <= b; ++d) out.push_back(d);
  }
  if (out.empty()) {
    msg = "--devices: the device list is empty (LIST: e.g. 0,1,2 or 0-7 or 0,0 or all)";
    return false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  for (int i = 1; i < argc; ++i) {
    const std::string k = argv[i];
    auto val = [&]() -> std::string {
      if (i + 1 >= argc) die("missing value for " + k);
      return argv[++i];
    };
    if (k == "-i" || k == "--input") a.input = val();
    else if (k == "-o" || k == "--output") { a.output = val(); a.have_output = true; }
    else if (k == "-s" || k == "--scores") { a.scores = val(); a.have_scores = true; }
    else if (k == "-x" || k == "--preset") { a.preset = val(); a.have_preset = true; }
    else if (k == "-t" || k == "--threads") a.threads = std::max(1, atoi(val().c_str()));
    else if (k == "-p" || k == "--sparsification") { a.sparsification = val(); a.have_sparsification = true; }
    else if (k == "--no-progress") a.no_progress = true;
    else if (k == "--mash-matrix") a.mash_matrix = true;
    else if (k == "--wfa-orientation") a.wfa_orientation = true;
    else if (k == "--wfa-orientation-full") a.wfa_orientation = a.wfa_orientation_full = true;
    else if (k == "--forward-only") a.forward_only = true;
    else if (k == "-k" || k == "--keep-prefixes") { a.keep = val(); a.have_keep = true; }
    else if (k == "-e" || k == "--exclude-prefixes") { a.exclude = val(); a.have_exclude = true; }
    else if (k == "--device") { a.device = atoi(val().c_str()); a.have_device = true; }
    else if (k == "--devices") { a.devices = val(); a.have_devices = true; }
    else if (k == "--score-only") a.score_only = true;
    else if (k == "--verify") a.verify = true;
    else if (k == "--check-paf") { a.check_paf = val(); a.have_check_paf = true; }
    else if (k == "--check-optimal") a.check_optimal = true;
    else if (k == "--partial") a.partial = true;
    else if (k == "--align-paf") { a.align_paf = val(); a.have_align_paf = true; }
    else if (k == "--plan-device") {
      const std::string v = val();
      if (v.empty() || v.size() > 6 || v.find_first_not_of("0123456789") != std::string::npos) die("--plan-device expects a device ordinal N >= 0");
      a.plan_device = atoi(v.c_str());
    }
    else if (k == "--max-penalty") {
      const std::string v = val();
      char* end = nullptr;
      a.max_penalty = strtol(v.c_str(), &end, 10);
      if (v.empty() || !end || *end != 0 || a.max_penalty < 0 || a.max_penalty > INT32_MAX) die("--max-penalty expects a penalty N >= 0");
      a.have_max_penalty = true;
    }
    else if (k == "--max-align-penalty") {
      const std::string v = val();
      char* end = nullptr;
      a.max_align_penalty = strtol(v.c_str(), &end, 10);
      if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || !end || *end != 0 || a.max_align_penalty > INT32_MAX)
        die("--max-align-penalty expects a penalty N >= 0");
      a.have_max_align_penalty = true;
    }
    else if (k == "--split" || k == "--split-min-score") {
      const std::string v = val();
      char* end = nullptr;
      const long n = strtol(v.c_str(), &end, 10);
      const bool bonus = k == "--split";
      if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || !end || *end != 0 || n < 1 || (bonus && n > AWV_CLIP_MAX_BONUS))
        die(bonus ? "--split expects a match bonus A with 1 <= A <= 32767" : "--split-min-score expects a score S >= 1");
      (bonus ? a.split : a.split_min_score) = n;
      (bonus ? a.have_split : a.have_split_min_score) = true;
    }
    else if (k == "--normalize") {
      const std::string v = val();
      if (v != "left" && v != "right") die("--normalize expects left or right");
      a.normalize = v == "left" ? AWV_NORM_LEFT : AWV_NORM_RIGHT;
      a.have_normalize = true;
    }
    else if (k == "--device-cigar") a.device_cigar = true;
    else if (k == "--cs") {
      const std::string v = val();
      if (v != "short" && v != "long") die("--cs expects short or long");
      a.cs = v == "short" ? AWV_CS_SHORT : AWV_CS_LONG;
    }
    else if (k == "--variants") {
      a.variants = val();
      if (a.variants.empty()) die("--variants expects a file name");
      a.have_variants = true;
    }
    else if (k == "--variants-min-count") {
      const std::string v = val();
      char* end = nullptr;
      a.variants_min_count = strtol(v.c_str(), &end, 10);
      if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || !end || *end != 0 || a.variants_min_count < 1)
        die("--variants-min-count expects a count N >= 1");
      a.have_variants_min_count = true;
    }
    else if (k == "--msa") {
      a.msa = val();
      if (a.msa.empty()) die("--msa expects a file name");
      a.have_msa = true;
    }
    else if (k == "--msa-target") {
      const std::string v = val();
      if (v.empty()) die("--msa-target expects a sequence name, or all");
      a.msa_targets.push_back(v);
    }
    else if (k == "--msa-max-bytes") {
      char* end = nullptr;
      const std::string v = val();
      a.msa_max_bytes = strtoull(v.c_str(), &end, 10);
      if (v.empty() || *end != '\0' || v[0] == '-' || a.msa_max_bytes < 1) die("--msa-max-bytes expects a number of bytes N >= 1");
      a.have_msa_max_bytes = true;
    }
    else if (k == "--liftover") {
      a.liftover = val();
      if (a.liftover.empty()) die("--liftover expects a BED file name");
      a.have_liftover = true;
    }
    else if (k == "--liftover-out") {
      a.liftover_out = val();
      if (a.liftover_out.empty()) die("--liftover-out expects a file name");
      a.have_liftover_out = true;
    }
    else if (k == "--liftover-from") {
      const std::string v = val();
      if (v != "target" && v != "query" && v != "both") die("--liftover-from expects target, query or both");
      a.liftover_from = v == "target" ? AWV_LIFT_FROM_TARGET : v == "query" ? AWV_LIFT_FROM_QUERY : AWV_LIFT_FROM_BOTH;
      a.have_liftover_from = true;
    }
    else if (k == "--coverage") {
      a.coverage = val();
      if (a.coverage.empty()) die("--coverage expects a file name");
      a.have_coverage = true;
    }
    else if (k == "--coverage-of") {
      const std::string v = val();
      if (v != "target" && v != "query" && v != "both") die("--coverage-of expects target, query or both");
      a.coverage_of = v == "target" ? AWV_COV_TARGET : v == "query" ? AWV_COV_QUERY : AWV_COV_BOTH;
      a.have_coverage_of = true;
    }
    else if (k == "--clip" || k == "--clip-min-score") {
      const std::string v = val();
      char* end = nullptr;
      const long n = strtol(v.c_str(), &end, 10);
      const bool bonus = k == "--clip";
      if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || !end || *end != 0 || n < 1 || (bonus && n > AWV_CLIP_MAX_BONUS))
        die(bonus ? "--clip expects a match bonus A with 1 <= A <= 32767" : "--clip-min-score expects a score S >= 1");
      (bonus ? a.clip : a.clip_min_score) = n;
      (bonus ? a.have_clip : a.have_clip_min_score) = true;
    }
    else if (k == "--max-divergence") {
      const std::string v = val();
      char* end = nullptr;
      a.max_divergence = strtod(v.c_str(), &end);
      if (v.empty() || v.find_first_not_of("0123456789.eE+-") != std::string::npos || !end || *end != 0 ||
          !(a.max_divergence >= 0.0 && a.max_divergence < 1.0))
        die("--max-divergence expects a divergence D with 0 <= D < 1");
      a.have_max_divergence = true;
    }
    else if (k == "--shard") {
      const std::string v = val();
      char* end = nullptr;
      a.have_shard = true;
      a.shard_rank = strtol(v.c_str(), &end, 10);
      if (!end || *end != '/') die("--shard expects R/N, e.g. 3/8");
      const char* w = end + 1;
      a.shard_world = strtol(w, &end, 10);
      if (end == w || *end != 0 || a.shard_world < 1 || a.shard_rank < 0 || a.shard_rank >= a.shard_world) die("--shard expects R/N with 0 <= R < N");
    }
    else if (k == "-h" || k == "--help") {
      std::cout << "usage: allwave_hip -i in.fa [-o out.paf] [-s m,x,o,e[,o2,e2] | -x ANI] [-p none|auto|random:f|giant:p|tree:n:f:r[:k]]\n"
                   "                   [-t threads] [--wfa-orientation|--wfa-orientation-full|--forward-only] [-k prefixes | -e prefixes] [--mash-matrix]\n"
                   "                   [--device N | --devices LIST] [--shard R/N] [--score-only [--max-penalty N]] [--plan-device N] [--verify]\n"
                   "                   [--max-align-penalty N] [--max-divergence D] [--clip A [--clip-min-score S]]\n"
                   "                   [--split A --split-min-score S] [--normalize left|right] [--device-cigar] [--cs short|long]\n"
                   "                   [--coverage FILE [--coverage-of target|query|both]] [--variants FILE [--variants-min-count N]]\n"
                   "                   [--liftover BED --liftover-out FILE [--liftover-from target|query|both]]\n"
                   "                   [--msa FILE --msa-target NAME|all ... [--msa-max-bytes N]]\n"
                   "       allwave_hip -i in.fa --check-paf FILE [-s scores | -x ANI] [--check-optimal] [--partial] [--device N]\n"
                   "       allwave_hip -i in.fa --align-paf FILE [-s scores | -x ANI] [-o out.paf] [--verify] [--score-only] [--device N | --devices LIST]\n"
                   "                   [--max-align-penalty N] [--max-divergence D] [--clip A [--clip-min-score S]]\n"
                   "                   [--split A --split-min-score S] [--normalize left|right] [--device-cigar] [--cs short|long]\n"
                   "                   [--coverage FILE [--coverage-of target|query|both]] [--variants FILE [--variants-min-count N]]\n"
                   "                   [--liftover BED --liftover-out FILE [--liftover-from target|query|both]]\n"
                   "                   [--msa FILE --msa-target NAME|all ... [--msa-max-bytes N]]\n"
                   "  --verify         check every alignment on the device before it is written (columns, counts, penalty); the summary\n"
                   "                   line gains `verified N pairs, F failed, K ms`, failures go to stderr, exit status 4 if any\n"
                   "  --check-paf FILE align nothing: check every line of FILE (12 columns + cg:Z:) against in.fa on the device; one line\n"
                   "                   `line qname tname strand class column penalty [optimum]` per failing PAF line, exit status 0 or 4\n"
                   "  --check-optimal  with --check-paf: also compare each op string's penalty with the optimal one (score-only alignment)\n"
                   "  --partial        with --check-paf: a line whose coordinates are a proper interval of both sequences is checked as the\n"
                   "                   global alignment of that interval pair instead of being reported `not_end_to_end`\n"
                   "  --align-paf FILE align the interval pairs FILE names (columns 1-9 of each line: names, lengths, intervals, strand; the\n"
                   "                   query interval on its forward strand) globally; one PAF line per input line, in input order; a bad\n"
                   "                   line is reported on stderr as `line class` and gives no output line (--score-only: the nine columns\n"
                   "                   and the penalty)\n"
                   "  --devices LIST   align on several devices in this process: ordinals and ranges, e.g. 0,1,2 / 0-7 / all;\n"
                   "                   an ordinal may repeat (0,0: two engines on device 0); -t is shared out among them\n"
                   "  --score-only     no PAF: one tab-separated line per pair, `qname qlen tname tlen strand penalty`, in pair-list\n"
                   "                   order (the optimal penalty without a CIGAR; `*` for a pair that failed)\n"
                   "  --max-penalty N  with --score-only: stop searching a pair once its penalty is proved above N and leave it out\n"
                   "  --max-align-penalty N  full alignments under a penalty bound: a pair whose optimal penalty is proved above N is\n"
                   "                   abandoned inside its top-level search and gets no PAF line; the PAF is the unbounded one minus those\n"
                   "                   lines, and the summary line gains `A pairs above the bound`\n"
                   "  --max-divergence D  0 <= D < 1: keep the alignments with (#X + #I + #D) <= D * columns; every pair is searched under\n"
                   "                   the penalty bound no such alignment can exceed, completed pairs are filtered on their counts\n"
                   "  --clip A         clip every alignment to its best-scoring segment on the device (+A per match, minus the penalties):\n"
                   "                   each PAF line is replaced by its segment's line (coordinates shifted, a '-' line's query coordinates on\n"
                   "                   the forward strand; columns 10, 11, gi:f: and cg:Z: the segment's) or dropped when nothing scores above 0;\n"
                   "                   the summary line gains `clipped N pairs, E empty, B below min score, K ms`\n"
                   "  --clip-min-score S  with --clip: also drop the segments that score below S (default 1)\n"
                   "  --split A        split every alignment into all its maximal segments that score at least S on the device (+A per match,\n"
                   "                   minus the penalties; needs --split-min-score S, not with --clip): each PAF line is replaced by its segments'\n"
                   "                   lines, in column order, or dropped; also with --align-paf, where one input line may give several lines;\n"
                   "                   the summary line gains `split N pairs into G segments, E without a segment, K ms`\n"
                   "  --split-min-score S  with --split: the least score of a segment (required: no default can be derived)\n"
                   "  --normalize left|right  move every alignment's gap runs as far left (right) as they go among co-optimal placements, on\n"
                   "                   the device, before --verify, --clip and --split see them: only cg:Z: changes; also with --align-paf;\n"
                   "                   the summary line gains `normalized N pairs, R runs moved, K ms`\n"
                   "  --device-cigar   make the run-length text behind cg:Z: on the device, after --normalize, --verify and --clip, and copy it\n"
                   "                   back in place of the op bytes: the PAF is byte-identical; also with --align-paf; not with --split; the\n"
                   "                   summary line gains `encoded N pairs, R runs, B text bytes, K ms`\n"
                   "  --cs short|long  append minimap2's cs difference string to every line (cs:Z:, after cg:Z:), made on the device after\n"
                   "                   --normalize, --verify, --clip and --device-cigar from the op string and the sequences: short writes\n"
                   "                   :N for N matches, long =BASES; also with --align-paf; not with --split; the summary line gains\n"
                   "                   `cs N pairs, F failed, B text bytes, K ms`\n"
                   "  --coverage FILE  accumulate on the device, for every base of every sequence, in how many of the run's alignments it is\n"
                   "                   aligned (= or X) and in how many it matches, and write FILE: one line name<TAB>beg<TAB>end<TAB>aligned<TAB>\n"
                   "                   matched per maximal interval on which both are constant, every sequence end to end, in input order; what\n"
                   "                   counts is what is written (the clip under --clip, every segment under --split, after --normalize); the\n"
                   "                   PAF is byte-identical; also with --align-paf; not with --score-only, --check-paf or --mash-matrix; under\n"
                   "                   --shard every process writes the depth of its own shard to its own FILE (add the files up by\n"
                   "                   position); the summary line gains `coverage I items, B boundaries, K ms`\n"
                   "  --coverage-of target|query|both  whose bases an aligned column counts for (default both)\n"
                   "  --variants FILE  tally on the device, per site of every target, which alleles the run's alignments carry and how many\n"
                   "                   carry each, and write FILE: one line tname<TAB>pos<TAB>snv|del|ins<TAB>len<TAB>ref<TAB>alt<TAB>count per\n"
                   "                   distinct (site, allele), sorted by target, position, type, length; ref: the target's bases (. for an\n"
                   "                   insertion), alt: the query's (. for a deletion), upper case; what counts is what is written, as for\n"
                   "                   --coverage; --normalize left makes indel sites canonical across queries; the PAF is byte-identical;\n"
                   "                   also with --align-paf; not with --score-only, --check-paf or --mash-matrix; under --shard every\n"
                   "                   process writes its own shard's table; the summary line gains `variants I items, E events, R rows, K ms`\n"
                   "  --variants-min-count N  write only rows that N or more alignments carry (default 1)\n"
                   "  --liftover BED   lift the regions of BED (name<TAB>beg<TAB>end[<TAB>label], names as in in.fa; a bad line is reported on\n"
                   "                   stderr as `line class` and gives no region) through the run's alignments on the device, to every sequence\n"
                   "                   their sequence was aligned with: the aligned core of a region, from its first aligned base to its last;\n"
                   "                   --liftover-out FILE gets one line src_name<TAB>src_beg<TAB>src_end<TAB>label<TAB>dst_name<TAB>dst_beg<TAB>\n"
                   "                   dst_end<TAB>strand<TAB>matches<TAB>mismatches<TAB>ins<TAB>del per region and alignment that has one, sorted\n"
                   "                   by region, then pair; what counts is what is written, as for --coverage; the PAF is byte-identical; also\n"
                   "                   with --align-paf; not with --score-only, --check-paf or --mash-matrix; under --shard every process writes\n"
                   "                   its own shard's file; the summary line gains `lifted Q queries, R rows, U unaligned, K ms`\n"
                   "  --liftover-from target|query|both  the side of an alignment a region is looked for on (default target)\n"
                   "  --msa FILE       lay every aligned sequence out against the targets named by --msa-target NAME (repeatable, names as in\n"
                   "                   in.fa; or all) as target-anchored multiple alignments, on the device, from the run's alignments: aligned\n"
                   "                   FASTA, `>` and the target's name for the first row, then `>qname/qbeg-qend` and the strand sign per\n"
                   "                   alignment of the target (the query interval on the forward strand), sorted by query, strand and\n"
                   "                   position; insertions are left-justified; with more than one target FILE must contain {}, which is\n"
                   "                   replaced by the target's 0-based index in in.fa; what counts is what is written, as for --coverage; the\n"
                   "                   PAF is byte-identical; also with --align-paf; not with --score-only, --check-paf, --mash-matrix or\n"
                   "                   --device-cigar; under --shard every process writes its own shard's file; the summary line gains\n"
                   "                   `msa T targets, R rows, B bytes, K ms`\n"
                   "  --msa-max-bytes N  the bound of the kept op bytes and of the blocks, each (default 2^30): beyond it the run's alignments\n"
                   "                   are written as always and the run then fails, naming the bound and the size needed\n"
                   "  --plan-device N  plan on device N: --mash-matrix, the -p pair list and mash orientation (the same output as\n"
                   "                   the host planner; with --shard every rank plans the whole list on its own plan device)\n";
      return 0;
    } else die("unexpected argument: " + k);
  }
  if (a.have_max_penalty && !a.score_only) die("the argument '--max-penalty' requires '--score-only'");
  auto bound_flag_alone = [&](bool have, const char* flag) {  // (before any device is opened)
    if (!have) return;
    const std::string f = std::string("the argument '") + flag + "' cannot be used with ";
    if (a.score_only) die(f + "'--score-only' (which has '--max-penalty')");
    if (a.have_check_paf) die(f + "'--check-paf'");
    if (a.mash_matrix) die(f + "'--mash-matrix'");
  };
  bound_flag_alone(a.have_max_align_penalty, "--max-align-penalty");
  bound_flag_alone(a.have_max_divergence, "--max-divergence");
  if (a.have_clip_min_score && !a.have_clip) die("the argument '--clip-min-score' requires '--clip'");
  if (a.have_split_min_score && !a.have_split) die("the argument '--split-min-score' requires '--split'");
  if (a.have_split && !a.have_split_min_score) die("the argument '--split' requires '--split-min-score'");
  if (a.have_split && a.have_clip) die("the argument '--split' cannot be used with '--clip'");
  if (a.have_split && a.score_only) die("the argument '--split' cannot be used with '--score-only'");
  if (a.have_split && a.have_check_paf) die("the argument '--split' cannot be used with '--check-paf'");
  if (a.have_split && a.mash_matrix) die("the argument '--split' cannot be used with '--mash-matrix'");
  if (a.have_clip && a.score_only) die("the argument '--clip' cannot be used with '--score-only'");
  if (a.have_clip && a.have_check_paf) die("the argument '--clip' cannot be used with '--check-paf'");
  if (a.have_clip && a.mash_matrix) die("the argument '--clip' cannot be used with '--mash-matrix'");
  if (a.have_normalize && a.score_only) die("the argument '--normalize' cannot be used with '--score-only'");
  if (a.have_normalize && a.have_check_paf) die("the argument '--normalize' cannot be used with '--check-paf'");
  if (a.have_normalize && a.mash_matrix) die("the argument '--normalize' cannot be used with '--mash-matrix'");
  if (a.device_cigar && a.have_split) die("the argument '--device-cigar' cannot be used with '--split'");
  if (a.device_cigar && a.score_only) die("the argument '--device-cigar' cannot be used with '--score-only'");
  if (a.device_cigar && a.have_check_paf) die("the argument '--device-cigar' cannot be used with '--check-paf'");
  if (a.device_cigar && a.mash_matrix) die("the argument '--device-cigar' cannot be used with '--mash-matrix'");
  if (a.cs != 0 && a.have_split) die("the argument '--cs' cannot be used with '--split'");
  if (a.cs != 0 && a.score_only) die("the argument '--cs' cannot be used with '--score-only'");
  if (a.cs != 0 && a.have_check_paf) die("the argument '--cs' cannot be used with '--check-paf'");
  if (a.cs != 0 && a.mash_matrix) die("the argument '--cs' cannot be used with '--mash-matrix'");
  if (a.have_coverage_of && !a.have_coverage) die("the argument '--coverage-of' requires '--coverage'");
  if (a.have_variants_min_count && !a.have_variants) die("the argument '--variants-min-count' requires '--variants'");
  if (a.have_variants && a.score_only) die("the argument '--variants' cannot be used with '--score-only'");
  if (a.have_variants && a.have_check_paf) die("the argument '--variants' cannot be used with '--check-paf'");
  if (a.have_variants && a.mash_matrix) die("the argument '--variants' cannot be used with '--mash-matrix'");
  if (a.have_msa && a.msa_targets.empty()) die("the argument '--msa' requires '--msa-target'");
  if (!a.have_msa && !a.msa_targets.empty()) die("the argument '--msa-target' requires '--msa'");
  if (a.have_msa_max_bytes && !a.have_msa) die("the argument '--msa-max-bytes' requires '--msa'");
  if (a.have_msa && a.score_only) die("the argument '--msa' cannot be used with '--score-only'");
  if (a.have_msa && a.have_check_paf) die("the argument '--msa' cannot be used with '--check-paf'");
  if (a.have_msa && a.mash_matrix) die("the argument '--msa' cannot be used with '--mash-matrix'");
  if (a.have_msa && a.device_cigar) die("the argument '--msa' cannot be used with '--device-cigar' (the sink then carries text, not op bytes)");
  if (a.have_liftover != a.have_liftover_out) die("the arguments '--liftover' and '--liftover-out' require each other");
  if (a.have_liftover_from && !a.have_liftover) die("the argument '--liftover-from' requires '--liftover'");
  if (a.have_liftover && a.score_only) die("the argument '--liftover' cannot be used with '--score-only'");
  if (a.have_liftover && a.have_check_paf) die("the argument '--liftover' cannot be used with '--check-paf'");
  if (a.have_liftover && a.mash_matrix) die("the argument '--liftover' cannot be used with '--mash-matrix'");
  if (a.have_coverage && a.score_only) die("the argument '--coverage' cannot be used with '--score-only'");
  if (a.have_coverage && a.have_check_paf) die("the argument '--coverage' cannot be used with '--check-paf'");
  if (a.have_coverage && a.mash_matrix) die("the argument '--coverage' cannot be used with '--mash-matrix'");
  if (a.check_optimal && !a.have_check_paf) die("the argument '--check-optimal' requires '--check-paf'");
  if (a.verify && a.score_only) die("the argument '--verify' cannot be used with '--score-only'");
  if (a.verify && a.mash_matrix) die("the argument '--verify' cannot be used with '--mash-matrix'");
  if (a.have_check_paf && (a.verify || a.score_only || a.mash_matrix || a.have_output || a.have_devices))
    die("the argument '--check-paf' cannot be used with '--verify', '--score-only', '--mash-matrix', '--output' or '--devices'");
  if (a.partial && !a.have_check_paf) die("the argument '--partial' requires '--check-paf'");
  if (a.have_align_paf && (a.have_sparsification || a.wfa_orientation || a.forward_only || a.have_shard || a.mash_matrix || a.have_check_paf ||
                           a.plan_device >= 0))
    die("the argument '--align-paf' cannot be used with '--sparsification', '--wfa-orientation', '--wfa-orientation-full', '--forward-only', "
        "'--shard', '--mash-matrix', '--plan-device' or '--check-paf'");
  if (a.input.empty()) die("the following required arguments were not provided: --input <INPUT>");
  if (a.have_scores && a.have_preset) die("the argument '--scores' cannot be used with '--preset'");
  if (a.have_keep && a.have_exclude) die("the argument '--keep-prefixes' cannot be used with '--exclude-prefixes'");
  if (a.have_device && a.have_devices) die("the argument '--device' cannot be used with '--devices'", 1);
  std::vector<int> devices(1, a.device);
  if (a.have_devices) {
    std::string msg;
    if (!parse_devices(a.devices, devices, msg)) die(msg, 1);
  }

  SparsificationStrategy strategy;
  try { strategy = SparsificationStrategy::parse(a.sparsification); } catch (const std::exception& e) { die(e.what(), 1); }

  std::vector<Sequence> sequences = read_fasta(a.input);
  auto filter = [&](const std::string& list, bool keep) {  // main.rs:236-278
    const auto prefixes = split_trim(list);
    const size_t before = sequences.size();
    std::vector<Sequence> kept;
    for (auto& s : sequences) {
      bool any = false;
      for (const auto& p : prefixes) any = any || s.id.compare(0, p.size(), p) == 0;
      if (any == keep) kept.push_back(std::move(s));
    }
    sequences.swap(kept);
    if (sequences.size() != before)
      std::cerr << (keep ? "Kept sequences with prefixes: " : "Excluded sequences with prefixes: ") << before << " -> "
                << sequences.size() << " (prefixes: " << list << ")\n";
    if (sequences.empty()) die(keep ? "No sequences match the specified keep prefixes" : "All sequences were excluded by the specified prefixes", 1);
  };
  if (a.have_keep) filter(a.keep, true);
  if (a.have_exclude) filter(a.exclude, false);

  planner::set_host_threads(a.threads);  // -t: sketching, mash orientation, PAF formatting
  if (a.mash_matrix) {  // main.rs:281-293
    const size_t k = strategy.kind == SparsificationStrategy::TreeSampling && strategy.kmer_size ? *strategy.kmer_size : 15;
    if (a.plan_device < 0) {
      std::cout << planner::format_distance_matrix(sequences, planner::compute_distance_matrix(sequences, k, 1000));
      return 0;
    }
    try {  // streamed a block of rows at a time
      planner::write_distance_matrix(sequences, k, 1000, a.plan_device, [](const std::string& block) {
        std::cout.write(block.data(), (std::streamsize)block.size());
        if (!std::cout) throw std::runtime_error("write error on the matrix output");
      });
      std::cout.flush();
    } catch (const std::exception& e) {
      die(e.what(), 1);
    }
    return 0;
  }

  std::string scores = a.scores;
  if (a.have_preset) {
    scores = parse_ani_preset(a.preset);
    std::cerr << "Using ANI preset " << a.preset << " -> alignment scores: " << scores << "\n";
  }
  AlignmentParams params;
  try { params = parse_scores(scores); } catch (const std::exception& e) { die(e.what(), 1); }

  if (a.have_check_paf) {
    try {
      std::ifstream fin(a.check_paf, std::ios::binary);
      if (!fin) die("cannot open " + a.check_paf, 1);
      std::stringstream ss;
      ss << fin.rdbuf();
      set_engine_flags(AWV_F_NO_ARENA_PROBE);
      const PafCheckReport r = check_paf(sequences, ss.str(), params, a.check_optimal, a.device, a.partial);
      std::cout << format_paf_check(r);
      std::cout.flush();
      char buf[200];
      snprintf(buf, sizeof(buf), "checked %zu of %zu PAF lines (%zu empty records skipped), %zu failed, %.2f ms", r.checked, r.lines,
               r.skipped, r.failures.size(), r.stats.kernel_ms);
      std::cerr << buf << "\n";
      return r.failures.empty() ? 0 : 4;
    } catch (const std::exception& e) {
      die(e.what(), 1);
    }
  }

  int verify_status = 0;
  try {
    // --align-paf: the list is the file's interval pairs (bad lines reported here, counted below, and left out)
    std::vector<AlignmentRange> ranges;
    size_t bad_lines = 0;
    if (a.have_align_paf) {
      std::ifstream fin(a.align_paf, std::ios::binary);
      if (!fin) die("cannot open " + a.align_paf, 1);
      std::stringstream ss;
      ss << fin.rdbuf();
      PafRanges pr = parse_paf_ranges(sequences, ss.str());
      for (const PafRangeLine& l : pr.lines)
        if (!l.cls.empty()) {
          std::cerr << l.line << ' ' << l.cls << "\n";
          ++bad_lines;
        }
      ranges = std::move(pr.ranges);
    }
    AllPairIterator it = a.have_align_paf ? AllPairIterator::for_ranges(sequences, ranges, params)
                                          : AllPairIterator::with_options(sequences, params, true, !a.wfa_orientation, strategy, a.plan_device);
    it.with_verify(a.verify);
    if (a.have_max_align_penalty) it.with_max_penalty((int)a.max_align_penalty);
    if (a.have_max_divergence) it.with_max_divergence(a.max_divergence);
    const bool bounded = a.have_max_align_penalty || a.have_max_divergence;
    if (a.have_clip) it.with_clip((int)a.clip, (int64_t)a.clip_min_score);
    if (a.have_split) it.with_split((int)a.split, (int64_t)a.split_min_score);
    if (a.have_normalize) it.with_normalize(a.normalize);
    it.with_device_cigar(a.device_cigar);
    it.with_cs(a.cs);
    if (a.have_coverage) it.with_coverage(a.coverage_of);
    it.with_variants(a.have_variants);
    BedRegions bed;
    if (a.have_liftover) {  // (bad lines reported here and left out)
      std::ifstream fin(a.liftover, std::ios::binary);
      if (!fin) die("cannot open " + a.liftover, 1);
      std::stringstream ss;
      ss << fin.rdbuf();
      std::vector<std::string> names;
      std::vector<size_t> lens;
      for (const Sequence& q : sequences) {
        names.push_back(q.id);
        lens.push_back(q.seq.size());
      }
      bed = parse_bed_regions(names, lens, ss.str());
      for (const BedLine& l : bed.bad) std::cerr << l.line << ' ' << l.cls << "\n";
      it.with_liftover(bed.regions, a.liftover_from);
    }
    std::vector<int> msa_idx;  // the targets' indices in in.fa, in the order they were named
    if (a.have_msa) {
      const bool all = a.msa_targets.size() == 1 && a.msa_targets[0] == "all";
      for (size_t i = 0; all && i < sequences.size(); ++i) msa_idx.push_back((int)i);
      for (size_t k = 0; !all && k < a.msa_targets.size(); ++k) {
        size_t i = 0;
        while (i < sequences.size() && sequences[i].id != a.msa_targets[k]) ++i;
        if (i == sequences.size()) die("--msa-target: no sequence named '" + a.msa_targets[k] + "' in " + a.input);
        if (std::find(msa_idx.begin(), msa_idx.end(), (int)i) != msa_idx.end()) die("--msa-target: '" + a.msa_targets[k] + "' is named twice");
        msa_idx.push_back((int)i);
      }
      if (msa_idx.size() > 1 && a.msa.find("{}") == std::string::npos) die("--msa: with more than one target the file name must contain {}");
      it.with_msa(msa_idx, a.msa_max_bytes);
    }
    if (a.forward_only) it.with_orientation(Orientation::ForwardOnly);
    it.with_full_wfa_orientation(a.wfa_orientation_full);
    it.with_devices(devices);
    it.with_shard((size_t)a.shard_rank, (size_t)a.shard_world);
    const size_t total = it.pair_count();
    // a short-lived process with little work: taking the ring arena as it comes beats choosing the
    // fastest of four candidates (1-3 s once per engine for up to 6 % of the kernel time)
    if (total < 2000000) set_engine_flags(AWV_F_NO_ARENA_PROBE);
    std::ofstream fout;
    if (a.have_output) {
      fout.open(a.output, std::ios::binary);
      if (!fout) die("cannot create " + a.output, 1);
    }
    std::ostream& out = a.have_output ? (std::ostream&)fout : (std::ostream&)std::cout;
    const auto t0 = std::chrono::steady_clock::now();
    size_t done = 0;
    if (a.score_only) {
      const std::vector<PairScore> sc = it.scores(a.have_max_penalty ? std::optional<int>((int)a.max_penalty) : std::nullopt);
      std::string buf;
      for (const PairScore& p : sc) {
        ++done;
        if (p.status == AWV_ST_ABOVE_BOUND) continue;
        const Sequence& q = sequences[p.query_idx];
        const Sequence& t = sequences[p.target_idx];
        const std::string pen_s = p.status == AWV_ST_COMPLETED ? std::to_string(p.penalty) : std::string("*");
        if (a.have_align_paf) {  // the mapping's nine columns, then the penalty
          const AlignmentRange& g = ranges[done - 1];
          buf += q.id + '\t' + std::to_string(q.seq.size()) + '\t' + std::to_string(g.query_start) + '\t' + std::to_string(g.query_end) + '\t' +
                 (g.is_reverse ? '-' : '+') + '\t' + t.id + '\t' + std::to_string(t.seq.size()) + '\t' + std::to_string(g.target_start) + '\t' +
                 std::to_string(g.target_end) + '\t' + pen_s + '\n';
        } else
        buf += q.id + '\t' + std::to_string(q.seq.size()) + '\t' + t.id + '\t' + std::to_string(t.seq.size()) + '\t' +
               (p.is_reverse ? '-' : '+') + '\t' + pen_s + '\n';
        if (buf.size() >= (1u << 20)) {
          out.write(buf.data(), (std::streamsize)buf.size());
          if (!out) throw std::runtime_error("write error on the score output");
          buf.clear();
        }
      }
      out.write(buf.data(), (std::streamsize)buf.size());
      if (!out) throw std::runtime_error("write error on the score output");
    } else {
      it.for_each_paf_batch([&](const std::string& chunk) {
        out.write(chunk.data(), (std::streamsize)chunk.size());
        // a short write (disk full, closed pipe) must not pass for a complete PAF: the reference propagates
        // the writer's error (main.rs:355 `writeln!(..)?`, joined at :451-453); throwing here makes the
        // engine stop with AWV_ERR_SINK before any further batch
        if (!out) throw std::runtime_error("write error on the PAF output");
        for (char c : chunk) done += c == '\n';
      }, a.threads);
    }
    out.flush();
    if (!out) die("write error on the PAF output (flush)", 1);
    if (a.have_output) {
      fout.close();
      if (fout.fail()) die("write error on the PAF output (close)", 1);
    }
    if (a.have_coverage) {  // name, beg, end, aligned, matched per maximal interval on which both tracks are constant
      const Coverage& cv = it.last_coverage();
      std::ofstream cout_(a.coverage, std::ios::binary);
      if (!cout_) die("cannot create " + a.coverage, 1);
      std::string buf;
      for (size_t s = 0; s < sequences.size(); ++s) {
        const size_t len = sequences[s].seq.size();
        const uint32_t* al = cv.aligned.data() + cv.offsets[s];
        const uint32_t* ma = cv.matched.data() + cv.offsets[s];
        for (size_t beg = 0, p = 1; p <= len; ++p) {
          if (p < len && al[p] == al[beg] && ma[p] == ma[beg]) continue;
          buf += sequences[s].id + '\t' + std::to_string(beg) + '\t' + std::to_string(p) + '\t' + std::to_string(al[beg]) + '\t' + std::to_string(ma[beg]) + '\n';
          beg = p;
        }
        if (buf.size() >= (1u << 20) || s + 1 == sequences.size()) {
          cout_.write(buf.data(), (std::streamsize)buf.size());
          buf.clear();
        }
      }
      cout_.close();
      if (cout_.fail()) die("write error on the coverage output", 1);
    }
    if (a.have_variants) {  // tname, pos, type, len, ref, alt, count per row of the table, in key order
      std::ofstream vout(a.variants, std::ios::binary);
      if (!vout) die("cannot create " + a.variants, 1);
      static const char* const type_names[3] = {"snv", "del", "ins"};
      const auto upper = [](uint8_t c) { return (char)(c >= 'a' && c <= 'z' ? c - 32 : c); };
      const auto comp = [](uint8_t c) {  // the engine's reverse complement: ACGT in either case, anything else N
        switch (c) {
          case 'A': case 'a': return 'T';
          case 'C': case 'c': return 'G';
          case 'G': case 'g': return 'C';
          case 'T': case 't': return 'A';
          default: return 'N';
        }
      };
      std::string buf;
      const std::vector<awv_variant>& rows = it.last_variants();
      for (size_t k = 0; k < rows.size(); ++k) {
        const awv_variant& r = rows[k];
        if ((long)r.count >= a.variants_min_count) {
          const std::vector<uint8_t>& tseq = sequences[(size_t)r.t_idx].seq;
          const std::vector<uint8_t>& qseq = sequences[(size_t)(r.rep >> 32)].seq;
          const bool rev = ((r.rep >> 31) & 1) != 0;
          const size_t p_beg = (size_t)(r.rep & 0x7fffffffu), len = (size_t)r.len;
          std::string ref, alt;
          if (r.type != AWV_VAR_INS)
            for (size_t i = 0; i < len && (size_t)r.pos + i < tseq.size(); ++i) ref += upper(tseq[(size_t)r.pos + i]);
          if (r.type != AWV_VAR_DEL)
            for (size_t i = 0; i < len && p_beg + i < qseq.size(); ++i) alt += rev ? comp(qseq[qseq.size() - 1 - (p_beg + i)]) : upper(qseq[p_beg + i]);
          buf += sequences[(size_t)r.t_idx].id + '\t' + std::to_string(r.pos) + '\t' + type_names[r.type >= 0 && r.type < 3 ? r.type : 0] + '\t' +
                 std::to_string(r.len) + '\t' + (r.type != AWV_VAR_INS ? ref : ".") + '\t' + (r.type != AWV_VAR_DEL ? alt : ".") + '\t' + std::to_string(r.count) + '\n';
        }
        if (buf.size() >= (1u << 20) || k + 1 == rows.size()) {
          vout.write(buf.data(), (std::streamsize)buf.size());
          buf.clear();
        }
      }
      vout.close();
      if (vout.fail()) die("write error on the variants output", 1);
    }
    if (a.have_liftover) {  // one line per row of the table, in its order
      std::ofstream lout(a.liftover_out, std::ios::binary);
      if (!lout) die("cannot create " + a.liftover_out, 1);
      std::string buf;
      const std::vector<awv_lift_row>& rows = it.last_liftover();
      for (size_t k = 0; k < rows.size(); ++k) {
        const awv_lift_row& r = rows[k];
        const bool from_q = (r.flags & AWV_LIFT_ROW_FROM_QUERY) != 0;
        const Sequence& src = sequences[(size_t)(from_q ? r.q_idx : r.t_idx)];
        const Sequence& dst = sequences[(size_t)(from_q ? r.t_idx : r.q_idx)];
        buf += src.id + '\t' + std::to_string(r.src_beg) + '\t' + std::to_string(r.src_end) + '\t' + bed.labels[(size_t)r.region] + '\t' + dst.id + '\t' +
               std::to_string(r.dst_beg) + '\t' + std::to_string(r.dst_end) + '\t' + ((r.flags & AWV_LIFT_ROW_REVCOMP) ? '-' : '+') + '\t' +
               std::to_string(r.num_matches) + '\t' + std::to_string(r.num_mismatches) + '\t' + std::to_string(r.num_ins) + '\t' + std::to_string(r.num_del) + '\n';
        if (buf.size() >= (1u << 20) || k + 1 == rows.size()) {
          lout.write(buf.data(), (std::streamsize)buf.size());
          buf.clear();
        }
      }
      lout.close();
      if (lout.fail()) die("write error on the liftover output", 1);
    }
    uint64_t msa_rows = 0;
    if (a.have_msa) {  // one aligned FASTA per target
      for (const MsaBlock& b : it.last_msa()) {
        std::string name = a.msa;
        const size_t at = name.find("{}");
        if (at != std::string::npos) name.replace(at, 2, std::to_string(b.t_idx));
        std::ofstream mout(name, std::ios::binary);
        if (!mout) die("cannot create " + name, 1);
        for (int64_t r = 0; r < b.rows; ++r) {
          mout << '>' << b.names[(size_t)r] << '\n';
          mout.write((const char*)b.bytes.data() + r * b.width, (std::streamsize)b.width);
          mout << '\n';
        }
        mout.close();
        if (mout.fail()) die("write error on the msa output", 1);
        msa_rows += (uint64_t)b.rows;
      }
    }
    const BoundStats bs = it.last_bound_stats();
    const size_t above = (size_t)(bs.above_penalty + bs.above_divergence);  // (pairs above a bound get no line)
    const ClipStats cs = it.last_clip_stats();
    const size_t unclipped = (size_t)(cs.empty + cs.below_min_score);  // (nor do pairs without a clip worth reporting)
    const SplitStats ss = it.last_split_stats();  // (a split pair gives one line per segment)
    if (done + above + unclipped + (size_t)ss.pairs != total + (size_t)ss.segments) die("internal: wrote " + std::to_string(done) + " of " + std::to_string(total) + (a.score_only ? " pairs" : " PAF lines"), 1);
    if (!a.no_progress) {
      const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      char buf[896];
      int w = snprintf(buf, sizeof(buf), "[%.1fs] %zu/%zu (100.0%%) %.1f alignments/sec", secs, done, total, done / std::max(secs, 1e-9));
      if (a.have_align_paf && w > 0 && (size_t)w < sizeof(buf)) w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", %zu bad lines", bad_lines);
      if (bounded && w > 0 && (size_t)w < sizeof(buf)) w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", %zu pairs above the bound", above);
      if (a.have_clip && w > 0 && (size_t)w < sizeof(buf))
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", clipped %llu pairs, %llu empty, %llu below min score, %.2f ms", (unsigned long long)cs.pairs,
                      (unsigned long long)cs.empty, (unsigned long long)cs.below_min_score, cs.kernel_ms);
      if (a.have_split && w > 0 && (size_t)w < sizeof(buf))
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", split %llu pairs into %llu segments, %llu without a segment, %.2f ms", (unsigned long long)ss.pairs,
                      (unsigned long long)ss.segments, (unsigned long long)ss.empty, ss.kernel_ms);
      if (a.have_normalize && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_norm_stats ns = it.last_normalize_stats();
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", normalized %llu pairs, %llu runs moved, %.2f ms", (unsigned long long)ns.pairs,
                      (unsigned long long)ns.runs_moved, ns.kernel_ms);
      }
      if (a.device_cigar && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_encode_stats es = it.last_encode_stats();
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", encoded %llu pairs, %llu runs, %llu text bytes, %.2f ms", (unsigned long long)es.pairs,
                      (unsigned long long)es.runs, (unsigned long long)es.text_bytes, es.kernel_ms);
      }
      if (a.cs != 0 && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_cs_stats xs = it.last_cs_stats();
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", cs %llu pairs, %llu failed, %llu text bytes, %.2f ms", (unsigned long long)xs.pairs,
                      (unsigned long long)xs.failed, (unsigned long long)xs.text_bytes, xs.kernel_ms);
      }
      if (a.have_coverage && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_cov_stats vs = it.last_report().coverage_stats;
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", coverage %llu items, %llu boundaries, %.2f ms", (unsigned long long)vs.items,
                      (unsigned long long)vs.boundaries, vs.kernel_ms);
      }
      if (a.have_variants && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_variants_stats vs = it.last_report().variants_stats;
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", variants %llu items, %llu events, %llu rows, %.2f ms", (unsigned long long)vs.items,
                      (unsigned long long)(vs.snv + vs.ins + vs.del), (unsigned long long)vs.rows, vs.kernel_ms + vs.fold_ms);
      }
      if (a.have_liftover && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_lift_stats ls = it.last_report().lift_stats;
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", lifted %llu queries, %zu rows, %llu unaligned, %.2f ms", (unsigned long long)ls.queries,
                      it.last_liftover().size(), (unsigned long long)ls.unaligned, ls.kernel_ms);
      }
      if (a.have_msa && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_msa_stats ms = it.last_report().msa_stats;
        w += snprintf(buf + w, sizeof(buf) - (size_t)w, ", msa %zu targets, %llu rows, %llu bytes, %.2f ms", it.last_msa().size(), (unsigned long long)msa_rows,
                      (unsigned long long)ms.bytes, ms.width_ms + ms.scan_ms + ms.emit_ms);
      }
      if (a.verify && w > 0 && (size_t)w < sizeof(buf)) {
        const awv_verify_stats vs = it.last_verify_stats();
        snprintf(buf + w, sizeof(buf) - (size_t)w, ", verified %llu pairs, %zu failed, %.2f ms", (unsigned long long)vs.pairs,
                 it.verify_failures().size(), vs.kernel_ms);
      }
      std::cerr << buf << "\n";
    }
    if (a.verify) {
      const auto& vf = it.verify_failures();
      if (a.no_progress)
        std::cerr << "verified " << it.last_verify_stats().pairs << " pairs, " << vf.size() << " failed, " << it.last_verify_stats().kernel_ms << " ms\n";
      std::string report;
      verify_status = report_verify_failures(vf, sequences, report);
      std::cerr << report;
    }
  } catch (const std::exception& e) {
    die(e.what(), 1);
  }
  return verify_status;
}
