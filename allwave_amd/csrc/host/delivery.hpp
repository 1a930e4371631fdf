// delivery.hpp -- which entries of one engine call reach a run's consumer, and as what: the rule of a bounded, clipping or
// splitting run (DESIGN.md 4.26 states it once).  Pure host arithmetic over the records of include/allwave_hip.h: no
// iterator, no threads, no engine calls, so tests/test_delivery_cpu.py runs it on a CPU under sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "allwave_hip.h"

namespace allwave {

// What the bounds of a run left out (AllPairIterator::with_max_penalty / with_max_divergence): pairs aligned under a bound,
// and of them the ones dropped because their penalty is above the penalty bound, or their divergence above the divergence
// bound (abandoned by the penalty bound derived from it, or completed and filtered on the record's counts).
struct BoundStats {
  uint64_t pairs = 0, above_penalty = 0, above_divergence = 0;
};

// What clipping did to a run (AllPairIterator::with_clip): finished pairs whose op string was clipped, and of them the ones
// that reached no consumer because the clip is empty, or scores below min_score; kernel_ms: summed clip kernel time.
struct ClipStats {
  uint64_t pairs = 0, empty = 0, below_min_score = 0;
  double kernel_ms = 0.0;
};

// What splitting did to a run (AllPairIterator::with_split): finished pairs whose op string was split, the segments they
// gave, and the pairs that reached no consumer because no segment scores min_score; kernel_ms: summed split kernel time.
struct SplitStats {
  uint64_t pairs = 0, segments = 0, empty = 0;
  double kernel_ms = 0.0;
};

// The record of a finished pair rewritten into its segment `cl` (a clip, or one segment of a split): the slice of the op
// string, the segment's counts and penalty, and the bases it consumes as q_end / t_end.
inline awv_result segment_record(const awv_result& r, const awv_clip_result& cl) {
  awv_result s = r;
  s.cigar_off += cl.col_beg;
  s.cigar_len = cl.col_end - cl.col_beg;
  s.num_matches = cl.num_matches;
  s.num_mismatches = cl.num_mismatches;
  s.num_ins = cl.num_ins;
  s.num_del = cl.num_del;
  s.penalty = cl.penalty;
  s.score = -cl.penalty;
  s.q_end = cl.num_matches + cl.num_mismatches + cl.num_del;
  s.t_end = cl.num_matches + cl.num_mismatches + cl.num_ins;
  return s;
}

// One engine call's filtering state.  Every array has one element per entry of the call's pair array and is indexed by
// first + i of a sink call (first, cnt, res); the engine fills clip / index / seg before the entry's sink call.
struct Delivery {
  const uint8_t* rev = nullptr;  // the entry's strand
  const size_t* idx = nullptr;   // its pair-list index; nullptr: the entry's own position
  // a bounded run (bounds != nullptr)
  const uint8_t* by_div = nullptr;  // whether the entry's penalty bound is the one derived from the divergence bound
  double div = -1.0;                // the divergence bound (< 0: none)
  BoundStats* bounds = nullptr;
  // a clipping run (clips != nullptr)
  const awv_clip_result* clip = nullptr;
  int64_t min_score = 1;
  ClipStats* clips = nullptr;
  // a splitting run (splits != nullptr): entry e's segments are seg[seg_first[e] + 0 .. index[e].count)
  const uint64_t* seg_first = nullptr;
  const awv_split_index* index = nullptr;
  const awv_clip_result* seg = nullptr;
  SplitStats* splits = nullptr;
  // an encoding run (text != nullptr): the entry's run-length text in the sink call's text arena -- of the clip in a clipping run
  const awv_cigar_text* text = nullptr;
  // a cs run (cs != nullptr): the entry's cs text in the sink call's cs arena -- of the clip in a clipping run
  const awv_cs_text* cs = nullptr;

  bool filters() const { return bounds || clips || splits; }  // false: every entry is delivered as it is, nothing is copied
};

// What one sink call delivers: the kept records, their strands and pair-list indices and, in a clipping or splitting run,
// their clips (else empty), in an encoding run their texts (else empty) and, in a cs run, their cs texts (else empty).
struct Delivered {
  std::vector<awv_result> res;
  std::vector<uint8_t> rev;
  std::vector<size_t> idx;
  std::vector<awv_clip_result> clip;
  std::vector<awv_cigar_text> text;
  std::vector<awv_cs_text> cs;
};

// The rule, entry by entry in call order, for a run that filters(); counts into the Delivery's stats.
inline Delivered deliver(const Delivery& d, int64_t first, int64_t cnt, const awv_result* res) {
  Delivered out;
  auto keep = [&](int64_t e, const awv_result& r, const awv_clip_result* cl) {
    out.res.push_back(r);
    out.rev.push_back(d.rev[e]);
    out.idx.push_back(d.idx ? d.idx[e] : (size_t)e);
    if (cl) out.clip.push_back(*cl);
    if (d.text) out.text.push_back(d.text[e]);
    if (d.cs) out.cs.push_back(d.cs[e]);
  };
  for (int64_t i = 0; i < cnt; ++i) {
    const awv_result& r = res[i];
    const int64_t e = first + i;
    const bool done = r.status == AWV_ST_COMPLETED;
    if (d.bounds && r.status == AWV_ST_ABOVE_BOUND) {
      ++(d.by_div[e] ? d.bounds->above_divergence : d.bounds->above_penalty);
      continue;
    }
    if (d.bounds && done && d.div >= 0.0) {  // the exact filter, on the full record's counts
      const double edits = (double)r.num_mismatches + (double)r.num_ins + (double)r.num_del;
      if (!(edits <= d.div * (edits + (double)r.num_matches))) {
        ++d.bounds->above_divergence;
        continue;
      }
    }
    if (d.splits && done) {  // one entry per segment, in slot order
      ++d.splits->pairs;
      if (d.index[e].code != AWV_CL_OK) {
        ++d.splits->empty;
        continue;
      }
      d.splits->segments += (uint64_t)d.index[e].count;
      for (int32_t j = 0; j < d.index[e].count; ++j) {
        const awv_clip_result& cl = d.seg[d.seg_first[e] + (uint64_t)j];
        keep(e, segment_record(r, cl), &cl);
      }
    } else if (d.splits) {  // a failed pair: as it is (the "empty" result)
      awv_clip_result cl{};
      cl.code = AWV_CL_SKIPPED;
      keep(e, r, &cl);
    } else if (d.clips && done) {
      const awv_clip_result& cl = d.clip[e];
      ++d.clips->pairs;
      if (cl.code != AWV_CL_OK) ++d.clips->empty;
      else if (cl.score < d.min_score) ++d.clips->below_min_score;
      else keep(e, segment_record(r, cl), &cl);
    } else {  // a failed pair of a clipping run: with the clip the engine wrote for it
      keep(e, r, d.clips ? &d.clip[e] : nullptr);
    }
  }
  return out;
}

}  // namespace allwave
