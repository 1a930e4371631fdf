// batch_items.hpp -- which items one batch of an aligning call contributes to the passes that sum over alignments (coverage.hip,
// variants.hip, lift.hip), once: whole completed records; in a clipping call the clip's slice when it scores enough; in a
// splitting call every segment; nothing of failed records or records above the bound.  Pure host code.
#pragma once

#include <cstdint>
#include <vector>

#include "cs_slice.hpp"        // slice_ok, apply_slice
#include "item_call.hpp"       // whole_span, Span
#include "planner_device.hpp"  // EngineView

namespace awvw {

struct BatchItems {
  std::vector<awv_pair> pairs;   // a batch's items
  std::vector<awv_result> recs;  // their records with the slices applied
  std::vector<awvr::Span> spans; // and their rectangles
};

// `pairs`, `results`: the batch's n entries (host; the indices were checked by the aligning call); clips (nullable): the batch's
// clips; seg_first / iout / sout (nullable): the call's split layout, seg_first and iout already offset to the batch; spans
// (nullable): the batch's rectangles.
inline void contributing_items(const awp::EngineView& v, const awv_pair* pairs, int64_t n, const awv_result* results, const awv_clip_result* clips,
                               int64_t clip_min_score, const uint64_t* seg_first, const awv_split_index* iout, const awv_clip_result* sout,
                               const awvr::Span* spans, BatchItems& out) {
  const auto slice_of = [](const awv_clip_result& c) { return awv_cs_slice{c.col_beg, c.col_end, c.q_skip, c.t_skip}; };
  out.pairs.clear();
  out.recs.clear();
  out.spans.clear();
  const auto push = [&](int64_t i, const awv_cs_slice* sl) {
    out.pairs.push_back(pairs[i]);
    out.recs.push_back(results[i]);
    out.spans.push_back(spans ? spans[i] : whole_span(v.len_host, pairs[i]));
    if (sl) awvcs::apply_slice(out.recs.back(), out.spans.back(), *sl);
  };
  for (int64_t i = 0; i < n; ++i) {
    if (results[i].status != AWV_ST_COMPLETED) continue;  // failed, above the bound: nothing
    if (iout) {  // every segment of the split is an item
      if (iout[i].code != AWV_CL_OK) continue;
      for (int32_t k = 0; k < iout[i].count; ++k) {
        const awv_cs_slice sl = slice_of(sout[seg_first[i] + (uint64_t)k]);
        if (awvcs::slice_ok(results[i], sl)) push(i, &sl);
      }
    } else if (clips) {  // the clip's segment, when it scores enough
      const awv_cs_slice sl = slice_of(clips[i]);
      if (clips[i].code == AWV_CL_OK && clips[i].score >= clip_min_score && awvcs::slice_ok(results[i], sl)) push(i, &sl);
    } else {
      push(i, nullptr);
    }
  }
}

}  // namespace awvw
