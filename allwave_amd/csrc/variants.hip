// variants.hip -- the alleles of all alignments per target site: the device pass that writes every item's events (awv_variants_cigars /
// awv_variants_ranges), the engine's accumulated table (awv_engine_variants_begin / _read / _stats, variants_batch) and the host
// yardsticks awv_variants_one_host and awv_variants_fold_host (include/allwave_hip.h).  Which events an item carries and how they
// fold is variants_device.hpp; the fold on the device is variants_fold.hip.
//
// A record pass (record_pass.hpp) in text_pass.hpp's three steps, with cs.hip's walk: one wave per item, persistent waves taking
// items (longest op string first) from a cursor, a string in chunks of 64 lanes x 16 op bytes.  measure counts every item's events
// and decides its code (awv_var_item, and the item's Place); awv_text_scan_kernel gives every item its rows in a dense arena; emit
// walks the sound items again and writes count-1 rows in column order: awv_variants_one_host's rows, byte for byte.
// Who owns which event: an 'X' column its SNV; the lane that holds the break that ends a gap run the run's event, before the
// break byte's own SNV; lane 0 the string's last run, behind the chunks.  A lane's first row is a wave add-scan of the lanes'
// event counts plus a uniform carry.  A column's pattern and text position are the packed add-scan of wave_ops.hpp (consumed_scan); a run's pos / p_beg are
// the positions at its end minus its length.  The allele hash of a 'D' run is a segmented wave scan of HashSeg elements over the
// lanes (a lane wholly inside a run is a pass-through) and one uniform hash carried from chunk to chunk.
// Hang discipline: every loop's trip count is a host-validated length or a 16-bit mask; scans, readlane and
// ballot stand where control flow is wave-uniform; no wave waits for another; every row store is guarded by the item's own rows.
#include "variants_device.hpp"

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "batch_items.hpp"  // contributing_items
#include "seq_load.hpp"     // load16
#include "text_pass.hpp"    // lane_runs, run_start_before's carry, awv_text_scan_kernel, TEXT_COUNTERS; record_pass.hpp below it: each_piece, resolve_call

namespace awvvar {

struct Place {  // an item's rows in the launch's row arena: what the scan reads and writes
  uint64_t off;
  uint32_t len;   // its events
  int32_t code;
};

struct RowArena {  // emit: rows[0] is the row at offset `base` of the scan, `count` rows of it (measure: all zero)
  awv_variant* rows;
  unsigned long long base, count;
};

struct KParams {
  const uint8_t* fwd;         // the engine's forward copies
  const uint8_t* rc;          // and reverse-complement copies (the pattern of a q_revcomp pair)
  const uint64_t* seq_off;
  const awv_pair* pairs;
  const Span* spans;          // item i's rectangle, behind the slice's skips (validated on the host)
  const awv_result* results;  // cigar_off relative to `arena`; a slice is a record of its own here
  const int32_t* order;       // dispatch slot -> item
  const uint8_t* arena;       // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  awv_var_item* items;        // measure writes them
  Place* place;               // measure writes len and code, the scan off, emit reads all three
  RowArena dest;
  unsigned long long* counters;  // [0] this kernel's cursor
  long long npairs;
};

using awvw::byte_at;
using awvw::CHUNK;
using awvw::LANE_BYTES;
using awvw::load16;
using awvw::u32x4;
using awvw::wave_scan_add;
using awvw::wave_sum_i64;

// one step of the segmented scan: the element `CTRL` lanes below (the identity where there is none) combined with the lane's own
template <int CTRL, int ROWS>
__device__ __forceinline__ HashSeg seg_step(const HashSeg& v) {
  HashSeg lo;
  lo.h = (uint64_t)awvw::dpp64<CTRL, ROWS>(0ll, (long long)v.h);
  lo.pw = (uint64_t)awvw::dpp64<CTRL, ROWS>(1ll, (long long)v.pw);
  lo.reset = (uint32_t)awvw::dpp32<CTRL, ROWS>(0, (int)v.reset);
  return seg_combine(lo, v);
}
// wave64 inclusive scan under seg_combine, wave_scan_add's network
__device__ __forceinline__ HashSeg seg_scan(HashSeg v) {
  v = seg_step<0x111, 0xf>(v);
  v = seg_step<0x112, 0xf>(v);
  v = seg_step<0x114, 0xf>(v);
  v = seg_step<0x118, 0xf>(v);
  v = seg_step<0x142, 0xa>(v);
  v = seg_step<0x143, 0xc>(v);
  return v;
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
  return (uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane) | ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane) << 32);
}

template <bool EMIT>
__global__ __launch_bounds__(64) void awv_variants_kernel(KParams kp) {
  const int lane = threadIdx.x;
  for (;;) {  // leaves when the cursor passes npairs: every trip takes one slot
    // The body ends on `if (lane == 0)` stores and take_record begins on `if (lane == 0)`: without a convergent operation between
    // the two the compiler threads lanes 1 .. 63 past both, straight to take_record's readfirstlane, where they read their own 0
    // and walk slot 0 again, for ever (seen in the assembly as one more loop level around the chunk loop).
    __builtin_amdgcn_wave_barrier();
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int item = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[item];
    if (rec.status != AWV_ST_COMPLETED) {
      if (!EMIT && lane == 0) {
        kp.items[item] = make_item(AWV_VR_SKIPPED, 0, 0, 0);
        kp.place[item] = Place{0, 0u, AWV_VR_SKIPPED};
      }
      continue;
    }
    const long long n = (long long)rec.cigar_len;
    const awv_pair pr = kp.pairs[item];
    const Span sp = kp.spans[item];
    const int plen = sp.pe - sp.pb, tlen = sp.te - sp.tb;
    if (n == 0) {
      if (!EMIT && lane == 0) {
        const int code = whole_code(false, 0, 0, plen, tlen);
        kp.items[item] = make_item(code, 0, 0, 0);
        kp.place[item] = Place{0, 0u, code};
      }
      continue;
    }
    // emit: only an item that measure found sound is walked again: its positions stay inside the two sequences (load16 clamps all
    // the same), and its rows are its own [off, off + len) of the arena -- checked all the same, so that nothing is ever stored outside
    awv_variant* dst = nullptr;
    unsigned room = 0;
    if (EMIT) {
      const Place pl = kp.place[item];
      if (pl.code == AWV_VR_OK && pl.off >= kp.dest.base && pl.off - kp.dest.base <= kp.dest.count && (unsigned long long)pl.len <= kp.dest.count - (pl.off - kp.dest.base)) {
        dst = kp.dest.rows + (pl.off - kp.dest.base);
        room = pl.len;
      }
      if (room == 0) continue;
    }
    const auto put = [&](unsigned& at, const awv_variant& ev) {
      if (at < room) dst[at] = ev;
      ++at;
    };
    const uint8_t* const pattern = (pr.q_revcomp ? kp.rc : kp.fwd) + kp.seq_off[pr.q_idx] + sp.pb;
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]
    const long long span = sh + n;

    int cq = 0, ct = 0;  // emit: bases consumed before the chunk (uniform, like everything carried)
    awvw::RunCarry carry;
    unsigned c_ev = 0;    // emit: events of the chunks before
    uint64_t hcarry = 0;  // emit: the hash of the 'D' run in progress at the chunk's first byte
    unsigned long long l_pos = 0, l_snv = 0, l_gap = 0;  // measure, lane-local: pattern | text bases << 32; SNVs; ended 'D' | 'I' runs << 32
    bool l_bad = false;
    for (long long base = 0; base < span; base += CHUNK) {  // ceil(span / 1,024) trips: span <= 2^30 + 15 by the host's check
      const awvw::LaneRuns r = awvw::lane_runs(ops, sh, span, base, lane, carry);
      awvw::OpMasks o = awvw::window_masks(r.jlo, r.jhi);  // (awvw::op_masks, written out: see there)
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) awvw::add_op(o, r.w, j);
      awvw::cut_to_window(o);
      LaneCols c;
      c.valid = o.valid;
      c.x = o.x;
      c.i = o.i;
      c.d = o.d;
      c.brk = r.brk;
      c.prev_i = r.prev == 'I';
      c.prev_d = r.prev == 'D';
      const unsigned takes_p = c.valid & ~c.i, takes_t = c.valid & ~c.d;
      if (!EMIT) {
        l_bad = l_bad || (o.valid & ~(o.m | o.x | o.i | o.d)) != 0;
        l_pos += (unsigned long long)__popc(takes_p) | ((unsigned long long)__popc(takes_t) << 32);
        l_snv += (unsigned long long)__popc(c.x);
        l_gap += (unsigned long long)__popc(ends_d(c)) | ((unsigned long long)__popc(ends_i(c)) << 32);
      } else {
        const awvw::ConsumedScan pos = awvw::consumed_scan(o);
        const int cnt = (int)lane_event_count(c);
        const int s_ev = wave_scan_add(cnt);
        u32x4 pb16 = u32x4{0u, 0u, 0u, 0u};
        if ((c.x | c.d) != 0) pb16 = load16(pattern, plen, cq + (pos.ex & 0xffff));
        const auto byte = [&](int k) { return byte_at(pb16, k); };
        uint64_t in_h = hcarry;  // (a chunk without a 'D': only its first column can end the run in progress)
        if (__ballot(c.d != 0) != 0) {  // (uniform)
          const HashSeg inc = seg_scan(lane_seg(c, byte));
          HashSeg lower;
          lower.h = (uint64_t)awvw::from_lower_lane((long long)inc.h, 0ll);
          lower.pw = (uint64_t)awvw::from_lower_lane((long long)inc.pw, 1ll);
          lower.reset = (uint32_t)awvw::from_lower_lane((int)inc.reset, 0);
          in_h = seg_behind(hcarry, lower);
          const HashSeg all{readlane64(inc.h, 63), readlane64(inc.pw, 63), (uint32_t)__builtin_amdgcn_readlane((int)inc.reset, 63)};
          hcarry = seg_behind(hcarry, all);
        } else {
          hcarry = 0;
        }
        if (cnt != 0) {
          unsigned at = c_ev + (unsigned)(s_ev - cnt);
          lane_events(c, pr.q_idx, pr.t_idx, pr.q_revcomp != 0, r.b0 - sh, r.rs0, (int64_t)sp.pb + cq + (pos.ex & 0xffff), (int64_t)sp.tb + ct + (pos.ex >> 16), in_h, byte,
                      [&](const awv_variant& ev) { put(at, ev); });
        }
        cq += pos.tot & 0xffff;
        ct += pos.tot >> 16;
        c_ev += (unsigned)__builtin_amdgcn_readlane(s_ev, 63);
      }
      awvw::carry_on(carry, r, sh, span, base);
    }
    // the string's last run has no break behind it
    const bool last_d = carry.prev == 'D', last_i = carry.prev == 'I';
    if (EMIT) {
      if (lane == 0 && (last_d || last_i))
        put(c_ev, gap_event(pr.q_idx, pr.t_idx, pr.q_revcomp != 0, last_d, (int64_t)sp.pb + cq, (int64_t)sp.tb + ct, n - carry.start, hcarry));
    } else {
      const unsigned long long pos = (unsigned long long)wave_sum_i64((long long)l_pos), snv = (unsigned long long)wave_sum_i64((long long)l_snv),
                               gap = (unsigned long long)wave_sum_i64((long long)l_gap);
      const int code = whole_code(__ballot(l_bad) != 0, (long long)(unsigned)pos, (long long)(pos >> 32), plen, tlen);
      const awv_var_item it = make_item(code, (unsigned)snv, (unsigned)gap + (unsigned)last_d, (unsigned)(gap >> 32) + (unsigned)last_i);
      if (lane == 0) {
        kp.items[item] = it;
        kp.place[item] = Place{0, it.snv + it.ins + it.del, code};
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

constexpr uint64_t DEFAULT_RESERVE_ROWS = (uint64_t)1 << 20;  // awv_engine_variants_begin with reserve_rows == 0: 40 MiB

struct Table {  // rows on the device: [0, n) in use
  awv_variant* p = nullptr;
  uint64_t cap = 0, n = 0;
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = n = 0;
  }
};

struct State : awvw::RecordPass {
  Buf<awv_pair> d_pairs;
  Buf<Span> d_spans;
  Buf<awv_var_item> d_items;
  Buf<Place> d_place;
  awvw::BatchItems items;  // a batch's items (batch_items.hpp)
  std::vector<awv_var_item> h_items;
  Table acc;               // the engine's table between awv_engine_variants_begin and its end
  Table call;              // the rows of one awv_variants_cigars / awv_variants_fold call
  FoldScratch* fs = nullptr;
  bool on = false;
  int64_t clip_min_score = 0;
  int32_t nseq = 0;
  awv_variants_stats stats{};
  void release() {
    RecordPass::release();
    d_pairs.release();
    d_spans.release();
    d_items.release();
    d_place.release();
    acc.release();
    call.release();
    fold_scratch_release(fs);
    fs = nullptr;
    on = false;
  }
};

void state_release(State* s) { awvw::release_pass(s); }
bool active(const State* s) { return s && s->on; }

namespace {

constexpr const char* TOO_LONG = "variants: an op string of more than 2^30 columns";

int open_state(awv_engine* e, awp::EngineView& v, State*& st, bool need_set = true) {
  if (int rc = awvw::open_pass(awv_internal_variants(e), e, v, st, need_set)) return rc;
  if (!st->fs) st->fs = fold_scratch_new();
  return AWV_OK;
}
int open_active(awv_engine* e, const char* who, awp::EngineView& v, State*& st) {  // (an engine that accumulates has its fold scratch: begin made it)
  if (int rc = awvw::open_active(awv_internal_variants(e), who, "variants", e, v, st)) return rc;
  if (v.n != st->nseq) return awv_internal_fail(AWV_ERR_STATE, "variants: the sequence set changed since awv_engine_variants_begin");
  return AWV_OK;
}

// rows [0, n) of tb folded in place
int fold_table(const awp::EngineView& v, State* st, Table& tb) {
  uint64_t left = tb.n;
  float ms = 0;
  if (int rc = fold_device(v.stream, st->fs, tb.p, tb.n, &left, &ms)) return rc;
  tb.n = left;
  st->stats.fold_ms += ms;
  if (&tb == &st->acc) {
    st->stats.folds += 1;
    st->stats.rows = left;
  }
  return AWV_OK;
}

// Room for `need` more rows behind tb's: when they would pass the capacity the table is folded in place (may_fold), and grows --
// to twice its size or what is needed -- when that is not enough or leaves it more than half full.  A failed allocation is
// AWV_ERR_OOM and the table is as it was (folded, at most).
int make_room(const awp::EngineView& v, State* st, Table& tb, uint64_t need, bool may_fold) {
  if (tb.n <= tb.cap && need <= tb.cap - tb.n) return AWV_OK;
  if (may_fold && tb.n > 0)
    if (int rc = fold_table(v, st, tb)) return rc;
  if (need <= tb.cap - tb.n && !(may_fold && tb.n > tb.cap / 2)) return AWV_OK;
  const uint64_t cap = std::max<uint64_t>(2 * tb.cap, tb.n + need);
  if (cap > MAX_FOLD_ROWS) return awv_internal_fail(AWV_ERR_ARG, "variants: a table of more than 2^31 rows");
  awv_variant* p = nullptr;
  if (hipMalloc((void**)&p, (size_t)cap * sizeof(awv_variant)) != hipSuccess) {
    (void)hipGetLastError();
    return awv_internal_fail(AWV_ERR_OOM, "variants: no device memory for a table of " + std::to_string(cap) + " rows");
  }
  if (tb.n) {
    const hipError_t err = hipMemcpyAsync(p, tb.p, (size_t)tb.n * sizeof(awv_variant), hipMemcpyDeviceToDevice, v.stream);
    const hipError_t err2 = err == hipSuccess ? hipStreamSynchronize(v.stream) : err;
    if (err2 != hipSuccess) {
      (void)hipFree(p);
      AWV_TRY(err2);
    }
  }
  if (tb.p) (void)hipFree(tb.p);
  tb.p = p;
  tb.cap = cap;
  if (&tb == &st->acc) st->stats.capacity_rows = cap;
  return AWV_OK;
}

// the rows of tb to the caller: *n_rows always, the rows when they fit cap -- all or none
int copy_out(const awp::EngineView& v, const Table& tb, awv_variant* rows, uint64_t cap, uint64_t* n_rows) {
  *n_rows = tb.n;
  if (rows && tb.n > 0 && tb.n <= cap) {
    AWV_TRY(hipMemcpyAsync(rows, tb.p, (size_t)tb.n * sizeof(awv_variant), hipMemcpyDeviceToHost, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
  }
  return AWV_OK;
}

// One launch over n items whose op bytes are on the device already; an item's slice has been applied to its record and to its
// rectangle.  Every index and rectangle is checked here, on the host, and so is every op string's place in the arena (begin) and
// length: the kernels read what the items say.  The items' events are appended to tb; items (host, nullable) is filled.
int launch(const awp::EngineView& v, State* st, Table& tb, bool may_fold, const awv_pair* pairs, const Span* spans, int64_t n, const awv_result* recs,
           const uint8_t* d_arena, uint64_t arena_bytes, awv_var_item* items) {
  if (n == 0) return AWV_OK;
  if (int rc = awvw::check_rectangles(v, "variants", pairs, spans, n)) return rc;
  if (int rc = awvw::check_lengths(recs, n, MAX_COLUMNS, TOO_LONG)) return rc;
  if (int rc = st->begin(v, "variants", n, recs, arena_bytes)) return rc;
  AWV_TRY(st->d_pairs.reserve((size_t)n));
  AWV_TRY(st->d_spans.reserve((size_t)n));
  AWV_TRY(st->d_items.reserve((size_t)n));
  AWV_TRY(st->d_place.reserve((size_t)n));
  AWV_TRY(hipMemcpyAsync(st->d_pairs.p, pairs, (size_t)n * sizeof(awv_pair), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_spans.p, spans, (size_t)n * sizeof(Span), hipMemcpyHostToDevice, v.stream));
  if (int rc = st->clear_counters(v, awvw::TEXT_COUNTERS)) return rc;
  KParams kp{};
  kp.fwd = v.fwd;
  kp.rc = v.rc;
  kp.seq_off = v.off;
  kp.pairs = st->d_pairs.p;
  kp.spans = st->d_spans.p;
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.items = st->d_items.p;
  kp.place = st->d_place.p;
  kp.npairs = n;
  const unsigned grid = st->grid(v, n);
  // measure and scan; the number of events is all the host waits for before it makes room
  kp.counters = st->d_counters.p;
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_variants_kernel<false>, dim3(grid), dim3(64), 0, v.stream, kp);
  hipLaunchKernelGGL(awvw::awv_text_scan_kernel<Place>, dim3(1), dim3(awvw::SCAN_THREADS), 0, v.stream, st->d_place.p, (long long)n, 0ull, st->d_counters.p + 4);
  if (int rc = st->stop(v)) return rc;
  unsigned long long total = 0;
  float ms = 0, ms_emit = 0;
  AWV_TRY(hipMemcpyAsync(&total, st->d_counters.p + 4, sizeof(total), hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  AWV_TRY(hipEventElapsedTime(&ms, st->ev0, st->ev1));
  if (total > 0) {
    if (int rc = make_room(v, st, tb, total, may_fold)) return rc;
    kp.counters = st->d_counters.p + 8;
    kp.dest = RowArena{tb.p + tb.n, 0ull, total};
    if (int rc = st->start(v)) return rc;
    hipLaunchKernelGGL(awv_variants_kernel<true>, dim3(grid), dim3(64), 0, v.stream, kp);
    if (int rc = st->stop(v)) return rc;
  }
  if (!items) {
    st->h_items.resize((size_t)n);
    items = st->h_items.data();
  }
  AWV_TRY(hipMemcpyAsync(items, st->d_items.p, (size_t)n * sizeof(awv_var_item), hipMemcpyDeviceToHost, v.stream));
  unsigned long long hc[4] = {0, 0, 0, 0};
  if (int rc = st->finish(v, hc, 4, ms_emit)) return rc;
  tb.n += total;
  awv_variants_stats& s = st->stats;
  s.kernel_ms += ms + (total > 0 ? ms_emit : 0.f);
  s.items += (uint64_t)n;
  for (int64_t i = 0; i < n; ++i) {
    s.failed += items[i].code != AWV_VR_OK && items[i].code != AWV_VR_SKIPPED;
    s.columns += recs[i].status == AWV_ST_COMPLETED ? recs[i].cigar_len : 0u;
    s.snv += items[i].snv;
    s.ins += items[i].ins;
    s.del += items[i].del;
  }
  return AWV_OK;
}

int too_many_items(const State* st, int64_t more) {
  if ((int64_t)st->stats.items + more > MAX_ITEMS) return awv_internal_fail(AWV_ERR_ARG, "variants: more than 2^31 - 1 items since awv_engine_variants_begin");
  return AWV_OK;
}

// ranges (nullable; awv_variants_ranges): the call is on ranges[0..n_all) -- `pairs` is not read
int variants_cigars_core(awv_engine* e, const awv_pair* pairs, const awv_range_pair* ranges, int64_t n_all, const awv_result* results,
                         const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_slice* slices, uint64_t max_arena, int32_t fold, awv_var_item* items,
                         awv_variant* rows, uint64_t cap, uint64_t* n_rows) {
  const char* who = ranges ? "variants_ranges" : "variants_cigars";
  if (fold != AWV_VTAB_EVENTS && fold != AWV_VTAB_FOLDED && fold != AWV_VTAB_ACCUMULATE)
    return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": fold must be an AWV_VTAB_* value");
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = fold == AWV_VTAB_ACCUMULATE ? open_active(e, who, v, st) : open_state(e, v, st)) return rc;
  awvw::ItemCall call;
  if (int rc = awvw::resolve_call(call, v, who, pairs, ranges, n_all, results, arena_bytes, slices)) return rc;
  if (int rc = awvw::check_lengths(call.recs, n_all, MAX_COLUMNS, TOO_LONG)) return rc;
  if (int rc = too_many_items(st, n_all)) return rc;
  Table& tb = fold == AWV_VTAB_ACCUMULATE ? st->acc : st->call;
  if (fold != AWV_VTAB_ACCUMULATE) tb.n = 0;
  const uint64_t events_before = st->stats.snv + st->stats.ins + st->stats.del;
  const auto piece = [&](int64_t first, int64_t n, const awv_result* recs, uint64_t bytes) {
    return launch(v, st, tb, fold != AWV_VTAB_EVENTS, call.pairs + first, call.spans.data() + first, n, recs, st->d_arena.p, bytes, items + first);
  };
  if (int rc = st->each_piece(v, call.recs, n_all, cigar_arena, max_arena, piece)) return rc;
  if (fold == AWV_VTAB_ACCUMULATE) {
    *n_rows = st->stats.snv + st->stats.ins + st->stats.del - events_before;
    return AWV_OK;
  }
  if (fold == AWV_VTAB_FOLDED && tb.n > 0)
    if (int rc = fold_table(v, st, tb)) return rc;
  return copy_out(v, tb, rows, cap, n_rows);
}

// list: the pairs or ranges
int check_args(const char* name, int64_t n, const void* list, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
               const awv_var_item* items, const awv_variant* rows, uint64_t cap, const uint64_t* n_rows) {
  if (int rc = awvw::check_call_args(name, n, list, results, n_rows && (n <= 0 || items), cigar_arena, arena_bytes)) return rc;
  if (cap > 0 && !rows) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": null row buffer");
  return AWV_OK;
}

int begin_core(awv_engine* e, int64_t clip_min_score, uint64_t reserve_rows) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->on = false;  // the table before this one ends
  st->acc.release();
  st->stats = awv_variants_stats{};
  if (int rc = make_room(v, st, st->acc, reserve_rows ? reserve_rows : DEFAULT_RESERVE_ROWS, false)) return rc;
  st->nseq = v.n;
  st->clip_min_score = clip_min_score;
  st->on = true;
  return AWV_OK;
}

int read_core(awv_engine* e, awv_variant* rows, uint64_t cap, uint64_t* n_rows) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_active(e, "variants_read", v, st)) return rc;
  if (st->acc.n > 0)
    if (int rc = fold_table(v, st, st->acc)) return rc;
  return copy_out(v, st->acc, rows, cap, n_rows);
}

int fold_core(awv_engine* e, awv_variant* rows, uint64_t n, uint64_t* n_rows) {
  *n_rows = 0;
  if (n == 0) return AWV_OK;
  if (n >= MAX_FOLD_ROWS) return awv_internal_fail(AWV_ERR_ARG, "variants_fold: 2^31 rows or more");
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st, false)) return rc;
  Table& tb = st->call;
  tb.n = 0;
  if (int rc = make_room(v, st, tb, n, false)) return rc;
  AWV_TRY(hipMemcpyAsync(tb.p, rows, (size_t)n * sizeof(awv_variant), hipMemcpyHostToDevice, v.stream));
  tb.n = n;
  if (int rc = fold_table(v, st, tb)) return rc;
  return copy_out(v, tb, rows, n, n_rows);
}

}  // namespace

int variants_batch(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
                   const awv_clip_result* clips, const uint64_t* seg_first, const awv_split_index* iout, const awv_clip_result* sout, const Span* spans) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_active(e, "variants_batch", v, st)) return rc;
  awvw::contributing_items(v, pairs, n, results, clips, st->clip_min_score, seg_first, iout, sout, spans, st->items);
  const int64_t m = (int64_t)st->items.pairs.size();
  if (int rc = too_many_items(st, m)) return rc;
  return launch(v, st, st->acc, true, st->items.pairs.data(), st->items.spans.data(), m, st->items.recs.data(), d_arena, arena_bytes, nullptr);
}

}  // namespace awvvar

extern "C" {

int awv_variants_one_host(int32_t q_idx, int32_t t_idx, int32_t q_revcomp, const uint8_t* pattern, int32_t qlen, int32_t tlen, int32_t pb, int32_t pe, int32_t tb,
                          int32_t te, const uint8_t* cigar, int64_t n, const awv_cs_slice* slice, awv_variant* events, uint64_t cap, uint64_t* n_events,
                          awv_var_item* out) {
  if (!out || !n_events || q_idx < 0 || t_idx < 0 || qlen < 0 || tlen < 0 || n < 0 || (qlen > 0 && !pattern) || (n > 0 && !cigar) || (cap > 0 && !events))
    return awv_internal_fail(AWV_ERR_ARG, "variants_one_host: bad argument");
  if (int rc = awvw::check_host_rectangle("variants_one_host", qlen, tlen, pb, pe, tb, te)) return rc;
  awvw::HostSlice sl;
  if (int rc = awvw::check_host_slice("variants_one_host", slice, n, awvvar::MAX_COLUMNS, sl)) return rc;
  *out = awvvar::var_one(q_idx, t_idx, q_revcomp != 0, pattern, awvvar::Span{pb, pe, tb, te}, cigar + sl.beg, sl.end - sl.beg, sl.q_skip, sl.t_skip, events, cap, n_events);
  return AWV_OK;
}

int awv_variants_fold_host(awv_variant* rows, uint64_t n, uint64_t* n_rows) {
  if (!n_rows || (n > 0 && !rows)) return awv_internal_fail(AWV_ERR_ARG, "variants_fold_host: null argument");
  *n_rows = awvvar::fold_rows(rows, n);
  return AWV_OK;
}

int awv_engine_variants_begin(awv_engine* e, int64_t clip_min_score, uint64_t reserve_rows) {
  if (!e) return awv_internal_null_engine();
  AWV_GUARDED(return awvvar::begin_core(e, clip_min_score, reserve_rows);)
}

int awv_engine_variants_end(awv_engine* e) {
  if (!e) return awv_internal_null_engine();
  if (awvvar::State* st = awv_internal_variants(e)) {
    st->on = false;
    st->acc.release();
  }
  return AWV_OK;
}

int awv_engine_variants_read(awv_engine* e, awv_variant* rows, uint64_t cap, uint64_t* n_rows) {
  if (!e) return awv_internal_null_engine();
  if (!n_rows || (cap > 0 && !rows)) return awv_internal_fail(AWV_ERR_ARG, "variants_read: null argument");
  AWV_GUARDED(return awvvar::read_core(e, rows, cap, n_rows);)
}

int awv_engine_variants_stats(const awv_engine* e, awv_variants_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "variants_stats: null argument");
  const awvvar::State* st = awv_internal_variants(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_variants_stats{};
  return AWV_OK;
}

int awv_variants_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                        const awv_cs_slice* slices, int32_t fold, awv_var_item* items, awv_variant* rows, uint64_t cap, uint64_t* n_rows) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvvar::check_args("variants_cigars", n, pairs, results, cigar_arena, arena_bytes, items, rows, cap, n_rows)) return rc;
  AWV_GUARDED(return awvvar::variants_cigars_core(e, pairs, nullptr, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), fold, items, rows,
                                                  cap, n_rows);)
}

int awv_variants_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                        const awv_cs_slice* slices, int32_t fold, awv_var_item* items, awv_variant* rows, uint64_t cap, uint64_t* n_rows) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvvar::check_args("variants_ranges", n, ranges, results, cigar_arena, arena_bytes, items, rows, cap, n_rows)) return rc;
  static const awv_range_pair none{};
  AWV_GUARDED(return awvvar::variants_cigars_core(e, nullptr, n > 0 ? ranges : &none, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), fold,
                                                  items, rows, cap, n_rows);)
}

int awv_variants_fold(awv_engine* e, awv_variant* rows, uint64_t n, uint64_t* n_rows) {
  if (!e) return awv_internal_null_engine();
  if (!n_rows || (n > 0 && !rows)) return awv_internal_fail(AWV_ERR_ARG, "variants_fold: null argument");
  AWV_GUARDED(return awvvar::fold_core(e, rows, n, n_rows);)
}

}  // extern "C"
