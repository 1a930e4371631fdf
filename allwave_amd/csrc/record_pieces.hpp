// record_pieces.hpp -- how a call on caller-supplied records (the awv_*_cigars / _ranges entry points of all ten record passes) is
// cut into launches: pure host code, no HIP, so a CPU program can run it (tests/record_pieces_driver.cpp).
//
// A piece holds at most max_arena op bytes (one record alone may exceed that) and at most max_records records.  The op bytes
// of a piece are packed into 16-byte slots of a staging buffer, so records may share, overlap or leave out parts of the
// caller's arena; a record that is not completed takes no bytes.  With keep_residue every string keeps its offset modulo 16
// (the kernels address a string from the 16-byte boundary at or below its first byte, and that addressing is part of what a
// caller may want to exercise); without it every string starts its slot.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "allwave_hip.h"

namespace awvw {

// a completed record whose op bytes do not lie inside an arena of arena_bytes
inline bool outside(const awv_result& r, uint64_t arena_bytes) {
  return r.status == AWV_ST_COMPLETED && (r.cigar_off > arena_bytes || (uint64_t)r.cigar_len > arena_bytes - r.cigar_off);
}

struct Piece {
  int64_t n;       // records results[first .. first + n)
  uint64_t bytes;  // of `stage`, a multiple of 16
};

// The piece that begins at record `first` (< n_all): `recs` are its records with cigar_off relative to `stage`, `stage` its
// op bytes, zero between the strings.
inline Piece pack_piece(const awv_result* results, int64_t n_all, int64_t first, const uint8_t* cigar_arena, uint64_t max_arena, bool keep_residue,
                        std::vector<awv_result>& recs, std::vector<uint8_t>& stage, int64_t max_records = (int64_t)1 << 20) {
  int64_t n = 0;
  uint64_t bytes = 0;
  recs.clear();
  while (first + n < n_all && n < max_records) {
    const awv_result& r = results[first + n];
    const uint64_t sh = keep_residue ? r.cigar_off & 15 : 0;
    const uint64_t need = r.status == AWV_ST_COMPLETED ? (sh + (uint64_t)r.cigar_len + 15) & ~(uint64_t)15 : 0;
    if (n > 0 && bytes + need > max_arena) break;
    recs.push_back(r);
    recs.back().cigar_off = bytes + sh;
    bytes += need;
    ++n;
  }
  stage.assign((size_t)bytes, 0);
  for (int64_t i = 0; i < n; ++i) {
    const awv_result& r = results[first + i];
    if (r.status == AWV_ST_COMPLETED && r.cigar_len) std::memcpy(stage.data() + recs[(size_t)i].cigar_off, cigar_arena + r.cigar_off, r.cigar_len);
  }
  return Piece{n, bytes};
}

// A piece that came back changed (awv_normalize_cigars): the strings of the records with code AWV_NM_OK return from `stage`
// to their place in the caller's arena.  results, nout: the piece's n entries.
inline void scatter_back(const awv_result* results, const awv_norm_result* nout, int64_t n, const std::vector<awv_result>& recs,
                         const std::vector<uint8_t>& stage, uint8_t* cigar_arena) {
  for (int64_t i = 0; i < n; ++i) {
    const awv_result& r = results[i];
    if (r.status == AWV_ST_COMPLETED && r.cigar_len && nout[i].code == AWV_NM_OK)
      std::memcpy(cigar_arena + r.cigar_off, stage.data() + recs[(size_t)i].cigar_off, r.cigar_len);
  }
}

}  // namespace awvw
