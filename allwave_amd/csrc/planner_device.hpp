// planner_device.hpp -- what planner.hip (device pair planning) needs of an engine, and what engine.hip keeps for it.
// The engine owns the resident sequence set; planner.hip owns the sketches built from it (one set per kind) and the
// scratch of its kernels, released with the engine and whenever a new sequence set is handed over.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "allwave_hip.h"
#include "host_errors.hpp"  // AWV_TRY, AWV_GUARDED, awv_internal_fail, awv_internal_null_engine

struct awv_engine;

namespace awp {

struct PlanState;                   // planner.hip
void plan_state_release(PlanState* p);  // frees its device buffers and the object itself (nullptr: nothing)

// zero bytes behind every sequence of the padded layout (engine.hip, upload_seqset): the extension kernels read 8 bytes at
// a time, and verify.hip reads whole dwords that start inside a sequence
constexpr int SEQ_PAD_BYTES = 8;

// the engine's resident sequences: forward and reverse-complement copies in the engine's padded layout
struct EngineView {
  int device = 0;
  hipStream_t stream = nullptr;
  int32_t n = 0;
  const uint8_t* fwd = nullptr;     // device
  const uint8_t* rc = nullptr;      // device (host reverse_complement: non-ACGT -> 'N')
  const uint64_t* off = nullptr;    // device, n + 1
  const int32_t* len = nullptr;     // device, n
  const int32_t* len_host = nullptr;  // host, n
  int workgroups = 0;               // awv_engine_config.workgroups: the grid cap of the record kernels (verify / clip / split), 0 = their default
};

}  // namespace awp

// engine.hip
int awv_internal_view(awv_engine* e, awp::EngineView* v);  // AWV_ERR_STATE without a sequence set
// the same for a caller that needs the device and the stream only: an engine without a sequence set is no failure (the view
// then names no sequences) and awv_last_error() is left alone
void awv_internal_device_view(awv_engine* e, awp::EngineView* v);
awp::PlanState*& awv_internal_plan(awv_engine* e);
int awv_internal_check_penalties(const awv_penalties* pen);  // the engine's sign rules for a penalty set (not the ring's size limit): AWV_OK or awv_align_pairs' error
