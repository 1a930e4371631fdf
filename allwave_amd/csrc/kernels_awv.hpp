// kernels_awv.hpp -- the one-wave-per-pair (throughput) kernels live in a translation unit of their own
// (kernels_awv.hip) so that they can be compiled with scheduler options of their own: allwave_amd/build.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// Launches awv::biwfa_align_kernel<two_piece, narrow ? int16_t : int32_t> -- `pair_span` non-null: its range instantiation, with that
// device array (an awvr::Span per pair) as the second argument -- with `grid` workgroups of 64 threads (one wave) and
// `dyn_lds` bytes of dynamic LDS on `stream`; `kparams` points to an awv::KParams.  Returns the hipError_t of the set-up
// (launch errors are picked up by the caller's hipGetLastError, as for the kernels it launches itself).
int awv_launch_one_wave(int two_piece, int narrow, const void* pair_span, unsigned grid, size_t dyn_lds, hipStream_t stream, const void* kparams);
