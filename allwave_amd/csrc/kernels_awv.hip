// kernels_awv.hip -- namespace awv:: of biwfa_device.hpp (one wave per pair: the throughput kernels) and their launcher.
// A translation unit of its own: these kernels are bound by VALU issue and gain 2-3 % from the compiler's
// "max-ilp" scheduling strategy, which in the multi-wave kernels of engine.hip spills a lane vector inside the pass
// loop (not allowed) -- so the option is given to this file only (allwave_amd/build.py).
#include "kernels_awv.hpp"
#define AWV_NS awv
#define AWV_WG 64
#include "biwfa_device.hpp"

namespace {
template <typename K, typename... PairSpan>
int launch(K kern, unsigned grid, size_t dyn_lds, hipStream_t stream, const awv::KParams& kp, PairSpan... pair_span) {
  const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(AWV_WG), dyn_lds, stream, kp, pair_span...);
  return (int)hipSuccess;
}
}  // namespace

int awv_launch_one_wave(int two_piece, int narrow, const void* pair_span, unsigned grid, size_t dyn_lds, hipStream_t stream, const void* kparams) {
  const awv::KParams& kp = *static_cast<const awv::KParams*>(kparams);
  if (pair_span) {
    const awvr::Span* sp = static_cast<const awvr::Span*>(pair_span);
    typedef const awvr::Span* S;
    if (two_piece) return narrow ? launch(awv::biwfa_align_kernel<true, int16_t, S>, grid, dyn_lds, stream, kp, sp)
                                 : launch(awv::biwfa_align_kernel<true, int32_t, S>, grid, dyn_lds, stream, kp, sp);
    return narrow ? launch(awv::biwfa_align_kernel<false, int16_t, S>, grid, dyn_lds, stream, kp, sp)
                  : launch(awv::biwfa_align_kernel<false, int32_t, S>, grid, dyn_lds, stream, kp, sp);
  }
  if (two_piece) return narrow ? launch(awv::biwfa_align_kernel<true, int16_t>, grid, dyn_lds, stream, kp)
                               : launch(awv::biwfa_align_kernel<true, int32_t>, grid, dyn_lds, stream, kp);
  return narrow ? launch(awv::biwfa_align_kernel<false, int16_t>, grid, dyn_lds, stream, kp)
                : launch(awv::biwfa_align_kernel<false, int32_t>, grid, dyn_lds, stream, kp);
}
