// variants_fold.hip -- the fold of the allele table on the device (variants_device.hpp: fold_device): rows in any order, events or
// rows already folded, become rows in key order with equal keys reduced -- count summed, rep the minimum -- in place: the rows of
// awvvar::fold_rows.  A unit of its own: it is the only one that includes rocPRIM.
//
// The order is a stable least-significant-word-first radix sort of (word, permutation) pairs over the key's three words
// (key_word 2, 1, 0; the signed fields with their sign bit flipped, so that the order is key_less' on any input): the rows
// themselves never move until the end.  Behind it one pass in four small kernels: flag the first row of every run of equal keys,
// an inclusive scan of the flags (a run's place), the flagged rows to their places, and every other row into its run's count and rep
// with one atomicAdd and one atomicMin.  rocPRIM's sort and scan use decoupled look-back inside (library code); the kernels here
// have no loop and wait for nothing: one thread per row, every index checked against n.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "variants_device.hpp"

#include <algorithm>
#include <new>
#include <string>

#include "planner_device.hpp"  // AWV_TRY, awv_internal_fail
#include "wave_ops.hpp"        // Buf

namespace awvvar {

constexpr int FOLD_THREADS = 256;

// key_word with the sign bits of the 32-bit fields flipped: unsigned order of the words is key_less' signed order
__device__ __forceinline__ uint64_t sort_word(const awv_variant& r, int k) { return k == 2 ? r.hash : key_word(r, k) ^ 0x8000000080000000ull; }

// keys[i] = word k of the row that stands at place i so far; FIRST: the places are the rows' own, and perm becomes the identity
template <bool FIRST>
__global__ __launch_bounds__(FOLD_THREADS) void awv_fold_keys_kernel(const awv_variant* rows, uint32_t* perm, uint32_t n, int k, uint64_t* keys) {
  const uint32_t i = blockIdx.x * (uint32_t)FOLD_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = FIRST ? i : perm[i];
  if (FIRST) perm[i] = i;
  keys[i] = p < n ? sort_word(rows[p], k) : ~0ull;
}

__global__ __launch_bounds__(FOLD_THREADS) void awv_fold_heads_kernel(const awv_variant* rows, const uint32_t* perm, uint32_t n, uint32_t* flags) {
  const uint32_t i = blockIdx.x * (uint32_t)FOLD_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = perm[i], q = i > 0 ? perm[i - 1] : 0u;
  flags[i] = i == 0 || p >= n || q >= n || !key_equal(rows[p], rows[q]) ? 1u : 0u;
}

// HEADS: the first row of every run goes to the run's place; else: every other row adds to its run's count and rep
template <bool HEADS>
__global__ __launch_bounds__(FOLD_THREADS) void awv_fold_reduce_kernel(const awv_variant* rows, const uint32_t* perm, const uint32_t* flags, const uint32_t* place,
                                                                        uint32_t n, awv_variant* out) {
  const uint32_t i = blockIdx.x * (uint32_t)FOLD_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = perm[i], o = place[i] - 1u;  // (place[i] >= 1: row 0 is flagged)
  if (p >= n || o >= n || (flags[i] != 0) != HEADS) return;
  if (HEADS) {
    out[o] = rows[p];
  } else {
    atomicAdd(&out[o].count, rows[p].count);
    atomicMin((unsigned long long*)&out[o].rep, (unsigned long long)rows[p].rep);
  }
}

struct FoldScratch {
  awvw::Buf<uint64_t> keys[2];
  awvw::Buf<uint32_t> perm[2];
  awvw::Buf<uint32_t> flags, place;
  awvw::Buf<awv_variant> out;
  awvw::Buf<uint8_t> temp;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

FoldScratch* fold_scratch_new() { return new FoldScratch(); }
void fold_scratch_release(FoldScratch* fs) {
  if (!fs) return;
  for (int k = 0; k < 2; ++k) {
    fs->keys[k].release();
    fs->perm[k].release();
  }
  fs->flags.release();
  fs->place.release();
  fs->out.release();
  fs->temp.release();
  if (fs->ev0) (void)hipEventDestroy(fs->ev0);
  if (fs->ev1) (void)hipEventDestroy(fs->ev1);
  delete fs;
}

int fold_device(hipStream_t stream, FoldScratch* fs, awv_variant* d_rows, uint64_t n64, uint64_t* n_out, float* ms) {
  *n_out = n64;
  if (n64 == 0) return AWV_OK;
  if (!fs || !d_rows || n64 > MAX_FOLD_ROWS) return awv_internal_fail(AWV_ERR_ARG, "variants: a fold of more than 2^31 rows");
  const uint32_t n = (uint32_t)n64;
  if (!fs->ev0) AWV_TRY(hipEventCreate(&fs->ev0));
  if (!fs->ev1) AWV_TRY(hipEventCreate(&fs->ev1));
  for (int k = 0; k < 2; ++k) {
    AWV_TRY(fs->keys[k].reserve(n));
    AWV_TRY(fs->perm[k].reserve(n));
  }
  AWV_TRY(fs->flags.reserve(n));
  AWV_TRY(fs->place.reserve(n));
  AWV_TRY(fs->out.reserve(n));
  const dim3 grid((n + FOLD_THREADS - 1) / FOLD_THREADS), block(FOLD_THREADS);
  AWV_TRY(hipEventRecord(fs->ev0, stream));
  int cur = 0;  // perm[cur]: the order so far
  for (int pass = 0; pass < 3; ++pass) {  // least significant word first; every pass is stable
    const int word = 2 - pass;
    if (pass == 0) hipLaunchKernelGGL(awv_fold_keys_kernel<true>, grid, block, 0, stream, d_rows, fs->perm[cur].p, n, word, fs->keys[0].p);
    else hipLaunchKernelGGL(awv_fold_keys_kernel<false>, grid, block, 0, stream, d_rows, fs->perm[cur].p, n, word, fs->keys[0].p);
    AWV_TRY(hipGetLastError());
    const unsigned end_bit = 64u;  // (an event's hash has 61 bits; a caller's row may hold any word)
    size_t bytes = 0;
    AWV_TRY(rocprim::radix_sort_pairs(nullptr, bytes, fs->keys[0].p, fs->keys[1].p, fs->perm[cur].p, fs->perm[cur ^ 1].p, n, 0u, end_bit, stream));
    AWV_TRY(fs->temp.reserve(std::max<size_t>(bytes, 16)));
    bytes = fs->temp.cap;
    AWV_TRY(rocprim::radix_sort_pairs(fs->temp.p, bytes, fs->keys[0].p, fs->keys[1].p, fs->perm[cur].p, fs->perm[cur ^ 1].p, n, 0u, end_bit, stream));
    cur ^= 1;
  }
  hipLaunchKernelGGL(awv_fold_heads_kernel, grid, block, 0, stream, d_rows, fs->perm[cur].p, n, fs->flags.p);
  AWV_TRY(hipGetLastError());
  size_t bytes = 0;
  AWV_TRY(rocprim::inclusive_scan(nullptr, bytes, fs->flags.p, fs->place.p, (size_t)n, rocprim::plus<uint32_t>(), stream));
  AWV_TRY(fs->temp.reserve(std::max<size_t>(bytes, 16)));
  bytes = fs->temp.cap;
  AWV_TRY(rocprim::inclusive_scan(fs->temp.p, bytes, fs->flags.p, fs->place.p, (size_t)n, rocprim::plus<uint32_t>(), stream));
  hipLaunchKernelGGL(awv_fold_reduce_kernel<true>, grid, block, 0, stream, d_rows, fs->perm[cur].p, fs->flags.p, fs->place.p, n, fs->out.p);
  hipLaunchKernelGGL(awv_fold_reduce_kernel<false>, grid, block, 0, stream, d_rows, fs->perm[cur].p, fs->flags.p, fs->place.p, n, fs->out.p);
  AWV_TRY(hipGetLastError());
  uint32_t left = 0;
  AWV_TRY(hipMemcpyAsync(&left, fs->place.p + (n - 1), sizeof(left), hipMemcpyDeviceToHost, stream));
  AWV_TRY(hipStreamSynchronize(stream));
  if (left == 0 || left > n) return awv_internal_fail(AWV_ERR_HIP, "variants: the fold's scan ends on " + std::to_string(left) + " of " + std::to_string(n) + " rows (a bug)");
  AWV_TRY(hipMemcpyAsync(d_rows, fs->out.p, (size_t)left * sizeof(awv_variant), hipMemcpyDeviceToDevice, stream));
  AWV_TRY(hipEventRecord(fs->ev1, stream));
  AWV_TRY(hipStreamSynchronize(stream));
  float t = 0;
  AWV_TRY(hipEventElapsedTime(&t, fs->ev0, fs->ev1));
  *ms += t;
  *n_out = left;
  return AWV_OK;
}

}  // namespace awvvar
