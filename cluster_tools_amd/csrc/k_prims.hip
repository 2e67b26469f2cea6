// k_prims.hip — the device-wide primitives of the feature calls, one instantiation each: radix
// sorts, exclusive sum, run-length encode and reduce-by-key from hipcub.  Besides the segmented
// sort of k_seeded.hip this is the library's only use of hipcub.
//
// Every function sizes the temporary storage when tmp == nullptr (bytes is set, nothing runs) and
// runs on `stream` otherwise.  The host sizes all primitives of a call first, grows the handle's
// prim_tmp to the largest, and only then launches (grow may hipFree, which waits for the device).
//
// The item count n is an int64_t in every signature.  Where every caller refuses 2^31 or more items
// (sort_keys_u64, sort_pairs_u64, runs_u64, reduce_by_key_sum_u64) it goes to hipcub as an int, as
// pair_sort, ef_sort and pair_reduce passed it: rocprim's radix sort picks its offset type by the
// count's type (32-bit for an int), and the run-length encode's interface has an int.  The other
// two cannot: sort_pairs_u64_u32 takes up to 2^32 - 1 graph edges, and exclusive_sum_u32 up to 2^32
// node degrees, so they pass a size_t.  For the scan the type picks nothing: hipcub hands the count
// to rocprim::exclusive_scan, whose size parameter is a size_t and no template argument, so the
// region features' scan (an int before) runs the same instantiation as before.
#include <hipcub/hipcub.hpp>

#include "ctws_kernels.h"

namespace ctws {

// keys over the bits [0, end_bit), n < 2^31; hipcub's LSD radix sort is stable
hipError_t sort_keys_u64(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out, int64_t n,
                         int end_bit, hipStream_t stream) {
    return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys_in, keys_out, (int)n, 0, end_bit, stream);
}

// (key, value) pairs by key over the bits [0, end_bit), n < 2^31
hipError_t sort_pairs_u64(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                          const uint64_t* vals_in, uint64_t* vals_out, int64_t n, int end_bit, hipStream_t stream) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit,
                                              stream);
}

// (key, 32-bit value) pairs by all 64 key bits
hipError_t sort_pairs_u64_u32(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                              const uint32_t* vals_in, uint32_t* vals_out, int64_t n, hipStream_t stream) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, 64,
                                              stream);
}

hipError_t exclusive_sum_u32(void* tmp, size_t& bytes, const uint32_t* in, uint32_t* out, int64_t n,
                             hipStream_t stream) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (size_t)n, stream);
}

// sorted -> (value, count) runs and their number, n < 2^31
hipError_t runs_u64(void* tmp, size_t& bytes, const uint64_t* sorted, uint64_t* uniq, uint64_t* counts,
                    uint64_t* n_runs, int64_t n, hipStream_t stream) {
    return hipcub::DeviceRunLengthEncode::Encode(tmp, bytes, sorted, uniq, counts, n_runs, (int)n, stream);
}

// sorted keys with values -> the distinct keys, the sums of their values, their number, n < 2^31
hipError_t reduce_by_key_sum_u64(void* tmp, size_t& bytes, const uint64_t* keys, uint64_t* uniq,
                                 const uint64_t* vals, uint64_t* sums, uint64_t* n_runs, int64_t n, hipStream_t stream) {
    return hipcub::DeviceReduce::ReduceByKey(tmp, bytes, keys, uniq, vals, sums, n_runs, hipcub::Sum(), (int)n,
                                             stream);
}

}  // namespace ctws
