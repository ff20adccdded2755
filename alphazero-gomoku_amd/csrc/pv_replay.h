// The replay ring, defined once for pv_replay.hip, pv_replay_weights.hip and pv_replay_average.hip.
// A ring is (cap_pos, head, count): count positions, the oldest in slot head, ring index i in
// slot (head + i) % cap_pos.  Below: that map, and the argument checks the entry points share.
#pragma once
#include "pv_internal.h"
#include <string>

namespace azg {
__host__ __device__ __forceinline__ int ring_slot(int head, int64_t i, int cap_pos)
{
    return (int)(((int64_t)head + i) % cap_pos);
}
// sym_src (pv_common.h) of square j = y * BOARD + x
__host__ __device__ __forceinline__ int sym_src_sq(int j, int s)
{
    const int y = j / BOARD;
    return sym_src(y, j - y * BOARD, s);
}

// The checks take the entry point's name (__func__) and return 0, or set_error's result, 1, with
// the message "<fn>: <which argument, and what is wrong with it>"; none makes a device call.
inline int32_t refused(const char* fn, const std::string& what, hipError_t e = hipSuccess)
{
    return set_error((std::string(fn) + ": " + what).c_str(), e);
}
#define AZG_NULL_ARG(p) ((p) ? 0 : azg::refused(__func__, #p " is null"))
// head_name / count_name: what the entry point calls the two (a write of n slots from slot at)
inline int32_t bad_ring(const char* fn, int cap_pos, int head, int count, const char* head_name = "head",
                        const char* count_name = "count")
{
    if (cap_pos < 1) return refused(fn, "cap_pos must be >= 1");
    if (count < 1 || count > cap_pos) return refused(fn, std::string(count_name) + " outside [1, cap_pos]");
    if (head < 0 || head >= cap_pos) return refused(fn, std::string(head_name) + " outside [0, cap_pos)");
    return 0;
}
inline int32_t bad_nsym(const char* fn, int nsym) { return nsym == 1 || nsym == 8 ? 0 : refused(fn, "nsym must be 1 or 8"); }
inline int32_t bad_batch(const char* fn, int batch) { return batch >= 1 ? 0 : refused(fn, "batch must be >= 1"); }
inline int32_t launched(const char* fn, const char* what)   // after a launch: 0, or "<fn>: <what>: <the HIP error>"
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : refused(fn, what, e);
}
}  // namespace azg
