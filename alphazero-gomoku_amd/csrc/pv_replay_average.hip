// Position averaging in the replay ring (include/azg_pv.h azg_pv_replay_canon_keys,
// azg_pv_replay_average), beside the gather of pv_replay.hip, which reads the arrays written
// here through the pointers it always took; ring_slot and the argument checks are pv_replay.h's.
//   canon_keys  one 64-bit key per position, equal for all 8 dihedral images of a board
//               (the minimum of the images' Zobrist-style hashes), and the image that attains it;
//   average     positions whose canonical boards are equal (adjacent after the caller's stable
//               sort by key; the boards themselves are compared, so a key collision can only
//               split a group, never merge two) get the mean of their targets, each in its own
//               orientation.
// Keys are integers; the means are fp64 sums in ring order rounded once: a host restatement
// (tests/replay_average_reference.py) reproduces every bit.  No atomics anywhere.
#include "pv_replay.h"

namespace azg {

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint64_t wave_xor(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64);
        const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        v ^= ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// ------------------------------------------------------------------------------- keys
constexpr int KEY_WAVES = 4;   // 256 threads: 225 squares, the last wave only partly used

// One 256-thread workgroup per position at a time (grid-stride over ring indices, so a
// thread hashes its square's two values once).  Thread j < 225 owns IMAGE square j: for
// each image s it contributes Z(j, img_s[j]) to that image's XOR, reduced over the wave by
// __shfl_xor and over the 4 waves through LDS.  Threads 225..255 contribute 0 to every XOR.
__global__ __launch_bounds__(256) void replay_canon_keys_kernel(const int8_t* __restrict__ stones, int cap_pos,
                                                                int head, int count, int nsym,
                                                                int64_t* __restrict__ keys, int8_t* __restrict__ syms)
{
    __shared__ int8_t board[PIX];
    __shared__ uint64_t part[KEY_WAVES][8];
    const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
    const uint64_t z1 = splitmix64(2ull * (uint64_t)j), z2 = splitmix64(2ull * (uint64_t)j + 1ull);
    int src[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) src[s] = j < PIX ? sym_src_sq(j, s) : 0;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const int slot = ring_slot(head, i, cap_pos);
        if (j < PIX) board[j] = stones[(size_t)slot * PIX + j];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            uint64_t h = 0;
            if (s < nsym && j < PIX) {
                const int8_t v = board[src[s]];
                h = v == 1 ? z1 : (v == 2 ? z2 : 0ull);
            }
            h = wave_xor(h);
            if (lane == 0) part[wave][s] = h;
        }
        __syncthreads();   // also: every thread is done with board[] before the next round's store
        if (j == 0) {
            uint64_t best = 0;
            int arg = 0;
            for (int s = 0; s < nsym; ++s) {
                uint64_t h = 0;
#pragma unroll
                for (int w = 0; w < KEY_WAVES; ++w) h ^= part[w][s];
                if (s == 0 || h < best) {   // unsigned; the smallest s among equal minima
                    best = h;
                    arg = s;
                }
            }
            keys[i] = (int64_t)best;
            syms[i] = (int8_t)arg;
        }
        // part[] is next written after the next round's first barrier, which thread 0 reaches
        // only after the reads above
    }
}

// ------------------------------------------------------------------------------ groups
__device__ __forceinline__ int ring_index(const int64_t* __restrict__ perm, int k, int count)
{
    const int64_t r = perm[k];   // clamped like the gather's ids: never outside the ring
    return r < 0 ? 0 : (r >= count ? count - 1 : (int)r);
}

// Group starts.  One wavefront per sorted place k (4 places per workgroup); a lane compares
// canonical squares lane, lane + 64, lane + 128, lane + 192 (< 225) of places k and k - 1,
// and only when their keys are equal.  The verdict is left in group_first, which the
// averaging launch overwrites with its final value:
//   group_first[r] = r   place k (ring index r) starts a group
//   group_first[r] = -1  it continues the group of place k - 1
__global__ __launch_bounds__(256) void replay_group_flags_kernel(const int8_t* __restrict__ stones, int cap_pos,
                                                                 int head, int count,
                                                                 const int64_t* __restrict__ keys_sorted,
                                                                 const int64_t* __restrict__ perm,
                                                                 const int8_t* __restrict__ syms,
                                                                 int32_t* __restrict__ group_first)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    if (k >= count) return;
    const int r = ring_index(perm, k, count);
    bool start = k == 0 || keys_sorted[k] != keys_sorted[k - 1];
    if (!start) {
        const int q = ring_index(perm, k - 1, count);
        const int8_t* a = stones + (size_t)ring_slot(head, r, cap_pos) * PIX;
        const int8_t* b = stones + (size_t)ring_slot(head, q, cap_pos) * PIX;
        const int ca = syms[r] & 7, cb = syms[q] & 7;
        bool differ = false;
        for (int j = lane; j < PIX; j += 64) differ |= a[sym_src_sq(j, ca)] != b[sym_src_sq(j, cb)];
        start = __any(differ);
    }
    if (lane == 0) group_first[r] = start ? r : -1;
}

constexpr int AVG_AHEAD = 32;   // members whose pis rows a thread has in flight at once

// lane `src` 's value in a scalar register (src is wave-uniform)
__device__ __forceinline__ int lane_int(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float lane_float(float v, int src)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// One 256-thread workgroup per sorted place; all but the groups' first places leave at once.
// Place k with ring index r starts a group iff group_first[r] == r.  This launch overwrites
// group_first while other workgroups still read it, and every value a reader can meet gives
// the same verdict: a start's entry is only ever (re)written with r itself, and a
// continuing place's entry holds -1 or its group's first ring index, neither of which is its
// own.  So the result is a fixed function of the inputs.
//
// Thread j < 225 owns CANONICAL square j and adds its fp64 sums in member order (= ring order:
// the sort is stable).  Each wavefront walks the members on its own, 64 at a time: lane l
// loads member l's (slot, image, weight, z) and the walk takes them from there into scalar
// registers (v_readlane), so a member costs no LDS access and no barrier, sym_src's switch is
// a scalar branch, and the loads from pis depend on registers only and can be in flight
// together.  A group may be the whole ring: the walk is one workgroup's, bounded by count.
__global__ __launch_bounds__(256) void replay_average_kernel(
    const float* __restrict__ pis, const float* __restrict__ zs, const float* __restrict__ pw, int cap_pos, int head,
    int count, const int64_t* __restrict__ perm, const int8_t* __restrict__ syms, float* __restrict__ pi_avg,
    float* __restrict__ z_avg, float* __restrict__ pw_avg, int32_t* group_first, int32_t* __restrict__ group_size)
{
    __shared__ int wave_first[4];
    const int k = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r0 = ring_index(perm, k, count);
    if (group_first[r0] != r0) return;   // workgroup-uniform

    // the group's length: the distance to the next start (or to the end of the ring)
    int n = 0;
    for (int base = k + 1;; base += 256) {   // at most count / 256 + 1 rounds
        const int p = base + t;
        bool stop = p >= count;
        if (!stop) {
            const int r = ring_index(perm, p, count);
            stop = group_first[r] == r;
        }
        const unsigned long long b = __ballot(stop);
        if (lane == 0) wave_first[wave] = b ? __ffsll((long long)b) - 1 : 64;
        __syncthreads();
        int first = 256;
#pragma unroll
        for (int w = 3; w >= 0; --w)
            if (wave_first[w] < 64) first = w * 64 + wave_first[w];
        __syncthreads();   // wave_first is rewritten next round
        if (first < 256) {
            n = base + first - k;
            break;
        }
    }

    // pass 1: W, Zs (in every thread) and the thread's A[j]
    double A = 0.0, W = 0.0, Zs = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int len = min(64, n - base);
        int my_slot = 0, my_sym = 0;
        float my_w = 0.f, my_z = 0.f;
        if (lane < len) {
            const int r = ring_index(perm, k + base + lane, count);
            my_slot = ring_slot(head, r, cap_pos);
            my_sym = syms[r] & 7;
            my_w = pw ? pw[my_slot] : 1.f;
            my_z = zs[my_slot];
        }
        // AVG_AHEAD rows are loaded before the first of them is added: a long walk is bound by
        // the latency of these loads, not by their number
        for (int m0 = 0; m0 < len; m0 += AVG_AHEAD) {
            float p[AVG_AHEAD];
#pragma unroll
            for (int u = 0; u < AVG_AHEAD; ++u) {
                const int m = m0 + u;
                p[u] = 0.f;
                if (m < len) {   // wave-uniform: a group of one issues one load
                    const int slot = lane_int(my_slot, m), c = lane_int(my_sym, m);
                    if (t < PIX) p[u] = pis[(size_t)slot * PIX + sym_src_sq(t, c)];
                }
            }
#pragma unroll
            for (int u = 0; u < AVG_AHEAD; ++u) {
                const int m = m0 + u;
                if (m < len) {
                    const double w = (double)lane_float(my_w, m);
                    A += w * (double)p[u];   // the product of two fp32 values is exact in fp64
                    W += w;
                    Zs += (double)lane_float(my_z, m);
                }
            }
        }
    }
    const bool weighted = W > 0.0;
    const float mean = weighted ? (float)(A / W) : 0.f;
    const float zf = (float)(Zs / (double)n), wf = (float)(W / (double)n);

    // pass 2: the mean back into every member's own orientation; wave 0 writes the scalars
    for (int base = 0; base < n; base += 64) {
        const int len = min(64, n - base);
        int my_slot = 0, my_sym = 0;
        if (lane < len) {
            const int r = ring_index(perm, k + base + lane, count);
            my_slot = ring_slot(head, r, cap_pos);
            my_sym = syms[r] & 7;
            if (wave == 0) {
                z_avg[my_slot] = zf;
                if (pw_avg) pw_avg[my_slot] = wf;
                group_first[r] = r0;
                group_size[r] = n;
            }
        }
        for (int m = 0; m < len; ++m) {
            const int slot = lane_int(my_slot, m), c = lane_int(my_sym, m);
            if (t < PIX) {
                const size_t at = (size_t)slot * PIX + sym_src_sq(t, c);
                pi_avg[at] = weighted ? mean : pis[at];   // no trusted target in the group: its own row
            }
        }
    }
}

}  // namespace azg

extern "C" int32_t azg_pv_replay_canon_keys(const int8_t* stones, int32_t cap_pos, int32_t head, int32_t count,
                                            int32_t nsym, int64_t* keys_out, int8_t* syms_out, void* stream)
{
    using namespace azg;
    if (AZG_NULL_ARG(stones) || AZG_NULL_ARG(keys_out) || AZG_NULL_ARG(syms_out)) return 1;
    if (bad_nsym(__func__, nsym) || bad_ring(__func__, cap_pos, head, count)) return 1;
    const int grid = count < 4096 ? count : 4096;
    hipLaunchKernelGGL(replay_canon_keys_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, stones,
                       cap_pos, head, count, nsym, keys_out, syms_out);
    return launched(__func__, "launch");
}

extern "C" int32_t azg_pv_replay_average(const int8_t* stones, const float* pis, const float* zs, const float* pw,
                                         int32_t cap_pos, int32_t head, int32_t count, const int64_t* keys_sorted,
                                         const int64_t* perm, const int8_t* syms, float* pi_avg, float* z_avg,
                                         float* pw_avg, int32_t* group_first, int32_t* group_size, void* stream)
{
    using namespace azg;
    if (AZG_NULL_ARG(stones) || AZG_NULL_ARG(pis) || AZG_NULL_ARG(zs) || AZG_NULL_ARG(keys_sorted) ||
        AZG_NULL_ARG(perm) || AZG_NULL_ARG(syms) || AZG_NULL_ARG(pi_avg) || AZG_NULL_ARG(z_avg) ||
        AZG_NULL_ARG(group_first) || AZG_NULL_ARG(group_size))
        return 1;
    if (!pw != !pw_avg) return refused(__func__, "pw and pw_avg must both be null or both be set");
    if (bad_ring(__func__, cap_pos, head, count)) return 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(replay_group_flags_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, st, stones, cap_pos,
                       head, count, keys_sorted, perm, syms, group_first);
    if (launched(__func__, "flags launch")) return 1;
    hipLaunchKernelGGL(replay_average_kernel, dim3((unsigned)count), dim3(256), 0, st, pis, zs, pw, cap_pos, head,
                       count, perm, syms, pi_avg, z_avg, pw_avg, group_first, group_size);
    return launched(__func__, "average launch");
}
