// Surprise-weighted sampling from the replay ring (include/azg_pv.h azg_pv_replay_surprise_weights,
// azg_pv_replay_prefix, azg_pv_replay_draw), beside the gather of pv_replay.hip, on pv_replay.h's ring.
// A position's weight is an integer number of quanta (one unit of weight = 2^16 quanta), so
//   prefix  the running sums in ring order are exact in any summation order, and
//   draw    the chosen position is an integer function of the random words:
//           t = floor(r * total / 2^64), j = the first position whose running sum exceeds t
// -- a host restatement in integers reproduces every id.  Only surprise_weights computes in
// floating point (fp64, operation order fixed by its contract).
#include "pv_replay.h"

namespace azg {

constexpr double kQuantaPerUnit = 65536.0;
constexpr double kQuantaMax = 2147483647.0;   // 2^31 - 1

// finite and > 0, else 0 (a NaN fails both comparisons)
__device__ __forceinline__ double sane_surprise(float v) { return (v > 0.f && v < INFINITY) ? (double)v : 0.0; }

// One workgroup.  Thread i adds the sanitised surprises i, i + 256, ... of ALL n_sum records
// in increasing order in fp64, the 256 partials are added by a fixed LDS tree (score_reduce's
// order, pv_score.hip: the sum depends on n_sum alone); then the newest n records' weights
// are written behind slot `at`, wrapping at cap_pos.
__global__ __launch_bounds__(256) void replay_surprise_weights_kernel(const float* __restrict__ surprise, int stride,
                                                                      int n, int n_sum, double mix,
                                                                      uint32_t* __restrict__ weights, int cap_pos,
                                                                      int at)
{
    __shared__ double part[256];
    const int i = threadIdx.x;
    double acc = 0.0;
    for (int b = i; b < n_sum; b += 256) {
        const float v = surprise[(size_t)b * stride];
        acc += sane_surprise(v);
    }
    part[i] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (i < s) part[i] += part[i + s];
        __syncthreads();
    }
    const double S = part[0];
    const int first = n_sum - n;   // the oldest record that survives
    for (int k = i; k < n; k += 256) {
        const float v = surprise[(size_t)(first + k) * stride];
        const double s = sane_surprise(v);
        const double w = S > 0.0 ? (1.0 - mix) + mix * (double)n_sum * s / S : 1.0;
        const double q = w * kQuantaPerUnit;
        const uint32_t out = q >= kQuantaMax ? 2147483647u : (q <= 0.0 ? 0u : (uint32_t)llrint(q));
        weights[ring_slot(at, k, cap_pos)] = out;
    }
}

// ------------------------------------------------------------------------ prefix sums
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 4;                             // contiguous elements per thread
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;      // elements per workgroup

__device__ __forceinline__ uint64_t wave_scan_incl(uint64_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)v, o, 64);
        const uint32_t hi = __shfl_up((uint32_t)(v >> 32), o, 64);
        if (lane >= o) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// Exclusive prefix of `mine` over the workgroup's 256 threads (4 waves): wavefront scan by
// __shfl_up, the waves' totals through LDS.  *block_total = the sum over all threads.
__device__ __forceinline__ uint64_t block_scan_excl(uint64_t mine, uint64_t* wave_tot /* LDS [4] */,
                                                    uint64_t* block_total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t incl = wave_scan_incl(mine, lane);
    __syncthreads();   // wave_tot may still be read from the caller's previous round
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
        const uint64_t t = wave_tot[w];
        if (w < wave) before += t;
        all += t;
    }
    *block_total = all;
    return before + (incl - mine);
}

// Pass 1: workgroup b scans logical elements [b * SCAN_TILE, ...) on its own; the tile's last
// element then holds the tile's total.
__global__ __launch_bounds__(SCAN_THREADS) void replay_prefix_tiles_kernel(const uint32_t* __restrict__ weights,
                                                                           int cap_pos, int head, int count,
                                                                           uint64_t* __restrict__ prefix)
{
    __shared__ uint64_t wave_tot[SCAN_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t v[SCAN_ITEMS];
    uint64_t mine = 0;
#pragma unroll
    for (int t = 0; t < SCAN_ITEMS; ++t) {
        const int64_t j = base + t;
        v[t] = j < count ? (uint64_t)weights[ring_slot(head, j, cap_pos)] : 0;
        mine += v[t];
        v[t] = mine;   // inclusive within the thread's chunk
    }
    uint64_t total;
    const uint64_t before = block_scan_excl(mine, wave_tot, &total);
#pragma unroll
    for (int t = 0; t < SCAN_ITEMS; ++t) {
        const int64_t j = base + t;
        if (j < count) prefix[j] = before + v[t];
    }
}

__device__ __forceinline__ int64_t tile_last(int tile, int count)
{
    const int64_t e = (int64_t)(tile + 1) * SCAN_TILE - 1;
    return e < count ? e : (int64_t)count - 1;
}

// Pass 2 (one workgroup): the tiles' totals, read from the tiles' last elements, are scanned
// in place, 256 tiles per round with the carry of the rounds before: afterwards the last
// element of every tile is final.
__global__ __launch_bounds__(SCAN_THREADS) void replay_prefix_totals_kernel(uint64_t* __restrict__ prefix, int count,
                                                                            int ntiles)
{
    __shared__ uint64_t wave_tot[SCAN_THREADS / 64];
    uint64_t carry = 0;
    for (int t0 = 0; t0 < ntiles; t0 += SCAN_THREADS) {
        const int tile = t0 + threadIdx.x;
        const uint64_t mine = tile < ntiles ? prefix[tile_last(tile, count)] : 0;
        uint64_t total;
        const uint64_t before = block_scan_excl(mine, wave_tot, &total);
        if (tile < ntiles) prefix[tile_last(tile, count)] = carry + before + mine;
        carry += total;
    }
}

// Pass 3: tile b > 0 adds the final last element of tile b - 1 to all its elements but its
// own last one (final since pass 2; no workgroup writes what another reads).
__global__ __launch_bounds__(SCAN_THREADS) void replay_prefix_offsets_kernel(uint64_t* __restrict__ prefix, int count)
{
    const int tile = blockIdx.x + 1;
    const uint64_t off = prefix[(int64_t)tile * SCAN_TILE - 1];
    const int64_t last = tile_last(tile, count);
    const int64_t base = (int64_t)tile * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
#pragma unroll
    for (int t = 0; t < SCAN_ITEMS; ++t) {
        const int64_t j = base + t;
        if (j < last) prefix[j] += off;
    }
}

// ------------------------------------------------------------------------------- draw
// One thread per batch element.  total > t always (r < 2^64), so a j with prefix[j] > t
// exists whenever total > 0; with total == 0 (nothing to choose from) the result is the
// clamp, count - 1: the id stays inside the ring either way.
__global__ __launch_bounds__(256) void replay_draw_kernel(const uint64_t* __restrict__ prefix, int count, int nsym,
                                                          const uint64_t* __restrict__ rnd, int batch,
                                                          int64_t* __restrict__ ids)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= batch) return;
    const uint64_t total = prefix[count - 1];
    const uint64_t t = __umul64hi(rnd[2 * (size_t)k], total);
    int lo = 0, hi = count - 1;   // the answer lies in [lo, hi]
#pragma unroll 1
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    const int64_t sym = nsym == 8 ? (int64_t)(rnd[2 * (size_t)k + 1] & 7u) : 0;
    ids[k] = (int64_t)lo * nsym + sym;
}

}  // namespace azg

extern "C" int32_t azg_pv_replay_surprise_weights(const float* surprise, int32_t stride, int32_t n, int32_t n_sum,
                                                  double mix, uint32_t* weights, int32_t cap_pos, int32_t at,
                                                  void* stream)
{
    using namespace azg;
    if (AZG_NULL_ARG(surprise) || AZG_NULL_ARG(weights)) return 1;
    if (!(mix >= 0.0 && mix <= 1.0)) return refused(__func__, "mix outside [0, 1]");
    if (stride < 1) return refused(__func__, "stride must be >= 1");
    if (bad_ring(__func__, cap_pos, at, n, "at", "n")) return 1;
    if (n_sum < n) return refused(__func__, "n_sum must be >= n");
    hipLaunchKernelGGL(replay_surprise_weights_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, surprise, stride, n,
                       n_sum, mix, weights, cap_pos, at);
    return launched(__func__, "launch");
}

extern "C" int32_t azg_pv_replay_prefix(const uint32_t* weights, int32_t cap_pos, int32_t head, int32_t count,
                                        uint64_t* prefix, void* stream)
{
    using namespace azg;
    if (AZG_NULL_ARG(weights) || AZG_NULL_ARG(prefix) || bad_ring(__func__, cap_pos, head, count)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = (int)(((int64_t)count + SCAN_TILE - 1) / SCAN_TILE);
    hipLaunchKernelGGL(replay_prefix_tiles_kernel, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, st, weights, cap_pos,
                       head, count, prefix);
    if (launched(__func__, "tiles launch")) return 1;
    if (ntiles > 1) {
        hipLaunchKernelGGL(replay_prefix_totals_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, prefix, count, ntiles);
        if (launched(__func__, "totals launch")) return 1;
        hipLaunchKernelGGL(replay_prefix_offsets_kernel, dim3((unsigned)(ntiles - 1)), dim3(SCAN_THREADS), 0, st,
                           prefix, count);
        if (launched(__func__, "offsets launch")) return 1;
    }
    return 0;
}

extern "C" int32_t azg_pv_replay_draw(const uint64_t* prefix, int32_t count, int32_t nsym, const uint64_t* rnd,
                                      int32_t batch, int64_t* ids, void* stream)
{
    using namespace azg;
    if (AZG_NULL_ARG(prefix) || AZG_NULL_ARG(rnd) || AZG_NULL_ARG(ids)) return 1;
    if (count < 1) return refused(__func__, "count must be >= 1");   // no cap_pos here: prefix is in ring order
    if (bad_nsym(__func__, nsym) || bad_batch(__func__, batch)) return 1;
    hipLaunchKernelGGL(replay_draw_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       prefix, count, nsym, rnd, batch, ids);
    return launched(__func__, "launch");
}
