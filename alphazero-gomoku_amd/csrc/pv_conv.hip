// Per-layer 3x3 convolution (pad 1, no bias) of the eval forward: the halo-staged
// fp32-MFMA / split-fp16 tile of pv_halo.h (halo_tile), one launch per conv, with the
// BatchNorm / residual / ReLU epilogue fused.
//
// Replaces the ATen conv2d + batch_norm + relu (+ in-place residual add) chain of
// the reference ResidualBlock (network.py:9-26).  The stem is pv_stem.hip, the
// persistent tower pv_tower.hip, the train step's conv pv_conv_train.hip.
//
// This file is the kernel wrapper (conv3x3_halo: one BM x BN tile per workgroup, in
// the XCD-aware tile order) and the host side: the tile shapes, the autotuner that
// times them on the real operands, the tail split of the 128x64 launch and key 22's
// tile-body variants.  Every shape and body computes the same per-element K order, so
// none of these choices changes a result bit.
#include "pv_internal.h"
#include "pv_halo.h"

#include <algorithm>
#include <map>
#include <utility>

namespace azg {

// Per-layer launch of the halo-staged tile (pv_halo.h), in the XCD-aware tile order.
template <int C, int BN_, int WM_, int TM_, int NW_, int EPI, int VAR = 0>
__global__ __launch_bounds__(64 * NW_, 2) void conv3x3_halo(
    const float* __restrict__ in, const float* __restrict__ wp,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ resid, float* __restrict__ out, int M, H3Guard guard)
{
    using T = ConvTile<C, BN_, WM_, TM_, NW_>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTN = C / T::BN;
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    halo_tile<C, BN_, WM_, TM_, NW_, EPI, false, VAR>(in, wp, scale, shift, resid, out,
                                     __builtin_amdgcn_make_buffer_rsrc(out, (short)0, 0, 0x00020000), M,
                                     (t / NTN) * T::BM, (t % NTN) * T::BN, smem, EpiX{}, ProX{}, FinX{}, guard);
}

// ---- host launchers ------------------------------------------------------
// `c` is the launch (pv_internal.h ConvCall); every launcher hands it down unchanged.

template <int C, int BN, int WM, int TM, int NW, int EPI, int VAR = 0>
static hipError_t launch_halo_t(const ConvCall& c, const H3Guard& guard = H3Guard{})
{
    using T = ConvTile<C, BN, WM, TM, NW>;
    constexpr int lds = halo_lds_bytes<C, BN, WM, TM, NW, VAR>();
    static bool attr_done = false;
    if (hipError_t e = set_dynamic_lds(conv3x3_halo<C, BN, WM, TM, NW, EPI, VAR>, lds, attr_done)) return e;
    dim3 grid(((c.M + T::BM - 1) / T::BM) * (C / T::BN));
    hipLaunchKernelGGL((conv3x3_halo<C, BN, WM, TM, NW, EPI, VAR>), grid, dim3(T::NT), lds, c.st, c.in, c.wp,
                       c.scale, c.shift, c.resid, c.out, c.M, guard);
    return hipGetLastError();
}

// The halo kernel's epilogues.  Only the plain body (VAR 0) is built with the residual-free
// EPI_ADD / EPI_RAW; the variant and H3 bodies take the two eval epilogues.
template <int C, int BN, int WM, int TM, int NW = 4, int VAR = 0>
static hipError_t launch_halo_epi(int epi, const ConvCall& c, const H3Guard& guard = H3Guard{})
{
    if (epi == EPI_BN_RELU) return launch_halo_t<C, BN, WM, TM, NW, EPI_BN_RELU, VAR>(c, guard);
    if (epi == EPI_BN_RES_RELU) return launch_halo_t<C, BN, WM, TM, NW, EPI_BN_RES_RELU, VAR>(c, guard);
    if constexpr (VAR == 0) {
        if (epi == EPI_ADD) return launch_halo_t<C, BN, WM, TM, NW, EPI_ADD>(c);
        return launch_halo_t<C, BN, WM, TM, NW, EPI_RAW>(c);
    }
    return hipErrorInvalidValue;
}

// Tile shapes {BM, BN}: index into the switch of launch_shape_c below.
struct TileShape { int bm, bn; };
// 0-5: 4 waves; 6-9: 8 waves (more waves per SIMD at the same LDS footprint).
static const TileShape kShapes[] = {{128, 128}, {96, 128}, {160, 128}, {64, 128}, {128, 64}, {64, 64},
                                    {128, 128}, {128, 128}, {128, 64}, {64, 128}};
constexpr int kNumShapes = (int)(sizeof(kShapes) / sizeof(kShapes[0]));   // autotuning times all of them
constexpr int kNumAutoShapes = 6;   // heuristic pick_conv_tile only considers 0-5
// 10-12 were the single-buffer tiles (measured slower everywhere, retired): key 1 still takes
// the numbers it took, and a launch forced to one fails with hipErrorInvalidValue
constexpr int kLastRetiredShape = 12;

static bool shape_ok(int shape, int C)
{
    if (shape < 0 || shape > kLastRetiredShape) return false;
    if (C == 64) return shape == 4 || shape == 5 || shape == 8 || shape == 10 || shape == 11;
    return true;
}
constexpr int kNumCUs = 256;

// Pick the shape that wastes the fewest workgroup slots: 2 workgroups fit per CU
// (LDS <= 80 KB, <= 128 VGPRs), tiles run in rounds of 512 slots, so the cost is
// rounds * slot work.  Ties go to the larger tile (more operand reuse).
int pick_conv_tile(int C, int M)
{
    int best = -1;
    double best_eff = -1.0;
    for (int i = 0; i < kNumAutoShapes; ++i) {
        const int bm = kShapes[i].bm, bn = kShapes[i].bn;
        if (bn > C) continue;
        if (C == 64 && !(bm == 128 || bm == 64)) continue;
        const long slots = 2L * kNumCUs;
        const long tiles = (long)((M + bm - 1) / bm) * (C / bn);
        const long rounds = (tiles + slots - 1) / slots;
        double eff = (double)M * C / ((double)rounds * slots * bm * bn);
        eff *= 1.0 - 0.03 * (bm * bn < 128 * 128) - 0.03 * (bm * bn < 64 * 128);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = i; }
    }
    return best;
}

// Tail split of the 128x64 / 8-wave launch (shape 8): its tiles run in rounds of 512
// resident workgroups (2 per CU), and a last round holding a few tiles costs a whole
// round (B = 2048: 7,200 tiles = 14 rounds + 32 tiles).  The boards of the last,
// partial round go to a second launch of 64x64 / 4-wave tiles, which spreads them
// over the chip at up to 4 per CU.  Every tile shape computes the same per-element K
// order, so the split is bitwise neutral.  Key 21 (default 1) switches it.
int g_conv_tail_split = 1;

int g_conv_var = 1;   // key 22: tile-body variant of the per-layer 128x64 launch (1 default: halo rows keyed on
                      // the board position, conflict-free fragment reads, +0.5 % in-process A/B; 0, 4, 5; bitwise identical)

// the 128x64 / 8-wave launch: key 22's body for the eval epilogues, the plain body otherwise
template <int CC>
static hipError_t launch_s8(int epi, const ConvCall& c)
{
    if (epi == EPI_BN_RELU || epi == EPI_BN_RES_RELU) {
        if (g_conv_var == 1) return launch_halo_epi<CC, 64, 4, 1, 8, HV_BOARD_SWZ>(epi, c);
        if (g_conv_var == 4) return launch_halo_epi<CC, 64, 4, 1, 8, HV_LDS_DMA>(epi, c);
        if (g_conv_var == 5) return launch_halo_epi<CC, 64, 4, 1, 8, HV_LDS_DMA | HV_BOARD_SWZ>(epi, c);
    }
    return launch_halo_epi<CC, 64, 4, 1, 8>(epi, c);
}

template <int CC>
static hipError_t launch_shape8_split(int epi, const ConvCall& c)
{
    constexpr int BM = 128, NTN = CC / 64, SLOTS = 512;
    const int B = c.M / PIX;
    const int ntiles = ((c.M + BM - 1) / BM) * NTN;
    const int rounds = ntiles / SLOTS, rem = ntiles - rounds * SLOTS;
    if (!g_conv_tail_split || c.M % PIX != 0 || rounds < 2 || rem == 0 || rem > SLOTS / 2) return launch_s8<CC>(epi, c);
    int B1 = (int)((long)rounds * SLOTS / NTN * BM / PIX);    // boards of whole rounds
    while (B1 > 0 && ((B1 * PIX + BM - 1) / BM) * NTN > rounds * SLOTS) --B1;
    if (B1 <= 0 || B1 >= B) return launch_s8<CC>(epi, c);
    ConvCall head = c, tail = c;
    head.M = B1 * PIX;
    const size_t off = (size_t)B1 * PADPIX * CC;
    tail.in += off;
    if (tail.resid) tail.resid += off;
    tail.out += off;
    tail.M = (B - B1) * PIX;
    if (hipError_t e = launch_s8<CC>(epi, head)) return e;
    return launch_halo_epi<CC, 64, 2, 1>(epi, tail);
}

// Shape -> tile.  C = 64 has the 64-channel tiles only (0 is 4 there; 8 without the tail split).
template <int CC>
static hipError_t launch_shape_c(int shape, int epi, const ConvCall& c)
{
    switch (shape) {
        case 0: return launch_halo_epi<CC, (CC < 128 ? CC : 128), 2, 2>(epi, c);
        case 4: return launch_halo_epi<CC, 64, 2, 2>(epi, c);
        case 5: return launch_halo_epi<CC, 64, 2, 1>(epi, c);
        case 8:
            if constexpr (CC == 64) return launch_halo_epi<CC, 64, 4, 1, 8>(epi, c);
            else return launch_shape8_split<CC>(epi, c);
    }
    if constexpr (CC > 64) {
        switch (shape) {
            case 1: return launch_halo_epi<CC, 128, 1, 3>(epi, c);
            case 2: return launch_halo_epi<CC, 128, 1, 5>(epi, c);
            case 3: return launch_halo_epi<CC, 128, 2, 1>(epi, c);
            case 6: return launch_halo_epi<CC, 128, 2, 2, 8>(epi, c);
            case 7: return launch_halo_epi<CC, 128, 4, 1, 8>(epi, c);
            case 9: return launch_halo_epi<CC, 128, 2, 1, 8>(epi, c);
        }
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_conv3x3_shape(int shape, int C, int epi, const ConvCall& c)
{
    switch (C) {
        case 64: return launch_shape_c<64>(shape, epi, c);
        case 128: return launch_shape_c<128>(shape, epi, c);
        case 256: return launch_shape_c<256>(shape, epi, c);
        default: return hipErrorInvalidValue;
    }
}

// Split-fp16 (H3) per-layer conv (pv_halo.h kHaloH3Eval; wp / scale = the H3 packs of
// pv_pack.hip pack_h3): the eval tower's arithmetic per layer (bitwise equal to it), the
// 64x64 / 4-wave tile (shape 5) or the 128x64 / 8-wave tile (shape 8).
template <int CC>
static hipError_t launch_h3_c(int shape, int epi, const ConvCall& c, const H3Guard& g)
{
    if (shape == 8) return launch_halo_epi<CC, 64, 4, 1, 8, kHaloH3Eval>(epi, c, g);
    return launch_halo_epi<CC, 64, 2, 1, 4, kHaloH3Eval>(epi, c, g);
}
hipError_t launch_conv3x3_h3(int shape, int C, int epi, const ConvCall& c, unsigned* ring, unsigned seq)
{
    const H3Guard g{ring, seq};
    switch (C) {
        case 128: return launch_h3_c<128>(shape, epi, c, g);
        case 256: return launch_h3_c<256>(shape, epi, c, g);
        default: return hipErrorInvalidValue;
    }
}

int g_conv_shape_override = -1;
int g_conv_autotune = 1;

// Autotune: the first launch for a (C, M) times every valid shape twice on the
// real operands (each launch fully rewrites `out`, so this is idempotent) and
// caches the fastest.  All shapes give bitwise-identical results (the K order is
// shape-independent), so tuning never changes numerics.  Skipped while the
// stream is being captured into a graph (falls back to pick_conv_tile).
static std::map<std::pair<int, int>, int>& tune_cache()
{
    static std::map<std::pair<int, int>, int> c;
    return c;
}

// Autotuning is cached per (C, batch bucket): exact batch up to 256 boards (rounded
// up to 16), then 1/8-octave buckets -- self-play batches vary every round and must
// not re-tune (each tuning synchronises the stream).
int conv_batch_bucket(int M)
{
    const int b = (M + PIX - 1) / PIX;
    if (b <= 256) return (b + 15) / 16 * 16;
    int p = 256;
    while (p * 2 <= b) p *= 2;
    const int q = p / 8;
    return (b + q - 1) / q * q;
}

// Times every candidate shape on the real operands: one untimed pass over all
// candidates (clocks, caches, code objects), then kTuneRounds interleaved timed
// rounds; a shape's score is its best round.  A preferred shape (see below) is
// kept unless another is > 2 % faster -- single-launch timings picked worse shapes
// on some boxes.
constexpr int kTuneRounds = 3;
constexpr int kPreferredShape = 5;

static int autotune_shape(int C, int epi, const ConvCall& c)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c.st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return -1;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return -1;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return -1; }
    float best_ms[kNumShapes];
    bool ok[kNumShapes];
    for (int s = 0; s < kNumShapes; ++s) {
        best_ms[s] = 1e30f;
        ok[s] = shape_ok(s, C) && launch_conv3x3_shape(s, C, epi, c) == hipSuccess;
    }
    for (int r = 0; r < kTuneRounds; ++r) {
        for (int s = 0; s < kNumShapes; ++s) {
            if (!ok[s]) continue;
            (void)hipEventRecord(e0, c.st);
            if (launch_conv3x3_shape(s, C, epi, c) != hipSuccess) {
                ok[s] = false;
                continue;
            }
            (void)hipEventRecord(e1, c.st);
            if (hipEventSynchronize(e1) != hipSuccess) { ok[s] = false; continue; }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (ms < best_ms[s]) best_ms[s] = ms;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipGetLastError();
    int best = -1;
    for (int s = 0; s < kNumShapes; ++s)
        if (ok[s] && (best < 0 || best_ms[s] < best_ms[best])) best = s;
    // timing noise: keep the preferred shape unless another is > 2 % faster -- 64x64
    // (shape 5) below ~1536 boards, 128x64 / 8 waves (shape 8, with the tail split)
    // above, where in-process A/B measured it ~1 % ahead (scripts/conv_shape_ab.py)
    const int pref = (c.M / PIX >= 1536 && ok[8]) ? 8 : kPreferredShape;
    if (best >= 0 && ok[pref] && best_ms[pref] <= 1.02f * best_ms[best]) best = pref;
    return best;
}

hipError_t launch_conv3x3(int C, int epi, const ConvCall& c)
{
    int shape = -1;
    if (g_conv_shape_override >= 0 && shape_ok(g_conv_shape_override, C)) {
        shape = g_conv_shape_override;
    } else {
        auto key = std::make_pair(C, conv_batch_bucket(c.M));
        auto it = tune_cache().find(key);
        if (it != tune_cache().end()) {
            shape = it->second;
        } else if (g_conv_autotune) {
            shape = autotune_shape(C, epi, c);
            if (shape >= 0) tune_cache()[key] = shape;
        }
        if (shape < 0) shape = pick_conv_tile(C, c.M);
    }
    if (C == 64 && !shape_ok(shape, C)) shape = 5;
    return launch_conv3x3_shape(shape, C, epi, c);
}

int conv_tuned_shape(int C, int M)
{
    auto it = tune_cache().find(std::make_pair(C, conv_batch_bucket(M)));
    return it == tune_cache().end() ? -1 : it->second;
}

}  // namespace azg
