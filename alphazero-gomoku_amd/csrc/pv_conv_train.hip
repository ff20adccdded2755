// Train-step 3x3 conv: the halo-staged tile (pv_halo.h) with the BatchNorm partial sums
// fused into the epilogue and, in the forward, the previous layer's BN apply fused into
// the staging.  Replaces the conv2d and the statistics / backward-sum passes of train-mode
// batch_norm in the reference ResidualBlock (network.py:9-26).
#include "pv_internal.h"
#include "pv_halo.h"

namespace azg {

// Train-step conv (forward z = conv(a), dgrad = conv(dZ, flipped W) [+ resid]) with
// the BatchNorm partial sums fused into the epilogue (pv_halo.h XE_STATS / XE_BNBWD):
// 128-row M tiles (the partials are per 128-row tile) x 64 channels, 8 waves, two
// workgroups per CU.  The eval convs' XCD-aware tile order (pv_halo.h xcd_tile).  WT: outputs stored
// write-through (no dirty L2 lines at the kernel boundary).  PRO (forward only): the
// input is the previous layer's raw output z and its BN + ReLU (+ residual) is applied
// in the halo staging (pv_halo.h ProX).
template <int C, int NWT>
struct TrainTile {
    static constexpr int BN = NWT >= 16 ? 128 : 64;
    using T = ConvTile<C, BN, 4, 1, NWT>;
};
template <int C, int EPI, int XE, bool WT, int PRO = PRO_NONE, int VAR = kHaloTrain, int NWT = 8>
__global__ __launch_bounds__(64 * NWT) __attribute__((amdgpu_waves_per_eu(4))) void conv3x3_train(
    const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ resid,
    float* __restrict__ out, int M, EpiX ex, ProX px, FinX fx, const float* __restrict__ oscale, H3Guard guard)
{
    using T = typename TrainTile<C, NWT>::T;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTN = C / T::BN;
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    halo_tile<C, T::BN, 4, 1, NWT, EPI, WT, VAR, XE, PRO>(in, wp, oscale, nullptr, resid, out,
                                                       wt_rsrc(out, padded_bytes(M, C)), M, (t / NTN) * T::BM,
                                                       (t % NTN) * T::BN, smem, ex, px, fx, guard);
}

// ---- host launchers ------------------------------------------------------

int g_train_h3 = 2;   // key 49: 0 fp32 MFMA, 1 split-fp16 (3 products), 2 split-fp16 with 4 products (default)
int g_train_dgrad_h3 = 0;   // key 50: the dgrad convs, likewise (inputs scaled by 2^k from their max); measured slower and
                            // below the two-step goldens: off by default

// Train convs: 128 x 64 tiles, 8 waves (two workgroups per CU), buffer-resource operand
// addressing (kHaloTrain and the H3 bodies), outputs stored write-through.
template <int C, int EPI, int XE, int PRO, int VAR>
static hipError_t launch_train_v(const TrainConv& c, const H3Guard& guard, hipStream_t st)
{
    using T = typename TrainTile<C, 8>::T;
    constexpr int lds = halo_lds_bytes<C, T::BN, 4, 1, 8, VAR, PRO>();
    static bool attr_done = false;
    if (hipError_t e = set_dynamic_lds(conv3x3_train<C, EPI, XE, true, PRO, VAR, 8>, lds, attr_done)) return e;
    dim3 grid(((c.M + T::BM - 1) / T::BM) * (C / T::BN));
    hipLaunchKernelGGL((conv3x3_train<C, EPI, XE, true, PRO, VAR, 8>), grid, dim3(T::NT), lds, st, c.in, c.wp,
                       c.resid, c.out, c.M, *c.ex, PRO != PRO_NONE ? *c.px : ProX{}, c.fx ? *c.fx : FinX{}, c.oscale,
                       guard);
    return hipGetLastError();
}

// The body of one (EPI, XE, PRO) launch: split-fp16 when the caller passed the H3 packs
// (c.oscale), else fp32 MFMA.
template <int C, int EPI, int XE, int PRO = PRO_NONE>
static hipError_t launch_train_t(const TrainConv& c, hipStream_t st)
{
    // split-fp16 dgrad (key 50; oscale = the layer's 2^-e, dmax = its input's max |dz| bits):
    // four products or three, the input staged times 2^k
    if constexpr (XE == XE_BNBWD && PRO == PRO_NONE) {
        if (c.oscale && c.dmax) {
            const H3Guard g{nullptr, 1u, c.dmax};
            return g_train_dgrad_h3 == 2 ? launch_train_v<C, EPI, XE, PRO, kHaloH3Train4>(c, g, st)
                                         : launch_train_v<C, EPI, XE, PRO, kHaloH3Train>(c, g, st);
        }
    }
    // split-fp16 forward (key 49 = 2: with the fourth, lo x lo product); a range overflow is
    // posted to h3ovf
    if constexpr (EPI == EPI_RAW && XE == XE_STATS) {
        if (c.oscale) {
            const H3Guard g{c.h3ovf, 1u, nullptr};
            return g_train_h3 == 2 ? launch_train_v<C, EPI, XE, PRO, kHaloH3Train4>(c, g, st)
                                   : launch_train_v<C, EPI, XE, PRO, kHaloH3Train>(c, g, st);
        }
    }
    if (c.oscale) return hipErrorInvalidValue;
    return launch_train_v<C, EPI, XE, PRO, kHaloTrain>(c, H3Guard{nullptr, 1u, nullptr}, st);
}

template <int CC>
static hipError_t launch_train_c(const TrainConv& c, hipStream_t st)
{
    if (c.epi == EPI_RAW && c.xe == XE_STATS) {
        if (c.px && c.px->res) return launch_train_t<CC, EPI_RAW, XE_STATS, PRO_BN_RES>(c, st);
        if (c.px) return launch_train_t<CC, EPI_RAW, XE_STATS, PRO_BN>(c, st);
        return launch_train_t<CC, EPI_RAW, XE_STATS>(c, st);
    }
    if (c.epi == EPI_RAW && c.xe == XE_BNBWD) return launch_train_t<CC, EPI_RAW, XE_BNBWD>(c, st);
    if (c.epi == EPI_ADD && c.xe == XE_BNBWD) return launch_train_t<CC, EPI_ADD, XE_BNBWD>(c, st);
    return hipErrorInvalidValue;
}

// Train conv with fused BN partials: (EPI_RAW, XE_STATS) forward, optionally with
// the input layer's BN applied in the staging (px: PRO_BN / PRO_BN_RES); (EPI_RAW |
// EPI_ADD, XE_BNBWD) dgrad.  Partials are per TRAIN_BM-row M tile; with fx (cnt set)
// the last workgroup of each N tile also runs the BN finalize (pv_halo.h FinX).
hipError_t launch_conv3x3_train(int C, const TrainConv& c, hipStream_t st)
{
    switch (C) {
        case 64: return launch_train_c<64>(c, st);
        case 128: return launch_train_c<128>(c, st);
        case 256: return launch_train_c<256>(c, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace azg
