// Split-fp16 (H3) residual-conv tile lab (round 5).
//
// Stand-alone executable: times per-layer launches of halo_tile (pv_halo.h, HV_H3)
// at several tile shapes / register blockings on synthetic operands (padded NHWC
// activations with a zero halo, split fp16 weights in the pack_h3 layout), reports
// device time per launch (hipEvents), fp32-equivalent TFLOP/s, and whether every
// variant's output is bitwise the first variant's (all shapes share the per-element K
// order).  Not linked into the product.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I alphazero-gomoku_amd/csrc \
//       scripts/h3_lab.hip -o scripts/h3_lab
//   scripts/h3_lab <C> <boards> <reps>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <string>

#include "pv_halo.h"
#include "pv_h3.h"

using namespace azg;

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

template <int C, int BN_, int WM_, int TM_, int NW_, int VAR, int WPE>
__global__ __launch_bounds__(64 * NW_, WPE) void lab_conv(const float* __restrict__ in, const float* __restrict__ wp,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const float* __restrict__ resid, float* __restrict__ out,
                                                          int M, H3Guard guard)
{
    using T = ConvTile<C, BN_, WM_, TM_, NW_>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTN = C / T::BN;
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    halo_tile<C, BN_, WM_, TM_, NW_, EPI_BN_RES_RELU, false, VAR>(
        in, wp, scale, shift, resid, out, __builtin_amdgcn_make_buffer_rsrc(out, (short)0, 0, 0x00020000), M,
        (t / NTN) * T::BM, (t % NTN) * T::BN, smem, EpiX{}, ProX{}, FinX{}, guard);
}

template <int C, int BN_, int WM_, int TM_, int NW_, int TPS, int NWB, int WPE, int ABL = 0>
__global__ __launch_bounds__(64 * NW_, WPE) void lab_h3(const float* __restrict__ in, const float* __restrict__ wp,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ shift,
                                                        const float* __restrict__ resid, float* __restrict__ out,
                                                        int M, H3Guard guard)
{
    using T = ConvTile<C, BN_, WM_, TM_, NW_>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTN = C / T::BN;
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    h3_tile<C, BN_, WM_, TM_, NW_, TPS, NWB, EPI_BN_RES_RELU, false, 0, ABL & 7, ABL & ~7>(
        in, wp, scale, shift, resid, out, __builtin_amdgcn_make_buffer_rsrc(out, (short)0, 0, 0x00020000), M,
        (t / NTN) * T::BM, (t % NTN) * T::BN, smem, guard);
}

// ---- 16x16x32 study: h3_tile's 128x128 / 4-wave body with v_mfma_f32_16x16x32_f16 (4x4 blocks
// of 16x16 per wave: the same LDS bytes per MFMA cycle, a different K order per instruction, so
// not bitwise the product).  Lab only: does the smaller MFMA shape run faster here?
template <int C>
__global__ __launch_bounds__(256, 2) void lab_h3_16(const float* __restrict__ in, const float* __restrict__ wp,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    const float* __restrict__ resid, float* __restrict__ out, int M)
{
    using H = H3Tile<C, 128, 2, 2, 4, 1, 3>;
    constexpr int BM = 128, BN = 128, BK = 32, CG = C / 32, NW = 4, NT = 256, RPP = H::RPP, H_LD = H::H_LD,
                  HR = H::HR, NST = 9, NSTAGE = CG * 9, PPW = H::PPW, BNP = BN / 8, NWB = 3;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTN = C / BN;
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    const int m0 = (t / NTN) * BM, n0 = (t % NTN) * BN;
    float* Ah = smem;
    float* Bs = smem + HR * BK;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / 2, wn = wid % 2;
    const int mlast = min(m0 + BM, M) - 1;
    const int hbase = pad_row(m0) - (PADW + 1);
    const int hmax = pad_row(mlast) + (PADW + 1);
    const int sr = tid >> 3, sc = (tid & 7) * 4;
    int hsrc[H_LD], hkey[H_LD];
#pragma unroll
    for (int i = 0; i < H_LD; ++i) {
        const int r = min(hbase + sr + RPP * i, hmax);
        hsrc[i] = (r * C + sc) * 4;
        hkey[i] = (halo_vkey(hbase + sr + RPP * i) >> 1) & 7;
    }
    const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), (short)0,
                                                                          0x7fffffff, 0x00020000);
    f32x4 rh[H_LD];
    auto hload = [&](int g, int i) {
        rh[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rs, hsrc[i] + g * BK * 4, 0, 0));
    };
    auto hstore = [&]() {
        const int q = (tid & 7) >> 1, half = (tid & 1) * 2;
#pragma unroll
        for (int i = 0; i < H_LD; ++i) {
            f16x4 hi, lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                hi[e] = (_Float16)rh[i][e];
                lo[e] = (_Float16)(rh[i][e] - (float)hi[e]);
            }
            float* row = Ah + (sr + RPP * i) * BK;
            *(f16x4*)(row + ((q ^ hkey[i]) * 4) + half) = hi;
            *(f16x4*)(row + (((4 + q) ^ hkey[i]) * 4) + half) = lo;
        }
    };
    const int lr = lane >> 3, ls = lane & 7;
    int woff[PPW], wdst[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int p = wid + NW * i;
        const int tt = p / BNP, row = (p % BNP) * 8 + lr;
        woff[i] = tt * C * BK * CG + (n0 + row) * BK + ((ls ^ ((row >> 1) & 7)) * 4);
        wdst[i] = (tt * BN + (p % BNP) * 8) * BK;
    }
    auto dma_stage = [&](int s) {
        const int g = s / NST, t0 = s % NST;
        const float* src = wp + (size_t)(t0 * CG + g) * C * BK;
        float* dst = Bs + (s % NWB) * BN * BK;
#pragma unroll
        for (int i = 0; i < PPW; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + woff[i]),
                                             (__attribute__((address_space(3))) void*)(dst + wdst[i]), 16, 0, 0);
    };
    // 16x16x32 fragments: lane -> row / col (lane & 15), K slot (lane >> 4) of the 32-channel row
    const int r16 = lane & 15, ks = lane >> 4;
    int hrow[4], vpix[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pr = pad_row(min(m0 + wm * 64 + i * 16 + r16, M - 1));
        hrow[i] = pr - hbase;
        vpix[i] = halo_vkey(pr);
    }
    const int bswz = (r16 >> 1) & 7;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    dma_stage(0);
    dma_stage(1);
#pragma unroll
    for (int i = 0; i < H_LD; ++i) hload(0, i);
    h3_wait_vm(0);
    hstore();
    h3_raw_barrier();
#pragma unroll
    for (int cg = 0; cg < CG; ++cg) {
        // (one accumulation chain: timing study -- no per-group partial sums, unlike the product)
        f32x4 (&at)[4][4] = acc;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int s = cg * 9 + tap;
            if (s + 2 < NSTAGE) dma_stage(s + 2);
            __builtin_amdgcn_sched_barrier(0);
            if (cg + 1 < CG && tap < H_LD) hload(cg + 1, tap);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(hrow[i]), "+v"(vpix[i]));
            const int d = (tap / 3 - 1) * PADW + (tap % 3 - 1);
            const int vd = (tap / 3 - 1) * BOARD + (tap % 3 - 1);
            const float* Bb = Bs + (s % NWB) * BN * BK;
            f16x8 ah[4], al[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ar = (hrow[i] + d) * BK, aw = ((vpix[i] + vd) >> 1) & 7;
                ah[i] = *(const f16x8*)(Ah + ar + ((ks ^ aw) * 4));
                al[i] = *(const f16x8*)(Ah + ar + (((4 + ks) ^ aw) * 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* br = Bb + (wn * 64 + j * 16 + r16) * BK;
                const f16x8 bh = *(const f16x8*)(br + ((ks ^ bswz) * 4));
                const f16x8 bl = *(const f16x8*)(br + (((4 + ks) ^ bswz) * 4));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    at[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, at[i][j], 0, 0, 0);
                    at[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, at[i][j], 0, 0, 0);
                    at[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, at[i][j], 0, 0, 0);
                }
            }
            if (s + 1 < NSTAGE) h3_wait_vm(h3_wait_next<C, 128, 2, 2, 4, 1, 3, 0>(s));
            else h3_wait_vm(0);
            h3_raw_barrier();
        }
        if (cg + 1 < CG) {
            h3_wait_vm(h3_wait_halo<C, 128, 2, 2, 4, 1, 3, 0>(cg));
            hstore();
            h3_raw_barrier();
        }
    }
    // epilogue through LDS: [BM][BN] tile, then 16-B runs of 4 channels per thread
    float* Es = smem;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Es[(wm * 64 + i * 16 + 4 * ks + r) * BN + wn * 64 + j * 16 + r16] = acc[i][j][r];
    __syncthreads();
    constexpr int CPR = BN / 4, RPI = NT / CPR, NPASS = BM / RPI;
    const int ec = (tid % CPR) * 4, er = tid / CPR, col = n0 + ec;
    const f32x4 s4 = *(const f32x4*)(scale + col), t4 = *(const f32x4*)(shift + col);
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        const int m = m0 + er + p * RPI;
        if (m < M) {
            f32x4 v = *(const f32x4*)(Es + (er + p * RPI) * BN + ec);
            const int o = pad_off(m, C) + col;
            const f32x4 rv = *(const f32x4*)(resid + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(v[e], s4[e], t4[e]) + rv[e], 0.f);
            *(f32x4*)(out + o) = v;
        }
    }
}
template <int C>
static void launch_16(const float* in, const float* wp, const float* sc, const float* sh, const float* rs, float* out,
                      int M, H3Guard, hipStream_t st)
{
    constexpr int lds = H3Tile<C, 128, 2, 2, 4, 1, 3>::LDS;
    dim3 grid(((M + 127) / 128) * (C / 128));
    hipLaunchKernelGGL((lab_h3_16<C>), grid, dim3(256), lds, st, in, wp, sc, sh, rs, out, M);
}
template <int C>
static hipError_t prep_16()
{
    return hipFuncSetAttribute((const void*)lab_h3_16<C>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               H3Tile<C, 128, 2, 2, 4, 1, 3>::LDS);
}

struct Variant {
    std::string name;
    int C;
    int bm, bn;
    size_t lds;
    void (*launch)(const float*, const float*, const float*, const float*, const float*, float*, int, H3Guard,
                   hipStream_t);
    hipError_t (*prep)();
};

template <int C, int BN, int WM, int TM, int NW, int VAR, int WPE>
static void launch_v(const float* in, const float* wp, const float* sc, const float* sh, const float* rs, float* out,
                     int M, H3Guard g, hipStream_t st)
{
    using T = ConvTile<C, BN, WM, TM, NW>;
    constexpr int lds = halo_lds_bytes<C, BN, WM, TM, NW, VAR>();
    dim3 grid(((M + T::BM - 1) / T::BM) * (C / T::BN));
    hipLaunchKernelGGL((lab_conv<C, BN, WM, TM, NW, VAR, WPE>), grid, dim3(T::NT), lds, st, in, wp, sc, sh, rs, out,
                       M, g);
}
template <int C, int BN, int WM, int TM, int NW, int VAR, int WPE>
static hipError_t prep_v()
{
    constexpr int lds = halo_lds_bytes<C, BN, WM, TM, NW, VAR>();
    return hipFuncSetAttribute((const void*)lab_conv<C, BN, WM, TM, NW, VAR, WPE>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}
template <int C, int BN, int WM, int TM, int NW, int TPS, int NWB, int WPE, int ABL = 0>
static void launch_h(const float* in, const float* wp, const float* sc, const float* sh, const float* rs, float* out,
                     int M, H3Guard g, hipStream_t st)
{
    using T = ConvTile<C, BN, WM, TM, NW>;
    constexpr int lds = h3_lds_bytes<C, BN, WM, TM, NW, TPS, NWB, ABL & ~7>();
    dim3 grid(((M + T::BM - 1) / T::BM) * (C / T::BN));
    hipLaunchKernelGGL((lab_h3<C, BN, WM, TM, NW, TPS, NWB, WPE, ABL>), grid, dim3(T::NT), lds, st, in, wp, sc, sh, rs,
                       out, M, g);
}
template <int C, int BN, int WM, int TM, int NW, int TPS, int NWB, int WPE, int ABL = 0>
static hipError_t prep_h()
{
    constexpr int lds = h3_lds_bytes<C, BN, WM, TM, NW, TPS, NWB, ABL & ~7>();
    return hipFuncSetAttribute((const void*)lab_h3<C, BN, WM, TM, NW, TPS, NWB, WPE, ABL>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}
#define VH(C, BN, WM, TM, NW, TPS, NWB, WPE)                                                                        \
    Variant{"h3_tile " #BN "x" #WM "x" #TM " nw" #NW " tps" #TPS " nwb" #NWB " wpe" #WPE, C,                      \
            ConvTile<C, BN, WM, TM, NW>::BM, BN, (size_t)H3Tile<C, BN, WM, TM, NW, TPS, NWB>::LDS,                  \
            launch_h<C, BN, WM, TM, NW, TPS, NWB, WPE>, prep_h<C, BN, WM, TM, NW, TPS, NWB, WPE>}
#define VA(C, BN, WM, TM, NW, TPS, NWB, WPE, ABL)                                                                   \
    Variant{"h3_tile " #BN "x" #WM "x" #TM " nw" #NW " tps" #TPS " nwb" #NWB " wpe" #WPE " ABLATION " #ABL, C,     \
            ConvTile<C, BN, WM, TM, NW>::BM, BN, (size_t)h3_lds_bytes<C, BN, WM, TM, NW, TPS, NWB, ABL & ~7>(),            \
            launch_h<C, BN, WM, TM, NW, TPS, NWB, WPE, ABL>, prep_h<C, BN, WM, TM, NW, TPS, NWB, WPE, ABL>}
#define V(C, BN, WM, TM, NW, VAR, WPE)                                                                              \
    Variant{#BN "x" #WM "x" #TM " nw" #NW " var" #VAR " wpe" #WPE, C, ConvTile<C, BN, WM, TM, NW>::BM, BN,         \
            (size_t)halo_lds_bytes<C, BN, WM, TM, NW, VAR>(), launch_v<C, BN, WM, TM, NW, VAR, WPE>,                \
            prep_v<C, BN, WM, TM, NW, VAR, WPE>}

template <int C>
static std::vector<Variant> variants()
{
    return {
        V(C, 64, 4, 1, 8, kHaloH3Eval, 2),    // product per-layer form: 128x64, 8 waves, wave 32x32
        Variant{"h3_tile 128x128 nw4 16x16x32 (not bitwise)", C, 128, 128,
                (size_t)H3Tile<C, 128, 2, 2, 4, 1, 3>::LDS, launch_16<C>, prep_16<C>},
        V(C, 128, 2, 2, 4, kHaloH3Eval, 2),   // 128x128, 4 waves as 2x2, wave 64x64
        // h3_tile (pv_h3.h): LDS-DMA weight stages, counted waits, raw barriers
        VH(C, 64, 4, 1, 8, 1, 2, 4),     // 128x64, wave 32x32, 1-tap stages
        VH(C, 64, 4, 1, 8, 1, 3, 4),     // ... three stage buffers
        VH(C, 64, 4, 1, 8, 3, 2, 2),     // ... 3-tap stages (one workgroup per CU by LDS)
        VH(C, 128, 2, 2, 4, 1, 2, 2),    // 128x128, wave 64x64, 1-tap stages
        VH(C, 128, 2, 2, 4, 1, 3, 2),    // ... three stage buffers
        VH(C, 128, 4, 1, 8, 1, 2, 2),    // 128x128, 8 waves, wave 32x64
        VH(C, 128, 2, 2, 8, 1, 2, 2),    // 128x128, 8 waves as 2x4, wave 64x32
        VH(C, 128, 2, 2, 4, 3, 2, 1),    // 128x128, wave 64x64, 3-tap stages, one workgroup per CU
        // OPT (ablation value bits >= 8): 8 = next-group halo loads at the group's first stage
        // -- bitwise identical
        VA(C, 128, 2, 2, 4, 1, 3, 2, 8), VA(C, 64, 4, 1, 8, 3, 2, 2, 8), VA(C, 64, 4, 1, 8, 1, 3, 4, 8),
        // OPT 32: direct epilogue (no LDS pass)
        VA(C, 128, 2, 2, 4, 1, 3, 2, 32), VA(C, 128, 4, 1, 8, 1, 2, 4, 32), VA(C, 64, 4, 1, 8, 3, 2, 2, 32),
        // 128x128 / 8 waves (wave 32x64) capped at 128 VGPRs: two workgroups per CU
        VH(C, 128, 4, 1, 8, 1, 2, 4), VH(C, 128, 4, 1, 8, 1, 3, 4), VA(C, 128, 4, 1, 8, 1, 3, 4, 8),
        VH(C, 128, 2, 2, 8, 1, 3, 4),
        // timing ablations (results invalid): 1 no epilogue, 2 no halo loads, 7 neither nor weights
        VA(C, 128, 2, 2, 4, 1, 3, 2, 1), VA(C, 128, 2, 2, 4, 1, 3, 2, 2), VA(C, 128, 2, 2, 4, 1, 3, 2, 7),
    };
}

static uint32_t lcg(uint64_t& s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

template <int C>
static int run(int B, int reps)
{
    const int M = B * PIX;
    const size_t act = (size_t)B * PADPIX * C;
    std::vector<float> h_in(act, 0.f), h_res(act, 0.f);
    uint64_t s = 12345;
    for (int b = 0; b < B; ++b)
        for (int y = 1; y <= BOARD; ++y)
            for (int x = 1; x <= BOARD; ++x)
                for (int c = 0; c < C; ++c) {
                    const size_t o = ((size_t)b * PADPIX + y * PADW + x) * C + c;
                    h_in[o] = (lcg(s) & 0xffff) / 65536.f * ((lcg(s) & 3) ? 1.f : 0.f);   // ReLU-like
                    h_res[o] = (lcg(s) & 0xffff) / 65536.f;
                }
    // split fp16 weights: [kchunk][n][hi 32 | lo 32] halves, scaled into fp16 range
    const size_t wn = (size_t)9 * C * C;
    std::vector<_Float16> h_w(2 * wn);
    for (size_t i = 0; i < wn; ++i) {
        const float v = ((float)(lcg(s) & 0xffff) / 65536.f - 0.5f) * 4096.f;
        const _Float16 hi = (_Float16)v;
        h_w[(i >> 5) * 64 + (i & 31)] = hi;
        h_w[(i >> 5) * 64 + 32 + (i & 31)] = (_Float16)(v - (float)hi);
    }
    std::vector<float> h_sc(C), h_sh(C);
    for (int c = 0; c < C; ++c) {
        h_sc[c] = 1.f / 4096.f / (float)(9 * C) * 4.f;
        h_sh[c] = ((lcg(s) & 0xff) / 256.f - 0.5f) * 0.1f;
    }
    float *d_in, *d_res, *d_out, *d_ref, *d_sc, *d_sh;
    void* d_w;
    unsigned* d_ring;
    CK(hipMalloc(&d_in, act * 4));
    CK(hipMalloc(&d_res, act * 4));
    CK(hipMalloc(&d_out, act * 4));
    CK(hipMalloc(&d_ref, act * 4));
    CK(hipMalloc(&d_w, 2 * wn * 2));
    CK(hipMalloc(&d_sc, C * 4));
    CK(hipMalloc(&d_sh, C * 4));
    CK(hipMalloc(&d_ring, kTowerRing * 4));
    CK(hipMemcpy(d_in, h_in.data(), act * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_res, h_res.data(), act * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_w, h_w.data(), 2 * wn * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_sc, h_sc.data(), C * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_sh, h_sh.data(), C * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_ring, 0, kTowerRing * 4));
    CK(hipMemset(d_out, 0, act * 4));
    CK(hipMemset(d_ref, 0, act * 4));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const H3Guard g{d_ring, 7};
    const double flop = 2.0 * M * C * 9.0 * C;
    auto vs = variants<C>();
    std::vector<float> h_out(act), h_ref(act);
    for (size_t vi = 0; vi < vs.size(); ++vi) {
        Variant& v = vs[vi];
        if (v.lds > 160 * 1024) {
            printf("{\"C\": %d, \"B\": %d, \"variant\": \"%s\", \"skipped\": \"lds %zu\"}\n", C, B, v.name.c_str(),
                   v.lds);
            continue;
        }
        CK(v.prep());
        float* dst = vi == 0 ? d_ref : d_out;
        CK(hipMemsetAsync(dst, 0, act * 4, st));
        v.launch(d_in, (const float*)d_w, d_sc, d_sh, d_res, dst, M, g, st);
        CK(hipGetLastError());
        CK(hipStreamSynchronize(st));
        float best = 1e30f, tot = 0.f;
        for (int r = 0; r < 3; ++r) {
            CK(hipEventRecord(e0, st));
            for (int i = 0; i < reps; ++i) v.launch(d_in, (const float*)d_w, d_sc, d_sh, d_res, dst, M, g, st);
            CK(hipEventRecord(e1, st));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            ms /= reps;
            best = ms < best ? ms : best;
            tot += ms;
        }
        bool same = true;
        double maxd = 0.0;
        if (vi > 0) {
            CK(hipMemcpy(h_out.data(), d_out, act * 4, hipMemcpyDeviceToHost));
            same = memcmp(h_out.data(), h_ref.data(), act * 4) == 0;
            for (size_t i = 0; i < act; ++i) {
                const double d = fabs((double)h_out[i] - (double)h_ref[i]);
                maxd = d > maxd ? d : maxd;
            }
        } else {
            CK(hipMemcpy(h_ref.data(), d_ref, act * 4, hipMemcpyDeviceToHost));
        }
        unsigned ring[kTowerRing];
        CK(hipMemcpy(ring, d_ring, sizeof(ring), hipMemcpyDeviceToHost));
        int posted = 0;
        for (unsigned k = 0; k < kTowerRing; ++k) posted += ring[k] != 0;
        printf("{\"C\": %d, \"B\": %d, \"variant\": \"%s\", \"tile\": \"%dx%d\", \"lds\": %zu, \"best_us\": %.2f, "
               "\"mean_us\": %.2f, \"tflops\": %.1f, \"bitwise_first\": %s, \"max_abs_diff\": %.3g, \"posted\": %d}\n",
               C, B, v.name.c_str(), v.bm, v.bn, v.lds, best * 1e3, tot / 3 * 1e3, flop / (best * 1e-3) / 1e12,
               same ? "true" : "false", maxd, posted);
        fflush(stdout);
    }
    return 0;
}

int main(int argc, char** argv)
{
    const int C = argc > 1 ? atoi(argv[1]) : 128;
    const int B = argc > 2 ? atoi(argv[2]) : 4096;
    const int reps = argc > 3 ? atoi(argv[3]) : 10;
    if (B < 1 || B > 8192 || reps < 1 || reps > 1000) {
        fprintf(stderr, "bad args\n");
        return 2;
    }
    if (C == 128) return run<128>(B, reps);
    if (C == 256) return run<256>(B, reps);
    fprintf(stderr, "C must be 128 or 256\n");
    return 2;
}
