// Stem conv 3 -> C (3x3, pad 1, no bias) with the BatchNorm / ReLU epilogue fused: the
// fp32-MFMA product kernel (stem_mfma) and the VALU kernel it is bitwise equal to
// (stem_conv, tuning key 9 = 0).  Replaces the ATen conv2d + batch_norm + relu of the
// reference stem (network.py:94-96).
#include "pv_internal.h"

namespace azg {

// Stem conv 3->C (K = 27) on the VALU: 0.2 % of the forward FLOPs.  One
// workgroup per board; the board's 3 input planes are staged into LDS with a
// zero halo; each thread owns one output channel (27 weights in registers) and a
// strided set of pixels.  Weight layout ws[k][c], k = ci*9 + ky*3 + kx.
//
// BOARDS: the input is the int8 game board [B][225] (0 empty, 1, 2) + side to move
// [B]; the reference encoding (games/gomoku.py:130-150: planes board==player,
// board==opponent, ones) is built straight into the LDS patch (on-GPU encode, no
// float planes in HBM).
// SYM (BOARDS only, pv_common.h SymMode): workgroup b builds image b -- board b read through
// symmetry syms[b] & 7 (SYM_EACH), or board b / 8 through symmetry b % 8 (SYM_MEAN8).
template <int C, int EPI, bool BOARDS = false, int SYM = SYM_NONE>
__global__ __launch_bounds__(256) void stem_conv(
    const float* __restrict__ x, const int8_t* __restrict__ boards, const int8_t* __restrict__ players,
    const float* __restrict__ ws, const float* __restrict__ scale, const float* __restrict__ shift,
    float* __restrict__ out, const int8_t* __restrict__ syms = nullptr)
{
    static_assert(SYM == SYM_NONE || BOARDS, "symmetries are applied to board inputs only");
    __shared__ float xs[3 * PADPIX];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* xb = x + (size_t)b * 3 * PIX;
    const int bsrc = SYM == SYM_MEAN8 ? b >> 3 : b;                       // the board of image b
    const int sym = SYM == SYM_MEAN8 ? b & 7 : SYM == SYM_EACH ? (int)syms[b] & 7 : 0;
    const int8_t* bb = boards + (size_t)bsrc * PIX;
    const int me = BOARDS ? (int)players[bsrc] : 0;
    for (int i = tid; i < 3 * PADPIX; i += 256) {
        const int ci = i / PADPIX, rem = i - ci * PADPIX;
        const int yy = rem / PADW, xx = rem - yy * PADW;
        float v = 0.f;
        if (yy >= 1 && yy <= BOARD && xx >= 1 && xx <= BOARD) {
            const int p = SYM != SYM_NONE ? sym_src(yy - 1, xx - 1, sym) : (yy - 1) * BOARD + (xx - 1);
            if (BOARDS) {
                const int c = bb[p];
                v = ci == 0 ? (c == me ? 1.f : 0.f) : ci == 1 ? (c == 3 - me ? 1.f : 0.f) : 1.f;
            } else {
                v = xb[ci * PIX + p];
            }
        }
        xs[i] = v;
    }
    __syncthreads();
    constexpr int CPT = C < 256 ? 1 : C / 256;      // channels per thread
    constexpr int TPP = C < 256 ? C : 256;          // threads per pixel
    constexpr int PPI = 256 / TPP;                  // pixels per iteration
    const int c0 = tid % TPP;
    const int pp = tid / TPP;
#pragma unroll
    for (int cc = 0; cc < CPT; ++cc) {
        const int c = c0 + cc * TPP;
        float w[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) w[k] = ws[k * C + c];
        float s_ = 1.f, t_ = 0.f;
        if (EPI != EPI_RAW) { s_ = scale[c]; t_ = shift[c]; }
        for (int p = pp; p < PIX; p += PPI) {
            const int y = p / BOARD, xq = p - y * BOARD;
            float acc = 0.f;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
                        acc = fmaf(xs[ci * PADPIX + (y + ky) * PADW + (xq + kx)], w[ci * 9 + ky * 3 + kx], acc);
            float v = acc;
            if (EPI == EPI_BN_RELU) v = fmaxf(v * s_ + t_, 0.f);
            out[(size_t)(b * PADPIX + (y + 1) * PADW + (xq + 1)) * C + c] = v;
        }
    }
}

// Stem conv 3->C on fp32 MFMA (the product stem; stem_conv above is kept as the
// bitwise reference, tuning key 9).  The stem is an M x C x K=27 GEMM (K padded to
// 28): each wave owns 32 pixels x CW channels (CW = min(C, 128), NJ = CW/32
// accumulators of v_mfma_f32_32x32x2_f32).  Both operands are built straight in
// registers -- no LDS: lane (r, h) holds A[pixel r][k = 2s + h] for the 14 steps s,
// computed from the 3x3 neighbourhood of its pixel (BOARDS: the int8 board cells,
// encoded as games/gomoku.py:130-150 does: board == player, board == opponent,
// ones inside the board; zero padding outside), and B[k][channel] = ws[k][c].  K
// order k = ci*9 + ky*3 + kx, step s = k 2s then 2s+1: the MFMA's exact fmaf chain
// (MI355X_MICROARCH.md: "exact f32 (= fmaf chain, bitwise)") in stem_conv's order, so
// the two stems are bitwise equal (tested).  The epilogue (BN + ReLU) writes 128-B
// runs of channels per pixel row straight from the accumulators.
constexpr int STEM_CW = 64;   // channels per wave (2 accumulators): twice the waves of 128
// STATS (train forward, EPI_RAW): per 128-row tile (the workgroup's 4 waves) and channel
// the mean and M2 of the raw stem output straight from the accumulators (two-pass, fp32)
// -> pa / pb [tile][C], combined exactly in fp64 by bn_fin_tiles_kernel (prow 128): the
// col_stats pass over z0 disappears.  Waves past M stay (barriers) but store nothing.
// SYM (BOARDS only, pv_common.h SymMode): pixel (y, x) of image i reads its neighbourhood
// cells as boards[board_of(i)][sym_src(yy, xx, s_i)] -- board_of(i) = i, s_i = syms[i] & 7
// (SYM_EACH) or board_of(i) = i / 8, s_i = i % 8 (SYM_MEAN8).  Off-board handling and the
// arithmetic are the BOARDS path's; a template flag, so SYM_NONE compiles to what it was.
template <int C, int EPI, bool BOARDS, bool STATS = false, int SYM = SYM_NONE>
__global__ __launch_bounds__(256) void stem_mfma(const float* __restrict__ x, const int8_t* __restrict__ boards,
                                                 const int8_t* __restrict__ players, const float* __restrict__ ws,
                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                 float* __restrict__ out, int M, float* __restrict__ pa = nullptr,
                                                 float* __restrict__ pb = nullptr,
                                                 const int8_t* __restrict__ syms = nullptr)
{
    static_assert(SYM == SYM_NONE || BOARDS, "symmetries are applied to board inputs only");
    constexpr int CW = C < STEM_CW ? C : STEM_CW;
    constexpr int NJ = CW / 32;
    constexpr int KS = 14;                       // MFMA steps (K = 27 padded to 28)
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const int m0 = (blockIdx.x * 4 + wid) * 32;
    if (!STATS && m0 >= M) return;               // wave-uniform; no barrier without STATS
    const int c0 = blockIdx.y * CW;

    float bw[NJ][KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k = 2 * s + h;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            bw[j][s] = k < 27 ? ws[k * C + c0 + 32 * j + r32] : 0.f;
    }

    const int m = min(m0 + r32, M - 1);
    const int b = m / PIX, p = m - b * PIX;
    const int y = p / BOARD, xq = p - y * BOARD;
    // the 9 neighbourhood values of each input plane (0 outside the board)
    float nb[3][9];
    if (BOARDS) {
        const int bsrc = SYM == SYM_MEAN8 ? b >> 3 : b;                   // the board of image b
        const int sym = SYM == SYM_MEAN8 ? b & 7 : SYM == SYM_EACH ? (int)syms[b] & 7 : 0;
        const int8_t* bb = boards + (size_t)bsrc * PIX;
        const int me = (int)players[bsrc];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = xq + t % 3 - 1;
            const bool in = yy >= 0 && yy < BOARD && xx >= 0 && xx < BOARD;
            const int c = in ? (int)bb[SYM != SYM_NONE ? sym_src(yy, xx, sym) : yy * BOARD + xx] : -1;
            nb[0][t] = c == me ? 1.f : 0.f;
            nb[1][t] = c == 3 - me ? 1.f : 0.f;
            nb[2][t] = in ? 1.f : 0.f;
        }
    } else {
        const float* xb = x + (size_t)b * 3 * PIX;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = xq + t % 3 - 1;
            const bool in = yy >= 0 && yy < BOARD && xx >= 0 && xx < BOARD;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
                nb[ci][t] = in ? xb[ci * PIX + yy * BOARD + xx] : 0.f;
        }
    }
    float av[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k0 = 2 * s, k1 = 2 * s + 1;
        const float v0 = nb[k0 / 9][k0 % 9];
        const float v1 = k1 < 27 ? nb[k1 / 9][k1 % 9] : 0.f;
        av[s] = h ? v1 : v0;
    }

    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bw[j][s], acc[j], 0, 0, 0);

    // epilogue through a wave-private LDS tile [32 px][32 ch] per accumulator: lane
    // (p = lane/8 + 8*it, 16-B run lane%8) finishes 4 channels of one pixel and
    // stores them as one 16 B (4x fewer store instructions than the 4-B C/D layout)
    __shared__ __attribute__((aligned(16))) float es[4][32][32 + 4];
    float (*E)[36] = es[wid];
    const int ec = (lane & 7) * 4;
    int orow[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int mm = m0 + (lane >> 3) + 8 * it;
        orow[it] = mm < M ? pad_off(mm, C) : -1;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) E[(r & 3) + 8 * (r >> 2) + 4 * h][r32] = acc[j][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int c = c0 + 32 * j + ec;
        f32x4 s4 = {1.f, 1.f, 1.f, 1.f}, t4 = {0.f, 0.f, 0.f, 0.f};
        if (EPI != EPI_RAW) {
            s4 = *(const f32x4*)(scale + c);
            t4 = *(const f32x4*)(shift + c);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            f32x4 v = *(const f32x4*)(&E[(lane >> 3) + 8 * it][ec]);
            if (orow[it] >= 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (EPI == EPI_BN_RELU) v[e] = fmaxf(v[e] * s4[e] + t4[e], 0.f);
                *(f32x4*)(out + orow[it] + c) = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if constexpr (STATS) {
        __shared__ float sred[4][CW];
        __shared__ float smean[CW];
        const int rows_w = m0 < M ? min(32, M - m0) : 0;      // valid rows of this wave
        const int tile = blockIdx.x, rows = min(128, M - tile * 128);
        const int tid = threadIdx.x;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float sv = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((r & 3) + 8 * (r >> 2) + 4 * h < rows_w) sv += acc[j][r];
            sv += __shfl_xor(sv, 32, 64);
            if (h == 0) sred[wid][32 * j + r32] = sv;
        }
        __syncthreads();
        if (tid < CW) {
            const float mu = (((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid]) / (float)rows;
            smean[tid] = mu;
            pa[(size_t)tile * C + c0 + tid] = mu;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float mu = smean[32 * j + r32];
            float q = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((r & 3) + 8 * (r >> 2) + 4 * h < rows_w) {
                    const float d = acc[j][r] - mu;
                    q = fmaf(d, d, q);
                }
            q += __shfl_xor(q, 32, 64);
            if (h == 0) sred[wid][32 * j + r32] = q;
        }
        __syncthreads();
        if (tid < CW) pb[(size_t)tile * C + c0 + tid] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
    }
}

// ---- host launchers ------------------------------------------------------

int g_stem_variant = 1;   // 1: fp32-MFMA stem (product); 0: VALU stem_conv (bitwise reference)

// stem_mfma's grid: 128 pixels (4 waves of 32) x STEM_CW channels per workgroup
static dim3 stem_grid(int C, int B)
{
    const int cw = C < STEM_CW ? C : STEM_CW;
    return dim3((B * PIX + 127) / 128, C / cw);
}

// train-forward stem with its BN statistics partials per 128-row tile (STATS)
hipError_t launch_stem_stats(int C, const float* x, const float* ws, float* out, int B, float* pa, float* pb,
                             hipStream_t st)
{
    if (B <= 0) return hipSuccess;
    const int M = B * PIX;
    const dim3 grid = stem_grid(C, B);
    switch (C) {
        case 64: hipLaunchKernelGGL((stem_mfma<64, EPI_RAW, false, true>), grid, dim3(256), 0, st, x, nullptr, nullptr, ws, nullptr, nullptr, out, M, pa, pb); break;
        case 128: hipLaunchKernelGGL((stem_mfma<128, EPI_RAW, false, true>), grid, dim3(256), 0, st, x, nullptr, nullptr, ws, nullptr, nullptr, out, M, pa, pb); break;
        case 256: hipLaunchKernelGGL((stem_mfma<256, EPI_RAW, false, true>), grid, dim3(256), 0, st, x, nullptr, nullptr, ws, nullptr, nullptr, out, M, pa, pb); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The eval / raw stem of one channel count (arguments checked by launch_stem): the kernel is
// picked by key 9 (MFMA or VALU), the symmetry mode, and board or float-plane input.
template <int CC>
static hipError_t launch_stem_c(int epi, const float* x, const float* ws, const float* scale, const float* shift,
                                float* out, int B, hipStream_t st, const int8_t* boards, const int8_t* players,
                                const int8_t* syms, int symmode)
{
    const int8_t* sy = symmode != SYM_NONE ? syms : nullptr;
    auto mfma = [&](auto* kernel) {
        hipLaunchKernelGGL(kernel, stem_grid(CC, B), dim3(256), 0, st, x, boards, players, ws, scale, shift, out,
                           B * PIX, nullptr, nullptr, sy);
    };
    auto valu = [&](auto* kernel) {
        hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, st, x, boards, players, ws, scale, shift, out, sy);
    };
    const bool use_mfma = g_stem_variant == 1;
    if (symmode == SYM_EACH) {
        if (use_mfma) mfma(stem_mfma<CC, EPI_BN_RELU, true, false, SYM_EACH>);
        else valu(stem_conv<CC, EPI_BN_RELU, true, SYM_EACH>);
    } else if (symmode == SYM_MEAN8) {
        if (use_mfma) mfma(stem_mfma<CC, EPI_BN_RELU, true, false, SYM_MEAN8>);
        else valu(stem_conv<CC, EPI_BN_RELU, true, SYM_MEAN8>);
    } else if (use_mfma) {
        if (boards) mfma(stem_mfma<CC, EPI_BN_RELU, true>);
        else if (epi == EPI_RAW) mfma(stem_mfma<CC, EPI_RAW, false>);
        else mfma(stem_mfma<CC, EPI_BN_RELU, false>);
    } else {
        if (boards) valu(stem_conv<CC, EPI_BN_RELU, true>);
        else if (epi == EPI_RAW) valu(stem_conv<CC, EPI_RAW>);
        else valu(stem_conv<CC, EPI_BN_RELU>);
    }
    return hipGetLastError();
}

hipError_t launch_stem(int C, int epi, const float* x, const float* ws, const float* scale,
                       const float* shift, float* out, int B, hipStream_t st, const int8_t* boards,
                       const int8_t* players, const int8_t* syms, int symmode)
{
    if (B <= 0) return hipSuccess;
    if (epi != EPI_RAW && epi != EPI_BN_RELU) return hipErrorInvalidValue;
    // symmode: B images of the caller's boards (SYM_EACH: syms [B]; SYM_MEAN8: B = 8 x boards)
    if (symmode != SYM_NONE &&
        (!boards || epi != EPI_BN_RELU || (symmode != SYM_EACH && symmode != SYM_MEAN8) ||
         (symmode == SYM_EACH && !syms) || (symmode == SYM_MEAN8 && B % 8 != 0)))
        return hipErrorInvalidValue;
    switch (C) {
        case 64: return launch_stem_c<64>(epi, x, ws, scale, shift, out, B, st, boards, players, syms, symmode);
        case 128: return launch_stem_c<128>(epi, x, ws, scale, shift, out, B, st, boards, players, syms, symmode);
        case 256: return launch_stem_c<256>(epi, x, ws, scale, shift, out, B, st, boards, players, syms, symmode);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace azg
