// 3x3 convolution (pad 1, no bias) as an fp32-MFMA implicit GEMM for gfx950,
// with the BatchNorm / residual / ReLU epilogue fused.
//
// Replaces the ATen conv2d + batch_norm + relu (+ in-place residual add) chain of
// the reference ResidualBlock (network.py:9-26) and stem (network.py:94-96).
//
// GEMM view: rows m = pixel of the batch (B*225), cols n = output channel,
// K = 9 taps x C input channels.  A[m][k] is read straight from the padded NHWC
// activation (the halo makes every tap an unconditional 16-byte load), B is the
// weight re-packed to [kchunk][n][32] so a K-chunk of 32 is one contiguous block.
//
// Tile: BM pixels x BN channels per 256-thread workgroup (shape picked per
// launch, see pick_conv_tile), K-chunk 32.  4 waves, each owning TM x TN 32x32
// accumulators of v_mfma_f32_32x32x2_f32 (exact f32 FMA chain: the parity budget
// is 1e-5 fp32, so no bf16/xf32).  LDS holds two chunks (double buffer) of
// unpadded 128-B rows whose 16-B chunks are XOR-swizzled by row, so every
// ds_read_b128 fragment load is bank-conflict free.  Global->LDS staging is
// register staged and issued before the MFMAs of the current chunk
// (async-STAGE split), one barrier per chunk.
//
// Lane l of an MFMA step s uses K index h*16+s (h = l>>5) for both A and B, so
// each lane's 16 A values and 16 B values of a chunk are contiguous in LDS.
#include "pv_internal.h"
#include "pv_halo.h"

#include <algorithm>
#include <map>
#include <utility>

namespace azg {

// ABL (ablation, timing studies only; 0 in every product launch): bit 1 skips the
// global loads, bit 2 replaces LDS fragment reads by register values, bit 4 drops
// the per-chunk barrier, bit 8 skips the epilogue stores (kept live by a never-true
// compare).  Results are garbage when ABL != 0.
template <int C, int BN_, int WM_, int TM_, int NW_, int EPI, int ABL = 0, int SB = 0>
__global__ __launch_bounds__(64 * NW_, NW_ / 2) void conv3x3_mfma(
    const float* __restrict__ in, const float* __restrict__ wp,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ resid, float* __restrict__ out, int M)
{
    using T = ConvTile<C, BN_, WM_, TM_, NW_, SB>;
    constexpr int RPP = T::RPP;
    constexpr int BM = T::BM, BN = T::BN, BK = T::BK, LDK = T::LDK;
    constexpr int CG = T::CG, NCH = T::NCH, WN = T::WN, TM = T::TM, TN = T::TN;
    constexpr int A_LD = T::A_LD, B_LD = T::B_LD;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                    // [2][BM][LDK]
    float* Bs = smem + (SB ? 1 : 2) * BM * LDK;   // [2 or 1][BN][LDK]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    // XCD-aware tile order: workgroup L is dispatched to XCD L % 8, so give each
    // XCD a contiguous run of logical tiles (N-halves of one M tile adjacent, then
    // neighbouring M tiles): the input halo rows and the other N-half's A tile are
    // then L2 hits on the same XCD instead of fabric re-reads.
    constexpr int NTN = C / BN;
    const int L = blockIdx.x, nt = gridDim.x;
    const int xcd = L & 7, q8 = nt >> 3, r8 = nt & 7;
    const int t = xcd * q8 + min(xcd, r8) + (L >> 3);
    const int m0 = (t / NTN) * BM;
    const int n0 = (t % NTN) * BN;

    // staging: thread -> (row sr + RPP i, floats sc..sc+3)
    const int sr = tid >> 3, sc = (tid & 7) * 4;
    int abase[A_LD];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        int m = m0 + sr + RPP * i;
        m = m < M ? m : M - 1;           // tail rows: clamp to a valid pixel, never stored
        abase[i] = pad_off(m, C) + sc;
    }
    const float* wsrc = wp + (size_t)(n0 + sr) * BK + sc;

    f32x4 ra[A_LD], rb[B_LD];
    auto gload = [&](int kc) {
        if (ABL & 1) return;
        const int tap = kc / CG, cg = kc - tap * CG;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int toff = ((ky - 1) * PADW + (kx - 1)) * C + cg * BK;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) ra[i] = *(const f32x4*)(in + abase[i] + toff);
        const float* wk = wsrc + (size_t)kc * C * BK;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) rb[i] = *(const f32x4*)(wk + RPP * i * BK);
    };
    // 16-B chunk c of LDS row r is stored at chunk c ^ ((r >> 1) & 7): the 16 rows a
    // ds_read_b128 lane group touches land on 16 distinct 4-bank slots.
    const int wchunk = ((tid & 7) ^ ((sr >> 1) & 7)) * 4;
    auto lstore = [&](int buf) {
        float* a = As + buf * BM * LDK;
        float* b = Bs + buf * BN * LDK;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) *(f32x4*)(a + (sr + RPP * i) * LDK + wchunk) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LD; ++i) *(f32x4*)(b + (sr + RPP * i) * LDK + wchunk) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int r32 = lane & 31, h = lane >> 5;
    const int swz = (r32 >> 1) & 7;
    const int arow = (wm * TM * 32 + r32) * LDK;
    const int brow = (wn * TN * 32 + r32) * LDK;

    gload(0);
    lstore(0);
    __syncthreads();

    // Two-level K sum for accuracy: each tap's C-long chain accumulates into `at`
    // (one MFMA chain of C/2 steps), which is then added into `acc`: the rounding
    // error grows like chain(C) + 9 instead of chain(9*C) (fp32 parity budget).
    for (int tap = 0; tap < 9; ++tap) {
        f32x16 at[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) at[i][j][r] = 0.f;
#pragma unroll
        for (int cg = 0; cg < CG; ++cg) {
            const int kc = tap * CG + cg;
            const int cur = SB ? 0 : (kc & 1);
            if (kc + 1 < NCH) gload(kc + 1);
            // keep the next chunk's global loads at the top of the chunk: without this
            // fence hipcc sinks them to just before their vmcnt wait (latency exposed)
            __builtin_amdgcn_sched_barrier(0);
            const float* Ab = As + cur * BM * LDK;
            const float* Bb = Bs + cur * BN * LDK;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 a[TM], b[TN];
                const int rc = ((h * 4 + q) ^ swz) * 4;
                if (ABL & 2) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) a[i] = f32x4{(float)kc, (float)q, (float)i, 1.f};
#pragma unroll
                    for (int j = 0; j < TN; ++j) b[j] = f32x4{(float)q, (float)kc, 1.f, (float)j};
                } else {
#pragma unroll
                    for (int i = 0; i < TM; ++i) a[i] = *(const f32x4*)(Ab + arow + i * 32 * LDK + rc);
#pragma unroll
                    for (int j = 0; j < TN; ++j) b[j] = *(const f32x4*)(Bb + brow + j * 32 * LDK + rc);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            at[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][s], b[j][s], at[i][j], 0, 0, 0);
            }
            if (kc + 1 < NCH) {
                if (SB) __syncthreads();   // every wave is done reading the buffer
                lstore(SB ? 0 : cur ^ 1);
            }
            if (!(ABL & 4)) __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] += at[i][j];
    }

    // epilogue: C/D map of 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * TN * 32 + j * 32 + r32;
        float s_ = 1.f, t_ = 0.f;
        if (EPI == EPI_BN_RELU || EPI == EPI_BN_RES_RELU) { s_ = scale[col]; t_ = shift[col]; }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < M && (!(ABL & 8) || acc[i][j][r] == 1234.5f)) {
                    const int o = pad_off(m, C) + col;
                    float v = acc[i][j][r];
                    if (EPI == EPI_BN_RELU) {
                        v = fmaxf(v * s_ + t_, 0.f);
                    } else if (EPI == EPI_BN_RES_RELU) {
                        v = fmaxf(v * s_ + t_ + resid[o], 0.f);
                    } else if (EPI == EPI_ADD) {
                        v = v + resid[o];
                    }
                    out[o] = v;
                }
            }
        }
    }
}

// Per-layer launch of the halo-staged tile (pv_halo.h); XCD-aware tile order:
// workgroup L is dispatched to XCD L % 8, so each XCD gets a contiguous run of
// logical tiles (the N-tiles of one M tile adjacent, then neighbouring M tiles) and
// the halo rows they share are L2 hits on that XCD.
template <int C, int BN_, int WM_, int TM_, int NW_, int EPI, int ABL = 0, int VAR = 0>
__global__ __launch_bounds__(64 * NW_, 2) void conv3x3_halo(
    const float* __restrict__ in, const float* __restrict__ wp,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ resid, float* __restrict__ out, int M, H3Guard guard)
{
    using T = ConvTile<C, BN_, WM_, TM_, NW_>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTN = C / T::BN;
    const int L = blockIdx.x, nt = gridDim.x;
    const int xcd = L & 7, q8 = nt >> 3, r8 = nt & 7;
    const int t = xcd * q8 + min(xcd, r8) + (L >> 3);
    halo_tile<C, BN_, WM_, TM_, NW_, EPI, false, ABL, VAR>(in, wp, scale, shift, resid, out,
                                          __builtin_amdgcn_make_buffer_rsrc(out, (short)0, 0, 0x00020000), M,
                                          (t / NTN) * T::BM, (t % NTN) * T::BN, smem, EpiX{}, ProX{}, FinX{}, guard);
}
// Train-step conv (forward z = conv(a), dgrad = conv(dZ, flipped W) [+ resid]) with
// the BatchNorm partial sums fused into the epilogue (pv_halo.h XE_STATS / XE_BNBWD):
// 128-row M tiles (the partials are per 128-row tile) x 64 channels, 8 waves, two
// workgroups per CU.  Same XCD-aware tile order as above.  WT: outputs stored
// write-through (no dirty L2 lines at the kernel boundary).  PRO (forward only): the
// input is the previous layer's raw output z and its BN + ReLU (+ residual) is applied
// in the halo staging (pv_halo.h ProX).
template <int C, int NWT>
struct TrainTile {
    static constexpr int BN = NWT >= 16 ? 128 : 64;
    using T = ConvTile<C, BN, 4, 1, NWT>;
};
template <int C, int EPI, int XE, bool WT, int PRO = PRO_NONE, int VAR = 32, int NWT = 8>
__global__ __launch_bounds__(64 * NWT) __attribute__((amdgpu_waves_per_eu(4))) void conv3x3_train(
    const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ resid,
    float* __restrict__ out, int M, EpiX ex, ProX px, FinX fx, const float* __restrict__ oscale, H3Guard guard)
{
    using T = typename TrainTile<C, NWT>::T;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTN = C / T::BN;
    const int L = blockIdx.x, nt = gridDim.x;
    const int xcd = L & 7, q8 = nt >> 3, r8 = nt & 7;
    const int t = xcd * q8 + min(xcd, r8) + (L >> 3);
    halo_tile<C, T::BN, 4, 1, NWT, EPI, WT, 0, VAR, XE, PRO>(in, wp, oscale, nullptr, resid, out,
                                                          wt_rsrc(out, padded_bytes(M, C)), M, (t / NTN) * T::BM,
                                                          (t % NTN) * T::BN, smem, ex, px, fx, guard);
}

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
// ABL (timing studies only, results invalid when set): 1 no stores, 2 no input
// loads, 4 no weight loads, 8 no MFMA.
// STATS (train forward, EPI_RAW): per 128-row tile (the workgroup's 4 waves) and channel
// the mean and M2 of the raw stem output straight from the accumulators (two-pass, fp32)
// -> pa / pb [tile][C], combined exactly in fp64 by bn_fin_tiles_kernel (prow 128): the
// col_stats pass over z0 disappears.  Waves past M stay (barriers) but store nothing.
// SYM (BOARDS only, pv_common.h SymMode): pixel (y, x) of image i reads its neighbourhood
// cells as boards[board_of(i)][sym_src(yy, xx, s_i)] -- board_of(i) = i, s_i = syms[i] & 7
// (SYM_EACH) or board_of(i) = i / 8, s_i = i % 8 (SYM_MEAN8).  Off-board handling and the
// arithmetic are the BOARDS path's; a template flag, so SYM_NONE compiles to what it was.
template <int C, int EPI, bool BOARDS, int ABL = 0, bool STATS = false, int SYM = SYM_NONE>
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
            bw[j][s] = (ABL & 4) ? (float)(k + j) : (k < 27 ? ws[k * C + c0 + 32 * j + r32] : 0.f);
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
                nb[ci][t] = (ABL & 2) ? (float)(yy + xx + ci) : (in ? xb[ci * PIX + yy * BOARD + xx] : 0.f);
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
        for (int j = 0; j < NJ; ++j) {
            if (ABL & 8) acc[j][s] = av[s] * bw[j][s];
            else acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bw[j][s], acc[j], 0, 0, 0);
        }

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
            if (orow[it] >= 0 && (!(ABL & 1) || v[0] == 1234.5f)) {
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

template <int C, int BN, int WM, int TM, int NW, int EPI, int SB = 0>
static hipError_t launch_conv_t(const float* in, const float* wp, const float* scale, const float* shift,
                                const float* resid, float* out, int M, hipStream_t st)
{
    using T = ConvTile<C, BN, WM, TM, NW, SB>;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)conv3x3_mfma<C, BN, WM, TM, NW, EPI, 0, SB>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, T::LDS_BYTES);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    dim3 grid(((M + T::BM - 1) / T::BM) * (C / T::BN));
    hipLaunchKernelGGL((conv3x3_mfma<C, BN, WM, TM, NW, EPI, 0, SB>), grid, dim3(T::NT), T::LDS_BYTES, st,
                       in, wp, scale, shift, resid, out, M);
    return hipGetLastError();
}

template <int C, int BN, int WM, int TM, int NW, int EPI, int VAR = 0>
static hipError_t launch_halo_t(const float* in, const float* wp, const float* scale, const float* shift,
                                const float* resid, float* out, int M, hipStream_t st, const H3Guard& guard = H3Guard{})
{
    using T = ConvTile<C, BN, WM, TM, NW>;
    constexpr int lds = halo_lds_bytes<C, BN, WM, TM, NW, VAR>();
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)conv3x3_halo<C, BN, WM, TM, NW, EPI, 0, VAR>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    dim3 grid(((M + T::BM - 1) / T::BM) * (C / T::BN));
    hipLaunchKernelGGL((conv3x3_halo<C, BN, WM, TM, NW, EPI, 0, VAR>), grid, dim3(T::NT), lds, st, in, wp, scale,
                       shift, resid, out, M, guard);
    return hipGetLastError();
}

int g_tower_mode = 2;   // 0 per-layer launches, 1 persistent tower, 2 tuned per batch bucket
int g_conv_variant = 1;   // 1: halo-staged (product); 0: per-chunk A staging (timing studies)

template <int C, int BN, int WM, int TM, int NW = 4, int SB = 0>
static hipError_t launch_conv_epi(int epi, const float* in, const float* wp, const float* scale, const float* shift,
                                  const float* resid, float* out, int M, hipStream_t st)
{
    if (g_conv_variant == 1 && SB == 0) {
        switch (epi) {
            case EPI_BN_RELU: return launch_halo_t<C, BN, WM, TM, NW, EPI_BN_RELU>(in, wp, scale, shift, resid, out, M, st);
            case EPI_BN_RES_RELU: return launch_halo_t<C, BN, WM, TM, NW, EPI_BN_RES_RELU>(in, wp, scale, shift, resid, out, M, st);
            case EPI_ADD: return launch_halo_t<C, BN, WM, TM, NW, EPI_ADD>(in, wp, scale, shift, resid, out, M, st);
            default: return launch_halo_t<C, BN, WM, TM, NW, EPI_RAW>(in, wp, scale, shift, resid, out, M, st);
        }
    }
#ifdef AZG_AB_STUDIES
    // per-chunk A staging / single-buffer tiles: A/B timing studies only
    switch (epi) {
        case EPI_BN_RELU: return launch_conv_t<C, BN, WM, TM, NW, EPI_BN_RELU, SB>(in, wp, scale, shift, resid, out, M, st);
        case EPI_BN_RES_RELU: return launch_conv_t<C, BN, WM, TM, NW, EPI_BN_RES_RELU, SB>(in, wp, scale, shift, resid, out, M, st);
        case EPI_ADD: return launch_conv_t<C, BN, WM, TM, NW, EPI_ADD, SB>(in, wp, scale, shift, resid, out, M, st);
        default: return launch_conv_t<C, BN, WM, TM, NW, EPI_RAW, SB>(in, wp, scale, shift, resid, out, M, st);
    }
#else
    return hipErrorInvalidValue;   // built without AZG_AB_STUDIES (make study)
#endif
}

// Tile shapes {BM, BN}: index into the switch below.
struct TileShape { int bm, bn; };
// 0-5: 4 waves; 6-9: 8 waves (more waves per SIMD at the same LDS footprint).
// 10-12: single LDS buffer (64x64, 128x64, 64x128; 4 waves).
static const TileShape kShapes[] = {{128, 128}, {96, 128}, {160, 128}, {64, 128}, {128, 64}, {64, 64},
                                    {128, 128}, {128, 128}, {128, 64}, {64, 128},
                                    {64, 64}, {128, 64}, {64, 128}};
constexpr int kNumShapes = (int)(sizeof(kShapes) / sizeof(kShapes[0]));
constexpr int kNumAutoShapes = 6;   // heuristic pick_conv_tile only considers 0-5
constexpr int kNumTunedShapes = 10; // autotuning times 0-9 (the single-buffer 10-12 measured slower everywhere)

static bool shape_ok(int shape, int C)
{
    if (shape < 0 || shape >= kNumShapes) return false;
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

template <int CC>
static hipError_t launch_s8(int epi, const float* in, const float* wp, const float* scale, const float* shift,
                            const float* resid, float* out, int M, hipStream_t st)
{
#define AZG_S8_VAR(V)                                                                                                  \
    if (g_conv_var == V) {                                                                                             \
        if (epi == EPI_BN_RELU) return launch_halo_t<CC, 64, 4, 1, 8, EPI_BN_RELU, V>(in, wp, scale, shift, resid, out, M, st); \
        if (epi == EPI_BN_RES_RELU) return launch_halo_t<CC, 64, 4, 1, 8, EPI_BN_RES_RELU, V>(in, wp, scale, shift, resid, out, M, st); \
    }
    AZG_S8_VAR(1) AZG_S8_VAR(4) AZG_S8_VAR(5)
#undef AZG_S8_VAR
    return launch_conv_epi<CC, 64, 4, 1, 8>(epi, in, wp, scale, shift, resid, out, M, st);
}

template <int CC>
static hipError_t launch_shape8_split(int epi, const float* in, const float* wp, const float* scale,
                                      const float* shift, const float* resid, float* out, int M, hipStream_t st)
{
    constexpr int BM = 128, NTN = CC / 64, SLOTS = 512;
    const int B = M / PIX;
    const int ntiles = ((M + BM - 1) / BM) * NTN;
    const int rounds = ntiles / SLOTS, rem = ntiles - rounds * SLOTS;
    if (!g_conv_tail_split || M % PIX != 0 || rounds < 2 || rem == 0 || rem > SLOTS / 2)
        return launch_s8<CC>(epi, in, wp, scale, shift, resid, out, M, st);
    int B1 = (int)((long)rounds * SLOTS / NTN * BM / PIX);    // boards of whole rounds
    while (B1 > 0 && ((B1 * PIX + BM - 1) / BM) * NTN > rounds * SLOTS) --B1;
    if (B1 <= 0 || B1 >= B) return launch_s8<CC>(epi, in, wp, scale, shift, resid, out, M, st);
    hipError_t e = launch_s8<CC>(epi, in, wp, scale, shift, resid, out, B1 * PIX, st);
    if (e != hipSuccess) return e;
    const size_t off = (size_t)B1 * PADPIX * CC;
    return launch_conv_epi<CC, 64, 2, 1>(epi, in + off, wp, scale, shift, resid ? resid + off : nullptr, out + off,
                                         (B - B1) * PIX, st);
}

hipError_t launch_conv3x3_shape(int shape, int C, int epi, const float* in, const float* wp, const float* scale,
                                const float* shift, const float* resid, float* out, int M, hipStream_t st)
{
#ifdef AZG_AB_STUDIES
#define AZG_SB_SHAPES(CC)                                                                                       \
        case 10: return launch_conv_epi<CC, 64, 2, 1, 4, 1>(epi, in, wp, scale, shift, resid, out, M, st);      \
        case 11: return launch_conv_epi<CC, 64, 2, 2, 4, 1>(epi, in, wp, scale, shift, resid, out, M, st);      \
        case 12: return launch_conv_epi<CC, 128, 2, 1, 4, 1>(epi, in, wp, scale, shift, resid, out, M, st);
#else
#define AZG_SB_SHAPES(CC)
#endif
#define AZG_SHAPES(CC)                                                                                          \
    switch (shape) {                                                                                            \
        case 0: return launch_conv_epi<CC, (CC < 128 ? CC : 128), 2, 2>(epi, in, wp, scale, shift, resid, out, M, st); \
        case 1: return launch_conv_epi<CC, 128, 1, 3>(epi, in, wp, scale, shift, resid, out, M, st);            \
        case 2: return launch_conv_epi<CC, 128, 1, 5>(epi, in, wp, scale, shift, resid, out, M, st);            \
        case 3: return launch_conv_epi<CC, 128, 2, 1>(epi, in, wp, scale, shift, resid, out, M, st);            \
        case 4: return launch_conv_epi<CC, 64, 2, 2>(epi, in, wp, scale, shift, resid, out, M, st);             \
        case 5: return launch_conv_epi<CC, 64, 2, 1>(epi, in, wp, scale, shift, resid, out, M, st);             \
        case 6: return launch_conv_epi<CC, 128, 2, 2, 8>(epi, in, wp, scale, shift, resid, out, M, st);         \
        case 7: return launch_conv_epi<CC, 128, 4, 1, 8>(epi, in, wp, scale, shift, resid, out, M, st);         \
        case 8: return launch_shape8_split<CC>(epi, in, wp, scale, shift, resid, out, M, st);                   \
        case 9: return launch_conv_epi<CC, 128, 2, 1, 8>(epi, in, wp, scale, shift, resid, out, M, st);         \
        AZG_SB_SHAPES(CC)                                                                                       \
        default: return hipErrorInvalidValue;                                                                   \
    }
    switch (C) {
        case 64:
            switch (shape) {
                case 0: return launch_conv_epi<64, 64, 2, 2>(epi, in, wp, scale, shift, resid, out, M, st);
                case 5: return launch_conv_epi<64, 64, 2, 1>(epi, in, wp, scale, shift, resid, out, M, st);
                case 4: return launch_conv_epi<64, 64, 2, 2>(epi, in, wp, scale, shift, resid, out, M, st);
                case 8: return launch_conv_epi<64, 64, 4, 1, 8>(epi, in, wp, scale, shift, resid, out, M, st);
#ifdef AZG_AB_STUDIES
                case 10: return launch_conv_epi<64, 64, 2, 1, 4, 1>(epi, in, wp, scale, shift, resid, out, M, st);
                case 11: return launch_conv_epi<64, 64, 2, 2, 4, 1>(epi, in, wp, scale, shift, resid, out, M, st);
#endif
                default: return hipErrorInvalidValue;
            }
        case 128: AZG_SHAPES(128)
        case 256: AZG_SHAPES(256)
        default: return hipErrorInvalidValue;
    }
#undef AZG_SHAPES
#undef AZG_SB_SHAPES
}

// Split-fp16 (H3) per-layer conv (pv_halo.h VAR bit 64; wp / scale = the H3 packs of
// pv_pack.hip pack_h3): the eval tower's arithmetic per layer (bitwise equal to it), the
// 64x64 / 4-wave tile (shape 5) or the 128x64 / 8-wave tile (shape 8), buffer addressing.
template <int CC, int BN, int WM, int NW, int VAR>
static hipError_t launch_h3_v(int epi, const float* in, const float* wp, const float* scale, const float* shift,
                              const float* resid, float* out, int M, hipStream_t st, const H3Guard& g)
{
    if (epi == EPI_BN_RELU) return launch_halo_t<CC, BN, WM, 1, NW, EPI_BN_RELU, VAR>(in, wp, scale, shift, resid, out, M, st, g);
    if (epi == EPI_BN_RES_RELU) return launch_halo_t<CC, BN, WM, 1, NW, EPI_BN_RES_RELU, VAR>(in, wp, scale, shift, resid, out, M, st, g);
    return hipErrorInvalidValue;
}
// VAR 99 = H3 + buffer addressing + weights two chunks ahead + board-keyed halo swizzle:
// the fastest per-layer form (+10 % over 96 at 128 boards, scripts/h3_tune_study.py)
template <int CC, int BN, int WM, int NW>
static hipError_t launch_h3_t(int epi, const float* in, const float* wp, const float* scale, const float* shift,
                              const float* resid, float* out, int M, hipStream_t st, const H3Guard& g)
{
    if (epi == EPI_BN_RELU) return launch_halo_t<CC, BN, WM, 1, NW, EPI_BN_RELU, 99>(in, wp, scale, shift, resid, out, M, st, g);
    if (epi == EPI_BN_RES_RELU) return launch_halo_t<CC, BN, WM, 1, NW, EPI_BN_RES_RELU, 99>(in, wp, scale, shift, resid, out, M, st, g);
    return hipErrorInvalidValue;
}
hipError_t launch_conv3x3_h3(int shape, int C, int epi, const float* in, const float* wp, const float* scale,
                             const float* shift, const float* resid, float* out, int M, hipStream_t st,
                             unsigned* ring, unsigned seq)
{
    const H3Guard g{ring, seq};
    switch (C) {
        case 128:
            if (shape == 8) return launch_h3_t<128, 64, 4, 8>(epi, in, wp, scale, shift, resid, out, M, st, g);
            return launch_h3_t<128, 64, 2, 4>(epi, in, wp, scale, shift, resid, out, M, st, g);
        case 256:
            if (shape == 8) return launch_h3_t<256, 64, 4, 8>(epi, in, wp, scale, shift, resid, out, M, st, g);
            return launch_h3_t<256, 64, 2, 4>(epi, in, wp, scale, shift, resid, out, M, st, g);
        default: return hipErrorInvalidValue;
    }
}

int g_conv_shape_override = -1;
int g_conv_autotune = 1;
int g_conv_ablation = 0;

// timing-only ablations of the product tile (halo kernel, 64x64 4 waves or
// 128x64 8 waves per g_ablation_shape; C = 128, EPI_BN_RELU launches only)
int g_ablation_shape = 5;

#ifdef AZG_AB_STUDIES
template <int ABL, int BN, int WM, int TM, int NW>
static hipError_t launch_ablation_s(const float* in, const float* wp, const float* scale, const float* shift,
                                    const float* resid, float* out, int M, hipStream_t st)
{
    using T = ConvTile<128, BN, WM, TM, NW>;
    constexpr int lds = halo_lds_bytes<128, BN, WM, TM, NW>();
    (void)hipFuncSetAttribute((const void*)conv3x3_halo<128, BN, WM, TM, NW, EPI_BN_RELU, ABL>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    dim3 grid(((M + T::BM - 1) / T::BM) * (128 / BN));
    hipLaunchKernelGGL((conv3x3_halo<128, BN, WM, TM, NW, EPI_BN_RELU, ABL>), grid, dim3(T::NT), lds, st, in, wp,
                       scale, shift, resid, out, M, H3Guard{});
    return hipGetLastError();
}

template <int ABL>
static hipError_t launch_ablation(const float* in, const float* wp, const float* scale, const float* shift,
                                  const float* resid, float* out, int M, hipStream_t st)
{
    if (g_ablation_shape == 8) return launch_ablation_s<ABL, 64, 4, 1, 8>(in, wp, scale, shift, resid, out, M, st);
    return launch_ablation_s<ABL, 64, 2, 1, 4>(in, wp, scale, shift, resid, out, M, st);
}

static hipError_t launch_ablated(const float* in, const float* wp, const float* scale, const float* shift,
                                 const float* resid, float* out, int M, hipStream_t st)
{
    switch (g_conv_ablation) {
#define AZG_ABL(k) case k: return launch_ablation<k>(in, wp, scale, shift, resid, out, M, st);
        AZG_ABL(1) AZG_ABL(2) AZG_ABL(3) AZG_ABL(4) AZG_ABL(8) AZG_ABL(16) AZG_ABL(7) AZG_ABL(31)
#undef AZG_ABL
        default: return launch_ablation<0>(in, wp, scale, shift, resid, out, M, st);
    }
}
#endif

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

static int autotune_shape(int C, int epi, const float* in, const float* wp, const float* scale, const float* shift,
                          const float* resid, float* out, int M, hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return -1;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return -1;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return -1; }
    float best_ms[kNumShapes];
    bool ok[kNumShapes];
    for (int s = 0; s < kNumShapes; ++s) {
        best_ms[s] = 1e30f;
        ok[s] = shape_ok(s, C) && s < kNumTunedShapes &&
                launch_conv3x3_shape(s, C, epi, in, wp, scale, shift, resid, out, M, st) == hipSuccess;
    }
    for (int r = 0; r < kTuneRounds; ++r) {
        for (int s = 0; s < kNumShapes; ++s) {
            if (!ok[s]) continue;
            (void)hipEventRecord(e0, st);
            if (launch_conv3x3_shape(s, C, epi, in, wp, scale, shift, resid, out, M, st) != hipSuccess) {
                ok[s] = false;
                continue;
            }
            (void)hipEventRecord(e1, st);
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
    const int pref = (M / PIX >= 1536 && ok[8]) ? 8 : kPreferredShape;
    if (best >= 0 && ok[pref] && best_ms[pref] <= 1.02f * best_ms[best]) best = pref;
    return best;
}

hipError_t launch_conv3x3(int C, int epi, const float* in, const float* wp, const float* scale,
                          const float* shift, const float* resid, float* out, int M, hipStream_t st)
{
#ifdef AZG_AB_STUDIES
    if (g_conv_ablation > 0 && C == 128 && epi == EPI_BN_RELU)
        return launch_ablated(in, wp, scale, shift, resid, out, M, st);
#endif
    int shape = -1;
    if (g_conv_shape_override >= 0 && shape_ok(g_conv_shape_override, C)) {
        shape = g_conv_shape_override;
    } else {
        auto key = std::make_pair(C, conv_batch_bucket(M));
        auto it = tune_cache().find(key);
        if (it != tune_cache().end()) {
            shape = it->second;
        } else if (g_conv_autotune) {
            shape = autotune_shape(C, epi, in, wp, scale, shift, resid, out, M, st);
            if (shape >= 0) tune_cache()[key] = shape;
        }
        if (shape < 0) shape = pick_conv_tile(C, M);
    }
    if (C == 64 && !shape_ok(shape, C)) shape = 5;
    return launch_conv3x3_shape(shape, C, epi, in, wp, scale, shift, resid, out, M, st);
}

// Train convs: 128 x 64 tiles, 8 waves (two workgroups per CU), buffer-resource operand
// addressing (halo_tile VAR 32), outputs stored write-through.
template <int C, int EPI, int XE, int PRO, int VAR>
static hipError_t launch_train_v(const float* in, const float* wp, const float* resid, float* out, int M,
                                 const EpiX& ex, const ProX& px, const FinX& fx, hipStream_t st,
                                 const float* oscale = nullptr, unsigned* h3ovf = nullptr,
                                 const unsigned* dmax = nullptr)
{
    using T = typename TrainTile<C, 8>::T;
    constexpr int lds = halo_lds_bytes<C, T::BN, 4, 1, 8, VAR, PRO>();
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)conv3x3_train<C, EPI, XE, true, PRO, VAR, 8>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    dim3 grid(((M + T::BM - 1) / T::BM) * (C / T::BN));
    hipLaunchKernelGGL((conv3x3_train<C, EPI, XE, true, PRO, VAR, 8>), grid, dim3(T::NT), lds, st, in, wp,
                       resid, out, M, ex, px, fx, oscale, H3Guard{h3ovf, 1u, dmax});
    return hipGetLastError();
}

template <int C, int EPI, int XE, int PRO = PRO_NONE>
static hipError_t launch_train_t(const float* in, const float* wp, const float* resid, float* out, int M,
                                 const EpiX& ex, const ProX& px, const FinX& fx, hipStream_t st,
                                 const float* oscale = nullptr, unsigned* h3ovf = nullptr,
                                 const unsigned* dmax = nullptr)
{
    // split-fp16 dgrad (key 50; oscale = the layer's 2^-e, dmax = its input's max |dz| bits):
    // four products (VAR 225) or three (97), the input staged times 2^k
    if constexpr (XE == XE_BNBWD && PRO == PRO_NONE) {
        if (oscale && dmax && g_train_dgrad_h3 == 2)
            return launch_train_v<C, EPI, XE, PRO, 225>(in, wp, resid, out, M, ex, px, fx, st, oscale, nullptr, dmax);
        if (oscale && dmax)
            return launch_train_v<C, EPI, XE, PRO, 97>(in, wp, resid, out, M, ex, px, fx, st, oscale, nullptr, dmax);
    }
    // split-fp16 forward (VAR 97 = 64 | 32 | 1: H3, buffer addressing, board-keyed halo rows;
    // + 128: the fourth, lo x lo product -- key 49 = 2)
    if constexpr (EPI == EPI_RAW && XE == XE_STATS) {
        if (oscale && g_train_h3 == 2)
            return launch_train_v<C, EPI, XE, PRO, 225>(in, wp, resid, out, M, ex, px, fx, st, oscale, h3ovf);
        if (oscale) return launch_train_v<C, EPI, XE, PRO, 97>(in, wp, resid, out, M, ex, px, fx, st, oscale, h3ovf);
    }
    if (oscale) return hipErrorInvalidValue;
    // (the board-keyed halo body, VAR 33, measured equal for the prologue-free train convs:
    // 2.865-2.869 vs 2.866-2.874 ms at 6x128 and within noise at 10x256, scripts/gpu_r4p.sh)
    return launch_train_v<C, EPI, XE, PRO, 32>(in, wp, resid, out, M, ex, px, fx, st);
}
int g_train_h3 = 2;   // key 49: 0 fp32 MFMA, 1 split-fp16 (3 products), 2 split-fp16 with 4 products (default)
int g_train_dgrad_h3 = 0;   // key 50: the dgrad convs, likewise (inputs scaled by 2^k from their max); measured slower and
                            // below the two-step goldens: off by default

// Train conv with fused BN partials: (EPI_RAW, XE_STATS) forward, optionally with
// the input layer's BN applied in the staging (px: PRO_BN / PRO_BN_RES); (EPI_RAW |
// EPI_ADD, XE_BNBWD) dgrad.  Partials are per TRAIN_BM-row M tile; with fx (cnt set)
// the last workgroup of each N tile also runs the BN finalize (pv_halo.h FinX).
hipError_t launch_conv3x3_train(int C, int epi, int xe, const float* in, const float* wp, const float* resid,
                                float* out, int M, const EpiX& ex, hipStream_t st, const ProX* px, const FinX* fxp,
                                const float* oscale, unsigned* h3ovf, const unsigned* dmax)
{
    const ProX p0{};
    const FinX fx = fxp ? *fxp : FinX{};
#define AZG_TRAIN_C(CC)                                                                            \
    case CC:                                                                                       \
        if (epi == EPI_RAW && xe == XE_STATS && px && px->res)                                     \
            return launch_train_t<CC, EPI_RAW, XE_STATS, PRO_BN_RES>(in, wp, resid, out, M, ex, *px, fx, st, oscale, h3ovf); \
        if (epi == EPI_RAW && xe == XE_STATS && px)                                                \
            return launch_train_t<CC, EPI_RAW, XE_STATS, PRO_BN>(in, wp, resid, out, M, ex, *px, fx, st, oscale, h3ovf); \
        if (epi == EPI_RAW && xe == XE_STATS) return launch_train_t<CC, EPI_RAW, XE_STATS>(in, wp, resid, out, M, ex, p0, fx, st, oscale, h3ovf); \
        if (epi == EPI_RAW && xe == XE_BNBWD) return launch_train_t<CC, EPI_RAW, XE_BNBWD>(in, wp, resid, out, M, ex, p0, fx, st, oscale, nullptr, dmax); \
        if (epi == EPI_ADD && xe == XE_BNBWD) return launch_train_t<CC, EPI_ADD, XE_BNBWD>(in, wp, resid, out, M, ex, p0, fx, st, oscale, nullptr, dmax); \
        return hipErrorInvalidValue;
    switch (C) {
        AZG_TRAIN_C(64)
        AZG_TRAIN_C(128)
        AZG_TRAIN_C(256)
        default: return hipErrorInvalidValue;
    }
#undef AZG_TRAIN_C
}

int conv_tuned_shape(int C, int M)
{
    auto it = tune_cache().find(std::make_pair(C, conv_batch_bucket(M)));
    return it == tune_cache().end() ? -1 : it->second;
}

// train-forward stem with its BN statistics partials per 128-row tile (STATS)
hipError_t launch_stem_stats(int C, const float* x, const float* ws, float* out, int B, float* pa, float* pb,
                             hipStream_t st)
{
    if (B <= 0) return hipSuccess;
    const int M = B * PIX;
    const int cw = C < STEM_CW ? C : STEM_CW;
    const dim3 grid((M + 127) / 128, C / cw);
    switch (C) {
        case 64: hipLaunchKernelGGL((stem_mfma<64, EPI_RAW, false, 0, true>), grid, dim3(256), 0, st, x, nullptr, nullptr, ws, nullptr, nullptr, out, M, pa, pb); break;
        case 128: hipLaunchKernelGGL((stem_mfma<128, EPI_RAW, false, 0, true>), grid, dim3(256), 0, st, x, nullptr, nullptr, ws, nullptr, nullptr, out, M, pa, pb); break;
        case 256: hipLaunchKernelGGL((stem_mfma<256, EPI_RAW, false, 0, true>), grid, dim3(256), 0, st, x, nullptr, nullptr, ws, nullptr, nullptr, out, M, pa, pb); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

int g_stem_variant = 1;   // 1: fp32-MFMA stem (product); 0: VALU stem_conv (bitwise reference)
int g_stem_ablation = 0;  // timing studies only (C = 128 float-plane stem)

hipError_t launch_stem(int C, int epi, const float* x, const float* ws, const float* scale,
                       const float* shift, float* out, int B, hipStream_t st, const int8_t* boards,
                       const int8_t* players, const int8_t* syms, int symmode)
{
    if (B <= 0) return hipSuccess;
    if (epi != EPI_RAW && epi != EPI_BN_RELU) return hipErrorInvalidValue;
    if (symmode != SYM_NONE) {
        // B images of the caller's boards (SYM_EACH: syms [B]; SYM_MEAN8: B = 8 x boards)
        if (!boards || epi != EPI_BN_RELU || (symmode != SYM_EACH && symmode != SYM_MEAN8) ||
            (symmode == SYM_EACH && !syms) || (symmode == SYM_MEAN8 && B % 8 != 0))
            return hipErrorInvalidValue;
        const int M = B * PIX;
        const int cw = C < STEM_CW ? C : STEM_CW;
        const dim3 grid((M + 127) / 128, C / cw);
#define AZG_STEM_SYM(CC)                                                                                        \
    case CC:                                                                                                    \
        if (g_stem_variant == 1 && symmode == SYM_EACH) hipLaunchKernelGGL((stem_mfma<CC, EPI_BN_RELU, true, 0, false, SYM_EACH>), grid, dim3(256), 0, st, x, boards, players, ws, scale, shift, out, M, nullptr, nullptr, syms); \
        else if (g_stem_variant == 1) hipLaunchKernelGGL((stem_mfma<CC, EPI_BN_RELU, true, 0, false, SYM_MEAN8>), grid, dim3(256), 0, st, x, boards, players, ws, scale, shift, out, M, nullptr, nullptr, syms); \
        else if (symmode == SYM_EACH) hipLaunchKernelGGL((stem_conv<CC, EPI_BN_RELU, true, SYM_EACH>), dim3(B), dim3(256), 0, st, x, boards, players, ws, scale, shift, out, syms); \
        else hipLaunchKernelGGL((stem_conv<CC, EPI_BN_RELU, true, SYM_MEAN8>), dim3(B), dim3(256), 0, st, x, boards, players, ws, scale, shift, out, syms); \
        return hipGetLastError();
        switch (C) {
            AZG_STEM_SYM(64)
            AZG_STEM_SYM(128)
            AZG_STEM_SYM(256)
            default: return hipErrorInvalidValue;
        }
#undef AZG_STEM_SYM
    }
    if (g_stem_variant == 1) {
        const int M = B * PIX;
        const int cw = C < STEM_CW ? C : STEM_CW;
        const dim3 grid((M + 127) / 128, C / cw);
#ifdef AZG_AB_STUDIES
        if (g_stem_ablation && C == 128 && !boards && epi == EPI_BN_RELU) {
#define AZG_STEM_ABL(A) \
    if (g_stem_ablation == A) hipLaunchKernelGGL((stem_mfma<128, EPI_BN_RELU, false, A>), grid, dim3(256), 0, st, x, boards, players, ws, scale, shift, out, M);
            AZG_STEM_ABL(1) AZG_STEM_ABL(2) AZG_STEM_ABL(4) AZG_STEM_ABL(8) AZG_STEM_ABL(6) AZG_STEM_ABL(14) AZG_STEM_ABL(15)
#undef AZG_STEM_ABL
            return hipGetLastError();
        }
#endif
#define AZG_STEM_MFMA(CC)                                                                                       \
    case CC:                                                                                                    \
        if (boards) hipLaunchKernelGGL((stem_mfma<CC, EPI_BN_RELU, true>), grid, dim3(256), 0, st, x, boards, players, ws, scale, shift, out, M); \
        else if (epi == EPI_RAW) hipLaunchKernelGGL((stem_mfma<CC, EPI_RAW, false>), grid, dim3(256), 0, st, x, boards, players, ws, scale, shift, out, M); \
        else hipLaunchKernelGGL((stem_mfma<CC, EPI_BN_RELU, false>), grid, dim3(256), 0, st, x, boards, players, ws, scale, shift, out, M); \
        return hipGetLastError();
        switch (C) {
            AZG_STEM_MFMA(64)
            AZG_STEM_MFMA(128)
            AZG_STEM_MFMA(256)
            default: return hipErrorInvalidValue;
        }
#undef AZG_STEM_MFMA
    }
#define AZG_STEM_CASE(CC)                                                                              \
    case CC:                                                                                           \
        if (boards) hipLaunchKernelGGL((stem_conv<CC, EPI_BN_RELU, true>), dim3(B), dim3(256), 0, st, x, boards, players, ws, scale, shift, out); \
        else if (epi == EPI_RAW) hipLaunchKernelGGL((stem_conv<CC, EPI_RAW>), dim3(B), dim3(256), 0, st, x, boards, players, ws, scale, shift, out); \
        else hipLaunchKernelGGL((stem_conv<CC, EPI_BN_RELU>), dim3(B), dim3(256), 0, st, x, boards, players, ws, scale, shift, out); \
        return hipGetLastError();
    switch (C) {
        AZG_STEM_CASE(64)
        AZG_STEM_CASE(128)
        AZG_STEM_CASE(256)
        default: return hipErrorInvalidValue;
    }
#undef AZG_STEM_CASE
}

}  // namespace azg
