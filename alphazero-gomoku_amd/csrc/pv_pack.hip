// Weight re-packing and BatchNorm folding (run when parameters change).
//
// Torch layouts in (network.py:41-73): conv [Cout][Cin][3][3], linear [out][in].
// Packed layouts out:
//   res conv  -> wp[kc][n][32], kc = tap*(C/32) + cin/32, tap = ky*3 + kx
//   dgrad     -> wd[kc][n=cin][32 of cout] for the flipped tap 8 - tap (transpose
//                conv: dX[ci] at q = sum over taps and cout of dY[co] at q + off(t') W[co][ci][2-ky'][2-kx'])
//   stem      -> ws[k][c], k = cin*9 + ky*3 + kx
//   FC        -> W^T [in][out]
// Eval-mode BN fold, as ATen's CPU inference path (alpha = invstd*gamma,
// beta = bias - mean*alpha, y = x*alpha + beta):
//   invstd = 1/sqrt(running_var + eps)
#include "pv_internal.h"

namespace azg {


// All residual convs at once: layer l = blockIdx.y reads params + offs[l] and
// writes the forward packing to wp + l*9*C*C and, when wd is given, the dgrad
// packing to wd + l*9*C*C (one launch instead of 2 per layer).
__global__ void pack_convs_kernel(const float* __restrict__ params, const int64_t* __restrict__ offs,
                                  float* __restrict__ wp, float* __restrict__ wd, int C)
{
    const int total = 9 * C * C;
    const int cg_n = C / 32;
    const float* w = params + offs[blockIdx.y];
    float* wpl = wp + (size_t)blockIdx.y * total;
    float* wdl = wd ? wd + (size_t)blockIdx.y * total : nullptr;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int k = idx & 31;
        const int n = (idx >> 5) % C;
        const int kc = idx / (32 * C);
        const int tap = kc / cg_n, cg = kc - tap * cg_n;
        const int c2 = cg * 32 + k;
        wpl[idx] = w[(n * C + c2) * 9 + tap];                 // = pack_conv3x3_kernel
        if (wdl) wdl[idx] = w[(c2 * C + n) * 9 + (8 - tap)];  // = pack_dgrad_kernel
    }
}

__global__ void pack_stem_kernel(const float* __restrict__ w, float* __restrict__ ws, int C)
{
    const int total = 27 * C;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int c = idx % C, k = idx / C;
        ws[idx] = w[c * 27 + k];
    }
}

__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int Cc)
{
    const int total = R * Cc;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int r = idx / Cc, c = idx - r * Cc;
        dst[c * R + r] = src[idx];
    }
}

// ---- activation exponents of the eval fold ----
// The split-fp16 eval convs (pv_halo.h VAR bit 64, pv_h3.h, pv_board*.hip) stage every
// activation x as hi = fp16(x), lo = fp16(x - hi): lo is a normal fp16 only while
// |x| >= ~2^-3 and carries a fixed 2^-25 absolute error below, which the next BN's
// gamma / sqrt(var + eps) (up to 316) scales back up.  A net whose BN gammas have shrunk
// has such activations, so the fold carries the trunk activation as 2^T x and block b's
// mid activation as 2^m_b x:
//   stem  scale, shift * 2^T          bn1_b  scale * 2^(m_b - T), shift * 2^m_b
//   heads scale * 2^-T                bn2_b  scale * 2^(T - m_b), shift * 2^T
// Powers of two commute with the ReLUs and the residual add, and every factor is exact:
// outputs change only through which bits hi / lo capture.  The exponents come from the
// parameters alone.  A(bn) = max_c(|beta_c| + 4 |gamma_c|) bounds the BN's output at 4
// sigma; an exponent lifts a bound below kActBand into [4, 8):
//   m_b = lift(A(bn1_b));  T = min(lift(A(stem)), kActTrunkCap - ilogb(A(stem) + sum_b A(bn2_b)))
// The cap keeps the trunk sum's bound below 2^13 (fp16 overflows at 2^16; the overflow
// guard stays the backstop).  Every bound of at least kActBand (gamma >= 1/16: seeded,
// calibrated and trained nets) gives exponent 0 and the fold is bit for bit the plain one.
// oracle/value_range.py act_exponents restates the rule.
constexpr float kActBand = 0.25f;
constexpr int kActTrunkCap = 12;
constexpr int kActMaxExp = 40;
constexpr int kActMaxBn = 256;   // BN layers a fold workgroup can bound (launch_repack_all checks)

__device__ __forceinline__ int act_lift(float bound)
{
    if (!(bound > 0.f && bound < kActBand)) return 0;
    const int e = 2 - ilogbf(bound);
    return e < kActMaxExp ? e : kActMaxExp;
}

// The fold of BN layer j (desc order: stem, (bn1, bn2) per block, policy, value; nl = 2 x
// blocks) by one workgroup of 256: eval-mode BN as ATen's CPU inference path (file header)
// times the activation exponents above.
__device__ __forceinline__ void fold_bn_layer(const float* __restrict__ params, const float* __restrict__ stats,
                                              const BnDesc* __restrict__ desc, int nbn, int nl, int j,
                                              float* __restrict__ scale, float* __restrict__ shift)
{
    __shared__ unsigned bound[kActMaxBn];   // bits of a non-negative float: their order is the floats' order
    __shared__ int ex[2];                   // the exponents of this layer's scale and shift
    for (int i = threadIdx.x; i < nbn; i += blockDim.x) bound[i] = 0u;
    __syncthreads();
    // the bounds this layer's exponents need: the stem's and every bn2's (T), its block's bn1 (m_b)
    const int own1 = j >= 1 && j <= nl ? ((j - 1) | 1) : -1;   // bn1 of j's block (bn1_b: 1 + 2b, bn2_b: 2 + 2b)
    for (int i = 0; i <= nl && i < nbn; ++i) {
        if (i != 0 && (i & 1) && i != own1) continue;
        const BnDesc d = desc[i];
        float m = 0.f;
        for (int c = threadIdx.x; c < d.c; c += blockDim.x)
            m = fmaxf(m, fabsf(params[d.beta_off + c]) + 4.f * fabsf(params[d.gamma_off + c]));
        if (m > 0.f) atomicMax(&bound[i], __float_as_uint(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float a_stem = __uint_as_float(bound[0]);
        float u = a_stem;
        for (int i = 2; i <= nl; i += 2) u += __uint_as_float(bound[i]);
        int T = act_lift(a_stem);
        if (T) {
            const int cap = kActTrunkCap - ilogbf(u);
            T = T < cap ? T : cap;
            T = T > 0 ? T : 0;
        }
        const int m = own1 > 0 ? act_lift(__uint_as_float(bound[own1])) : 0;
        int es, eh;
        if (j == 0) { es = T; eh = T; }
        else if (j > nl) { es = -T; eh = 0; }
        else if (j == own1) { es = m - T; eh = m; }
        else { es = T - m; eh = T; }
        ex[0] = es;
        ex[1] = eh;
    }
    __syncthreads();
    const int es = ex[0], eh = ex[1];
    const BnDesc d = desc[j];
    for (int c = threadIdx.x; c < d.c; c += blockDim.x) {
        const float invstd = 1.0f / sqrtf(stats[d.stat_off + d.c + c] + BN_EPS);
        const float alpha = invstd * params[d.gamma_off + c];
        scale[d.out_off + c] = ldexpf(alpha, es);
        shift[d.out_off + c] = ldexpf(params[d.beta_off + c] - stats[d.stat_off + c] * alpha, eh);
    }
}

// Every re-pack of repack() in ONE launch (it runs at the start of every train step,
// on the critical path): blockIdx.y < nl packs residual conv l (as pack_convs_kernel),
// y == nl the stem, y == nl + 1 the head FCs, y == nl + 2 folds the eval BN (one
// layer per blockIdx.x).  Same per-element arithmetic as the separate kernels.
struct RepackArgs {
    const float* params;
    const int64_t* conv_offs;
    float* wp;
    float* wd;
    int C, nl;
    const float* stem_w;
    float* ws;
    const float* wpf;
    const float* wv1;
    float* wfc;
    const float* stats;
    const BnDesc* desc;
    int nbn;
    float* scale;
    float* shift;
    int y0;       // first section of this launch (grid.y covers y0 .. y0 + grid.y - 1)
    int skip;     // a section to skip (-1: none)
};

__global__ __launch_bounds__(256) void repack_all_kernel(const RepackArgs a)
{
    const int y = a.y0 + (int)blockIdx.y;
    if (y == a.skip) return;
    const int C = a.C;
    const int stride = gridDim.x * blockDim.x;
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (y < a.nl) {
        const int total = 9 * C * C, cg_n = C / 32;
        const float* w = a.params + a.conv_offs[y];
        float* wpl = a.wp + (size_t)y * total;
        float* wdl = a.wd ? a.wd + (size_t)y * total : nullptr;
        for (int idx = i0; idx < total; idx += stride) {
            const int k = idx & 31, n = (idx >> 5) % C, kc = idx / (32 * C);
            const int tap = kc / cg_n, c2 = (kc - tap * cg_n) * 32 + k;
            wpl[idx] = w[(n * C + c2) * 9 + tap];
            if (wdl) wdl[idx] = w[(c2 * C + n) * 9 + (8 - tap)];
        }
    } else if (y == a.nl) {
        for (int idx = i0; idx < 27 * C; idx += stride) a.ws[idx] = a.stem_w[(idx % C) * 27 + idx / C];
    } else if (y == a.nl + 1) {
        for (int idx = i0; idx < FC_OUT * FC_KP; idx += stride) {
            const int j = idx / FC_KP, k = idx - j * FC_KP;
            float v = 0.f;
            if (j < ACTIONS) {
                if (k < 2 * PIX) v = a.wpf[j * 2 * PIX + k];
            } else if (k < PIX) {
                v = a.wv1[(j - ACTIONS) * PIX + k];
            }
            a.wfc[idx] = v;
        }
    } else if (blockIdx.x < (unsigned)a.nbn) {
        fold_bn_layer(a.params, a.stats, a.desc, a.nbn, a.nl, (int)blockIdx.x, a.scale, a.shift);
    }
}

// part: 0 every section; 1 the stem only (y = nl); 2 the residual convs (+ dgrad packs)
// and the head FCs -- neither the stem nor the eval BN fold (the train step's split
// repack: part 1 on the caller's stream, part 2 on the side stream)
hipError_t launch_repack_all(const float* params, const int64_t* conv_offs, int nl, float* wp, float* wd, int C,
                             const float* stem_w, float* ws, const float* wpf, const float* wv1, float* wfc,
                             const float* stats, const void* desc, int nbn, float* scale, float* shift,
                             hipStream_t st, int part)
{
    RepackArgs a{params, conv_offs, wp, wd, C, nl, stem_w, ws, wpf, wv1, wfc, stats, (const BnDesc*)desc, nbn,
                 scale, shift, part == 1 ? nl : 0, part == 2 ? nl : -1};
    if (nbn > kActMaxBn) return hipErrorInvalidValue;
    int nb = (9 * C * C + 255) / 256;
    nb = nb > 256 ? 256 : nb;
    nb = nb < nbn ? nbn : nb;
    if (part == 1) nb = (27 * C + 255) / 256;
    hipLaunchKernelGGL(repack_all_kernel, dim3(nb, part == 1 ? 1 : part == 2 ? nl + 2 : nl + 3), dim3(256), 0, st, a);
    return hipGetLastError();
}

static inline int nblk(int total) { int b = (total + 255) / 256; return b > 4096 ? 4096 : b; }

// ---- split-fp16 (H3) eval weights (pv_halo.h halo_tile VAR bit 64) ----
// e_l = 14 - floor(log2 max|w_l|): max|w_l| * 2^e < 2^15, so hi = fp16(w 2^e) never
// overflows and the lo parts of every weight above 2^-10 of the layer's largest stay
// normal fp16 (the rest carry 2^-25 absolute error).  The max runs on H3_MAXB workgroups
// per layer (float4 loads, one atomicMax on the bits of a non-negative float: their
// order is the floats' order); exps[l] holds those bits until scale_h3_kernel turns them
// into e_l (the train step re-packs every step: one workgroup per layer took 90 us).
constexpr int H3_MAXB = 32;
__device__ __forceinline__ int h3_exp_of(unsigned maxbits)
{
    const float m = __uint_as_float(maxbits);
    return m > 0.f ? 14 - ilogbf(m) : 0;
}
__global__ __launch_bounds__(256) void h3_max_kernel(const float* __restrict__ params, const int64_t* __restrict__ offs,
                                                     int C, unsigned* __restrict__ maxbits)
{
    __shared__ float red[256];
    const int l = blockIdx.y;
    const float* wl = params + offs[l];
    float m = 0.f;
    if ((offs[l] & 3) == 0) {   // the conv weights of the parameter layout start 16-B aligned (C % 32 == 0)
        const f32x4* w = (const f32x4*)wl;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < 9 * C * C / 4; i += H3_MAXB * 256) {
            const f32x4 v = w[i];
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < 9 * C * C; i += H3_MAXB * 256) m = fmaxf(m, fabsf(wl[i]));
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(maxbits + l, __float_as_uint(red[0]));
}

// packed row (kc * C + n) of 32 K values -> 64 halves [hi 32 | lo 32] of w * 2^e, in
// the fp32 packing's order (repack_all_kernel)
__global__ __launch_bounds__(256) void pack_h3_kernel(const float* __restrict__ params, const int64_t* __restrict__ offs,
                                                      int C, const unsigned* __restrict__ maxbits,
                                                      _Float16* __restrict__ out)
{
    const int total = 9 * C * C, cg_n = C / 32;
    const int l = blockIdx.y;
    const float* w = params + offs[l];
    _Float16* o = out + (size_t)l * 2 * total;
    const float sc = ldexpf(1.f, h3_exp_of(maxbits[l]));
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int k = idx & 31, n = (idx >> 5) % C, kc = idx / (32 * C);
        const int tap = kc / cg_n, c2 = (kc - tap * cg_n) * 32 + k;
        const float v = w[(n * C + c2) * 9 + tap] * sc;
        const _Float16 hi = (_Float16)v;
        const int row = idx >> 5;
        o[row * 64 + k] = hi;
        o[row * 64 + 32 + k] = (_Float16)(v - (float)hi);
    }
}

// scale16 = the eval BN scale of every residual conv's BN times 2^-e (exact); inv (train
// forward, optional) = 2^-e per layer and output channel: the raw conv output's factor;
// exps[l] <- e_l (it held the max bits)
__global__ void scale_h3_kernel(const float* __restrict__ scale, const int* __restrict__ conv_bn_off,
                                int* __restrict__ exps, int C, float* __restrict__ scale16,
                                float* __restrict__ inv)
{
    const int l = blockIdx.x, o = conv_bn_off[l];
    const int e = h3_exp_of((unsigned)exps[l]);
    __syncthreads();   // every thread has read the bits before thread 0 replaces them
    const float f = ldexpf(1.f, -e);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        scale16[o + c] = scale[o + c] * f;
        if (inv) inv[l * C + c] = f;
    }
    if (threadIdx.x == 0) exps[l] = e;
}

hipError_t launch_pack_h3(const float* params, const int64_t* offs, int nl, int C, const int* conv_bn_off,
                          const float* scale, int* exps, void* wp16, float* scale16, float* inv, hipStream_t st)
{
    if (nl <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(exps, 0, (size_t)nl * sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(h3_max_kernel, dim3(H3_MAXB, nl), dim3(256), 0, st, params, offs, C, (unsigned*)exps);
    int nb = nblk(9 * C * C);
    nb = nb > 256 ? 256 : nb;
    hipLaunchKernelGGL(pack_h3_kernel, dim3(nb, nl), dim3(256), 0, st, params, offs, C, (const unsigned*)exps,
                       (_Float16*)wp16);
    hipLaunchKernelGGL(scale_h3_kernel, dim3(nl), dim3(256), 0, st, scale, conv_bn_off, exps, C, scale16, inv);
    return hipGetLastError();
}

// the one-product fp16 eval precision's weights: the hi halves of pack_h3's rows alone, 64-B
// rows [kc * C + n][32] of fp16(w * 2^e) with the layer's e (exps, after scale_h3_kernel) --
// the operand the board16 tower's one-product form streams (pv_board16.hip, NP = 1)
__global__ __launch_bounds__(256) void pack_h1_kernel(const float* __restrict__ params, const int64_t* __restrict__ offs,
                                                      int C, const int* __restrict__ exps, _Float16* __restrict__ out)
{
    const int total = 9 * C * C, cg_n = C / 32;
    const int l = blockIdx.y;
    const float* w = params + offs[l];
    _Float16* o = out + (size_t)l * total;
    const float sc = ldexpf(1.f, exps[l]);
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int k = idx & 31, n = (idx >> 5) % C, kc = idx / (32 * C);
        const int tap = kc / cg_n, c2 = (kc - tap * cg_n) * 32 + k;
        o[idx] = (_Float16)(w[(n * C + c2) * 9 + tap] * sc);
    }
}

hipError_t launch_pack_h1(const float* params, const int64_t* offs, int nl, int C, const int* exps, void* wp1,
                          hipStream_t st)
{
    if (nl <= 0) return hipSuccess;
    int nb = nblk(9 * C * C);
    nb = nb > 256 ? 256 : nb;
    hipLaunchKernelGGL(pack_h1_kernel, dim3(nb, nl), dim3(256), 0, st, params, offs, C, exps, (_Float16*)wp1);
    return hipGetLastError();
}

// the split-fp16 dgrad packing (key 50): pack_h3's rows for the flipped, transposed taps
// of pack_convs_kernel's wd (row kc * C + n = cin n, K values = 32 couts of group kc % CG
// at tap 8 - kc / CG), w * 2^e with the layer's e (exps, after scale_h3_kernel)
__global__ __launch_bounds__(256) void pack_h3_dgrad_kernel(const float* __restrict__ params,
                                                            const int64_t* __restrict__ offs, int C,
                                                            const int* __restrict__ exps, _Float16* __restrict__ out)
{
    const int total = 9 * C * C, cg_n = C / 32;
    const int l = blockIdx.y;
    const float* w = params + offs[l];
    _Float16* o = out + (size_t)l * 2 * total;
    const float sc = ldexpf(1.f, exps[l]);
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int k = idx & 31, n = (idx >> 5) % C, kc = idx / (32 * C);
        const int tap = kc / cg_n, c2 = (kc - tap * cg_n) * 32 + k;
        const float v = w[(c2 * C + n) * 9 + (8 - tap)] * sc;
        const _Float16 hi = (_Float16)v;
        const int row = idx >> 5;
        o[row * 64 + k] = hi;
        o[row * 64 + 32 + k] = (_Float16)(v - (float)hi);
    }
}

hipError_t launch_pack_h3_dgrad(const float* params, const int64_t* offs, int nl, int C, const int* exps, void* wd16,
                                hipStream_t st)
{
    if (nl <= 0) return hipSuccess;
    int nb = nblk(9 * C * C);
    nb = nb > 256 ? 256 : nb;
    hipLaunchKernelGGL(pack_h3_dgrad_kernel, dim3(nb, nl), dim3(256), 0, st, params, offs, C, exps, (_Float16*)wd16);
    return hipGetLastError();
}

hipError_t launch_pack_convs(const float* params, const int64_t* offs, int nl, float* wp, float* wd, int C,
                             hipStream_t st)
{
    int nb = nblk(9 * C * C);
    nb = nb > 256 ? 256 : nb;
    hipLaunchKernelGGL(pack_convs_kernel, dim3(nb, nl), dim3(256), 0, st, params, offs, wp, wd, C);
    return hipGetLastError();
}

hipError_t launch_pack_stem(const float* w, float* ws, int C, hipStream_t st)
{
    hipLaunchKernelGGL(pack_stem_kernel, dim3(nblk(27 * C)), dim3(256), 0, st, w, ws, C);
    return hipGetLastError();
}

// head FC weights -> wfc[FC_OUT][FC_KP] (pv_common.h): policy_fc rows (K = 450) then
// value_fc1 rows (K = 225), zero-padded to FC_KP
__global__ void pack_fc_kernel(const float* __restrict__ wpf, const float* __restrict__ wv1, float* __restrict__ wfc)
{
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < FC_OUT * FC_KP; idx += gridDim.x * blockDim.x) {
        const int j = idx / FC_KP, k = idx - j * FC_KP;
        float v = 0.f;
        if (j < ACTIONS) {
            if (k < 2 * PIX) v = wpf[j * 2 * PIX + k];
        } else if (k < PIX) {
            v = wv1[(j - ACTIONS) * PIX + k];
        }
        wfc[idx] = v;
    }
}

hipError_t launch_pack_fc(const float* wpf, const float* wv1, float* wfc, hipStream_t st)
{
    hipLaunchKernelGGL(pack_fc_kernel, dim3(nblk(FC_OUT * FC_KP)), dim3(256), 0, st, wpf, wv1, wfc);
    return hipGetLastError();
}

hipError_t launch_transpose(const float* src, float* dst, int R, int Cc, hipStream_t st)
{
    hipLaunchKernelGGL(transpose_kernel, dim3(nblk(R * Cc)), dim3(256), 0, st, src, dst, R, Cc);
    return hipGetLastError();
}

}  // namespace azg
