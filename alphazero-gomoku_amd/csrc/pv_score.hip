// Scoring of eval-forward outputs against targets (include/azg_pv.h azg_pv_score_outputs):
// the two loss terms of the train step (reference network.py:162-163,216-219) and a few
// policy / value metrics per board, without a train step -- nothing is written but the
// records and their sums.
//   score_heads  one wave per board: log_softmax, KL, entropy, argmaxes, (v - z)^2
//   score_reduce one workgroup: the records summed in fp64 in an order fixed by B alone
#include "pv_internal.h"

namespace azg {

__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// per board (one wave, four boards per workgroup: the geometry of heads_finalize and
// heads_loss_kernel).  lp and the KL term are heads_loss_kernel's expressions (pv_train.hip).
__global__ __launch_bounds__(256) void score_heads(const float* __restrict__ logits, const float* __restrict__ values,
                                                   const float* __restrict__ pis, const float* __restrict__ zs,
                                                   float* __restrict__ per_board, int B)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* lrow = logits + (size_t)b * ACTIONS;
    const float* tp = pis + (size_t)b * ACTIONS;
    float lg[4], tv[4];
    float mx = -INFINITY, tmx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = lane + 64 * t;
        lg[t] = j < ACTIONS ? lrow[j] : -INFINITY;
        tv[t] = j < ACTIONS ? tp[j] : 0.f;
        mx = fmaxf(mx, lg[t]);
        if (j < ACTIONS) tmx = fmaxf(tmx, tv[t]);
    }
    mx = wave_max(mx);
    tmx = wave_max(tmx);
    float se = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (lane + 64 * t < ACTIONS) se += expf(lg[t] - mx);
    se = wave_sum(se);
    const float lse = logf(se);
    // both argmaxes: the lowest index among equal maxima
    int jl = ACTIONS, jt = ACTIONS;
#pragma unroll
    for (int t = 3; t >= 0; --t) {
        const int j = lane + 64 * t;
        if (j < ACTIONS && lg[t] == mx) jl = j;
        if (j < ACTIONS && tv[t] == tmx) jt = j;
    }
    jl = wave_min_i(jl);
    jt = wave_min_i(jt);
    float kl = 0.f, st = 0.f, ent = 0.f, pb = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = lane + 64 * t;
        if (j < ACTIONS) {
            const float lp = (lg[t] - mx) - lse;
            if (tv[t] > 0.f) kl += tv[t] * (logf(tv[t]) - lp);
            st += tv[t];
            // from lp, never from log(p): an underflowed probability contributes exactly 0
            const float p = expf(lp);
            if (p > 0.f) ent -= p * lp;
            if (j == jt) pb = p;
        }
    }
    kl = wave_sum(kl);
    st = wave_sum(st);
    ent = wave_sum(ent);
    pb = wave_sum(pb);   // one lane holds it, the others 0: exact
    if (lane == 0) {
        const float v = values[b], z = zs[b];
        float* r = per_board + (size_t)b * AZG_PV_SCORE_FIELDS;
        r[AZG_PV_SCORE_KL] = kl;
        r[AZG_PV_SCORE_SQ] = (v - z) * (v - z);
        r[AZG_PV_SCORE_ENTROPY] = ent;
        r[AZG_PV_SCORE_TOP1] = jl == jt ? 1.f : 0.f;
        r[AZG_PV_SCORE_P_BEST] = pb;
        r[AZG_PV_SCORE_V_AGREE] = v * z > 0.f ? 1.f : 0.f;
        r[AZG_PV_SCORE_DECIDED] = z != 0.f ? 1.f : 0.f;
        r[AZG_PV_SCORE_TARGET_MASS] = st;
    }
}

// One workgroup.  Thread i adds records i, i + 256, ... in increasing order in fp64; the
// 256 partials of a field are then added by a fixed LDS tree.  No atomics: the order, and
// so the result, depends on B alone.
__global__ __launch_bounds__(256) void score_reduce(const float* __restrict__ per_board, int B,
                                                    double* __restrict__ sums)
{
    constexpr int F = AZG_PV_SCORE_FIELDS;
    __shared__ double part[256][F + 1];
    const int i = threadIdx.x;
    double acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0;
    for (int b = i; b < B; b += 256) {
        const float* r = per_board + (size_t)b * F;
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] += (double)r[f];
    }
#pragma unroll
    for (int f = 0; f < F; ++f) part[i][f] = acc[f];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (i < s) {
#pragma unroll
            for (int f = 0; f < F; ++f) part[i][f] += part[i + s][f];
        }
        __syncthreads();
    }
    if (i < F) sums[i] = part[0][i];
}

}  // namespace azg

extern "C" int32_t azg_pv_score_outputs(const float* logits, const float* values, const float* pis, const float* zs,
                                        int32_t batch, float* per_board, double* sums, void* stream)
{
    using namespace azg;
    if (!logits) return set_error("azg_pv_score_outputs: logits is null", hipSuccess);
    if (!values) return set_error("azg_pv_score_outputs: values is null", hipSuccess);
    if (!pis) return set_error("azg_pv_score_outputs: pis is null", hipSuccess);
    if (!zs) return set_error("azg_pv_score_outputs: zs is null", hipSuccess);
    if (!per_board) return set_error("azg_pv_score_outputs: per_board is null", hipSuccess);
    if (batch < 1) return set_error("azg_pv_score_outputs: batch must be >= 1", hipSuccess);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(score_heads, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, logits, values, pis, zs,
                       per_board, batch);
    if (hipError_t e = hipGetLastError()) return set_error("azg_pv_score_outputs: score_heads launch", e);
    if (sums) {
        hipLaunchKernelGGL(score_reduce, dim3(1), dim3(256), 0, st, (const float*)per_board, batch, sums);
        if (hipError_t e = hipGetLastError()) return set_error("azg_pv_score_outputs: score_reduce launch", e);
    }
    return 0;
}
