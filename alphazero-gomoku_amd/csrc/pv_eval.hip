// How an eval forward runs (the work behind the C-ABI's forward and recover entry points,
// pv_capi.hip): the eval workspace, the packs of the current parameters, the residual
// tower's dispatchers and autotuner, the forward itself, and the recompute of a posted launch.
#include "pv_internal.h"

#include <chrono>
#include <map>
#include <tuple>

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace azg;

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

namespace azg {
int g_tower_breaker_s = 30;   // key 18 (0: off)
}

static int32_t fail(const char* what, hipError_t e = hipSuccess) { return set_error(what, e); }

namespace azg {

// The shared tail of the public forwards (their argument checks done): workspace for the
// call's images, the packs of the current parameters, the forward.
int32_t run_eval(azg_pv* h, const EvalCall& c, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (int32_t r = ensure_eval_workspace(h, c.images(), st)) return r;
    if (h->dirty) {
        if (int32_t r = repack(h, st)) return r;
        h->dirty = false;
    }
    return forward_eval(h, c, st);
}

// Fold every recorded event pair into the per-class sums (waits for them).
hipError_t prof_harvest(azg_pv* h)
{
    for (int i = 0; i < h->prof_used; ++i) {
        if (hipError_t e = hipEventSynchronize(h->prof_ev[2 * i + 1])) return e;
        float t = 0.f;
        if (hipError_t e = hipEventElapsedTime(&t, h->prof_ev[2 * i], h->prof_ev[2 * i + 1])) return e;
        h->prof_ms[h->prof_cls[i]] += t;
        h->prof_n[h->prof_cls[i]] += 1;
    }
    h->prof_used = 0;
    return hipSuccess;
}

int prof_begin(azg_pv* h, int cls, hipStream_t st, int64_t boards)
{
    if (!h->prof_on) return -1;
    // event pool full (long self-play runs): fold the recorded pairs in first
    if (h->prof_used >= (int)h->prof_cls.size() && prof_harvest(h) != hipSuccess) return -1;
    h->prof_work[cls] += boards;
    const int i = h->prof_used++;
    h->prof_cls[i] = cls;
    (void)hipEventRecord(h->prof_ev[2 * i], st);
    return i;
}

void prof_end(azg_pv* h, int pair, hipStream_t st)
{
    if (pair >= 0) (void)hipEventRecord(h->prof_ev[2 * pair + 1], st);
}

// the eval workspace (sized by act_cap images): activations, head features, tower records
static void free_eval_workspace(azg_pv* h)
{
    for (int i = 0; i < 3; ++i) {
        if (h->act[i]) (void)hipFree(h->act[i]);
        h->act[i] = nullptr;
    }
    if (h->hbuf) (void)hipFree(h->hbuf);
    h->hbuf = nullptr;
    if (h->tower_sync) (void)hipFree(h->tower_sync);
    h->tower_sync = nullptr;
    if (h->tower_prod) (void)hipFree(h->tower_prod);
    h->tower_prod = nullptr;
    h->act_cap = 0;
}

void free_workspace(azg_pv* h)
{
    free_eval_workspace(h);
    free_train_workspace(h);
}

int32_t ensure_eval_workspace(azg_pv* h, int images, hipStream_t st)
{
    if (images <= h->act_cap) return 0;
    int cap = h->act_cap ? h->act_cap : 64;
    while (cap < images) cap *= 2;
    free_eval_workspace(h);
    {
        hipError_t e = hipMalloc(&h->tower_sync, tower_sync_bytes(2 * h->NB, cap * PIX));
        // azg_pv_tower_status reads its timeout word before any tower launch has written it
        // (a handle that has only run per-layer convs or the board tower): 0, not what hipMalloc left
        if (e == hipSuccess) e = hipMemsetAsync(h->tower_sync, 0, tower_sync_bytes(2 * h->NB, cap * PIX), st);
        if (e != hipSuccess) return fail("ensure_eval_workspace: tower sync words", e);
        e = hipMalloc(&h->tower_prod, tower_prod_bytes(2 * h->NB, cap * PIX));
        if (e == hipSuccess) e = hipMemsetAsync(h->tower_prod, 0, tower_prod_bytes(2 * h->NB, cap * PIX), st);
        if (e != hipSuccess) return fail("ensure_eval_workspace: tower producer records", e);
    }
    {
        const size_t hb = (size_t)cap * (FC_FS + FC_OUT) * sizeof(float);
        hipError_t e = hipMalloc(&h->hbuf, hb);
        if (e != hipSuccess) return fail("ensure_eval_workspace: hipMalloc(head features)", e);
        e = hipMemsetAsync(h->hbuf, 0, hb, st);   // feature pads: zero, never written
        if (e != hipSuccess) return fail("ensure_eval_workspace: hipMemsetAsync(head features)", e);
    }
    const size_t bytes = (size_t)cap * PADPIX * h->C * sizeof(float);
    for (int i = 0; i < 3; ++i) {
        hipError_t e = hipMalloc(&h->act[i], bytes);
        if (e != hipSuccess) return fail("ensure_eval_workspace: hipMalloc(activations)", e);
        // zero halo: written once, never touched by the kernels
        e = hipMemsetAsync(h->act[i], 0, bytes, st);
        if (e != hipSuccess) return fail("ensure_eval_workspace: hipMemsetAsync", e);
    }
    h->act_cap = cap;
    return 0;
}

int32_t repack(azg_pv* h, hipStream_t st, float* dgrad_dst, int part)
{
    const int C = h->C;
    h->h3_dirty = true;
    const float* P = h->params;
    // stem, head FCs, every residual conv (+ its dgrad packing when training) and
    // the eval BN fold: one launch
    AZG_TRY(launch_repack_all(P, h->conv_off_dev, 2 * h->NB, h->wpack, dgrad_dst, C, P + h->poff[h->t_stem_w],
                              h->wstem, P + h->poff[h->t_pfc_w], P + h->poff[h->t_vfc1_w], h->wfc, h->bn,
                              h->bn_desc_dev, (int)h->bn_desc.size(), h->scale, h->shift, st, part),
            "repack");
    return 0;
}

// The split-fp16 (H3) eval weights of the current parameters (pv_pack.hip pack_h3):
// allocated on first use, re-packed after every repack.
int32_t ensure_h3(azg_pv* h, hipStream_t st, bool fp16)
{
    const int C = h->C, nl = 2 * h->NB;
    if (!h->wpack16) {
        const std::vector<int>& off = h->conv_bn_off;
        hipError_t e = handle_malloc(h, &h->wpack16, (size_t)(nl > 0 ? nl : 1) * 9 * C * C * sizeof(float));
        if (e == hipSuccess) e = handle_malloc(h, &h->scale16, (size_t)h->nfold * sizeof(float));
        if (e == hipSuccess) e = handle_malloc(h, &h->h3exp, (size_t)(nl > 0 ? nl : 1) * sizeof(int));
        if (e == hipSuccess) e = handle_malloc(h, &h->h3inv, (size_t)(nl > 0 ? nl : 1) * C * sizeof(float));
        if (e == hipSuccess) e = handle_malloc(h, &h->conv_bn_off_dev, off.size() * sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(h->conv_bn_off_dev, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail("forward: split-fp16 weight buffers", e);
        h->h3_dirty = true;
    }
    if (h->h3_dirty) {
        AZG_TRY(launch_pack_h3(h->params, h->conv_off_dev, nl, C, h->conv_bn_off_dev, h->scale, h->h3exp, h->wpack16,
                               h->scale16, h->h3inv, st),
                "forward: split-fp16 weight pack");
        h->h3_dirty = false;
        ++h->h3_gen;
    }
    if (fp16) {   // the hi halves alone, for handles that selected the one-product precision
        if (!h->wpack1) {
            AZG_TRY(handle_malloc(h, &h->wpack1, (size_t)nl * 9 * C * C * sizeof(_Float16)), "forward: fp16 weight buffer");
            h->h1_gen = 0;
        }
        if (h->h1_gen != h->h3_gen) {
            AZG_TRY(launch_pack_h1(h->params, h->conv_off_dev, nl, C, h->h3exp, h->wpack1, st), "forward: fp16 weight pack");
            h->h1_gen = h->h3_gen;
        }
    }
    return 0;
}

// H3 per-layer tile: the 64x64 / 4-wave tile (shape 5, up to 4 workgroups per CU) or the
// 128x64 / 8-wave tile (shape 8, 2 per CU), whichever needs fewer 128-row-equivalent
// rounds of resident slots (ties: the 128-row tile).  Both compute the same arithmetic.
static int conv_tuned_shape_h3(const azg_pv* h, int images)
{
    if (g_conv_shape_override == 5 || g_conv_shape_override == 8) return g_conv_shape_override;   // CONV_SHAPE
    const int M = images * PIX, ntn = h->C / 64;
    const long t5 = (long)((M + 63) / 64) * ntn, t8 = (long)((M + 127) / 128) * ntn;
    const long r5 = (t5 + 1023) / 1024, r8 = (t8 + 511) / 512;
    return r5 < 2 * r8 ? 5 : 8;
}

// How one forward runs its residual tower (forward_eval decides, the autotuner tries each).
struct TowerPlan {
    int variant = 0;          // see stem_and_tower
    bool h3 = false;          // split-fp16 residual convs
    unsigned seq = 0;         // the launch's number (0: not posted)
    bool fp16 = false;        // the one-product fp16 precision (variant 14 with one product)
    bool recompute = false;   // azg_pv_recover's rerun: must not wait across workgroups
    bool unsplit = false;     // the breaker is open: variant 14 runs one workgroup per board (no exchange waits)
};

// The heads' 1x1 projection weights and folded BN: policy (2 channels) then value (1), contiguous.
struct HeadProj { const float *wpc, *wvc, *scale, *shift; };
static HeadProj head_proj(const azg_pv* h)
{
    const int ho = h->bn_desc[h->bn_pol].out_off;
    return {h->params + h->poff[h->t_pc_w], h->params + h->poff[h->t_vc_w], h->scale + ho, h->shift + ho};
}

static int32_t stem(azg_pv* h, const EvalCall& c, hipStream_t st)
{
    const int o = h->bn_desc[h->bn_stem].out_off;
    const int pr = prof_begin(h, AZG_PROF_STEM, st, c.images());
    AZG_TRY(launch_stem(h->C, EPI_BN_RELU, c.x, h->wstem, h->scale + o, h->shift + o, h->act[0], c.images(), st,
                        c.boards, c.players, c.syms, c.symmode),
            "forward: stem");
    prof_end(h, pr, st);
    return 0;
}

// The exchange buffers of a split board16 launch (allocated on first use) and its flag epoch.
static int32_t next_b16_split(azg_pv* h, hipStream_t st, Board16Split* sp)
{
    if (!h->b16x) {
        AZG_TRY(handle_malloc(h, &h->b16x, (size_t)kB16SplitCap * 2 * kB16ImgBytes), "forward: split images");
        AZG_TRY(handle_malloc(h, &h->b16flag, (size_t)kB16SplitCap * 3 * sizeof(unsigned)), "forward: split flags");
        AZG_TRY(hipMemsetAsync(h->b16x, 0, (size_t)kB16SplitCap * 2 * kB16ImgBytes, st), "forward: split images");
        h->b16epoch = 1u << 25;   // forces the flag reset below
    }
    if (++h->b16epoch >= 1u << 25) {   // tags epoch * 64 + layer stay monotonic: restart them at 1
        AZG_TRY(hipMemsetAsync(h->b16flag, 0, (size_t)kB16SplitCap * 3 * sizeof(unsigned), st), "forward: split flags");
        h->b16epoch = 1;
    }
    *sp = Board16Split{h->b16x, h->b16flag, h->b16epoch, h->posted.ring_dev, h->tower_diag};
    return 0;
}

// True when board_tower runs some board of a variant-14 launch of `images` split (the whole
// small batch, or the last partial round): the launches that wait across workgroups.
static bool board16_would_split(int images)
{
    const int smax = board16_split_max(), grid = board16_grid();
    if (images > 0 && images <= smax) return true;
    return images > grid && grid > 0 && images % grid != 0 && images % grid <= smax;
}

// The board-resident tower (pv_board.hip, pv_board16.hip; variants 13 and 14): every conv of
// one board from LDS, the tower output in place over the stem output in act[0].
static int32_t board_tower(azg_pv* h, int images, hipStream_t st, const TowerPlan& p)
{
    const bool b16 = p.variant == 14;
    const int* off = h->conv_bn_off.data();
    float* X = h->act[0];
    // EVAL_ARITH = 2: small batches run split (three workgroups per board, heads unfused; not
    // for a recompute or under an open breaker, which must not wait across workgroups), the
    // rest one workgroup per board with the heads' projections fused (features into hbuf,
    // forward_eval)
    // a one-workgroup launch of B = k * grid + r boards ends with r boards on r CUs: for
    // r <= BOARD16_SPLIT_MAX those r run split after the k full rounds (their heads projected here)
    const int smax = b16 && !p.recompute && !p.unsplit ? board16_split_max() : 0;
    const int grid = b16 ? board16_grid() : 0;
    const int tail = b16 && images > grid && grid > 0 && images % grid <= smax ? images % grid : 0;
    h->b16_split = b16 && images <= smax;
    // one hipEvent bracket per tower launch (the tail's is a second board16 launch)
    int pr = prof_begin(h, b16 ? AZG_PROF_BOARD16 : AZG_PROF_BOARD, st, images - tail);
    const HeadProj hp = head_proj(h);
    // one workgroup per board with the heads fused (sp null), or split with the heads left out
    auto tower16 = [&](float* x, int n, const Board16Split* sp) {
        const bool fused = sp == nullptr;
        return launch_board16_tower(h->NB, (const float*)(p.fp16 ? h->wpack1 : h->wpack16), h->scale16, h->shift, off, x,
                                    n, h->posted.ovf_dev, p.seq, st, fused ? hp.wpc : nullptr,
                                    fused ? hp.wvc : nullptr, fused ? hp.scale : nullptr, fused ? hp.shift : nullptr,
                                    fused ? h->hbuf : nullptr, sp, p.fp16 ? 1 : 3);
    };
    if (!b16) {
        AZG_TRY(launch_board_tower(h->NB, (const float*)h->wpack16, h->scale16, h->shift, off, X, images,
                                   h->posted.ovf_dev, p.seq, st),
                "forward: board tower");
    } else if (!h->b16_split && !tail) {
        AZG_TRY(tower16(X, images, nullptr), "forward: board tower (16x16x32)");
    } else {
        Board16Split sp{};
        if (int32_t r = next_b16_split(h, st, &sp)) return r;
        if (!tail) {
            AZG_TRY(tower16(X, images, &sp), "forward: board tower (16x16x32, split)");
        } else {   // the k full rounds one workgroup per board, heads fused
            const int nmain = images - tail;
            AZG_TRY(tower16(X, nmain, nullptr), "forward: board tower (16x16x32)");
            prof_end(h, pr, st);
            float* Xt = X + (size_t)nmain * PADPIX * h->C;
            pr = prof_begin(h, AZG_PROF_BOARD16, st, tail);
            AZG_TRY(tower16(Xt, tail, &sp), "forward: board tower (16x16x32, split tail)");
            prof_end(h, pr, st);
            pr = prof_begin(h, AZG_PROF_HEADS, st, 0);
            AZG_TRY(launch_heads_project(h->C, true, Xt, hp.wpc, hp.wvc, hp.scale, hp.shift,
                                         h->hbuf + (size_t)nmain * FC_FS, tail * PIX, st, FC_FS, FC_KP),
                    "forward: heads projection (split tail)");
        }
    }
    prof_end(h, pr, st);
    return 0;
}

// The whole residual tower in one persistent launch of tiles (pv_tower.hip).
static int32_t tile_tower(azg_pv* h, int images, hipStream_t st, const TowerPlan& p, float** out)
{
    const bool wide = p.variant == 10 || p.variant == 12;
    const int pr = prof_begin(h, wide ? AZG_PROF_TOWER_WIDE : AZG_PROF_TOWER, st, images);
    const TowerSync ts{h->tower_sync, h->posted.ring_dev, h->posted.ovf_dev, h->tower_diag, h->tower_prod, p.seq};
    AZG_TRY(launch_tower(h->C, h->NB, p.variant, h->act, p.h3 ? (const float*)h->wpack16 : h->wpack,
                         p.h3 ? h->scale16 : h->scale, h->shift, h->conv_bn_off.data(), images * PIX, ts, st, out,
                         p.h3),
            "forward: tower");
    prof_end(h, pr, st);
    return 0;
}

// One launch per conv: fp32 MFMA, or the split-fp16 tile (the tower's arithmetic, layer by layer).
static int32_t per_layer_tower(azg_pv* h, int images, hipStream_t st, const TowerPlan& p, float** out)
{
    const int C = h->C, M = images * PIX;
    const int shape = p.h3 ? conv_tuned_shape_h3(h, images) : 0;
    const float* wp = p.h3 ? (const float*)h->wpack16 : h->wpack;
    const float* scale = p.h3 ? h->scale16 : h->scale;
    auto conv = [&](int l, int epi, const float* in, const float* resid, float* dst) {
        const int o = h->conv_bn_off[l];
        const ConvCall cc{in, wp + (size_t)l * 9 * C * C, scale + o, h->shift + o, resid, dst, M, st};
        const int pr = prof_begin(h, AZG_PROF_CONV3X3, st, images);
        const hipError_t e = p.h3 ? launch_conv3x3_h3(shape, C, epi, cc, h->posted.ovf_dev, p.seq)
                                  : launch_conv3x3(C, epi, cc);
        if (e == hipSuccess) prof_end(h, pr, st);
        return e;
    };
    float *X = h->act[0], *H = h->act[1], *Y = h->act[2];
    for (int i = 0; i < h->NB; ++i) {
        AZG_TRY(conv(2 * i, EPI_BN_RELU, X, nullptr, H), "forward: conv1");
        AZG_TRY(conv(2 * i + 1, EPI_BN_RES_RELU, H, X, Y), "forward: conv2");
        float* t = X; X = Y; Y = t;
    }
    *out = X;
    return 0;
}

// Stem + residual tower.  variant 0: one launch per conv; 5 / 8 / 10 / 12: the persistent
// tower (pv_tower.hip) with 64x64 / 128x64 / 128x128 (16-wave) / h3_tile tiles; 13 / 14: the
// board-resident tower on 32x32x16 / 16x16x32 MFMAs.  Within one arithmetic all are bitwise
// identical.  *out: the activation buffer that holds the tower output.
static int32_t stem_and_tower(azg_pv* h, const EvalCall& c, hipStream_t st, const TowerPlan& p, float** out)
{
    if (int32_t r = stem(h, c, st)) return r;
    if ((p.variant == 13 || p.variant == 14) && h->NB > 0) {
        *out = h->act[0];
        return board_tower(h, c.images(), st, p);
    }
    if (p.variant != 0 && h->NB > 0) return tile_tower(h, c.images(), st, p, out);
    return per_layer_tower(h, c.images(), st, p, out);
}

int g_tower_mode = 2;   // 0 per-layer launches, 1 persistent tower, 2 tuned per batch bucket

// Tower variant per (C, blocks, batch bucket): g_tower_mode 0 = per-layer launches,
// 1 = persistent tower with shape g_tower_shape, 2 = timed on first use of the
// bucket (stem + tower, every variant, best of 2 after a warm pass).  Candidates: 0
// per-layer launches; 5 / 8 the tower with 64x64 / 128x64 tiles (2-4 workgroups per
// CU, acquire hand-off, buffer-resource addressing).  The 128x64 tower is preferred
// for batches >= 128 (round 3, scripts/tower_r3_ab.py: 87.0 / 90.2 / 91.0 / 91.2 % of
// peak at 512 / 1024 / 2048 / 4096 boards vs 80.7 / 84.1 / 86.4 / 87.8 % per-layer) and
// kept unless another candidate is > 2 % faster, so timing noise cannot flip
// near-equal choices.  Shape 10 (16-wave 128x128 tiles, one workgroup per CU: 1.30x
// algorithmic HBM bytes instead of 1.76x) is measured slower at every batch (83.6 %)
// and is not a candidate; key 6 = 10 forces it.  While the stream is being captured
// the untuned default is used.  All variants are bitwise identical.
static int tower_variant(azg_pv* h, const EvalCall& c, hipStream_t st, bool h3)
{
    const int batch = c.images();   // what the stem and the tower process
    if (h->NB == 0 || h->NB > kTowerMaxBlocks) return 0;
    if ((size_t)batch * PADPIX * h->C * sizeof(float) >= (size_t)INT32_MAX) return 0;
    if (g_tower_mode == 0) return 0;
    const bool board_ok = h3 && h->C == 128;   // the board-resident tower: split-fp16, C = 128 (LDS)
    if (g_tower_mode == 1)
        return ((g_tower_shape == 10 && (h->C != 128 || h3)) || (g_tower_shape == 12 && !h3) ||
                (g_tower_shape == 13 && !board_ok))
                   ? 8
                   : g_tower_shape == 14 ? (board_ok ? 13 : 8)   // 14 is key 19 = 2's form
                                         : g_tower_shape;
    const int bucket = conv_batch_bucket(batch * PIX);
    static std::map<std::tuple<int, int, int, int>, int> cache;
    const auto key = std::make_tuple(h->C, h->NB, bucket, (int)h3);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    const int fallback = batch >= 128 ? 8 : 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return fallback;
    const bool prof = h->prof_on;
    h->prof_on = false;
    // split-fp16: + shape 12, the h3_tile 128x128 tower (pv_h3.h); C = 128: + 13, the
    // board-resident tower (pv_board.hip)
    const int cand[5] = {0, 5, 8, 12, 13};
    const int ncand = board_ok ? 5 : h3 ? 4 : 3;
    float best_ms[5] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f};
    hipEvent_t e0, e1;
    int choice = fallback;
    if (hipEventCreate(&e0) == hipSuccess) {
        if (hipEventCreate(&e1) == hipSuccess) {
            bool ok = true;
            float* out = nullptr;
            for (int r = 0; r < 3 && ok; ++r)
                for (int k = 0; k < ncand && ok; ++k) {
                    ok = hipEventRecord(e0, st) == hipSuccess &&
                         stem_and_tower(h, c, st, TowerPlan{cand[k], h3}, &out) == 0 &&
                         hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
                    float ms = 0.f;
                    if (ok && r > 0 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < best_ms[k]) best_ms[k] = ms;
                }
            if (ok) {
                int b = 0;
                for (int k = 1; k < ncand; ++k)
                    if (best_ms[k] < best_ms[b]) b = k;
                if (batch >= 128 && best_ms[2] <= 1.02f * best_ms[b]) b = 2;   // the 128x64 tower
                if (h3 && batch >= 128 && best_ms[3] < 0.98f * best_ms[b]) b = 3;   // unless h3_tile beats it by 2 %
                if (board_ok && best_ms[4] < 0.98f * best_ms[b]) b = 4;            // or the board tower does
                choice = cand[b];
            }
            if (getenv("AZG_TUNE_LOG"))
                fprintf(stderr, "[azg tune] C=%d NB=%d batch=%d h3=%d ok=%d per-layer %.4f tower64 %.4f tower128 %.4f "
                        "h3tile %.4f board %.4f -> %d\n", h->C, h->NB, batch, (int)h3, (int)ok, best_ms[0], best_ms[1],
                        best_ms[2], best_ms[3], best_ms[4], choice);
            (void)hipEventDestroy(e1);
        }
        (void)hipEventDestroy(e0);
    }
    (void)hipGetLastError();
    h->prof_on = prof;
    cache[key] = choice;
    return choice;
}

int32_t forward_eval(azg_pv* h, const EvalCall& c, hipStream_t st, const EvalOpts& o)
{
    const int C = h->C;
    const float* P = h->params;
    // split-fp16 residual convs (EVAL_ARITH, C = 128 / 256): every path of the forward -- tower,
    // per-layer, the autotuner's candidates, a recompute -- then computes the same arithmetic
    TowerPlan p;
    p.recompute = o.per_layer;
    // a handle in AZG_PV_EVAL_FP16 (checked by the setter: C = 128, 1..32 blocks): the board16
    // tower with one product, whatever keys 5, 6 and 19 say; a recompute takes the launch's own
    const int prec = o.precision >= 0 ? o.precision : h->eval_precision;
    p.fp16 = prec == AZG_PV_EVAL_FP16 && !o.fp32_only;
    p.h3 = p.fp16 || (g_tower_h3 != 0 && !o.fp32_only && (C == 128 || C == 256) && h->NB > 0);
    if (p.h3)
        if (int32_t r = ensure_h3(h, st, p.fp16)) return r;
    // EVAL_ARITH = 2 at C = 128: the 16x16x32 board tower is the one form of its arithmetic, for
    // every batch and path.  One workgroup per board it waits on no other workgroup; its split
    // form (small batches, a launch's last partial round) exchanges boundary rows and does.
    const bool k32 = p.fp16 || (p.h3 && g_tower_h3 == 2 && C == 128 && h->NB <= kTowerMaxBlocks);
    p.variant = k32 ? 14 : o.per_layer ? 0 : tower_variant(h, c, st, p.h3);
    // an open breaker keeps the forward off every cross-workgroup wait: per-layer convs, or
    // for the 16x16x32 board tower one workgroup per board.  breaker_launches counts the
    // forwards it changed: a board16 launch that would not have split runs as it always does
    if (p.variant != 0 && !o.per_layer && (!k32 || board16_would_split(c.images())) &&
        h->posted.breaker_open(now_s())) {
        if (k32)
            p.unsplit = true;
        else
            p.variant = 0;
        ++h->posted.breaker_launches;
    }
    // a tower or H3 launch gets a number and a record of its call (azg_pv_recover);
    // a recompute (per_layer) posts nothing
    p.seq = o.per_layer ? o.guard_seq : 0u;
    if ((p.variant != 0 || p.h3) && h->NB > 0 && h->posted.attached() && !o.per_layer)
        p.seq = h->posted.begin(c, p.h3, prec);
    if (!o.per_layer) h->posted.last_seq = p.seq;
    float* X = nullptr;
    h->b16_split = false;
    if (int32_t r = stem_and_tower(h, c, st, p, &X)) return r;
    const HeadProj hp = head_proj(h);
    const int pr = prof_begin(h, AZG_PROF_HEADS, st, c.images());
    AZG_TRY(launch_heads_fwd(C, X, hp.wpc, hp.wvc, hp.scale, hp.shift, h->wfc, P + h->poff[h->t_pfc_b],
                             P + h->poff[h->t_vfc1_b], P + h->poff[h->t_vfc2_w], P + h->poff[h->t_vfc2_b], h->hbuf,
                             c.probs, c.values, c.logits, c.images(), st, c.boards, c.priors,
                             p.variant == 14 && !h->b16_split, c.syms, c.symmode),
            "forward: heads");
    prof_end(h, pr, st);
    return 0;
}

// azg_pv_recover's body: if launch `seq` is posted, recompute it from its record.
int32_t recover_eval(azg_pv* h, uint32_t seq, int32_t* recovered, void* stream)
{
    *recovered = 0;
    PostedLaunches& pl = h->posted;
    const int posted = pl.posted(seq);
    const bool ovf = posted & 2, tmo = posted & 1;
    if (!ovf && !tmo) return 0;
    const PostedLaunches::LaunchRec* rec = pl.record(seq);
    if (!rec)
        return fail("azg_pv_recover: the posted launch is older than the launch record ring (recover it sooner)");
    const PostedLaunches::LaunchRec r = *rec;
    // per-layer convs from the same inputs into the same outputs: bitwise what the tower
    // computes when no wait times out; an H3 launch whose activations left fp16's range
    // is recomputed with fp32 MFMA.  A timed-out split-fp16 launch is recomputed split
    // under its own number, so a range overflow the stale-input tower could not see is
    // posted by the recompute and settled here with fp32 MFMA as well.
    // released before the recompute has succeeded (azg_pv_recover clears slots first)
    pl.release(seq);
    hipStream_t rst = (hipStream_t)stream;
    const bool guard = !ovf && r.h3;
    EvalOpts redo;
    redo.precision = r.precision;
    redo.per_layer = true;
    redo.fp32_only = ovf;
    redo.guard_seq = guard ? seq : 0u;
    if (int32_t e = forward_eval(h, r.call, rst, redo)) return e;
    bool late_ovf = false;
    if (guard) {
        AZG_TRY(hipStreamSynchronize(rst), "azg_pv_recover: sync");
        late_ovf = pl.posted(seq) & 2;
        if (late_ovf) {
            pl.release_overflow(seq);
            redo.fp32_only = true;
            redo.guard_seq = 0u;
            if (int32_t e = forward_eval(h, r.call, rst, redo)) return e;
        }
    }
    if (late_ovf) ++pl.h3_overflows;
    if (ovf) ++pl.h3_overflows;
    if (!tmo) {   // a range overflow alone: no breaker (the dispatch ran as one)
        *recovered = 1;
        return 0;
    }
    ++pl.recovered;
    *recovered = 1;
    pl.trip(now_s(), g_tower_breaker_s);
    return 0;
}

}  // namespace azg
