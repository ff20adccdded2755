// C-ABI of the policy/value engine (include/azg_pv.h): the entry points and their argument
// checks, handle lifecycle, flat-buffer layout and bind, the status, profile and diag readers.
// How a forward runs is pv_eval.hip; the status words' protocol is pv_posted.h.
// Compiled by hipcc for gfx950 together with the kernel translation units.
#include "../../include/azg_pv.h"
#include "pv_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace azg;

static thread_local std::string g_err;

static int32_t fail(const char* what, hipError_t e = hipSuccess)
{
    g_err = what;
    if (e != hipSuccess) {
        g_err += ": ";
        g_err += hipGetErrorString(e);
    }
    return 1;
}

extern "C" {

int32_t azg_pv_abi_version(void) { return 3; }

const char* azg_pv_last_error(void) { return g_err.c_str(); }

int32_t azg_pv_create(const azg_pv_config* cfg, azg_pv** out)
{
    if (!cfg || !out) return fail("azg_pv_create: null argument");
    *out = nullptr;
    if (cfg->board != BOARD) return fail("azg_pv_create: only board=15 is built");
    if (cfg->in_ch != 3) return fail("azg_pv_create: in_ch must be 3 (games/gomoku.py:146-150)");
    if (cfg->channels != 64 && cfg->channels != 128 && cfg->channels != 256)
        return fail("azg_pv_create: channels must be 64, 128 or 256");
    if (cfg->blocks < 0 || cfg->blocks > 64) return fail("azg_pv_create: blocks out of range");
    azg_pv* h = new (std::nothrow) azg_pv();
    if (!h) return fail("azg_pv_create: out of host memory");
    h->cfg = *cfg;
    h->C = cfg->channels;
    h->NB = cfg->blocks;
    build_layout(h);
    *out = h;
    return 0;
}

int32_t azg_pv_destroy(azg_pv* h)
{
    if (!h) return 0;
    if (h->wbase) (void)hipDeviceSynchronize();
    free_workspace(h);
    for (void* p : h->dev_allocs) (void)hipFree(p);
    if (h->posted.attached()) (void)hipHostFree(h->posted.host_words());
    for (auto& e : h->prof_ev) (void)hipEventDestroy(e);
    delete h;
    return 0;
}

int64_t azg_pv_param_count(const azg_pv* h) { return h ? h->nparams : -1; }
int64_t azg_pv_bn_count(const azg_pv* h) { return h ? h->nbn : -1; }
int32_t azg_pv_num_param_tensors(const azg_pv* h) { return h ? (int32_t)h->poff.size() : -1; }

int32_t azg_pv_param_layout(const azg_pv* h, int64_t* offsets, int64_t* numels)
{
    if (!h || !offsets || !numels) return fail("azg_pv_param_layout: null argument");
    for (size_t i = 0; i < h->poff.size(); ++i) {
        offsets[i] = h->poff[i];
        numels[i] = h->pnum[i];
    }
    return 0;
}

int32_t azg_pv_bind(azg_pv* h, float* params, float* grads, float* bn_stats)
{
    if (!h || !params || !bn_stats) return fail("azg_pv_bind: null handle/params/bn_stats");
    if (!h->wbase) {   // device workspace is allocated at first bind (create is host-only)
        const int C = h->C;
        size_t floats = 0;
        floats += (size_t)2 * h->NB * 9 * C * C;   // wpack
        floats += (size_t)27 * C;                  // wstem
        floats += (size_t)FC_OUT * FC_KP;          // wfc
        floats += (size_t)h->nfold * 2;            // scale, shift
        float* base = nullptr;
        hipError_t e = handle_malloc(h, &base, floats * sizeof(float));
        if (e != hipSuccess) return fail("azg_pv_bind: hipMalloc(packed weights)", e);
        h->wbase = base;
        h->wpack = base; base += (size_t)2 * h->NB * 9 * C * C;
        h->wstem = base; base += (size_t)27 * C;
        h->wfc = base; base += (size_t)FC_OUT * FC_KP;
        h->scale = base; base += h->nfold;
        h->shift = base; base += h->nfold;
        e = handle_malloc(h, &h->bn_desc_dev, sizeof(BnDesc) * h->bn_desc.size());
        if (e == hipSuccess)
            e = hipMemcpy(h->bn_desc_dev, h->bn_desc.data(), sizeof(BnDesc) * h->bn_desc.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail("azg_pv_bind: bn descriptor upload", e);
        std::vector<int64_t> offs(2 * h->NB > 0 ? 2 * h->NB : 1, 0);
        for (int i = 0; i < h->NB; ++i) {
            offs[2 * i] = h->poff[h->t_blk[i].w1];
            offs[2 * i + 1] = h->poff[h->t_blk[i].w2];
        }
        e = handle_malloc(h, &h->conv_off_dev, sizeof(int64_t) * offs.size());
        if (e == hipSuccess)
            e = hipMemcpy(h->conv_off_dev, offs.data(), sizeof(int64_t) * offs.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail("azg_pv_bind: conv offset upload", e);
        void* sp = nullptr;
        // two rings in one pinned, mapped allocation: timed-out tower launches, H3 overflows
        // (+ the train forward's overflow flags)
        e = hipHostMalloc(&sp, kStatusWords * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) return fail("azg_pv_bind: hipHostMalloc(tower ring)", e);
        void* dp = nullptr;
        e = hipHostGetDevicePointer(&dp, sp, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(sp);
            return fail("azg_pv_bind: hipHostGetDevicePointer(tower ring)", e);
        }
        h->posted.attach((unsigned*)sp, (unsigned*)dp);
        e = handle_malloc(h, &h->tower_diag, kTowerDiagWords * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemset(h->tower_diag, 0, kTowerDiagWords * sizeof(unsigned));
        if (e != hipSuccess) return fail("azg_pv_bind: tower wait record", e);
    }
    h->params = params;
    h->grads = grads;
    h->bn = bn_stats;
    h->dirty = true;
    h->train_packs = false;
    h->bn_bak_ok = false;
    return 0;
}

int32_t azg_pv_bind_counters(azg_pv* h, int64_t* num_batches_tracked)
{
    if (!h) return fail("azg_pv_bind_counters: null handle");
    h->nbt = num_batches_tracked;
    h->bn_bak_ok = false;
    return 0;
}

int32_t azg_pv_bind_ema(azg_pv* h, float* ema_params, float* ema_bn, float decay)
{
    // host state only: no device call, before or after azg_pv_bind
    if (!h) return fail("azg_pv_bind_ema: null handle");
    if (!ema_params != !ema_bn)
        return fail("azg_pv_bind_ema: ema_params and ema_bn must both be set (bind) or both be null (unbind)");
    if (!ema_params) {   // unbind: decay is ignored
        h->ema_params = h->ema_bn = nullptr;
        h->ema_decay = 0.f;
        return 0;
    }
    if (!(decay >= 0.f && decay < 1.f)) return fail("azg_pv_bind_ema: decay must be in [0, 1)");   // NaN fails too
    h->ema_params = ema_params;
    h->ema_bn = ema_bn;
    h->ema_decay = decay;
    return 0;
}

int32_t azg_pv_get_ema(const azg_pv* h, float** ema_params, float** ema_bn, float* decay)
{
    if (!h) return -1;
    if (ema_params) *ema_params = h->ema_params;
    if (ema_bn) *ema_bn = h->ema_bn;
    if (decay) *decay = h->ema_decay;
    return h->ema_params ? 1 : 0;
}

int32_t azg_pv_num_bn_layers(const azg_pv* h) { return h ? (int32_t)h->bn_desc.size() : -1; }

int32_t azg_pv_mark_dirty(azg_pv* h)
{
    if (!h) return fail("azg_pv_mark_dirty: null handle");
    h->dirty = true;
    h->train_packs = false;
    h->bn_bak_ok = false;
    return 0;
}

int32_t azg_pv_forward(azg_pv* h, const float* x, int32_t batch, float* probs, float* values,
                       float* logits, void* stream)
{
    if (!h || !h->params) return fail("azg_pv_forward: handle not bound (azg_pv_bind)");
    if (batch < 0) return fail("azg_pv_forward: negative batch");
    if (batch == 0) return 0;            // empty batch: nothing to do (empty tensors have null data)
    if (!x || !probs || !values) return fail("azg_pv_forward: null x/probs/values");
    EvalCall c;
    c.x = x;
    c.batch = batch;
    c.probs = probs;
    c.values = values;
    c.logits = logits;
    return run_eval(h, c, stream);
}

int32_t azg_pv_forward_boards(azg_pv* h, const int8_t* boards, const int8_t* players, int32_t batch, float* probs,
                              float* values, float* priors, void* stream)
{
    if (!h || !h->params) return fail("azg_pv_forward_boards: handle not bound (azg_pv_bind)");
    if (h->cfg.board != BOARD || h->cfg.in_ch != 3) return fail("azg_pv_forward_boards: needs a 15x15, 3-plane net");
    if (batch < 0) return fail("azg_pv_forward_boards: negative batch");
    if (batch == 0) return 0;
    if (!boards || !players || !probs || !values) return fail("azg_pv_forward_boards: null boards/players/probs/values");
    EvalCall c;
    c.boards = boards;
    c.players = players;
    c.batch = batch;
    c.probs = probs;
    c.values = values;
    c.priors = priors;
    return run_eval(h, c, stream);
}

int32_t azg_pv_forward_boards_sym(azg_pv* h, const int8_t* boards, const int8_t* players, const int8_t* syms,
                                  int32_t mode, int32_t batch, float* probs, float* values, float* priors,
                                  void* stream)
{
    // argument checks first: before the bound check and before any device call
    if (!h) return fail("azg_pv_forward_boards_sym: null handle");
    if (mode != 0 && mode != 1) return fail("azg_pv_forward_boards_sym: mode must be 0 (per-board syms) or 1 (mean of 8)");
    if (batch < 0) return fail("azg_pv_forward_boards_sym: negative batch");
    if (mode == 1 && batch > 2048)
        return fail("azg_pv_forward_boards_sym: mode 1 takes at most 2048 boards per call (8 images each)");
    if (batch > 0 && (!boards || !players || !probs || !values))
        return fail("azg_pv_forward_boards_sym: null boards/players/probs/values");
    if (!h->params) return fail("azg_pv_forward_boards_sym: handle not bound (azg_pv_bind)");
    if (h->cfg.board != BOARD || h->cfg.in_ch != 3)
        return fail("azg_pv_forward_boards_sym: needs a 15x15, 3-plane net");
    if (batch == 0) return 0;
    EvalCall c;
    c.boards = boards;
    c.players = players;
    c.symmode = mode == 1 ? SYM_MEAN8 : syms ? SYM_EACH : SYM_NONE;   // no syms: the plain forward
    c.syms = c.symmode == SYM_EACH ? syms : nullptr;
    c.batch = batch;
    c.probs = probs;
    c.values = values;
    c.priors = priors;
    return run_eval(h, c, stream);
}

int32_t azg_pv_set_eval_precision(azg_pv* h, int32_t precision)
{
    if (!h) return fail("azg_pv_set_eval_precision: null handle");
    if (precision != AZG_PV_EVAL_EXACT && precision != AZG_PV_EVAL_FP16)
        return fail("azg_pv_set_eval_precision: unknown precision (0 = exact, 1 = fp16)");
    if (precision == AZG_PV_EVAL_FP16 && (h->C != 128 || h->NB <= 0 || h->NB > kTowerMaxBlocks))
        return fail("azg_pv_set_eval_precision: fp16 needs channels == 128 and 1..32 residual blocks "
                    "(channels 256 and 64 have no one-product tower)");
    h->eval_precision = precision;
    return 0;
}

int32_t azg_pv_get_eval_precision(const azg_pv* h) { return h ? h->eval_precision : -1; }

int32_t azg_pv_profile_enable(azg_pv* h, int32_t enable)
{
    if (!h) return fail("azg_pv_profile_enable: null handle");
    if (enable && h->prof_ev.empty()) {
        h->prof_ev.resize(2 * 8192);
        for (auto& e : h->prof_ev) AZG_TRY(hipEventCreate(&e), "azg_pv_profile_enable: hipEventCreate");
        h->prof_cls.assign(8192, 0);
    }
    if (enable) AZG_TRY(hipDeviceSynchronize(), "azg_pv_profile_enable: sync");
    h->prof_on = enable != 0;
    h->prof_used = 0;
    for (int i = 0; i < AZG_PROF_NCLASS; ++i) { h->prof_ms[i] = 0.0; h->prof_n[i] = 0; h->prof_work[i] = 0; }
    return 0;
}

int32_t azg_pv_profile_read(azg_pv* h, double* ms, int64_t* launches)
{
    if (!h || !ms || !launches) return fail("azg_pv_profile_read: null argument");
    if (hipError_t e = prof_harvest(h)) return fail("azg_pv_profile_read: event sync/elapsed", e);
    for (int i = 0; i < AZG_PROF_NCLASS; ++i) { ms[i] = h->prof_ms[i]; launches[i] = h->prof_n[i]; }
    return 0;
}

int32_t azg_pv_profile_boards(const azg_pv* h, int64_t* boards)
{
    if (!h || !boards) return fail("azg_pv_profile_boards: null argument");
    for (int i = 0; i < AZG_PROF_NCLASS; ++i) boards[i] = h->prof_work[i];
    return 0;
}

// posted eval launches not yet recovered: timed-out tower launches and split-fp16 launches
// whose activations left fp16's range (their outputs are invalid until recomputed)
int32_t azg_pv_status(const azg_pv* h) { return h ? h->posted.count() : 0; }

int32_t azg_pv_posted(const azg_pv* h, uint32_t seq) { return h ? h->posted.posted(seq) : 0; }

int32_t azg_pv_train_status(const azg_pv* h) { return h ? (int32_t)h->posted.train_skips() : 0; }

int64_t azg_pv_grad_count(const azg_pv* h) { return h ? h->nparams + 1 : -1; }

int32_t azg_pv_train_fp32_once(azg_pv* h)
{
    if (!h) return fail("azg_pv_train_fp32_once: null handle");
    h->train_fp32_once = true;
    return 0;
}

int32_t azg_pv_clear_status(azg_pv* h)
{
    if (!h) return fail("azg_pv_clear_status: null handle");
    h->posted.clear();
    return 0;
}

int32_t azg_pv_tower_status(azg_pv* h, void* stream)
{
    if (!h) return fail("azg_pv_tower_status: null handle");
    if (!h->tower_sync) return 0;
    unsigned w[2] = {0, 0};
    hipStream_t st = (hipStream_t)stream;
    AZG_TRY(hipMemcpyAsync(w, h->tower_sync, sizeof(w), hipMemcpyDeviceToHost, st), "azg_pv_tower_status: copy");
    AZG_TRY(hipStreamSynchronize(st), "azg_pv_tower_status: sync");
    return (int32_t)w[1];
}

uint32_t azg_pv_last_seq(const azg_pv* h) { return h ? h->posted.last_seq : 0u; }

int32_t azg_pv_recover(azg_pv* h, uint32_t seq, int32_t* recovered, void* stream)
{
    if (!h || !recovered) return fail("azg_pv_recover: null argument");
    return recover_eval(h, seq, recovered, stream);
}

int32_t azg_pv_tower_diag_read(azg_pv* h, azg_pv_tower_diag* out, void* stream)
{
    if (!h || !out) return fail("azg_pv_tower_diag_read: null argument");
    memset(out, 0, sizeof(*out));
    out->recovered = h->posted.recovered;
    out->breaker_trips = h->posted.breaker_trips;
    out->breaker_launches = h->posted.breaker_launches;
    out->h3_overflows = h->posted.h3_overflows;
    out->train_h3_overflows = h->posted.train_skips();
    if (!h->tower_diag) return 0;
    unsigned w[kTowerDiagWords];
    hipStream_t st = (hipStream_t)stream;
    AZG_TRY(hipMemcpyAsync(w, h->tower_diag, sizeof(w), hipMemcpyDeviceToHost, st), "azg_pv_tower_diag_read: copy");
    AZG_TRY(hipStreamSynchronize(st), "azg_pv_tower_diag_read: sync");
    auto us = [](unsigned ticks) { return ticks / 100u; };   // s_memrealtime: 100 MHz
    out->timeouts = w[1];
    out->waits_over_100us = w[2];
    out->waits_over_1ms = w[3];
    out->waits_over_10ms = w[4];
    out->waits_over_100ms = w[5];
    out->max_wait_us = us(w[6]);
    out->seq = w[7];
    out->layer = w[8];
    out->mtile = w[9];
    out->wait_mtile = w[10];
    out->observed = w[11];
    out->needed = w[12];
    out->waited_us = us(w[13]);
    out->wall_us = us(w[14]);
    out->waiter_hwid = w[15];
    out->waiter_xcc = w[16];
    out->claims = w[17];
    out->producer_claimed = w[18];
    out->producer_started = w[19];
    out->producer_hwid = w[20];
    out->producer_xcc = w[21];
    out->producer_start_us = (int32_t)w[22] / 100;
    out->max_wall_us = us(w[23]);
    out->waits_suspended = w[24];
    return 0;
}

int32_t azg_pv_tower_diag_clear(azg_pv* h, void* stream)
{
    if (!h) return fail("azg_pv_tower_diag_clear: null handle");
    h->posted.reset_counters();
    if (!h->tower_diag) return 0;
    hipStream_t st = (hipStream_t)stream;
    AZG_TRY(hipMemsetAsync(h->tower_diag, 0, kTowerDiagWords * sizeof(unsigned), st), "azg_pv_tower_diag_clear");
    AZG_TRY(hipStreamSynchronize(st), "azg_pv_tower_diag_clear: sync");
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------

namespace azg {

int32_t set_error(const char* what, hipError_t e) { return fail(what, e); }
}  // namespace azg

namespace azg {

void build_layout(azg_pv* h)
{
    const int C = h->C, NB = h->NB;
    h->poff.clear();
    h->pnum.clear();
    int64_t off = 0;
    auto add = [&](int64_t n) { h->poff.push_back(off); h->pnum.push_back(n); off += n; return (int)h->poff.size() - 1; };
    // nn.Module.parameters() order of network.py:41-73
    h->t_stem_w = add((int64_t)C * 27);
    h->t_stem_g = add(C);
    h->t_stem_b = add(C);
    h->t_blk.assign(NB, {});
    for (int i = 0; i < NB; ++i) {
        h->t_blk[i].w1 = add((int64_t)C * C * 9);
        h->t_blk[i].g1 = add(C);
        h->t_blk[i].b1 = add(C);
        h->t_blk[i].w2 = add((int64_t)C * C * 9);
        h->t_blk[i].g2 = add(C);
        h->t_blk[i].b2 = add(C);
    }
    h->t_pc_w = add(2 * C);
    h->t_pbn_g = add(2);
    h->t_pbn_b = add(2);
    h->t_pfc_w = add((int64_t)ACTIONS * 2 * PIX);
    h->t_pfc_b = add(ACTIONS);
    h->t_vc_w = add(C);
    h->t_vbn_g = add(1);
    h->t_vbn_b = add(1);
    h->t_vfc1_w = add((int64_t)VHID * PIX);
    h->t_vfc1_b = add(VHID);
    h->t_vfc2_w = add(VHID);
    h->t_vfc2_b = add(1);
    h->nparams = off;

    // BN layers: stem, (bn1, bn2) per block, policy_bn, value_bn
    h->bn_desc.clear();
    int stat = 0, fold = 0;
    auto addbn = [&](int g, int b, int c) {
        BnDesc d{};
        d.gamma_off = (int)h->poff[g];
        d.beta_off = (int)h->poff[b];
        d.stat_off = stat;
        d.c = c;
        d.out_off = fold;
        h->bn_desc.push_back(d);
        stat += 2 * c;
        fold += c;
        return (int)h->bn_desc.size() - 1;
    };
    h->bn_stem = addbn(h->t_stem_g, h->t_stem_b, C);
    h->bn_blk.assign(NB, {});
    for (int i = 0; i < NB; ++i) {
        h->bn_blk[i].first = addbn(h->t_blk[i].g1, h->t_blk[i].b1, C);
        h->bn_blk[i].second = addbn(h->t_blk[i].g2, h->t_blk[i].b2, C);
    }
    h->bn_pol = addbn(h->t_pbn_g, h->t_pbn_b, 2);
    h->bn_val = addbn(h->t_vbn_g, h->t_vbn_b, 1);
    h->nbn = stat;
    h->nfold = fold;
    h->conv_bn_off.assign(NB > 0 ? 2 * NB : 1, 0);
    for (int i = 0; i < NB; ++i) {
        h->conv_bn_off[2 * i] = h->bn_desc[h->bn_blk[i].first].out_off;
        h->conv_bn_off[2 * i + 1] = h->bn_desc[h->bn_blk[i].second].out_off;
    }
}

}  // namespace azg
