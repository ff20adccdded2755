// azg_pv_set_tuning (include/azg_pv.h, enum azg_pv_tuning_key): the process-wide tuning
// variables of every translation unit, one table row per key.  Host code only.
#include "../../include/azg_pv.h"
#include "pv_internal.h"

using namespace azg;

namespace {

#ifdef AZG_AB_STUDIES
constexpr bool kStudy = true;
#else
constexpr bool kStudy = false;   // the product library: timing-study keys are read-only
#endif

// Rules: does the key accept this value (a rule may normalise it)?  A rejected value
// leaves the variable as it is; the call still returns the previous value.
bool any(int&) { return true; }
bool flag(int& v) { v = v ? 1 : 0; return true; }
bool zero_one(int& v) { return v == 0 || v == 1; }
bool upto2(int& v) { return v >= 0 && v <= 2; }
bool nonneg(int& v) { return v >= 0; }
bool tower_shape(int& v) { return v == 5 || v == 8 || v == 10 || (v >= 12 && v <= 14); }
bool conv_body(int& v) { return v == 0 || v == 1 || v == 4 || v == 5; }
bool wgrad_splits(int& v) { return v == 0 || (v >= 8 && v <= 64 && v % 8 == 0); }

struct Row {
    int key;
    int* var;
    bool (*rule)(int&);
    bool product;   // false: only a study build (AZG_AB_STUDIES) sets it
};

const Row kRows[] = {
    {AZG_PV_TUNE_CONV_SHAPE, &g_conv_shape_override, any, true},
    {AZG_PV_TUNE_CONV_AUTOTUNE, &g_conv_autotune, any, true},
    {AZG_PV_TUNE_TOWER_MODE, &g_tower_mode, any, true},
    {AZG_PV_TUNE_TOWER_SHAPE, &g_tower_shape, tower_shape, true},
    {AZG_PV_TUNE_TOWER_ABLATION, &g_tower_ablation, any, false},
    {AZG_PV_TUNE_STEM_KERNEL, &g_stem_variant, zero_one, true},
    {AZG_PV_TUNE_TOWER_CLAIM, &g_tower_group, zero_one, true},
    {AZG_PV_TUNE_BREAKER_SECONDS, &g_tower_breaker_s, nonneg, true},
    {AZG_PV_TUNE_EVAL_ARITH, &g_tower_h3, upto2, true},
    {AZG_PV_TUNE_H3_TOWER_BODY, &g_h3_tower_var, zero_one, true},
    {AZG_PV_TUNE_CONV_TAIL_SPLIT, &g_conv_tail_split, flag, true},
    {AZG_PV_TUNE_CONV_BODY, &g_conv_var, conv_body, true},
    {AZG_PV_TUNE_TRAIN_FUSE_APPLY, &g_train_fuse_apply, zero_one, true},
    {AZG_PV_TUNE_TRAIN_FUSE_FINALIZE, &g_train_fuse_fin, zero_one, true},
    {AZG_PV_TUNE_WGRAD_SPLITS, &g_wgrad_splits, wgrad_splits, true},
    {AZG_PV_TUNE_TRAIN_APPLY_GRID, &g_train_apply_grid, nonneg, true},
    {AZG_PV_TUNE_WGRAD_TILE, &g_wgrad_variant, zero_one, true},
    {AZG_PV_TUNE_TRAIN_ARITH, &g_train_h3, upto2, true},
    {AZG_PV_TUNE_TRAIN_DGRAD_ARITH, &g_train_dgrad_h3, upto2, true},
#ifdef AZG_AB_STUDIES   // the product library does not know the key (-1)
    {AZG_PV_TUNE_BOARD_ABLATION, &g_board_abl, any, true},
#endif
    {AZG_PV_TUNE_BOARD16_SPLIT_MAX, &g_board16_split, nonneg, true},
};

// Retired keys (finished conv-tile studies): they set nothing and return what the product
// library always returned for them.
const struct { int key, value; } kRetired[] = {
    {AZG_PV_TUNE_CONV_ABLATION, 0}, {AZG_PV_TUNE_CONV_STAGING, 1}, {AZG_PV_TUNE_ABLATION_SHAPE, 5},
    {AZG_PV_TUNE_TOWER_BODY, 0},    {AZG_PV_TUNE_STEM_ABLATION, 0}, {AZG_PV_TUNE_TOWER_SC1_LOADS, 0},
};

}  // namespace

extern "C" int32_t azg_pv_set_tuning(int32_t key, int32_t value)
{
    switch (key) {
        case AZG_PV_TUNE_QUERY_CONV_SHAPE:   // value = M * 1024 + C
            return conv_tuned_shape(value & 1023, value >> 10);
        case AZG_PV_TUNE_QUERY_STUDY_BUILD:
            return kStudy ? 1 : 0;
        case AZG_PV_TUNE_TOWER_WAIT_US: {   // unsigned; a negative value restores the default
            const int prev = (int)g_tower_wait_us;
            g_tower_wait_us = value < 0 ? kTowerWaitUs : (unsigned)value;
            return prev;
        }
    }
    for (const Row& r : kRows) {
        if (r.key != key) continue;
        const int prev = *r.var;
        int v = value;
        if ((r.product || kStudy) && r.rule(v)) *r.var = v;
        return prev;
    }
    for (const auto& r : kRetired)
        if (r.key == key) return r.value;
    return -1;
}
