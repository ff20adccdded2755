// Host AddressSanitizer driver of the policy/value C-ABI's host side
// (include/azg_pv.h, csrc/pv_capi.hip and csrc/pv_eval.hip built with -Xarch_host
// -fsanitize=address):
// handle lifecycle, flat-buffer layout for every supported shape, the status and
// tuning entry points, and every argument-error path.  No kernel runs (the driver
// also works without a GPU: device work is only reached after azg_pv_bind).
#include "../../../include/azg_pv.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++fails;                                                                      \
        }                                                                                 \
    } while (0)

int main()
{
    CHECK(azg_pv_abi_version() == 3);
    const int shapes[4][2] = {{3, 64}, {6, 128}, {10, 256}, {0, 64}};
    const long long want[3] = {340010, 1892650, 11930922};
    for (int s = 0; s < 4; ++s) {
        azg_pv_config cfg{shapes[s][0], shapes[s][1], 15, 3};
        azg_pv* h = nullptr;
        CHECK(azg_pv_create(&cfg, &h) == 0 && h);
        const int64_t n = azg_pv_param_count(h);
        if (s < 3) CHECK(n == want[s]);
        CHECK(azg_pv_grad_count(h) == n + 1);   // + the step's skip word (ABI 3)
        const int nt = azg_pv_num_param_tensors(h);
        std::vector<int64_t> off(nt), num(nt);
        CHECK(azg_pv_param_layout(h, off.data(), num.data()) == 0);
        int64_t o = 0;
        for (int i = 0; i < nt; ++i) {
            CHECK(off[i] == o);
            o += num[i];
        }
        CHECK(o == n);
        CHECK(azg_pv_bn_count(h) > 0 && azg_pv_num_bn_layers(h) == 2 * shapes[s][0] + 3);
        CHECK(azg_pv_status(h) == 0);
        CHECK(azg_pv_train_status(h) == 0);
        CHECK(azg_pv_clear_status(h) == 0);
        CHECK(azg_pv_mark_dirty(h) == 0);
        // tower recovery / wait record before any launch: nothing posted, nothing to do
        CHECK(azg_pv_last_seq(h) == 0);
        CHECK(azg_pv_posted(h, 0) == 0 && azg_pv_posted(h, 7) == 0);
        CHECK(azg_pv_train_fp32_once(h) == 0);
        int32_t rec = -1;
        CHECK(azg_pv_recover(h, 0, &rec, nullptr) == 0 && rec == 0);
        CHECK(azg_pv_recover(h, 7, &rec, nullptr) == 0 && rec == 0);
        CHECK(azg_pv_recover(h, 7, nullptr, nullptr) != 0);
        azg_pv_tower_diag d;
        std::memset(&d, 0xff, sizeof(d));
        CHECK(azg_pv_tower_diag_read(h, &d, nullptr) == 0 && d.timeouts == 0 && d.recovered == 0);
        CHECK(azg_pv_tower_diag_read(h, nullptr, nullptr) != 0);
        CHECK(azg_pv_tower_diag_clear(h, nullptr) == 0);
        // not bound yet: every compute entry point must fail cleanly
        float dummy = 0.f;
        CHECK(azg_pv_forward(h, &dummy, 1, &dummy, &dummy, nullptr, nullptr) != 0);
        CHECK(std::strlen(azg_pv_last_error()) > 0);
        CHECK(azg_pv_forward_boards(h, nullptr, nullptr, 1, &dummy, &dummy, nullptr, nullptr) != 0);
        {   // the symmetric board forward: argument errors first, then "not bound"
            int8_t i8 = 0;
            const auto names_it = [] { return std::strstr(azg_pv_last_error(), "azg_pv_forward_boards_sym") != nullptr; };
            CHECK(azg_pv_forward_boards_sym(nullptr, &i8, &i8, &i8, 0, 1, &dummy, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, &i8, 2, 1, &dummy, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, &i8, -1, 1, &dummy, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(std::strstr(azg_pv_last_error(), "mode") != nullptr);
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, nullptr, 1, 2049, &dummy, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(std::strstr(azg_pv_last_error(), "2048") != nullptr);
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, &i8, 0, -1, &dummy, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(azg_pv_forward_boards_sym(h, nullptr, &i8, &i8, 0, 1, &dummy, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(azg_pv_forward_boards_sym(h, &i8, nullptr, &i8, 0, 1, &dummy, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, &i8, 0, 1, nullptr, &dummy, &dummy, nullptr) != 0 && names_it());
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, &i8, 1, 1, &dummy, nullptr, &dummy, nullptr) != 0 && names_it());
            CHECK(std::strstr(azg_pv_last_error(), "null") != nullptr);
            // valid arguments (syms and priors are optional) on the unbound handle
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, nullptr, 0, 1, &dummy, &dummy, nullptr, nullptr) != 0 && names_it());
            CHECK(std::strstr(azg_pv_last_error(), "not bound") != nullptr);
            CHECK(azg_pv_forward_boards_sym(h, &i8, &i8, &i8, 1, 2048, &dummy, &dummy, &dummy, nullptr) != 0);
            CHECK(std::strstr(azg_pv_last_error(), "not bound") != nullptr);
        }
        {   // azg_pv_set_eval_precision / azg_pv_get_eval_precision: checked before any device call
            const bool ok16 = shapes[s][1] == 128 && shapes[s][0] >= 1;   // fp16: C = 128, 1..32 blocks
            CHECK(azg_pv_get_eval_precision(h) == AZG_PV_EVAL_EXACT);
            CHECK(azg_pv_set_eval_precision(h, 2) != 0 && azg_pv_set_eval_precision(h, -1) != 0);
            CHECK(std::strstr(azg_pv_last_error(), "azg_pv_set_eval_precision") != nullptr);
            CHECK(azg_pv_get_eval_precision(h) == AZG_PV_EVAL_EXACT);
            CHECK((azg_pv_set_eval_precision(h, AZG_PV_EVAL_FP16) == 0) == ok16);
            if (!ok16) CHECK(std::strstr(azg_pv_last_error(), "128") != nullptr);
            CHECK(azg_pv_get_eval_precision(h) == (ok16 ? AZG_PV_EVAL_FP16 : AZG_PV_EVAL_EXACT));
            // the forwards' argument checks do not depend on the precision (the handle is unbound)
            CHECK(azg_pv_forward(h, &dummy, 1, &dummy, &dummy, nullptr, nullptr) != 0);
            CHECK(azg_pv_set_eval_precision(h, AZG_PV_EVAL_EXACT) == 0);
            CHECK(azg_pv_get_eval_precision(h) == AZG_PV_EVAL_EXACT);
        }
        {   // azg_pv_bind_ema / azg_pv_get_ema: host state only, checked before any device call
            float ep = 0.f, eb = 0.f, *gp = &dummy, *gb = &dummy, gd = -1.f;
            const auto names_it = [] { return std::strstr(azg_pv_last_error(), "azg_pv_bind_ema") != nullptr; };
            const auto bound = [&](float* p, float* b, float d) {
                return azg_pv_get_ema(h, &gp, &gb, &gd) == (p ? 1 : 0) && gp == p && gb == b && gd == d;
            };
            CHECK(bound(nullptr, nullptr, 0.f));   // off by default
            CHECK(azg_pv_bind_ema(h, &ep, nullptr, 0.9f) != 0 && names_it());
            CHECK(azg_pv_bind_ema(h, nullptr, &eb, 0.9f) != 0 && names_it());
            CHECK(azg_pv_bind_ema(h, &ep, &eb, 1.f) != 0 && names_it());
            CHECK(std::strstr(azg_pv_last_error(), "decay") != nullptr);
            CHECK(azg_pv_bind_ema(h, &ep, &eb, -0.1f) != 0 && names_it());
            CHECK(azg_pv_bind_ema(h, &ep, &eb, std::nanf("")) != 0 && names_it());
            CHECK(bound(nullptr, nullptr, 0.f));   // refused calls change nothing
            CHECK(azg_pv_bind_ema(h, &ep, &eb, 0.999f) == 0 && bound(&ep, &eb, 0.999f));
            CHECK(azg_pv_bind_ema(h, &ep, nullptr, 0.5f) != 0 && azg_pv_bind_ema(h, &eb, &ep, 2.f) != 0);
            CHECK(bound(&ep, &eb, 0.999f));
            CHECK(azg_pv_bind_ema(h, nullptr, nullptr, std::nanf("")) == 0);   // unbind ignores decay
            CHECK(bound(nullptr, nullptr, 0.f));
            CHECK(azg_pv_bind_ema(h, &eb, &ep, 0.f) == 0 && bound(&eb, &ep, 0.f));   // bind -> unbind -> bind
            CHECK(azg_pv_get_ema(h, nullptr, nullptr, nullptr) == 1);
            CHECK(azg_pv_bind_ema(h, nullptr, nullptr, 0.f) == 0 && azg_pv_get_ema(h, nullptr, nullptr, nullptr) == 0);
        }
        CHECK(azg_pv_train_backward(h, &dummy, &dummy, &dummy, 4, &dummy, nullptr) != 0);
        // the weighted step: the batch and the pointers are checked before the binding, on an unbound handle
        CHECK(azg_pv_train_backward_weighted(h, &dummy, &dummy, &dummy, &dummy, nullptr, 1, &dummy, nullptr) != 0);
        CHECK(std::strstr(azg_pv_last_error(), "batch") != nullptr);
        CHECK(azg_pv_train_backward_weighted(h, &dummy, &dummy, nullptr, nullptr, nullptr, 4, &dummy, nullptr) != 0);
        CHECK(azg_pv_train_backward_weighted(h, &dummy, &dummy, &dummy, nullptr, nullptr, 4, &dummy, nullptr) != 0);
        CHECK(std::strstr(azg_pv_last_error(), "not bound") != nullptr);
        CHECK(azg_pv_train_apply(h, &dummy, &dummy, 1, 1e-3f, 0.9f, 0.999f, 1e-8f, 1e-4f, 3.f, nullptr, nullptr) != 0);
        CHECK(azg_pv_destroy(h) == 0);
    }
    // invalid configurations
    azg_pv* h = nullptr;
    azg_pv_config bad1{6, 96, 15, 3}, bad2{6, 128, 19, 3}, bad3{6, 128, 15, 4}, bad4{-1, 64, 15, 3};
    CHECK(azg_pv_create(&bad1, &h) != 0 && h == nullptr);
    CHECK(azg_pv_create(&bad2, &h) != 0);
    CHECK(azg_pv_create(&bad3, &h) != 0);
    CHECK(azg_pv_create(&bad4, &h) != 0);
    CHECK(azg_pv_create(nullptr, &h) != 0);
    CHECK(azg_pv_destroy(nullptr) == 0);
    CHECK(azg_pv_param_count(nullptr) == -1);
    CHECK(azg_pv_status(nullptr) == 0);
    CHECK(azg_pv_train_status(nullptr) == 0);
    CHECK(azg_pv_posted(nullptr, 3) == 0);
    CHECK(azg_pv_grad_count(nullptr) == -1);
    CHECK(azg_pv_train_fp32_once(nullptr) != 0);
    CHECK(azg_pv_train_backward_weighted(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 4, nullptr, nullptr) != 0);
    CHECK(azg_pv_last_seq(nullptr) == 0);
    CHECK(azg_pv_set_eval_precision(nullptr, AZG_PV_EVAL_EXACT) != 0);
    CHECK(azg_pv_get_eval_precision(nullptr) == -1);
    CHECK(azg_pv_bind_ema(nullptr, nullptr, nullptr, 0.9f) != 0);
    CHECK(std::strstr(azg_pv_last_error(), "azg_pv_bind_ema: null handle") != nullptr);
    CHECK(azg_pv_get_ema(nullptr, nullptr, nullptr, nullptr) == -1);
    CHECK(azg_pv_tower_diag_clear(nullptr, nullptr) != 0);
    CHECK(azg_pv_bind(nullptr, nullptr, nullptr, nullptr) != 0);
    // replay gather: every argument is checked before any device call
    {
        int8_t st = 0;
        float f = 0.f;
        int64_t id = 0;
        CHECK(azg_pv_replay_gather(nullptr, &f, &f, 4, 0, 2, 8, &id, 1, &f, &f, &f, nullptr) != 0);
        CHECK(std::strlen(azg_pv_last_error()) > 0);
        CHECK(azg_pv_replay_gather(&st, &f, &f, 4, 0, 2, 3, &id, 1, &f, &f, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather(&st, &f, &f, 4, 0, 2, 8, &id, 0, &f, &f, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather(&st, &f, &f, 0, 0, 1, 8, &id, 1, &f, &f, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather(&st, &f, &f, 4, 0, 5, 8, &id, 1, &f, &f, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather(&st, &f, &f, 4, 4, 2, 8, &id, 1, &f, &f, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather(&st, &f, &f, 4, 0, 2, 8, nullptr, 1, &f, &f, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather_weight(nullptr, 4, 0, 2, 8, &id, 1, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather_weight(&f, 4, 0, 2, 8, &id, 1, nullptr, nullptr) != 0);
        CHECK(azg_pv_replay_gather_weight(&f, 4, 0, 2, 3, &id, 1, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather_weight(&f, 4, 4, 2, 8, &id, 1, &f, nullptr) != 0);
        CHECK(azg_pv_replay_gather_weight(&f, 4, 0, 5, 8, &id, 0, &f, nullptr) != 0);
    }
    // weighted replay sampling: likewise
    {
        float f = 0.f;
        uint32_t w = 0;
        uint64_t u = 0;
        int64_t id = 0;
        CHECK(azg_pv_replay_surprise_weights(nullptr, 1, 1, 1, 0.5, &w, 4, 0, nullptr) != 0);
        CHECK(std::strstr(azg_pv_last_error(), "azg_pv_replay_surprise_weights") != nullptr);
        CHECK(azg_pv_replay_surprise_weights(&f, 1, 1, 1, 1.5, &w, 4, 0, nullptr) != 0);
        CHECK(azg_pv_replay_surprise_weights(&f, 0, 1, 1, 0.5, &w, 4, 0, nullptr) != 0);
        CHECK(azg_pv_replay_surprise_weights(&f, 1, 5, 5, 0.5, &w, 4, 0, nullptr) != 0);
        CHECK(azg_pv_replay_surprise_weights(&f, 1, 2, 1, 0.5, &w, 4, 0, nullptr) != 0);
        CHECK(azg_pv_replay_surprise_weights(&f, 1, 1, 1, 0.5, &w, 4, 4, nullptr) != 0);
        CHECK(azg_pv_replay_prefix(nullptr, 4, 0, 2, &u, nullptr) != 0);
        CHECK(std::strstr(azg_pv_last_error(), "azg_pv_replay_prefix") != nullptr);
        CHECK(azg_pv_replay_prefix(&w, 4, 0, 5, &u, nullptr) != 0);
        CHECK(azg_pv_replay_prefix(&w, 4, 4, 2, &u, nullptr) != 0);
        CHECK(azg_pv_replay_draw(&u, 2, 8, nullptr, 1, &id, nullptr) != 0);
        CHECK(std::strstr(azg_pv_last_error(), "azg_pv_replay_draw") != nullptr);
        CHECK(azg_pv_replay_draw(&u, 0, 8, &u, 1, &id, nullptr) != 0);
        CHECK(azg_pv_replay_draw(&u, 2, 3, &u, 1, &id, nullptr) != 0);
        CHECK(azg_pv_replay_draw(&u, 2, 8, &u, 0, &id, nullptr) != 0);
    }
    // tuning keys round-trip (previous value returned)
    const int prev = azg_pv_set_tuning(AZG_PV_TUNE_TOWER_MODE, 0);
    CHECK(azg_pv_set_tuning(AZG_PV_TUNE_TOWER_MODE, prev) == 0);
    CHECK(azg_pv_set_tuning(999, 1) == -1);
    const int prev_wait = azg_pv_set_tuning(AZG_PV_TUNE_TOWER_WAIT_US, 0);   // wait bound (us): default 100 ms
    CHECK(prev_wait == 100000);
    CHECK(azg_pv_set_tuning(AZG_PV_TUNE_TOWER_WAIT_US, -1) == 0);
    CHECK(azg_pv_set_tuning(AZG_PV_TUNE_TOWER_WAIT_US, -1) == 100000);
    const int prev_breaker = azg_pv_set_tuning(AZG_PV_TUNE_BREAKER_SECONDS, 0);   // breaker seconds: default 30
    CHECK(prev_breaker == 30 && azg_pv_set_tuning(AZG_PV_TUNE_BREAKER_SECONDS, prev_breaker) == 0);
    std::printf("asan_pv: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
