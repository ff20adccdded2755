// Host AddressSanitizer / UBSan driver of the native search's value mode
// (AZG_MCTS_SEARCH_VALUE, include/azg_mcts.h; csrc/mcts_engine.cpp): games of Gomoku and
// Pente played through the C-ABI with a deterministic stand-in evaluator whose value is
// backed up -- collisions (early emits with a suspended simulation), final flushes, root
// noise on a root that already exists, tree reuse, azg_mcts_clear and a mode change after
// it, playout-cap budgets, multi-threaded advance, and every error path of the new entry
// points.  Built by `make -C csrc asan`.
#include "../../../include/azg_mcts.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static const int A = 225;

static void fake_eval(const int8_t* boards, const int8_t* players, int n, std::vector<float>& p,
                      std::vector<float>& v)
{
    p.assign((size_t)n * A, 0.f);
    v.assign(n, 0.f);
    for (int i = 0; i < n; ++i) {
        double s = 0, t = 0;
        for (int a = 0; a < A; ++a) {
            const int8_t b = boards[(size_t)i * A + a];
            const float x = b == 0 ? 1.f + 0.5f * std::sin(0.37f * a) : 0.f;
            p[(size_t)i * A + a] = x;
            s += x;
            t += b == players[i] ? std::cos(0.21f * a) : (b != 0 ? -std::cos(0.21f * a) : 0.0);
        }
        for (int a = 0; a < A; ++a) p[(size_t)i * A + a] = (float)(p[(size_t)i * A + a] / (s > 0 ? s : 1));
        v[i] = (float)std::tanh(0.3 * t);
    }
}

static azg_mcts_config config(int rules, int sims, int batch)
{
    azg_mcts_config cfg{};
    cfg.rules = rules;
    cfg.board = 15;
    cfg.n_simulations = sims;
    cfg.batch_size = batch;
    cfg.apply_dirichlet_n_first_moves = 6;
    cfg.add_dirichlet_noise = 1;
    cfg.cpuct = 1.2;
    cfg.dirichlet_alpha = 0.3;
    cfg.epsilon = 0.25;
    return cfg;
}

// answer every pending noise request; returns how many there were
static int mix_noise(azg_mcts* h, int games)
{
    int n = 0;
    std::vector<float> p32(A);
    for (int g = 0; g < games; ++g) {
        if (azg_mcts_noise_request(h, g, p32.data()) != 1) continue;
        std::vector<double> mix(A);
        double s = 0;
        for (int a = 0; a < A; ++a) s += (mix[a] = 0.75 * p32[a] + 0.25 / A);
        for (auto& m : mix) m /= s;
        CHECK(azg_mcts_set_root_prior(h, g, mix.data()) == 0);
        ++n;
    }
    return n;
}

static void play(int rules, int games, int sims, int batch, int threads, int max_moves)
{
    const azg_mcts_config cfg = config(rules, sims, batch);
    azg_mcts* h = nullptr;
    CHECK(azg_mcts_create(&cfg, games, &h) == 0 && h);
    CHECK(azg_mcts_get_search_mode(h) == AZG_MCTS_SEARCH_REFERENCE);
    CHECK(azg_mcts_set_search_mode(h, AZG_MCTS_SEARCH_VALUE) == 0);
    CHECK(azg_mcts_get_search_mode(h) == AZG_MCTS_SEARCH_VALUE);
    std::vector<std::vector<int8_t>> board(games, std::vector<int8_t>(A, 0));
    std::vector<int> player(games, 1), moves(games, 0), done(games, 0), budget(games, sims);
    std::vector<int> caps(2 * games, 0);
    std::vector<int64_t> before(games, 0);
    std::vector<int> existed(games, 0);
    for (int g = 0; g < games; ++g) CHECK(azg_mcts_set_root(h, g, board[g].data(), 1, -1, -1, 0, 0, 0) == 0);
    CHECK(mix_noise(h, games) == 0);   // no root exists yet
    std::vector<float> p, v, pi(A);
    std::vector<int8_t> lb((size_t)games * batch * A), lp((size_t)games * batch);
    std::vector<int32_t> counts(games), status(games);
    int live = games, rounds = 0, short_emits = 0, noisy_existing_roots = 0;
    while (live > 0 && rounds < 40000) {
        ++rounds;
        int32_t n = 0;
        CHECK(azg_mcts_advance_boards(h, lb.data(), lp.data(), counts.data(), status.data(), &n, threads) == 0);
        for (int g = 0; g < games; ++g) {
            if (status[g] == AZG_MCTS_NEED_EVAL) {
                CHECK(counts[g] >= 1 && counts[g] <= batch);
                if (counts[g] < batch) ++short_emits;   // a collision or a final flush
            }
            if (done[g] || status[g] != AZG_MCTS_DONE) continue;
            CHECK(azg_mcts_inflight(h, g) == 0);
            double q = 2;
            float vn = 2;
            int64_t visits = -1;
            CHECK(azg_mcts_get_root_value(h, g, &q, &vn, &visits) == 0);
            CHECK(q >= -1.0 && q <= 1.0 && vn >= -1.f && vn <= 1.f);
            CHECK(visits - before[g] == budget[g] - (existed[g] ? 0 : 1));
            CHECK(azg_mcts_get_root_value(h, g, nullptr, nullptr, nullptr) == 0);
            CHECK(azg_mcts_get_pi(h, g, pi.data()) == 0);
            int best = -1;
            for (int a = 0; a < A; ++a)
                if (board[g][a] == 0 && (best < 0 || pi[a] > pi[best])) best = a;
            CHECK(best >= 0);
            int8_t nb[A];
            int32_t cp[2], w = 0, over = 0;
            const int32_t act = best;
            CHECK(azg_mcts_replay(rules, 15, board[g].data(), player[g], caps[2 * g], caps[2 * g + 1], &act, 1, nb,
                                  cp, &w, &over) == 0);
            std::memcpy(board[g].data(), nb, A);
            caps[2 * g] = cp[0];
            caps[2 * g + 1] = cp[1];
            player[g] = 3 - player[g];
            ++moves[g];
            if (over || moves[g] >= max_moves) {
                done[g] = 1;
                --live;
                CHECK(azg_mcts_tree_size(h, g) > 0);
                CHECK(azg_mcts_set_search_mode(h, AZG_MCTS_SEARCH_REFERENCE) != 0);   // this tree is not empty
                CHECK(azg_mcts_clear(h, g) == 0);
                CHECK(azg_mcts_tree_size(h, g) == 0 && azg_mcts_inflight(h, g) == 0);
                CHECK(azg_mcts_collisions(h, g) == 0);
            } else {
                // playout cap: every third move at a small budget without noise
                const bool fast = moves[g] % 3 == 1;
                budget[g] = fast ? 5 : sims;
                CHECK(azg_mcts_set_budget(h, g, fast ? 5 : -1, fast ? 0 : -1) == 0);
                CHECK(azg_mcts_set_root(h, g, board[g].data(), player[g], best / 15, best % 15, caps[2 * g],
                                        caps[2 * g + 1], moves[g]) == 0);
                int64_t vis = 0;
                existed[g] = azg_mcts_get_root_value(h, g, nullptr, nullptr, &vis) == 0;
                before[g] = existed[g] ? vis : 0;
                // value mode: an existing root under the noise condition asks for its mix at once
                float dummy[A];
                const int want = existed[g] && !fast && moves[g] < cfg.apply_dirichlet_n_first_moves;
                CHECK(azg_mcts_noise_request(h, g, dummy) == want);
                noisy_existing_roots += want;
            }
        }
        mix_noise(h, games);   // the requests of the roots just set
        if (n > 0) {
            fake_eval(lb.data(), lp.data(), n, p, v);
            CHECK(azg_mcts_feed(h, p.data(), v.data()) == 0);
            mix_noise(h, games);
        }
    }
    CHECK(live == 0);
    CHECK(batch == 1 || short_emits > 0);
    CHECK(max_moves < 2 || noisy_existing_roots > 0);
    // every tree was cleared: the mode may change again
    CHECK(azg_mcts_set_search_mode(h, AZG_MCTS_SEARCH_REFERENCE) == 0);
    CHECK(azg_mcts_get_search_mode(h) == AZG_MCTS_SEARCH_REFERENCE);
    CHECK(azg_mcts_destroy(h) == 0);
    std::printf("value mode: rules %d games %d sims %d batch %d threads %d: %d rounds, %d short emits\n", rules,
                games, sims, batch, threads, rounds, short_emits);
}

// One game driven by hand: a collision leaves a simulation suspended, a pending noise
// request on an existing root blocks the advance, clear in the middle of a search.
static void by_hand()
{
    const azg_mcts_config cfg = config(0, 12, 4);
    azg_mcts* h = nullptr;
    CHECK(azg_mcts_create(&cfg, 1, &h) == 0);
    CHECK(azg_mcts_set_search_mode(h, AZG_MCTS_SEARCH_VALUE) == 0);
    std::vector<int8_t> board(A, 0), lb((size_t)4 * A), lp(4);
    std::vector<float> p, v;
    int32_t counts = 0, status = 0, n = 0;
    CHECK(azg_mcts_set_root(h, 0, board.data(), 1, -1, -1, 0, 0, 0) == 0);
    CHECK(azg_mcts_set_search_mode(h, AZG_MCTS_SEARCH_REFERENCE) != 0);   // search in progress
    // the second simulation meets the queued root: one leaf, emitted at once
    CHECK(azg_mcts_advance_boards(h, lb.data(), lp.data(), &counts, &status, &n, 1) == 0);
    CHECK(n == 1 && status == AZG_MCTS_NEED_EVAL && azg_mcts_collisions(h, 0) == 1);
    CHECK(azg_mcts_inflight(h, 0) == 0);   // the root's path is empty
    fake_eval(lb.data(), lp.data(), n, p, v);
    CHECK(azg_mcts_feed(h, p.data(), v.data()) == 0);
    CHECK(mix_noise(h, 1) == 1);
    int emits = 0;
    int64_t most = 0;
    for (;;) {
        CHECK(azg_mcts_advance_boards(h, lb.data(), lp.data(), &counts, &status, &n, 1) == 0);
        if (status != AZG_MCTS_NEED_EVAL) break;
        ++emits;
        const int64_t fl = azg_mcts_inflight(h, 0);
        CHECK(fl >= n);   // every pending leaf below the root holds at least one edge
        if (fl > most) most = fl;
        // an advance before the feed emits the same leaves again
        std::vector<int8_t> again((size_t)4 * A), againp(4);
        int32_t c2 = 0, s2 = 0, n2 = 0;
        CHECK(azg_mcts_advance_boards(h, again.data(), againp.data(), &c2, &s2, &n2, 1) == 0);
        CHECK(n2 == n && std::memcmp(again.data(), lb.data(), (size_t)n * A) == 0);
        fake_eval(lb.data(), lp.data(), n, p, v);
        CHECK(azg_mcts_feed(h, p.data(), v.data()) == 0);
    }
    CHECK(status == AZG_MCTS_DONE && emits >= 3 && most > 0 && azg_mcts_inflight(h, 0) == 0);
    int64_t visits = 0;
    CHECK(azg_mcts_get_root_value(h, 0, nullptr, nullptr, &visits) == 0 && visits == 11);
    // the same root again: noise on an existing root, pending straight after set_root
    CHECK(azg_mcts_set_root(h, 0, board.data(), 1, -1, -1, 0, 0, 1) == 0);
    CHECK(azg_mcts_noise_request(h, 0, nullptr) == 1);
    CHECK(azg_mcts_advance_boards(h, lb.data(), lp.data(), &counts, &status, &n, 1) != 0);
    CHECK(std::strlen(azg_mcts_last_error()) > 0);
    CHECK(mix_noise(h, 1) == 1);
    CHECK(azg_mcts_advance_boards(h, lb.data(), lp.data(), &counts, &status, &n, 1) == 0);
    CHECK(status == AZG_MCTS_NEED_EVAL && azg_mcts_inflight(h, 0) > 0);
    // clear with leaves pending and virtual losses in place, then search anew
    CHECK(azg_mcts_clear(h, 0) == 0);
    CHECK(azg_mcts_inflight(h, 0) == 0 && azg_mcts_tree_size(h, 0) == 0);
    CHECK(azg_mcts_get_root_value(h, 0, nullptr, nullptr, &visits) != 0);
    CHECK(azg_mcts_set_budget(h, 0, 0, 0) == 0);   // a budget of no simulations: done at once
    CHECK(azg_mcts_set_root(h, 0, board.data(), 1, -1, -1, 0, 0, 0) == 0);
    CHECK(azg_mcts_advance_boards(h, lb.data(), lp.data(), &counts, &status, &n, 1) == 0);
    CHECK(n == 0 && status == AZG_MCTS_DONE);
    CHECK(azg_mcts_destroy(h) == 0);
}

int main()
{
    play(0, 4, 48, 8, 4, 40);
    play(0, 2, 33, 32, 1, 12);
    play(1, 3, 40, 8, 3, 40);
    play(1, 2, 24, 1, 2, 10);
    by_hand();
    // bad arguments
    const azg_mcts_config cfg = config(0, 8, 4);
    azg_mcts* h = nullptr;
    CHECK(azg_mcts_create(&cfg, 2, &h) == 0);
    CHECK(azg_mcts_set_search_mode(nullptr, 1) != 0 && std::strlen(azg_mcts_last_error()) > 0);
    CHECK(azg_mcts_set_search_mode(h, 2) != 0 && std::strstr(azg_mcts_last_error(), "unknown mode"));
    CHECK(azg_mcts_set_search_mode(h, -1) != 0);
    CHECK(azg_mcts_get_search_mode(nullptr) == -1 && azg_mcts_get_search_mode(h) == 0);
    double q;
    CHECK(azg_mcts_get_root_value(h, 2, &q, nullptr, nullptr) != 0);
    CHECK(azg_mcts_get_root_value(h, -1, &q, nullptr, nullptr) != 0);
    CHECK(azg_mcts_get_root_value(nullptr, 0, &q, nullptr, nullptr) != 0);
    CHECK(azg_mcts_get_root_value(h, 0, &q, nullptr, nullptr) != 0);   // no root yet
    CHECK(azg_mcts_inflight(h, 2) == -1 && azg_mcts_inflight(nullptr, 0) == -1 && azg_mcts_inflight(h, 1) == 0);
    CHECK(azg_mcts_collisions(h, 2) == -1 && azg_mcts_collisions(nullptr, 0) == -1);
    azg_mcts_config wide = config(0, 8, 70000);
    azg_mcts* hw = nullptr;
    CHECK(azg_mcts_create(&wide, 1, &hw) == 0);
    CHECK(azg_mcts_set_search_mode(hw, AZG_MCTS_SEARCH_VALUE) != 0);   // more in flight than an edge can count
    CHECK(azg_mcts_destroy(hw) == 0);
    CHECK(azg_mcts_destroy(h) == 0);
    std::printf("asan_mcts_value: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
