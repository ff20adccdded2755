// Posted eval launches: the one owner of their status words, launch records, circuit breaker
// and counters.  A posted launch is a tower launch whose dependency wait timed out, or a
// split-fp16 launch whose activations left fp16's range; its outputs are invalid until
// azg_pv_recover recomputes it.
//
// The protocol.  Every tower or split-fp16 launch gets a number `seq` (never 0: 0 means "not
// posted") and the slot seq & (kTowerRing - 1) of two rings of words in pinned, mapped host
// memory.  A kernel posts by storing seq into its slot of the timeout ring or the overflow
// ring (the device post sites: pv_tower.hip, pv_h3.h, pv_halo.h, pv_board.hip,
// pv_board16.hip); a slot belongs to seq only while its word equals seq, and begin() zeroes
// both before the launch.  The train step's words lie behind the two rings in the same
// memory.  Host code only, no HIP call: the owner hands in the host and device addresses of
// the words (azg_pv_bind), so a stand-alone program can drive it over a plain array
// (asan/asan_posted_main.cpp).
#pragma once
#include "pv_common.h"
#include "../../include/azg_pv.h"

#include <cstring>
#include <vector>

namespace azg {

constexpr unsigned kTowerRing = 256;          // slots of each ring (power of 2)
constexpr unsigned kTrainOvfWords = 16;       // + the train step's words (same memory): [kTrainFlag] the split-fp16
                                              // train forward's overflow flag of the step in flight (moved into the
                                              // gradient buffer's skip slot and cleared by heads_small_grads),
                                              // [kTrainSkips] steps the Adam kernel skipped (azg_pv_train_status)
constexpr unsigned kTrainFlag = 1, kTrainSkips = 2;
constexpr unsigned kStatusWords = 2 * kTowerRing + kTrainOvfWords;

// What one eval forward reads and writes.  `batch` counts BOARDS, here and in every host
// function that takes an EvalCall; the kernel launchers' B / M count IMAGES (images():
// 8 per board under SYM_MEAN8, the stem reading each board through its symmetries), and so
// do the workspace size and the profile's board counts.
struct EvalCall {
    const float* x = nullptr;          // float planes [batch][3][15][15], or
    const int8_t* boards = nullptr;    // int8 boards and players to move (x null)
    const int8_t* players = nullptr;
    const int8_t* syms = nullptr;      // SYM_EACH: one symmetry per board
    int symmode = SYM_NONE;
    int batch = 0;
    float *probs = nullptr, *values = nullptr;
    float *logits = nullptr, *priors = nullptr;   // optional
    int images() const { return symmode == SYM_MEAN8 ? 8 * batch : batch; }
};

struct PostedLaunches {
    // the status words: kStatusWords in one pinned, mapped allocation (kernels post, the host reads)
    unsigned* ring_host = nullptr;       // timed-out launch numbers [kTowerRing]
    unsigned* ring_dev = nullptr;        // device alias of ring_host
    unsigned* ovf_host = nullptr;        // launches whose activations left fp16's range [kTowerRing]
    unsigned* ovf_dev = nullptr;
    unsigned* train_ovf_dev = nullptr;   // [kTrainOvfWords] the train step's words (device alias)
    unsigned seq = 0;                    // last launch number handed out (0 = none yet)
    unsigned last_seq = 0;               // the last forward's launch number (0: it ran per-layer convs)
    // what each launch read and wrote, by slot (azg_pv_recover re-runs it)
    struct LaunchRec {
        unsigned seq = 0;
        bool h3 = false;
        int precision = AZG_PV_EVAL_EXACT;   // of the launch (the handle may have been switched since)
        EvalCall call;
    };
    std::vector<LaunchRec> launches;
    uint32_t recovered = 0;              // launches recomputed per layer
    uint32_t h3_overflows = 0;           // launches recomputed with fp32 MFMA (activations beyond fp16's range)
    // circuit breaker: a recovered launch means the dispatch did not run as one (the GPU is
    // shared and parts of it were suspended); until then forwards wait on no other workgroup
    // (per-layer convs; the 16x16x32 board tower one workgroup per board)
    double breaker_until = 0.0;          // steady-clock seconds (0: closed)
    uint32_t breaker_trips = 0;
    uint32_t breaker_launches = 0;       // forwards it changed: per layer, or board16 unsplit (the caller counts)

    static unsigned slot(unsigned s) { return s & (kTowerRing - 1); }
    static unsigned load(const unsigned* w) { return __atomic_load_n(w, __ATOMIC_ACQUIRE); }
    static void zero(unsigned* w) { __atomic_store_n(w, 0u, __ATOMIC_RELEASE); }

    bool attached() const { return ring_host != nullptr; }
    unsigned* host_words() const { return ring_host; }   // what attach() was given (its owner frees it)

    // host and device addresses of kStatusWords words: zeroes them, sizes the record ring
    void attach(unsigned* host, unsigned* dev)
    {
        ring_host = host;
        ovf_host = host + kTowerRing;
        memset(host, 0, kStatusWords * sizeof(unsigned));
        ring_dev = dev;
        ovf_dev = dev + kTowerRing;
        train_ovf_dev = dev + 2 * kTowerRing;
        launches.assign(kTowerRing, LaunchRec{});
    }

    // a new launch: its number, with its record written and both of its slots zeroed
    unsigned begin(const EvalCall& c, bool h3, int precision)
    {
        if (++seq == 0) ++seq;   // 0 means "not posted"
        launches[slot(seq)] = LaunchRec{seq, h3, precision, c};
        zero(ring_host + slot(seq));
        zero(ovf_host + slot(seq));
        return seq;
    }

    // bit 1: a wait of launch s timed out; bit 2: its activations left fp16's range
    int posted(unsigned s) const
    {
        if (!ring_host || s == 0) return 0;
        return (load(ring_host + slot(s)) == s ? 1 : 0) | (load(ovf_host + slot(s)) == s ? 2 : 0);
    }

    // posted eval launches not yet recovered (the two rings; not the train words)
    int count() const
    {
        if (!ring_host) return 0;
        int n = 0;
        for (unsigned i = 0; i < 2 * kTowerRing; ++i) n += load(ring_host + i) != 0u;
        return n;
    }

    // the record of launch s, or null once a newer launch has taken its slot
    const LaunchRec* record(unsigned s) const
    {
        if (launches.empty() || launches[slot(s)].seq != s) return nullptr;
        return &launches[slot(s)];
    }

    void release_overflow(unsigned s) { zero(ovf_host + slot(s)); }
    void release(unsigned s)
    {
        zero(ring_host + slot(s));
        release_overflow(s);
    }

    // train steps the Adam kernel skipped (a split-fp16 train forward met an activation
    // beyond fp16's range on some rank) since the last clear()
    unsigned train_skips() const { return ring_host ? load(ring_host + 2 * kTowerRing + kTrainSkips) : 0u; }

    void clear()
    {
        // the two rings and the skip count.  Not kTrainFlag: it belongs to a train step that may
        // still be queued, whose heads_small_grads moves it into the skip slot and clears it.
        // (A step whose host code fails between the forward that set the flag and
        // heads_small_grads leaves it set: the next step is then skipped and redone in fp32
        // once -- the safe direction -- and clears it.)
        if (ring_host) {
            for (unsigned i = 0; i < 2 * kTowerRing; ++i) zero(ring_host + i);
            zero(ring_host + 2 * kTowerRing + kTrainSkips);
        }
        breaker_until = 0.0;   // and the breaker closes
    }

    // true while the breaker is open; at its expiry it closes itself
    bool breaker_open(double now)
    {
        if (!(breaker_until > 0.0)) return false;
        if (now < breaker_until) return true;
        breaker_until = 0.0;
        return false;
    }

    void trip(double now, int seconds)
    {
        if (seconds <= 0) return;
        breaker_until = now + seconds;
        ++breaker_trips;
    }

    void reset_counters() { recovered = h3_overflows = breaker_trips = breaker_launches = 0; }
};

}  // namespace azg
