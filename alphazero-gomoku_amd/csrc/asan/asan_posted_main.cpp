// Host AddressSanitizer + UBSan driver of the posted-launch bookkeeping (csrc/pv_posted.h):
// PostedLaunches over a plain array of status words, the array standing in for both the
// host words and their device alias.  Sequence numbers and slots, posted state, the breaker
// and the counters.  No GPU and no HIP call.
#include "../pv_posted.h"

#include <cstdio>

using namespace azg;

static int fails = 0;
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++fails;                                                                      \
        }                                                                                 \
    } while (0)

static EvalCall call_of(int batch)
{
    EvalCall c;
    c.batch = batch;
    return c;
}

static void sequence_numbers_and_slots()
{
    unsigned w[kStatusWords];
    for (unsigned& x : w) x = 0xdeadbeefu;
    PostedLaunches p;
    CHECK(!p.attached() && p.posted(1) == 0 && p.count() == 0 && p.train_skips() == 0 && p.record(1) == nullptr);
    p.clear();   // unattached: touches no word
    p.attach(w, w);
    CHECK(p.attached() && p.launches.size() == kTowerRing);
    for (unsigned i = 0; i < kStatusWords; ++i) CHECK(w[i] == 0);
    CHECK(p.host_words() == w);
    CHECK(p.ring_dev == w && p.ovf_dev == w + kTowerRing && p.train_ovf_dev == w + 2 * kTowerRing);

    // 1, 2, ...: each launch takes its slot from an older launch's number
    w[1] = 0xffffff01u;                 // seq 1's slot, words of an older launch in the same slot
    w[kTowerRing + 1] = 0xffffff01u;
    for (unsigned n = 1; n <= kTowerRing + 1; ++n) {
        const unsigned s = p.begin(call_of((int)n), n % 2 == 1, n % 2 ? AZG_PV_EVAL_FP16 : AZG_PV_EVAL_EXACT);
        CHECK(s == n && p.seq == n);
        if (n == 1) CHECK(w[1] == 0 && w[kTowerRing + 1] == 0);
    }
    CHECK(p.last_seq == 0);             // the caller's to set
    // 257 launches: launch 257 has taken launch 1's slot and record
    CHECK(p.record(1) == nullptr);
    const PostedLaunches::LaunchRec* r = p.record(kTowerRing + 1);
    CHECK(r && r->seq == kTowerRing + 1 && r->h3 && r->precision == AZG_PV_EVAL_FP16 &&
          r->call.batch == (int)kTowerRing + 1);
    r = p.record(kTowerRing);
    CHECK(r && !r->h3 && r->precision == AZG_PV_EVAL_EXACT && r->call.batch == (int)kTowerRing);
    CHECK(p.record(0) == nullptr);      // slot 0 holds launch 256
    w[1] = kTowerRing + 1;              // a slot belongs to a number only while the word equals it
    CHECK(p.posted(kTowerRing + 1) == 1 && p.posted(1) == 0);
    w[1] = 0xffffff01u;
    w[kTowerRing + 1] = 0xffffff01u;
    CHECK(p.begin(call_of(1), false, 0) == kTowerRing + 2 && w[1] == 0xffffff01u);   // slot 2: not slot 1
    p.seq = 2 * kTowerRing;
    CHECK(p.begin(call_of(1), false, 0) == 2 * kTowerRing + 1 && w[1] == 0 && w[kTowerRing + 1] == 0);

    // the number wraps past 0: 0 means "not posted"
    p.seq = 0xfffffffeu;
    CHECK(p.begin(call_of(1), false, 0) == 0xffffffffu);
    CHECK(p.begin(call_of(2), false, 0) == 1u);
    CHECK(p.seq == 1u && p.record(1) && p.record(1)->call.batch == 2 && p.record(0) == nullptr);
    p.seq = 0xffffffffu;
    CHECK(p.begin(call_of(3), false, 0) == 1u);
}

static void posted_state()
{
    unsigned w[kStatusWords];
    PostedLaunches p;
    p.attach(w, w);
    const unsigned a = p.begin(call_of(1), true, 0), b = p.begin(call_of(1), true, 0), c = p.begin(call_of(1), true, 0);
    CHECK(p.posted(a) == 0 && p.posted(b) == 0 && p.posted(c) == 0 && p.count() == 0);
    w[a] = a;                           // what a kernel's post stores
    w[kTowerRing + b] = b;
    w[c] = c;
    w[kTowerRing + c] = c;
    CHECK(p.posted(a) == 1 && p.posted(b) == 2 && p.posted(c) == 3);
    CHECK(p.posted(0) == 0 && p.posted(a + kTowerRing) == 0);
    CHECK(p.count() == 4);
    // the train words are not posted launches
    w[2 * kTowerRing + kTrainFlag] = 1;
    w[2 * kTowerRing + kTrainSkips] = 7;
    CHECK(p.count() == 4 && p.train_skips() == 7);
    p.release_overflow(c);
    CHECK(p.posted(c) == 1 && w[c] == c && w[kTowerRing + c] == 0 && p.count() == 3);
    p.release(c);
    CHECK(p.posted(c) == 0 && p.count() == 2);
    p.release(a);
    CHECK(p.posted(a) == 0 && p.posted(b) == 2 && p.count() == 1);
    CHECK(w[2 * kTowerRing + kTrainFlag] == 1 && p.train_skips() == 7);

    p.trip(100.0, 30);
    for (unsigned i = 0; i < kStatusWords; ++i) w[i] = i + 1;
    p.clear();
    // the two rings and the skip count are zeroed; the other train words are not clear()'s
    for (unsigned i = 0; i < 2 * kTowerRing; ++i) CHECK(w[i] == 0);
    for (unsigned i = 2 * kTowerRing; i < kStatusWords; ++i)
        CHECK(w[i] == (i == 2 * kTowerRing + kTrainSkips ? 0u : i + 1));
    CHECK(p.count() == 0 && p.train_skips() == 0);
    CHECK(!p.breaker_open(100.0));      // and the breaker is closed
    CHECK(p.breaker_trips == 1 && p.seq == c && p.record(c));
}

// clear() while a train step is in flight: the step's overflow flag is not clear()'s to drop
static void clear_leaves_the_step_in_flight_alone()
{
    unsigned w[kStatusWords];
    PostedLaunches p;
    p.attach(w, w);
    const unsigned a = p.begin(call_of(1), true, 0), b = p.begin(call_of(1), true, 0);
    w[a] = a;                                      // a timed-out launch
    w[kTowerRing + b] = b;                         // a range overflow
    w[2 * kTowerRing + kTrainFlag] = 1;            // set by the split-fp16 forward of a queued step
    w[2 * kTowerRing + kTrainSkips] = 3;
    p.trip(50.0, 30);
    CHECK(p.count() == 2 && p.train_skips() == 3 && p.breaker_open(51.0));
    p.clear();
    CHECK(p.posted(a) == 0 && p.posted(b) == 0 && p.count() == 0 && p.train_skips() == 0);
    CHECK(w[2 * kTowerRing + kTrainFlag] == 1);    // only kTrainFlag survives
    for (unsigned i = 0; i < kStatusWords; ++i) CHECK(w[i] == (i == 2 * kTowerRing + kTrainFlag ? 1u : 0u));
    CHECK(!p.breaker_open(51.0));                  // the breaker is closed
}

static void breaker_and_counters()
{
    unsigned w[kStatusWords];
    PostedLaunches p;
    p.attach(w, w);
    const double t = 1000.0;
    CHECK(!p.breaker_open(t));
    p.trip(t, 0);
    p.trip(t, -1);
    CHECK(!p.breaker_open(t) && p.breaker_trips == 0);
    p.trip(t, 30);
    CHECK(p.breaker_trips == 1);
    CHECK(p.breaker_open(t) && p.breaker_open(t + 29));
    CHECK(!p.breaker_open(t + 31));
    CHECK(!p.breaker_open(t));          // it closed itself at its expiry
    CHECK(p.breaker_trips == 1 && p.breaker_launches == 0);

    const unsigned s = p.begin(call_of(5), true, AZG_PV_EVAL_FP16);
    w[s] = s;
    p.last_seq = s;
    p.recovered = 3;
    p.h3_overflows = 4;
    p.breaker_launches = 5;
    p.trip(t, 30);
    p.reset_counters();
    CHECK(p.recovered == 0 && p.h3_overflows == 0 && p.breaker_trips == 0 && p.breaker_launches == 0);
    CHECK(p.seq == s && p.last_seq == s && p.posted(s) == 1 && p.count() == 1);
    CHECK(p.record(s) && p.record(s)->call.batch == 5 && p.record(s)->precision == AZG_PV_EVAL_FP16);
    CHECK(p.breaker_open(t + 1));       // the breaker itself is not a counter
}

int main()
{
    sequence_numbers_and_slots();
    posted_state();
    clear_leaves_the_step_in_flight_alone();
    breaker_and_counters();
    if (fails) {
        std::fprintf(stderr, "asan_posted: %d check(s) failed\n", fails);
        return 1;
    }
    std::printf("asan_posted: ok\n");
    return 0;
}
