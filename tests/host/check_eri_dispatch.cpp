// test-only: the placement rule of the integral stage's dispatcher (metalquicha_amd/csrc/eri_dispatch.hpp) on the host.
// A stand-alone program: tests/test_eri_dispatch_host.py compiles it with -fsanitize=address,undefined and runs it.
//   (a) properties of pick_stream over every small state;
//   (b) a discrete-event replay of the 23 dense launches of the (H2O)64 dimer batch, with the durations recorded in
//       profiles/r05_b_integral_stage_timeline_deferred_groups.txt, through the rule: it must end within 6 % of the
//       lower bound at depth 1 and at depth 2, and the static placement recorded there must not;
//   (c) every launch issued exactly once, no stream ever above the depth limit, no ring slot handed out twice.
// Exit status 0 and a last line "ok" when everything holds; the first violation is printed and ends the program with 1.
#include "../../metalquicha_amd/csrc/eri_dispatch.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mqc::eri_dispatch;

#define REQUIRE(cond, ...)                                                                                             \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::printf("FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond);                                            \
            std::printf(__VA_ARGS__);                                                                                  \
            std::printf("\n");                                                                                         \
            std::exit(1);                                                                                              \
        }                                                                                                              \
    } while (0)

// ---- (a) ------------------------------------------------------------------------------------------------------------
static long check_rule_properties()
{
    long states = 0;
    for (int n = 1; n <= 4; ++n)
        for (int depth = 1; depth <= 3; ++depth) {
            int total = 1;
            for (int k = 0; k < n; ++k) total *= depth + 2;           // counts 0 .. depth + 1 (one above the limit too)
            // issue times: every assignment of n values out of {0 .. n-1}, repeats included where two streams are idle
            int times = 1;
            for (int k = 0; k < n; ++k) times *= n;
            for (int code = 0; code < total; ++code)
                for (int tcode = 0; tcode < times; ++tcode) {
                    int count[MAX_STREAMS];
                    long oldest[MAX_STREAMS];
                    int c = code, t = tcode;
                    bool distinct = true;
                    for (int k = 0; k < n; ++k) { count[k] = c % (depth + 2); c /= depth + 2; oldest[k] = t % n; t /= n; }
                    // two busy streams never issued their oldest launch at the same tick of the host's clock
                    for (int a = 0; a < n; ++a)
                        for (int b = a + 1; b < n; ++b)
                            if (count[a] > 0 && count[b] > 0 && oldest[a] == oldest[b]) distinct = false;
                    if (!distinct) continue;
                    ++states;
                    const int got = pick_stream(count, oldest, n, depth);
                    bool all_full = true;
                    int fewest = 1 << 30;
                    for (int k = 0; k < n; ++k) { if (count[k] < depth) all_full = false; fewest = std::min(fewest, count[k]); }
                    REQUIRE((got == NONE) == all_full, "n %d depth %d code %d: got %d, all streams full: %d", n, depth, code, got, (int)all_full);
                    if (got == NONE) continue;
                    REQUIRE(got >= 0 && got < n, "n %d depth %d code %d: stream %d out of range", n, depth, code, got);
                    REQUIRE(count[got] < depth, "n %d depth %d code %d: stream %d is at the limit (%d)", n, depth, code, got, count[got]);
                    REQUIRE(count[got] == fewest, "n %d depth %d code %d: stream %d holds %d, the fewest is %d", n, depth, code, got, count[got], fewest);
                    for (int k = 0; k < n; ++k) {
                        if (k == got || count[k] != fewest) continue;
                        if (fewest > 0)
                            REQUIRE(oldest[got] < oldest[k], "n %d depth %d code %d tcode %d: tie between %d and %d went to the younger", n, depth, code, tcode, got, k);
                        else
                            REQUIRE(got < k, "n %d depth %d code %d: tie between idle streams %d and %d went to the later", n, depth, code, got, k);
                    }
                }
        }
    return states;
}

// ---- (b), (c) -------------------------------------------------------------------------------------------------------
// ms, in the order of the timeline's streams: nine on the caller's stream, eight on s3, six on the chain stream s4
static const double RECORDED[23] = {5.85, 8.95, 3.55, 6.01, 2.19, 0.69, 0.38, 1.19, 0.44, 5.23, 3.26, 5.75,
                                    4.03, 2.07, 2.81, 0.93, 0.81, 6.10, 5.97, 2.42, 1.06, 0.85, 1.03};
static const int RECORDED_ON[3] = {9, 8, 6};
static const double CHAIN_FREE = 8.57, TASK_FREE = 17.96;     // ms after the first dense launch

struct Replay {
    double end = 0.0;
    std::vector<int> times_issued, stream_of;
};

// durations in issue order; free_at[k] > 0: stream k carries other work until then.  The host reacts at once.
static Replay replay(const std::vector<double>& dur, const std::vector<double>& free_at, int depth)
{
    const int n = (int)free_at.size();
    Book book(n, depth);
    REQUIRE(book.nstreams == n && book.depth == depth, "book of %d streams, depth %d", n, depth);
    std::vector<std::vector<double>> ends(n);       // end times of the outstanding launches, oldest first
    std::vector<std::vector<int>> slots(n);         // ... and their ring slots
    std::vector<double> tail(n, 0.0);               // when the stream's last queued work ends
    for (int k = 0; k < n; ++k) if (free_at[k] > 0.0) { book.block(k); tail[k] = free_at[k]; }
    Replay r;
    r.times_issued.assign(dur.size(), 0);
    r.stream_of.assign(dur.size(), -1);
    double t = 0.0;
    auto drain = [&]() {        // what the polls would see at time t
        for (int k = 0; k < n; ++k) {
            if (book.blocked[k]) { if (free_at[k] <= t) book.unblock(k); continue; }
            while (!ends[k].empty() && ends[k].front() <= t) {
                REQUIRE(book.oldest_slot(k) == slots[k].front(), "stream %d: oldest slot %d, expected %d", k, book.oldest_slot(k), slots[k].front());
                ends[k].erase(ends[k].begin()); slots[k].erase(slots[k].begin());
                book.pop(k);
            }
        }
    };
    for (size_t i = 0; i < dur.size(); ++i) {
        int q;
        for (;;) {
            drain();
            if ((q = book.pick()) != NONE) break;
            double next = 1e300;
            for (int k = 0; k < n; ++k) next = std::min(next, book.blocked[k] ? free_at[k] : (ends[k].empty() ? 1e300 : ends[k].front()));
            REQUIRE(next < 1e300 && next > t, "launch %zu: nothing to wait for at %.3f", i, t);
            t = next;
        }
        REQUIRE(q >= 0 && q < n && !book.blocked[q], "launch %zu went to stream %d", i, q);
        REQUIRE((int)ends[q].size() < depth, "launch %zu: stream %d already holds %zu", i, q, ends[q].size());
        const int slot = book.push(q);
        REQUIRE(slot >= 0 && slot < depth, "slot %d", slot);
        for (int s : slots[q]) REQUIRE(s != slot, "launch %zu: ring slot %d of stream %d is still in use", i, slot, q);
        const double start = std::max(t, tail[q]);
        tail[q] = start + dur[i];
        ends[q].push_back(tail[q]); slots[q].push_back(slot);
        REQUIRE(book.outstanding[q] == (int)ends[q].size() && book.outstanding[q] <= depth, "stream %d: %d outstanding", q, book.outstanding[q]);
        ++r.times_issued[i];
        r.stream_of[i] = q;
        r.end = std::max(r.end, tail[q]);
    }
    t = r.end;
    for (double f : free_at) t = std::max(t, f);
    drain();
    for (int k = 0; k < n; ++k) REQUIRE(book.outstanding[k] == 0 && !book.blocked[k], "stream %d not drained", k);
    return r;
}

int main()
{
    const long states = check_rule_properties();
    std::printf("(a) rule properties hold in %ld states\n", states);

    std::vector<double> heaviest_first(RECORDED, RECORDED + 23);
    std::sort(heaviest_first.begin(), heaviest_first.end(), [](double a, double b) { return a > b; });
    double sum = 0.0;
    for (double d : heaviest_first) sum += d;
    const double lower = (sum + CHAIN_FREE + TASK_FREE) / 4.0, bound = 1.06 * lower;
    std::printf("(b) 23 launches, %.2f ms; lower bound on four streams %.2f ms, bound %.2f ms\n", sum, lower, bound);
    REQUIRE(std::fabs(sum - 71.57) < 0.005 && std::fabs(lower - 24.525) < 0.005, "table: sum %.3f, lower bound %.3f", sum, lower);
    const std::vector<double> four = {0.0, 0.0, CHAIN_FREE, TASK_FREE};
    for (int depth = 1; depth <= 2; ++depth) {
        const Replay r = replay(heaviest_first, four, depth);
        std::printf("    depth %d: launches end after %.2f ms (+%.1f %%)\n", depth, r.end, 100.0 * (r.end / lower - 1.0));
        REQUIRE(r.end <= bound, "depth %d ends after %.3f ms, bound %.3f", depth, r.end, bound);
        REQUIRE(r.end >= lower - 1e-9, "depth %d ends before the lower bound: %.3f", depth, r.end);
        for (size_t i = 0; i < r.times_issued.size(); ++i) REQUIRE(r.times_issued[i] == 1, "launch %zu issued %d times", i, r.times_issued[i]);
        bool task_stream_used = false;
        for (int q : r.stream_of) task_stream_used = task_stream_used || q == 3;
        REQUIRE(task_stream_used, "depth %d: nothing ran on the task stream behind the copy", depth);
    }
    {
        // the static placement of the timeline: the recorded launches in their recorded order on their recorded streams
        double static_end = 0.0;
        const double from[3] = {0.0, 0.0, CHAIN_FREE};
        int i = 0;
        for (int k = 0; k < 3; ++k) {
            double t = from[k];
            for (int j = 0; j < RECORDED_ON[k]; ++j) t += RECORDED[i++];
            static_end = std::max(static_end, t);
        }
        std::printf("    static placement of the timeline: %.2f ms (+%.1f %%)\n", static_end, 100.0 * (static_end / lower - 1.0));
        REQUIRE(i == 23 && std::fabs(static_end - 29.24) < 0.02, "static replay ends after %.3f ms", static_end);
        REQUIRE(static_end > bound, "the static placement passes the bound (%.3f <= %.3f): the check does not discriminate", static_end, bound);
    }

    // (c) on other loads: 1 .. 8 streams, depth 1 .. 4, a fixed pseudo-random sequence of durations and head starts
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 40) / (double)(1ull << 24); };
    long runs = 0;
    for (int n = 1; n <= MAX_STREAMS; ++n)
        for (int depth = 1; depth <= MAX_DEPTH; ++depth)
            for (int rep = 0; rep < 8; ++rep) {
                std::vector<double> dur(1 + (int)(rnd() * 40.0)), free_at(n, 0.0);
                for (double& d : dur) d = 0.05 + 9.0 * rnd() * rnd();
                std::sort(dur.begin(), dur.end(), [](double a, double b) { return a > b; });
                for (int k = 1; k < n; ++k) if (rnd() < 0.4) free_at[k] = 20.0 * rnd();
                const Replay r = replay(dur, free_at, depth);
                for (size_t i = 0; i < dur.size(); ++i) REQUIRE(r.times_issued[i] == 1, "n %d depth %d: launch %zu issued %d times", n, depth, i, r.times_issued[i]);
                ++runs;
            }
    std::printf("(c) every launch issued exactly once in %ld further replays\n", runs);
    std::printf("ok\n");
    return 0;
}
