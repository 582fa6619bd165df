// eri_dispatch.hpp -- placement of the integral stage's class launches on the streams as they drain (launch_eri,
// kern_eri.hip).  No HIP in here: the rule and its bookkeeping are plain host code, checked by
// tests/host/check_eri_dispatch.cpp.
//
// The host hands the launches out one by one, heaviest first.  For each it asks pick(): the stream with the fewest
// launches issued and not yet seen complete, if that is below the depth limit; otherwise nobody, and the host polls
// the streams' events until one drains.  No cost model is involved: a stream that got a long launch simply comes back
// later.
#pragma once

namespace mqc {
namespace eri_dispatch {

constexpr int MAX_STREAMS = 8;      // the caller's stream and ERI_SIDE_MAX side streams
constexpr int MAX_DEPTH = 4;
constexpr int NONE = -1;

// The rule.  outstanding[k]: launches issued on stream k and not yet complete; oldest[k]: when the oldest of them was
// issued (any monotonic count; read only where outstanding[k] > 0).  Among streams below `depth` the one with the fewest
// outstanding launches; of two with equally many the one whose oldest launch was issued first (it has run longest and
// is the likelier to drain first), of two idle ones the first.  NONE: every stream is at the limit, wait.
inline int pick_stream(const int* outstanding, const long* oldest, int nstreams, int depth)
{
    int best = NONE;
    for (int k = 0; k < nstreams; ++k) {
        if (outstanding[k] >= depth) continue;
        if (best == NONE || outstanding[k] < outstanding[best] ||
            (outstanding[k] == outstanding[best] && outstanding[k] > 0 && oldest[k] < oldest[best]))
            best = k;
    }
    return best;
}

// What the dispatcher knows about its streams.  A stream that carries other work when the stage starts (the
// one-electron chain, the task launches and their copy, an earlier call's launches) is block()ed: that work is several
// launches deep, so the stream counts as full until the one event behind it has been seen complete (unblock).  Each
// launch issued takes a slot of the stream's ring (push), which is also the index of the event recorded behind it; the
// oldest slot is given back when that event has been seen complete (pop).
struct Book {
    int nstreams = 0, depth = 1;
    int outstanding[MAX_STREAMS] = {};
    bool blocked[MAX_STREAMS] = {};
    int head[MAX_STREAMS] = {};                  // ring slot of the oldest outstanding launch
    long issued_at[MAX_STREAMS][MAX_DEPTH] = {};
    long clock = 0;

    Book(int nstreams_, int depth_)
        : nstreams(nstreams_ < 1 ? 1 : (nstreams_ > MAX_STREAMS ? MAX_STREAMS : nstreams_)),
          depth(depth_ < 1 ? 1 : (depth_ > MAX_DEPTH ? MAX_DEPTH : depth_)) {}

    void block(int k) { blocked[k] = true; }
    void unblock(int k) { blocked[k] = false; }
    int pick() const
    {
        int count[MAX_STREAMS];
        long oldest[MAX_STREAMS];
        for (int k = 0; k < nstreams; ++k) {
            count[k] = blocked[k] ? depth : outstanding[k];
            oldest[k] = issued_at[k][head[k]];
        }
        return pick_stream(count, oldest, nstreams, depth);
    }
    int oldest_slot(int k) const { return head[k]; }
    // a launch goes onto stream k (which pick() named): the ring slot it takes
    int push(int k)
    {
        const int slot = (head[k] + outstanding[k]) % depth;
        issued_at[k][slot] = clock++;
        ++outstanding[k];
        return slot;
    }
    // the oldest launch of stream k is complete
    void pop(int k)
    {
        head[k] = (head[k] + 1) % depth;
        --outstanding[k];
    }
};

}  // namespace eri_dispatch
}  // namespace mqc
