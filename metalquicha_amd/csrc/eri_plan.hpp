// eri_plan.hpp -- the launch sequence of the integral stage (launch_eri, kern_eri.hip), planned ahead of any launch.
// No HIP in here: the cost of a launch entry, the order and the static placement of the launches and the walk that
// issues them are plain host code, checked by tests/host/check_eri_plan.cpp.
//
// A launch entry has a dense half (every fragment forms the entry's blocks) and, in a batch with a share plan, a task
// half (one representative fragment per distinct geometry forms them; a copy kernel hands them to the others).
// Lane 0 is the caller's stream, lane k + 1 side stream k.
#pragma once

#include "eri_dispatch.hpp"

#include <algorithm>
#include <utility>
#include <vector>

namespace mqc {
namespace eri_plan {

// A small-batch launch lasts as long as its heaviest thread: primitive quartets of the first (deepest) entry x work
// per primitive quartet x passes.  l[]: the class's angular momenta; passes: 1 for the one-shot kernels.
inline double entry_cost(const int nprim[4], const int l[4], int passes, bool twin)
{
    double prims = 1.0;
    int ncart = 1, L = 0;
    for (int q = 0; q < 4; ++q) { prims *= nprim[q]; ncart *= (l[q] + 1) * (l[q] + 2) / 2; L += l[q]; }
    const int nherm = (L + 1) * (L + 2) * (L + 3) / 6;
    return prims * (ncart + 8.0 * nherm) * passes * (twin ? 1.5 : 1.0);
}

// dense_cost: 0 for an entry without a dense half
struct Entry { double dense_cost = 0.0, task_cost = 0.0; bool has_tasks = false; };

struct Plan {
    std::vector<int> dense_order;   // the entries in the order their dense halves are issued
    std::vector<int> lane;          // per entry: the static lane of its dense half
    std::vector<int> task_order;    // task stream only: the entries with a task half in the order they go on it
};

// spread: longest-processing-time-first assignment of the dense halves to the lanes 0 .. nside, issued heaviest first
// (stream order = issue order); otherwise list order on lane 0.  The chain lane (chain + 1, when the call may use it)
// carries the one-electron chain of the chunk ahead of anything queued here and starts with 1.5 x the heaviest launch.
// task_stream: lane 1 belongs to the task halves and the copy, heaviest first; no dense half goes there.
// Entries of equal cost keep what std::sort / std::stable_sort make of them: every entry without a dense half costs
// 0, and without the task stream their task halves go out in that order, round-robin over the side streams.
inline Plan plan(const std::vector<Entry>& entries, int nside, int chain, bool spread, bool task_stream)
{
    Plan p;
    const size_t n = entries.size();
    p.lane.assign(n, 0);
    if (spread) {
        std::vector<std::pair<double, int>> cost(n);
        for (size_t k = 0; k < n; ++k) cost[k] = {entries[k].dense_cost, (int)k};
        std::sort(cost.begin(), cost.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
        for (auto& ck : cost) p.dense_order.push_back(ck.second);
        double load[eri_dispatch::MAX_STREAMS] = {};
        if (chain < nside && !cost.empty()) load[chain + 1] = 1.5 * cost.front().first;
        for (auto& ck : cost) {
            int best = 0;
            for (int q = 1; q <= nside; ++q) {
                if (task_stream && q == 1) continue;
                if (load[q] < load[best]) best = q;
            }
            load[best] += ck.first;
            p.lane[ck.second] = best;
        }
    } else {
        for (size_t k = 0; k < n; ++k) p.dense_order.push_back((int)k);
    }
    if (task_stream) {
        std::vector<std::pair<double, int>> tc;
        for (size_t k = 0; k < n; ++k)
            if (entries[k].has_tasks) tc.push_back({entries[k].task_cost, (int)k});
        std::stable_sort(tc.begin(), tc.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
        for (auto& t : tc) p.task_order.push_back(t.second);
    }
    return p;
}

// What the walk hands out.  DENSE_WITH_TASKS: without the task stream an entry's task half goes out with its dense half.
// entry: -1 for the copy; lane: of the dense half, 1 for the side queue's items; dispatched: the lane came from the
// dispatcher, not from the plan.  A Placement of lane WAIT: the dispatcher has no stream yet.
enum Kind { DENSE, DENSE_WITH_TASKS, TASKS, COPY };
struct Item { Kind kind; int entry, lane; bool dispatched; };
struct Placement { int lane; bool dispatched; };
constexpr int WAIT = eri_dispatch::NONE;

// The walk over two queues.  Dense queue: the entries in issue order.  Side queue (task stream only): the task halves
// in task order, the copy directly behind the last of them.  After each dense item one side item goes out; what is
// left of the side queue goes out at the end.
//   place(entry): the lane of the entry's dense half -- the plan's, or the dispatcher's choice; WAIT while the
//                 dispatcher has no stream: side items then go out ahead of their turn, and once there are none
//                 idle() is called before place() is asked again.
//   emit(item):   issues it.
// An empty task list leaves the copy alone in the side queue: with the dispatcher on from the start (dispatching) it
// goes out ahead of the dense items -- the task stream stays blocked until it is done --, otherwise behind them.
template <class Place, class Idle, class Emit>
inline void walk(const Plan& p, bool task_stream, bool dispatching, Place&& place, Idle&& idle, Emit&& emit)
{
    const size_t nt = p.task_order.size();
    size_t ti = 0;
    bool copy_out = !task_stream;
    auto side_item = [&]() {
        if (ti < nt) emit(Item{TASKS, p.task_order[ti++], 1, false});
        if (ti == nt && !copy_out) { emit(Item{COPY, -1, 1, false}); copy_out = true; }
    };
    const bool copy_last = nt == 0 && !dispatching;
    if (nt == 0 && dispatching) side_item();
    for (int k : p.dense_order) {
        Placement at;
        while ((at = place(k)).lane == WAIT) { if (!copy_out) side_item(); else idle(); }
        emit(Item{task_stream ? DENSE : DENSE_WITH_TASKS, k, at.lane, at.dispatched});
        if (!copy_last) side_item();
    }
    while (!copy_out) side_item();
}

}  // namespace eri_plan
}  // namespace mqc
