// test-only: the planned launch sequence of the integral stage (metalquicha_amd/csrc/eri_plan.hpp) on the host.
// A stand-alone program: tests/test_eri_plan_host.py compiles it with -fsanitize=address,undefined and runs it.
//   (a) goldens: the cost tables of three recorded calls of the build before the planner existed
//       (profiles/r07_a_launch_sequence_parent_vs_tree.log, configurations a, c and e) with the dense order, the lanes
//       and the task order that build used;
//   (b) properties of the plan over randomised small tables (many equal and zero costs), every combination of spread
//       and task stream;
//   (c) the walk over the two queues with scripted answers of the lane source.
// Exit status 0 and a last line "ok" when everything holds; the first violation is printed and ends the program with 1.
#include "../../metalquicha_amd/csrc/eri_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

using namespace mqc::eri_plan;

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
struct Golden {
    const char* name;
    int nside, chain;
    bool spread, task_stream;
    std::vector<Entry> entries;                      // dense cost, task cost, has a task half
    std::vector<int> dense_order, lane, task_order;  // what the recorded build did
};
// one issued launch of a recorded call: entry (-1: the copy), 0 dense / 1 tasks, lane
struct Issued { int entry, half, lane; };

// The tables are the costs the recorded build printed with %.17g, the orders and lanes what it computed inline.
static const std::vector<Golden> GOLDENS = {
    {"a: 20 fragments that share nothing, plain spread", 3, 2, true, false,
     {{1093.5, 0.0, false}, {729.0, 0.0, false}, {4252.5, 0.0, false}, {2835.0, 0.0, false}, {7209.0, 0.0, false},
      {7209.0, 0.0, false}, {15147.0, 0.0, false}, {58482.0, 0.0, false}, {6966.0, 0.0, false},
      {14418.0, 0.0, false}, {27054.0, 0.0, false}, {25596.0, 0.0, false}, {14418.0, 0.0, false},
      {27054.0, 0.0, false}, {148230.0, 0.0, false}, {90072.0, 0.0, false}, {403380.0, 0.0, false},
      {25596.0, 0.0, false}, {90072.0, 0.0, false}, {403380.0, 0.0, false}, {215784.0, 0.0, false},
      {1041984.0, 0.0, false}, {2754648.0, 0.0, false}},
     {22, 21, 19, 16, 20, 14, 18, 15, 7, 10, 13, 11, 17, 6, 12, 9, 5, 4, 8, 2, 3, 0, 1},
     {1, 2, 2, 1, 2, 2, 1, 2, 1, 1, 1, 1, 2, 2, 2, 1, 2, 2, 1, 2, 2, 1, 0},
     {}},
    {"c: 384 fragments with shared sets, static task stream", 3, 2, true, true,
     {{1093.5, 1093.5, true}, {486.0, 729.0, true}, {4252.5, 4252.5, true}, {2835.0, 1890.0, true},
      {7209.0, 7209.0, true}, {7209.0, 7209.0, true}, {15147.0, 15147.0, true}, {38988.0, 58482.0, true},
      {6966.0, 6966.0, true}, {14418.0, 9612.0, true}, {27054.0, 18036.0, true}, {25596.0, 25596.0, true},
      {14418.0, 9612.0, true}, {27054.0, 18036.0, true}, {148230.0, 98820.0, true}, {90072.0, 60048.0, true},
      {403380.0, 179280.0, true}, {25596.0, 25596.0, true}, {90072.0, 60048.0, true}, {403380.0, 179280.0, true},
      {215784.0, 215784.0, true}, {1041984.0, 694656.0, true}, {1836432.0, 2754648.0, true}},
     {22, 21, 19, 16, 20, 14, 18, 15, 7, 10, 13, 11, 17, 6, 12, 9, 5, 4, 8, 2, 3, 0, 1},
     {2, 2, 0, 0, 0, 2, 2, 2, 2, 0, 2, 2, 2, 0, 2, 0, 2, 0, 2, 2, 0, 2, 0},
     {22, 21, 20, 16, 19, 14, 15, 18, 7, 11, 17, 10, 13, 6, 9, 12, 4, 5, 8, 2, 3, 0, 1}},
    {"e: 16 fragments with shared sets, one side stream, static task stream", 1, 2, true, true,
     {{729.0, 1093.5, true}, {486.0, 729.0, true}, {2835.0, 4252.5, true}, {1890.0, 2835.0, true},
      {4806.0, 7209.0, true}, {4806.0, 7209.0, true}, {10098.0, 15147.0, true}, {19494.0, 58482.0, true},
      {4644.0, 6966.0, true}, {9612.0, 14418.0, true}, {18036.0, 27054.0, true}, {17064.0, 25596.0, true},
      {9612.0, 14418.0, true}, {18036.0, 27054.0, true}, {49410.0, 148230.0, true}, {60048.0, 90072.0, true},
      {134460.0, 403380.0, true}, {17064.0, 25596.0, true}, {60048.0, 90072.0, true}, {134460.0, 403380.0, true},
      {143856.0, 215784.0, true}, {347328.0, 1041984.0, true}, {918216.0, 2754648.0, true}},
     {22, 21, 20, 19, 16, 18, 15, 14, 7, 10, 13, 11, 17, 6, 12, 9, 5, 4, 8, 2, 3, 0, 1},
     {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
     {22, 21, 16, 19, 20, 14, 15, 18, 7, 10, 13, 11, 17, 6, 9, 12, 4, 5, 8, 2, 3, 0, 1}},
};
// every launch of recorded call c in the order it was issued: {entry, half, lane}, the copy last
static const std::vector<Issued> ISSUED_C = {
    {22, 0, 0}, {22, 1, 1}, {21, 0, 2}, {21, 1, 1}, {19, 0, 2}, {20, 1, 1}, {16, 0, 2}, {16, 1, 1}, {20, 0, 0},
    {19, 1, 1}, {14, 0, 2}, {14, 1, 1}, {18, 0, 2}, {15, 1, 1}, {15, 0, 0}, {18, 1, 1}, {7, 0, 2}, {7, 1, 1},
    {10, 0, 2}, {11, 1, 1}, {13, 0, 0}, {17, 1, 1}, {11, 0, 2}, {10, 1, 1}, {17, 0, 0}, {13, 1, 1}, {6, 0, 2},
    {6, 1, 1}, {12, 0, 2}, {9, 1, 1}, {9, 0, 0}, {12, 1, 1}, {5, 0, 2}, {4, 1, 1}, {4, 0, 0}, {5, 1, 1}, {8, 0, 2},
    {8, 1, 1}, {2, 0, 0}, {2, 1, 1}, {3, 0, 0}, {3, 1, 1}, {0, 0, 2}, {0, 1, 1}, {1, 0, 2}, {1, 1, 1}, {-1, 1, 1}
};

static void check_goldens()
{
    for (const Golden& g : GOLDENS) {
        const Plan p = plan(g.entries, g.nside, g.chain, g.spread, g.task_stream);
        REQUIRE(p.dense_order == g.dense_order, "%s: dense order differs from the recorded one", g.name);
        REQUIRE(p.lane == g.lane, "%s: lanes differ from the recorded ones", g.name);
        REQUIRE(p.task_order == g.task_order, "%s: task order differs from the recorded one", g.name);
    }
    // entry_cost by hand: (pp|pp) of four one-primitive shells in one pass, 81 components + 8 x 35 Hermite terms; a twin
    // (ss|ss) entry of 3-primitive shells, 81 primitive quartets x (1 + 8) x 1.5
    const int one[4] = {1, 1, 1, 1}, three[4] = {3, 3, 3, 3}, pppp[4] = {1, 1, 1, 1}, ssss[4] = {0, 0, 0, 0};
    REQUIRE(entry_cost(one, pppp, 1, false) == 361.0, "(pp|pp): %.17g", entry_cost(one, pppp, 1, false));
    REQUIRE(entry_cost(three, ssss, 1, true) == 81.0 * 9.0 * 1.5, "twin (ss|ss): %.17g", entry_cost(three, ssss, 1, true));
    REQUIRE(entry_cost(one, pppp, 3, false) == 3.0 * 361.0, "three passes");
}

// ---- (b) ------------------------------------------------------------------------------------------------------------
static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 40) / (double)(1ull << 24);
}

struct Table {
    std::vector<Entry> entries;
    int nside, chain;
};
static Table random_table()
{
    static const double COSTS[8] = {0.0, 0.0, 0.0, 81.0, 81.0, 361.0, 1093.5, 2816.0};     // many ties and zeros
    Table t;
    t.entries.resize((size_t)(rnd() * 13.0));       // 0 .. 12
    for (Entry& e : t.entries) {
        e.dense_cost = COSTS[(int)(rnd() * 8.0)];
        e.has_tasks = rnd() < 0.5;
        e.task_cost = e.has_tasks ? COSTS[3 + (int)(rnd() * 5.0)] : 0.0;
    }
    t.nside = 1 + (int)(rnd() * 7.0);               // 1 .. 7
    t.chain = (int)(rnd() * 8.0);                   // 0 .. 7: at or above nside the call has no chain lane
    return t;
}

template <class T>
static bool is_permutation_of_range(const std::vector<T>& v, size_t n)
{
    std::vector<int> seen(n, 0);
    if (v.size() != n) return false;
    for (T k : v) { if (k < 0 || (size_t)k >= n || seen[k]++) return false; }
    return true;
}

static void check_plan_properties(const Table& t, bool spread, bool task_stream)
{
    const std::vector<Entry>& e = t.entries;
    const size_t n = e.size();
    const Plan p = plan(e, t.nside, t.chain, spread, task_stream);
    // every dense half exactly once
    REQUIRE(is_permutation_of_range(p.dense_order, n) && p.lane.size() == n, "dense order is no permutation of %zu entries", n);
    // every task half exactly once, only for entries that have one, heaviest first, equal costs in list order
    std::vector<int> in_task_order(n, 0);
    for (int k : p.task_order) { REQUIRE(k >= 0 && (size_t)k < n && e[k].has_tasks, "task order names entry %d", k); ++in_task_order[k]; }
    for (size_t k = 0; k < n; ++k) REQUIRE(in_task_order[k] == (task_stream && e[k].has_tasks ? 1 : 0), "entry %zu: %d times in the task order", k, in_task_order[k]);
    for (size_t i = 1; i < p.task_order.size(); ++i) {
        const int a = p.task_order[i - 1], b = p.task_order[i];
        REQUIRE(e[a].task_cost > e[b].task_cost || (e[a].task_cost == e[b].task_cost && a < b), "task order: %d ahead of %d", a, b);
    }
    if (!spread) {
        for (size_t k = 0; k < n; ++k) REQUIRE(p.dense_order[k] == (int)k && p.lane[k] == 0, "unspread: entry %zu at %d on lane %d", k, p.dense_order[k], p.lane[k]);
        return;
    }
    for (size_t i = 1; i < n; ++i) REQUIRE(e[p.dense_order[i - 1]].dense_cost >= e[p.dense_order[i]].dense_cost, "dense order not heaviest first at %zu", i);
    // the loads as the placement saw them, rebuilt from the lanes it returned
    const int nlanes = t.nside + 1, chain_lane = t.chain < t.nside ? t.chain + 1 : -1;
    const double head_start = n > 0 ? 1.5 * e[p.dense_order[0]].dense_cost : 0.0;
    std::vector<double> load(nlanes, 0.0);
    std::vector<int> placed(nlanes, 0);
    if (chain_lane >= 0) load[chain_lane] = head_start;
    auto permitted = [&](int q) { return !(task_stream && q == 1); };
    for (int k : p.dense_order) {
        const int q = p.lane[k];
        REQUIRE(q >= 0 && q <= t.nside, "entry %d on lane %d of 0 .. %d", k, q, t.nside);
        REQUIRE(permitted(q), "entry %d: dense half on the task stream's lane", k);
        // longest first: without this item its lane is no heavier than any other permitted lane at that moment
        for (int r = 0; r < nlanes; ++r)
            if (permitted(r)) REQUIRE(load[q] <= load[r], "entry %d went to lane %d (%.1f) while lane %d held %.1f", k, q, load[q], r, load[r]);
        // the head start: the chain lane takes a launch only when every other permitted lane carries at least that much
        if (q == chain_lane)
            for (int r = 0; r < nlanes; ++r)
                if (permitted(r)) REQUIRE(load[r] >= head_start, "entry %d on the chain lane while lane %d held %.1f < %.1f", k, r, load[r], head_start);
        load[q] += e[k].dense_cost;
        ++placed[q];
    }
    // ... so a chain lane that was used leaves every other permitted lane with the head start or more.  An unused one
    // promises nothing about the others: a list of one launch puts it on lane 0 and leaves every other lane empty
    if (chain_lane >= 0 && placed[chain_lane] > 0)
        for (int r = 0; r < nlanes; ++r)
            if (permitted(r)) REQUIRE(load[r] >= head_start, "chain lane used, lane %d ends with %.1f < %.1f", r, load[r], head_start);
}

// ---- (c) ------------------------------------------------------------------------------------------------------------
enum Script { ALWAYS, NEVER_UNTIL_SIDE_EMPTY, ALTERNATING };

struct Walked {
    std::vector<Item> items;
    long idles = 0;
};

// the lane source answers by script; a lane it grants is the plan's, marked as dispatched
static Walked run_walk(const Plan& p, bool task_stream, bool dispatching, Script script)
{
    Walked w;
    bool copy_seen = !task_stream;
    long asked = 0;
    auto place = [&](int k) -> Placement {
        ++asked;
        const bool yes = script == ALWAYS || (script == NEVER_UNTIL_SIDE_EMPTY ? copy_seen : asked % 2 == 0);
        return yes ? Placement{p.lane[k], dispatching} : Placement{WAIT, false};
    };
    auto idle = [&]() { ++w.idles; REQUIRE(copy_seen, "idle() with side items still queued"); };
    auto emit = [&](const Item& it) { w.items.push_back(it); if (it.kind == COPY) copy_seen = true; };
    walk(p, task_stream, dispatching, place, idle, emit);
    return w;
}

static void check_walk(const std::vector<Entry>& e, const Plan& p, bool task_stream, bool dispatching, Script script)
{
    const size_t n = e.size();
    const Walked w = run_walk(p, task_stream, dispatching, script);
    std::vector<int> dense(n, 0), tasks(n, 0);
    int copies = 0;
    long last_task = -1, copy_at = -1;
    size_t next_dense = 0, next_task = 0;
    for (size_t i = 0; i < w.items.size(); ++i) {
        const Item& it = w.items[i];
        if (it.kind == COPY) { ++copies; copy_at = (long)i; REQUIRE(it.lane == 1 && it.entry == -1, "copy on lane %d", it.lane); continue; }
        REQUIRE(it.entry >= 0 && (size_t)it.entry < n, "item %zu names entry %d", i, it.entry);
        if (it.kind == TASKS) {
            REQUIRE(task_stream && it.lane == 1 && copies == 0, "item %zu: a task item outside the side queue, or behind the copy", i);
            REQUIRE(next_task < p.task_order.size() && it.entry == p.task_order[next_task], "item %zu: task item out of order", i);
            ++next_task; ++tasks[it.entry]; last_task = (long)i;
            continue;
        }
        REQUIRE(it.kind == (task_stream ? DENSE : DENSE_WITH_TASKS), "item %zu: kind %d", i, (int)it.kind);
        REQUIRE(it.entry == p.dense_order[next_dense] && it.lane == p.lane[it.entry], "item %zu: dense item out of order or off its lane", i);
        ++next_dense; ++dense[it.entry];
        if (it.kind == DENSE_WITH_TASKS) ++tasks[it.entry];
    }
    for (size_t k = 0; k < n; ++k) {
        REQUIRE(dense[k] == 1, "entry %zu: dense half issued %d times", k, dense[k]);
        // without the task stream every entry goes out with its task half, empty or not (the round-robin counter)
        REQUIRE(tasks[k] == (task_stream ? (e[k].has_tasks ? 1 : 0) : 1), "entry %zu: task half issued %d times", k, tasks[k]);
    }
    REQUIRE(copies == (task_stream ? 1 : 0), "%d copies", copies);
    if (!task_stream) return;
    if (last_task >= 0) REQUIRE(copy_at == last_task + 1, "the copy is item %ld, the last task item %ld", copy_at, last_task);
    // an empty task list: the copy ahead of everything under the dispatcher, behind everything without
    else REQUIRE(copy_at == (dispatching ? 0 : (long)w.items.size() - 1), "empty task list: the copy is item %ld of %zu", copy_at, w.items.size());
    // a lane source that never makes the walk wait: one side item behind each dense item, the rest at the end
    if (script == ALWAYS && last_task >= 0) {
        std::vector<std::pair<Kind, int>> expect;
        const size_t nt = p.task_order.size();
        for (size_t i = 0; i < n || i < nt; ++i) {
            if (i < n) expect.push_back({DENSE, p.dense_order[i]});
            if (i < nt) expect.push_back({TASKS, p.task_order[i]});
            if (i + 1 == nt) expect.push_back({COPY, -1});
        }
        REQUIRE(expect.size() == w.items.size(), "%zu items, expected %zu", w.items.size(), expect.size());
        for (size_t i = 0; i < expect.size(); ++i)
            REQUIRE(w.items[i].kind == expect[i].first && w.items[i].entry == expect[i].second, "item %zu: kind %d entry %d", i, (int)w.items[i].kind, w.items[i].entry);
        REQUIRE(w.idles == 0, "%ld idles", w.idles);
    }
    if (script == NEVER_UNTIL_SIDE_EMPTY && n > 0)
        REQUIRE(copy_at == (long)p.task_order.size(), "the side queue did not go out ahead of the first dense item: copy at %ld", copy_at);
}

int main()
{
    check_goldens();
    std::printf("(a) %zu recorded calls: dense order, lanes and task order reproduced\n", GOLDENS.size());

    long tables = 0;
    for (int rep = 0; rep < 4000; ++rep) {
        const Table t = random_table();
        for (int spread = 0; spread < 2; ++spread)
            for (int task_stream = 0; task_stream < 2; ++task_stream) {
                check_plan_properties(t, spread != 0, task_stream != 0);
                const Plan p = plan(t.entries, t.nside, t.chain, spread != 0, task_stream != 0);
                for (int dispatching = 0; dispatching < 2; ++dispatching)
                    for (Script s : {ALWAYS, NEVER_UNTIL_SIDE_EMPTY, ALTERNATING}) {
                        if (!dispatching && s != ALWAYS) continue;          // the plan never makes the walk wait
                        check_walk(t.entries, p, task_stream != 0, dispatching != 0, s);
                    }
                ++tables;
            }
    }
    std::printf("(b) plan properties hold for %ld tables\n", tables);
    std::printf("(c) the walk issues every item once, the copy right behind the last task item, under three scripts\n");

    // the static interleaving of recorded configuration c: the walk over its plan, lane source "always"
    const Golden& g = GOLDENS[1];
    const Plan p = plan(g.entries, g.nside, g.chain, g.spread, g.task_stream);
    const Walked w = run_walk(p, g.task_stream, false, ALWAYS);
    size_t at = 0;
    for (const Item& it : w.items) {
        if (it.kind == DENSE && g.entries[it.entry].dense_cost == 0.0) continue;       // no dense half: nothing was launched
        REQUIRE(at < ISSUED_C.size(), "more items than the recorded call launched");
        const Issued& r = ISSUED_C[at++];
        REQUIRE(r.entry == it.entry && r.half == (it.kind == DENSE ? 0 : 1) && r.lane == it.lane, "launch %zu: entry %d half %d lane %d, recorded %d %d %d",
                at - 1, it.entry, it.kind == DENSE ? 0 : 1, it.lane, r.entry, r.half, r.lane);
    }
    REQUIRE(at == ISSUED_C.size(), "%zu of %zu recorded launches", at, ISSUED_C.size());
    std::printf("    configuration c: %zu launches in the recorded order on the recorded lanes\n", at);
    std::printf("ok\n");
    return 0;
}
