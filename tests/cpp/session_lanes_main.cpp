// session_lanes_main.cpp -- jtk_amd/csrc/session_lanes.h with mock streams and a recording launch, as a program of its own
// (tests/test_session_lanes.py builds it with a sanitizer and runs it).  Prints what the test compares (PLAN / ASSIGN lines)
// and checks the gathering rule itself: any violated expectation prints FAIL ... and makes the exit status 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "session_lanes.h"

static std::atomic<int> g_failures{0};
#define EXPECT(cond, ...)                \
    do {                                 \
        if (!(cond)) {                   \
            printf("FAIL %s:%d ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);         \
            printf("\n");                \
            g_failures++;                \
        }                                \
    } while (0)

struct MockStreams {
    int stream = 0, side = 0;
};
enum { IDLE = 0, BEFORE = 1, ARRIVED = 2 };
struct Member {
    int id = 0;
    std::atomic<int> state{IDLE};     // BEFORE: enter() has returned and arrive() has not been called yet
    std::atomic<int> launched{0};     // launches that carried this member
};
typedef LaneTable<MockStreams, Member> Table;

static void plans() {
    const int qs[] = {1, 2, 3, 4, 6, 7, 8, 9, 12, 16, 32, 100};
    for (int q : qs) {
        const LanePlan p = lane_plan(q, 0, -1);
        printf("PLAN %d %d %d\n", q, p.max_lanes, p.side ? 1 : 0);
    }
    const LanePlan a = lane_plan(4, 3, 0), b = lane_plan(12, 1, -1), c = lane_plan(4, 0, 1);
    printf("FORCED %d %d %d %d %d %d\n", a.max_lanes, a.side ? 1 : 0, b.max_lanes, b.side ? 1 : 0, c.max_lanes, c.side ? 1 : 0);
}

// sessions 1 .. 10 created one after the other at Q queues; then sessions 2 and 5 leave and two more arrive
static void assignment(int q) {
    const LanePlan p = lane_plan(q, 0, -1);
    Table t;
    int made = 0;
    auto make = [&](MockStreams &s) {
        s.stream = ++made;
        return true;
    };
    std::vector<int> lane;
    printf("ASSIGN %d", q);
    for (int i = 0; i < 10; i++) {
        lane.push_back(t.acquire(p.max_lanes, make));
        printf(" %d", lane.back());
    }
    t.release(lane[1]);
    t.release(lane[4]);
    const int x = t.acquire(p.max_lanes, make), y = t.acquire(p.max_lanes, make);
    printf(" | %d %d | lanes %d\n", x, y, t.size());
    EXPECT(made == t.size(), "a lane was made %d times for %d lanes", made, t.size());
    // a smaller limit later (JTK_LC_LANES changed between two sessions) keeps to the first lanes
    const int z = t.acquire(1, make);
    EXPECT(z == 0, "limit 1 gave lane %d", z);
    // a failing make gives -1 and leaves the table as it was
    Table u;
    EXPECT(u.acquire(2, [](MockStreams &) { return false; }) == -1 && u.size() == 0, "failed make");
}

struct Recorder {
    std::vector<Member *> lane_members;  // everybody who may be in a pass on this lane
    std::mutex m;
    std::vector<int> sizes;
    int rc = 0;
    int operator()(Member *const *g, int n) {
        EXPECT(n >= 1 && n <= JTK_LANE_MAX_SEGMENTS, "a launch of %d members", n);
        for (Member *x : lane_members) EXPECT(x->state.load() != BEFORE, "launch while member %d is before its chain point", x->id);
        for (int i = 0; i < n; i++) {
            EXPECT(g[i]->state.load() == ARRIVED, "member %d launched in state %d", g[i]->id, g[i]->state.load());
            g[i]->launched++;
        }
        std::lock_guard<std::mutex> lock(m);
        sizes.push_back(n);
        return rc;
    }
};

// 3 sessions x 4 passes on one lane from 3 threads, seeded random delays before and after the chain point
static void three_by_four() {
    LaneGather<Member> g;
    Member mem[3];
    Recorder rec;
    for (int i = 0; i < 3; i++) {
        mem[i].id = i;
        rec.lane_members.push_back(&mem[i]);
    }
    std::vector<std::thread> th;
    for (int i = 0; i < 3; i++)
        th.emplace_back([&, i]() {
            std::mt19937 rng(1234u + 77u * (unsigned)i);
            for (int pass = 0; pass < 4; pass++) {
                {
                    LanePass<Member> p(&g);
                    mem[i].state = BEFORE;
                    std::this_thread::sleep_for(std::chrono::microseconds(rng() % 3000));
                    mem[i].state = ARRIVED;
                    const int rc = p.arrive(&mem[i], rec);
                    EXPECT(rc == 0, "rc %d", rc);
                    EXPECT(mem[i].launched.load() == pass + 1, "member %d launched %d times after pass %d", i, mem[i].launched.load(), pass);
                    mem[i].state = IDLE;
                }
                std::this_thread::sleep_for(std::chrono::microseconds(rng() % 1500));
            }
        });
    for (auto &t : th) t.join();
    int total = 0;
    for (int n : rec.sizes) total += n;
    EXPECT(total == 12, "12 arrivals, %d launched", total);
    printf("THREE_BY_FOUR launches %zu members %d\n", rec.sizes.size(), total);
}

// nine sessions in a pass at once: the ninth goes into the next launch
static void nine() {
    LaneGather<Member> g;
    Member mem[9];
    Recorder rec;
    for (int i = 0; i < 9; i++) {
        mem[i].id = i;
        rec.lane_members.push_back(&mem[i]);
        g.enter();
        mem[i].state = BEFORE;
    }
    std::vector<std::thread> th;
    for (int i = 0; i < 9; i++)
        th.emplace_back([&, i]() {
            mem[i].state = ARRIVED;
            EXPECT(g.arrive(&mem[i], rec) == 0, "rc");
            EXPECT(mem[i].launched.load() == 1, "member %d launched %d times", i, mem[i].launched.load());
        });
    for (auto &t : th) t.join();
    EXPECT(rec.sizes.size() == 2 && rec.sizes[0] == 8 && rec.sizes[1] == 1, "nine members: %zu launches", rec.sizes.size());
    printf("NINE");
    for (int n : rec.sizes) printf(" %d", n);
    printf("\n");
}

// a session that leaves its pass through a failure path is not waited for; the launch's status reaches every member
static void withdraw_and_status() {
    LaneGather<Member> g;
    Member a, b;
    a.id = 0;
    b.id = 1;
    Recorder rec;
    rec.lane_members = {&a, &b};
    rec.rc = -7;
    std::atomic<int> b_rc{1};
    std::thread tb;
    {
        LanePass<Member> pa(&g);   // a is in its pass ...
        a.state = BEFORE;
        LanePass<Member> *pb = new LanePass<Member>(&g);
        b.state = ARRIVED;
        tb = std::thread([&, pb]() {
            b_rc = pb->arrive(&b, rec);
            delete pb;
        });
        {   // b is (or will be) waiting for a: nothing may have been launched
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
            std::lock_guard<std::mutex> lock(rec.m);
            EXPECT(rec.sizes.empty(), "launched while a mate was in its pass");
        }
        a.state = IDLE;
    }                              // ... and fails: its pass ends without arrive()
    tb.join();
    EXPECT(b_rc.load() == -7, "status %d", b_rc.load());
    EXPECT(rec.sizes.size() == 1 && rec.sizes[0] == 1 && b.launched.load() == 1 && a.launched.load() == 0, "withdraw");
    printf("WITHDRAW ok\n");
}

// a session alone in its lane, or with mates that are not in a pass, launches from its own thread inside arrive()
static void lone() {
    LaneGather<Member> g;
    Member a, idle_mate;
    const std::thread::id me = std::this_thread::get_id();
    int calls = 0;
    for (int pass = 0; pass < 3; pass++) {
        LanePass<Member> p(&g);
        a.state = ARRIVED;
        const int rc = p.arrive(&a, [&](Member *const *grp, int n) {
            EXPECT(n == 1 && grp[0] == &a && std::this_thread::get_id() == me, "lone launch");
            calls++;
            return 0;
        });
        EXPECT(rc == 0 && calls == pass + 1, "lone pass %d", pass);
    }
    (void)idle_mate;
    // no gather at all (a session that launches alone): the pass is inert
    LanePass<Member> none(nullptr);
    printf("LONE %d\n", calls);
}

// ---- holds: an outsider's enter() / withdraw() around the members' arrivals (what jtk_lc_debug_lane_hold does to a lane)

// poll `done` every 50 us for at most 30 s (a sanitizer build on a loaded machine is slow; nothing here waits that long)
template <class Done>
static bool wait_for(Done &&done) {
    const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(30);
    while (!done()) {
        if (std::chrono::steady_clock::now() > until) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    return true;
}

struct OrderRecorder {  // the members of every launch, by id, in the order the launch was given them
    std::mutex m;
    std::vector<std::vector<int>> launches;
    int operator()(Member *const *g, int n) {
        EXPECT(n >= 1 && n <= JTK_LANE_MAX_SEGMENTS, "a launch of %d members", n);
        std::vector<int> ids;
        for (int i = 0; i < n; i++) {
            EXPECT(g[i]->state.load() == ARRIVED, "member %d launched in state %d", g[i]->id, g[i]->state.load());
            g[i]->launched++;
            ids.push_back(g[i]->id);
        }
        std::lock_guard<std::mutex> lock(m);
        launches.push_back(ids);
        return 0;
    }
    size_t count() {
        std::lock_guard<std::mutex> lock(m);
        return launches.size();
    }
};

// one member's pass on a thread of its own, started once `pending_before` members pend: the arrival order is the caller's
static std::thread arrive_after(LaneGather<Member> &g, OrderRecorder &rec, Member &me, int pending_before) {
    EXPECT(wait_for([&]() { return g.pending() == pending_before; }), "member %d: pending never reached %d", me.id, pending_before);
    return std::thread([&g, &rec, &me]() {
        LanePass<Member> p(&g);
        me.state = ARRIVED;
        EXPECT(p.arrive(&me, rec) == 0, "rc");
        EXPECT(me.launched.load() == 1, "member %d launched %d times", me.id, me.launched.load());
    });
}

static void expect_launches(OrderRecorder &rec, LaneGather<Member> &g, const std::vector<std::vector<int>> &want, const char *what) {
    EXPECT(rec.launches == want, "%s: %zu launches, %zu wanted, or other members", what, rec.launches.size(), want.size());
    int ring[JTK_LANE_LEDGER], in_pass = -1, pending = -1;
    unsigned long long calls = 0;
    const int have = g.recent(ring, &in_pass, &pending, &calls);
    EXPECT(calls == want.size() && g.launch_calls() == want.size(), "%s: %llu calls counted", what, calls);
    EXPECT(in_pass == 0 && pending == 0 && g.in_pass() == 0 && g.pending() == 0, "%s: in pass %d, pending %d afterwards", what, in_pass, pending);
    EXPECT(have == (int)std::min<size_t>(want.size(), JTK_LANE_LEDGER), "%s: %d records", what, have);
    for (int i = 0; i < have; i++) {
        const size_t call = want.size() - have + i;
        EXPECT(ring[i] == (int)want[call].size(), "%s: call %zu recorded with %d members", what, call, ring[i]);
    }
}

// an outsider holds, n members arrive one after the other from n threads: all pend, nothing is launched; the release gives the
// first min(n, 8) in arrival order, then the rest, 8 at a time
static void held(int n) {
    LaneGather<Member> g;
    std::vector<Member> mem(n);
    OrderRecorder rec;
    g.enter();
    EXPECT(g.in_pass() == 1 && g.pending() == 0 && g.launch_calls() == 0, "a fresh hold");
    std::vector<std::thread> th;
    for (int i = 0; i < n; i++) {
        mem[i].id = i;
        th.push_back(arrive_after(g, rec, mem[i], i));
    }
    EXPECT(wait_for([&]() { return g.pending() == n; }), "held %d: pending stays at %d", n, g.pending());
    EXPECT(g.in_pass() == 1, "held %d: %d in a pass beside the hold", n, g.in_pass() - 1);
    EXPECT(g.launch_calls() == 0 && rec.count() == 0, "held %d: launched under the hold", n);
    g.withdraw();
    for (auto &t : th) t.join();
    std::vector<std::vector<int>> want;
    for (int i = 0; i < n; i++) {
        if (i % JTK_LANE_MAX_SEGMENTS == 0) want.emplace_back();
        want.back().push_back(i);
    }
    expect_launches(rec, g, want, "held");
    printf("HELD %d", n);
    for (auto &l : rec.launches) printf(" %zu", l.size());
    printf("\n");
}

// a member that leaves its pass while the lane is held is neither launched nor waited for: once between two arrivals, once
// after the hold itself has gone
static void held_withdraw() {
    LaneGather<Member> g;
    Member a, b, c;
    a.id = 0, b.id = 1, c.id = 2;
    OrderRecorder rec;
    g.enter();
    std::thread ta = arrive_after(g, rec, a, 0);
    EXPECT(wait_for([&]() { return g.pending() == 1; }), "a pends");
    {
        LanePass<Member> pb(&g);
        b.state = BEFORE;
        EXPECT(g.in_pass() == 2, "b in its pass under the hold");
        b.state = IDLE;
    }  // b fails: no arrive()
    EXPECT(g.in_pass() == 1 && g.pending() == 1 && g.launch_calls() == 0, "b's withdrawal under the hold launched or unpended");
    std::thread tc = arrive_after(g, rec, c, 1);
    EXPECT(wait_for([&]() { return g.pending() == 2; }), "c pends");
    g.withdraw();
    ta.join();
    tc.join();
    expect_launches(rec, g, {{0, 2}}, "withdraw under a hold");
    EXPECT(b.launched.load() == 0, "the withdrawn member was launched");

    // the hold goes while b is still in a pass: a goes on waiting for b, and launches alone when b leaves
    LaneGather<Member> g2;
    Member a2, b2;
    a2.id = 0, b2.id = 1;
    OrderRecorder rec2;
    g2.enter();
    std::thread ta2 = arrive_after(g2, rec2, a2, 0);
    EXPECT(wait_for([&]() { return g2.pending() == 1; }), "a2 pends");
    {
        LanePass<Member> pb(&g2);
        b2.state = ARRIVED;  // (never arrives; ARRIVED so that no launch check trips over it)
        g2.withdraw();       // the hold
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        EXPECT(g2.launch_calls() == 0 && g2.pending() == 1 && g2.in_pass() == 1, "released with a mate in its pass: launched at once");
    }
    ta2.join();
    expect_launches(rec2, g2, {{0}}, "a mate that leaves after the release");
    EXPECT(b2.launched.load() == 0, "the withdrawn member was launched");
    printf("HELD_WITHDRAW ok\n");
}

// a second hold taken while members pend: the release of the first launches nothing, later arrivals join the same gather
static void second_hold() {
    LaneGather<Member> g;
    Member mem[3];
    OrderRecorder rec;
    for (int i = 0; i < 3; i++) mem[i].id = i;
    g.enter();
    std::vector<std::thread> th;
    th.push_back(arrive_after(g, rec, mem[0], 0));
    th.push_back(arrive_after(g, rec, mem[1], 1));
    EXPECT(wait_for([&]() { return g.pending() == 2; }), "two pend");
    g.enter();     // the second hold
    g.withdraw();  // the first one's release
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
    EXPECT(g.launch_calls() == 0 && g.pending() == 2 && g.in_pass() == 1, "the first release launched under the second hold");
    th.push_back(arrive_after(g, rec, mem[2], 2));
    EXPECT(wait_for([&]() { return g.pending() == 3; }), "three pend");
    EXPECT(g.launch_calls() == 0, "launched under the second hold");
    g.withdraw();
    for (auto &t : th) t.join();
    expect_launches(rec, g, {{0, 1, 2}}, "second hold");
    printf("SECOND_HOLD ok\n");
}

int main() {
    plans();
    const int qs[] = {1, 4, 8, 12};
    for (int q : qs) assignment(q);
    three_by_four();
    nine();
    withdraw_and_status();
    lone();
    const int held_sizes[] = {1, 3, 8, 9, 17};
    for (int n : held_sizes) held(n);
    held_withdraw();
    second_hold();
    printf("FAILURES %d\n", g_failures.load());
    return g_failures.load() ? 1 : 0;
}
