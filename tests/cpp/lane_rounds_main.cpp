// lane_rounds_main.cpp -- the round gather of jtk_amd/csrc/session_lanes.h (RoundGather / RoundPass) with mock launches, as a
// program of its own (tests/test_lane_rounds.py builds it plain and with a sanitizer and runs it).  Every launch is checked
// where it is made: at most JTK_LANE_MAX_SEGMENTS members, no member twice, every member parked, and nobody that is in its
// rounds left out unless a step asked for it.  Any violated expectation prints FAIL ... and makes the exit status 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <random>
#include <set>
#include <thread>
#include <vector>

#include "session_lanes.h"

static std::atomic<int> g_failures{0};
#define EXPECT(cond, ...)                              \
    do {                                               \
        if (!(cond)) {                                 \
            printf("FAIL %s:%d ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                       \
            printf("\n");                              \
            g_failures++;                              \
        }                                              \
    } while (0)

enum { OUT = 0, RUNNING = 1, PARKED = 2 };  // RUNNING: in its rounds, host thread on its way to arrive() or leave()
struct Member {
    int id = 0;
    std::atomic<int> state{OUT};
    std::atomic<int> round{-1};     // what it asks for: -1 the opening, then 0, 1, ...
    std::atomic<int> launched{0};   // launches that carried it
};
typedef RoundGather<Member> Rounds;

struct Launch {
    std::vector<int> ids, rounds;
};
struct Recorder {
    std::vector<Member *> lane;   // everybody who may be in its rounds on this lane
    std::atomic<bool> stepping{false};  // a step may leave RUNNING members out
    std::mutex m;
    std::vector<Launch> launches;
    int rc = 0;
    int operator()(Member *const *g, int n) {
        EXPECT(n >= 1 && n <= JTK_LANE_MAX_SEGMENTS, "a launch of %d members", n);
        std::set<int> seen;
        Launch l;
        for (int i = 0; i < n; i++) {
            EXPECT(seen.insert(g[i]->id).second, "member %d twice in one launch", g[i]->id);
            EXPECT(g[i]->state.load() == PARKED, "member %d launched in state %d", g[i]->id, g[i]->state.load());
            g[i]->launched++;
            l.ids.push_back(g[i]->id);
            l.rounds.push_back(g[i]->round.load());
        }
        if (!stepping.load())
            for (Member *x : lane) EXPECT(x->state.load() != RUNNING, "launch while member %d is in its rounds and not parked", x->id);
        std::lock_guard<std::mutex> lock(m);
        launches.push_back(l);
        return rc;
    }
    size_t count() {
        std::lock_guard<std::mutex> lock(m);
        return launches.size();
    }
    std::vector<Launch> all() {
        std::lock_guard<std::mutex> lock(m);
        return launches;
    }
    std::vector<std::vector<int>> ids() {
        std::lock_guard<std::mutex> lock(m);
        std::vector<std::vector<int>> v;
        for (auto &l : launches) v.push_back(l.ids);
        return v;
    }
};

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

// one arrival of a member that is in its rounds
static int park(Rounds &g, Recorder &rec, Member &me) {
    me.state = PARKED;
    const int rc = g.arrive(&me, rec);
    me.state = RUNNING;
    return rc;
}

// a member's polish phase: the opening and `rounds` rounds, seeded delays between them
static void phase(Rounds &g, Recorder &rec, Member &me, int rounds, unsigned seed) {
    std::mt19937 rng(seed);
    RoundPass<Member> p(&g);
    me.state = RUNNING;   // (after enter(): until the gather counts it, a launch may be made without it)
    for (int r = -1; r < rounds; r++) {
        std::this_thread::sleep_for(std::chrono::microseconds(rng() % 800));
        me.round = r;
        const int before = me.launched.load();
        EXPECT(park(g, rec, me) == 0, "rc");
        EXPECT(me.launched.load() == before + 1, "member %d: %d launches for one arrival", me.id, me.launched.load() - before);
    }
    me.state = OUT;
}

// n members, each leaves after its own number of rounds: every arrival is launched exactly once, everybody ends
static void different_lengths(int n) {
    Rounds g;
    std::vector<Member> mem(n);
    Recorder rec;
    for (int i = 0; i < n; i++) {
        mem[i].id = i;
        rec.lane.push_back(&mem[i]);
    }
    std::vector<std::thread> th;
    int arrivals = 0;
    for (int i = 0; i < n; i++) {
        const int rounds = 1 + (i * 3) % 7;
        arrivals += rounds + 1;
        th.emplace_back([&, i, rounds]() { phase(g, rec, mem[i], rounds, 99u + 31u * (unsigned)i); });
    }
    for (auto &t : th) t.join();
    int carried = 0;
    for (auto &l : rec.launches) carried += (int)l.ids.size();
    EXPECT(carried == arrivals, "%d members: %d arrivals, %d carried", n, arrivals, carried);
    EXPECT(g.in_rounds() == 0 && g.parked() == 0, "%d members: %d in rounds, %d parked afterwards", n, g.in_rounds(), g.parked());
    printf("LENGTHS %d arrivals %d launches %zu\n", n, arrivals, rec.launches.size());
}

// n members park under a hold one after the other; the release launches them in arrival order, 8 per call
static void held(int n) {
    Rounds g;
    std::vector<Member> mem(n);
    Recorder rec;
    g.hold();
    std::vector<std::thread> th;
    for (int i = 0; i < n; i++) {
        mem[i].id = i;
        rec.lane.push_back(&mem[i]);
    }
    for (int i = 0; i < n; i++) {
        EXPECT(wait_for([&]() { return g.parked() == i; }), "held %d: parked never reached %d", n, i);
        th.emplace_back([&, i]() {
            RoundPass<Member> p(&g);
            mem[i].state = RUNNING;
            EXPECT(park(g, rec, mem[i]) == 0, "rc");
            mem[i].state = OUT;
        });
    }
    EXPECT(wait_for([&]() { return g.parked() == n; }), "held %d: %d parked", n, g.parked());
    EXPECT(g.in_rounds() == n && g.holds() == 1 && g.launch_calls() == 0 && rec.count() == 0, "held %d: launched under the hold", n);
    EXPECT(g.release(), "release");
    EXPECT(!g.release(), "a second release of one hold");
    for (auto &t : th) t.join();
    std::vector<std::vector<int>> want;
    for (int i = 0; i < n; i++) {
        if (i % JTK_LANE_MAX_SEGMENTS == 0) want.emplace_back();
        want.back().push_back(i);
    }
    EXPECT(rec.ids() == want, "held %d: %zu launches, %zu wanted, or other members", n, rec.count(), want.size());
    int ring[JTK_LANE_LEDGER];
    unsigned long long calls = 0;
    const int have = g.recent(ring, nullptr, nullptr, &calls);
    EXPECT(calls == want.size() && have == (int)std::min<size_t>(want.size(), JTK_LANE_LEDGER), "held %d: %llu calls counted", n, calls);
    for (int i = 0; i < have; i++) EXPECT(ring[i] == (int)want[want.size() - have + i].size(), "held %d: ring", n);
    printf("HELD %d", n);
    for (auto &l : rec.launches) printf(" %zu", l.ids.size());
    printf("\n");
}

// a member enters its rounds while two others are parked under a hold: the release waits for it; and a step under a hold
// launches the parked ones without it, so that the next launch holds members of different rounds
static void enter_while_parked_and_step() {
    Rounds g;
    Member a, b, c;
    a.id = 0, b.id = 1, c.id = 2;
    Recorder rec;
    rec.lane = {&a, &b, &c};
    g.hold();
    std::thread ta([&]() { phase(g, rec, a, 1, 1); }), tb([&]() { phase(g, rec, b, 1, 2); });
    EXPECT(wait_for([&]() { return g.parked() == 2; }), "two parked");
    g.enter();   // c is in its rounds, on its way
    c.state = RUNNING;
    EXPECT(g.in_rounds() == 3, "three in their rounds");
    rec.stepping = true;
    g.step();    // a and b get their opening although c is not parked
    EXPECT(wait_for([&]() { return rec.count() == 1 && g.parked() == 2; }), "the step launched once and a, b parked again");
    rec.stepping = false;
    EXPECT(g.holds() == 1, "the step dropped the hold");
    EXPECT(g.release(), "release");
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
    EXPECT(rec.count() == 1, "released with a member in its rounds and not parked: launched at once");
    c.round = -1;
    std::thread tc([&]() {
        EXPECT(park(g, rec, c) == 0, "rc");   // the launch: a round 0, b round 0, c opening
        c.round = 0;
        EXPECT(park(g, rec, c) == 0, "rc");
        c.state = OUT;
        g.leave();
    });
    ta.join();
    tb.join();
    tc.join();
    EXPECT(rec.launches.size() == 3, "%zu launches", rec.launches.size());
    if (rec.launches.size() == 3) {
        const Launch &l = rec.launches[1];
        EXPECT(l.ids.size() == 3 && l.ids[2] == 2 && l.rounds[0] == 0 && l.rounds[1] == 0 && l.rounds[2] == -1, "members of different rounds in one launch");
        EXPECT(rec.launches[2].ids == std::vector<int>{2}, "the last member goes on alone");
    }
    printf("STEP ok\n");
}

// a member at its chain point while its mate still takes rounds: the rounds go on without it, the chain waits for the mate; a
// hold of the chain gather does not stall rounds either
static void chain_point_and_chain_hold() {
    Rounds g;
    LaneGather<Member> chain;
    Member a, b;
    a.id = 0, b.id = 1;
    Recorder rec;
    rec.lane = {&a, &b};
    std::atomic<int> chain_launches{0}, chain_members{0};
    auto chain_launch = [&](Member *const *, int n) {
        chain_launches++;
        chain_members += n;
        return 0;
    };
    chain.enter();   // an outsider's hold of the chain gather
    auto pass = [&](Member &me, int rounds, unsigned seed) {
        LanePass<Member> p(&chain);
        phase(g, rec, me, rounds, seed);   // leaves its rounds at the end
        EXPECT(p.arrive(&me, chain_launch) == 0, "rc");
    };
    std::thread ta([&]() { pass(a, 1, 5); }), tb([&]() { pass(b, 6, 6); });
    // both finish their polish phase under the chain hold and pend at the chain point
    EXPECT(wait_for([&]() { return chain.pending() == 2; }), "the chain hold stalled rounds: %d pend", chain.pending());
    EXPECT(chain_launches.load() == 0 && g.in_rounds() == 0, "launched under the chain hold");
    EXPECT(a.launched.load() == 2 && b.launched.load() == 7, "rounds carried: %d, %d", a.launched.load(), b.launched.load());
    bool alone = false;   // b took rounds alone after a had left for its chain point
    for (auto &l : rec.all()) alone = alone || (l.ids == std::vector<int>{1} && l.rounds[0] >= 1);
    EXPECT(alone, "b never launched a round alone");
    chain.withdraw();
    ta.join();
    tb.join();
    EXPECT(chain_launches.load() == 1 && chain_members.load() == 2, "chain: %d launches, %d members", chain_launches.load(), chain_members.load());
    printf("CHAIN ok\n");
}

// a member that returns early while its mate is parked: the mate launches alone, and the launch's status reaches its members
static void withdraw_and_status() {
    Rounds g;
    Member a, b;
    a.id = 0, b.id = 1;
    Recorder rec;
    rec.lane = {&a, &b};
    rec.rc = -7;
    std::atomic<int> b_rc{1};
    std::thread tb;
    {
        RoundPass<Member> pa(&g);
        a.state = RUNNING;
        tb = std::thread([&]() {
            RoundPass<Member> pb(&g);
            b.state = RUNNING;
            b_rc = park(g, rec, b);
            b.state = OUT;
        });
        EXPECT(wait_for([&]() { return g.parked() == 1 && g.in_rounds() == 2; }), "b parked");
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        EXPECT(rec.count() == 0, "launched while a mate was in its rounds");
        a.state = OUT;
    }   // a fails: its scope ends without another arrive()
    tb.join();
    EXPECT(b_rc.load() == -7, "status %d", b_rc.load());
    EXPECT(rec.ids() == (std::vector<std::vector<int>>{{1}}) && a.launched.load() == 0, "withdraw");
    EXPECT(g.in_rounds() == 0 && g.parked() == 0, "left behind");
    // no gather at all: the pass is inert
    RoundPass<Member> none(nullptr);
    none.leave();
    printf("WITHDRAW ok\n");
}

// release in a chosen order: c parks first, then a, then b
static void chosen_order() {
    Rounds g;
    Member m[3];
    Recorder rec;
    for (int i = 0; i < 3; i++) {
        m[i].id = i;
        rec.lane.push_back(&m[i]);
    }
    g.hold();
    g.hold();   // holds count
    const int order[3] = {2, 0, 1};
    std::vector<std::thread> th;
    for (int k = 0; k < 3; k++) {
        EXPECT(wait_for([&]() { return g.parked() == k; }), "parked %d", k);
        Member &me = m[order[k]];
        th.emplace_back([&]() {
            RoundPass<Member> p(&g);
            me.state = RUNNING;
            EXPECT(park(g, rec, me) == 0, "rc");
            me.state = OUT;
        });
    }
    EXPECT(wait_for([&]() { return g.parked() == 3; }), "three parked");
    g.release();
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
    EXPECT(rec.count() == 0 && g.holds() == 1, "the first release launched under the second hold");
    g.release();
    for (auto &t : th) t.join();
    EXPECT(rec.ids() == (std::vector<std::vector<int>>{{2, 0, 1}}), "arrival order");
    printf("ORDER ok\n");
}

int main() {
    const int sizes[] = {1, 2, 3, 8, 9, 17};
    for (int n : sizes) different_lengths(n);
    for (int n : sizes) held(n);
    enter_while_parked_and_step();
    chain_point_and_chain_hold();
    withdraw_and_status();
    chosen_order();
    printf("FAILURES %d\n", g_failures.load());
    return g_failures.load() ? 1 : 0;
}
