// The host pieces by which a session leaves a merged chain launch (jtk_amd/csrc/session_lanes.h: lane_round_stream, lane_member_may_leave,
// LaneFlow, LaneFlightLeave, ChainDone, lane_leave_wait), as a program with its own main: plain C++, no HIP.  tests/test_lane_leave.py builds it plain and under
// -fsanitize=address,undefined and reads the marks it prints.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "session_lanes.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);       \
            failures++;                                                 \
        }                                                               \
    } while (0)

// ---- the stream of a pass, with the in-flight state given
static void stream_choice() {
    const bool none[2] = {false, false}, on0[2] = {true, false}, on1[2] = {false, true}, both[2] = {true, true};
    for (int current = 0; current < 2; current++) {
        CHECK(lane_round_stream(on0, current) == 1);   // a light chain in flight on either stream: the other one
        CHECK(lane_round_stream(on1, current) == 0);
        CHECK(lane_round_stream(none, current) == current);  // both idle: rounds stay where they are
        CHECK(lane_round_stream(both, current) == current);  // (no lane produces it)
    }
    printf("CHOICE ok\n");
}

// A lane as session.hip drives it, without HIP: the decisions are LaneFlow's and lane_member_may_leave's (the code session.hip
// runs); only the queues are mock -- per stream a list of what was put on it: 'L' light chain, 'G' general chain, 'H' a
// member's global-memory chain behind the merged launch, 'f' fetch, 'r' rounds.
struct MockMember {
    uint32_t workgroups = 6, huge_chunks = 0;
    bool pinned = true, uses_side = true;
    int stream = 0;                      // where its rounds ran (bound at the start of its pass)
    std::shared_ptr<LaneFlight> flight;  // what the launch gave it
    bool may_leave = false;              // through its word; otherwise it waits for the event behind its own last kernel
};
struct MockLane {
    LaneFlow flow;
    std::vector<char> queued[2];
    std::vector<MockMember *> in_pass;  // between the start of a pass and the chain point
    void begin_pass(MockMember &m) {
        m.stream = flow.round_stream(true);
        queued[m.stream].push_back('r');
        for (auto *o : in_pass) CHECK(o->stream == m.stream);  // whoever may park at the same round gather is on one stream
        in_pass.push_back(&m);
    }
    // launch_lane_chains: the light chain behind the members' rounds, the general chain where LaneFlow allows, a flight for
    // the members that may leave if there are several
    bool launch(std::vector<MockMember *> members) {
        const int main_idx = members[0]->stream;
        bool all_side = true;
        for (auto *m : members) {
            CHECK(m->stream == main_idx);  // every member of a gather was bound to the same stream
            all_side = all_side && m->uses_side;
            m->flight.reset();
            m->may_leave = false;
            in_pass.erase(std::find(in_pass.begin(), in_pass.end(), m));
        }
        CHECK(in_pass.empty());  // LaneGather launches when nobody is in a pass
        CHECK(queued[main_idx].back() == 'r');  // the light chain follows the rounds
        const bool other = flow.general_on_other(main_idx, all_side);
        queued[other ? 1 - main_idx : main_idx].push_back('G');
        queued[main_idx].push_back('L');
        if (members.size() > 1 && flow.may_fly()) {
            auto f = std::make_shared<LaneFlight>();
            f->members = (int)members.size();
            f->light_stream = main_idx;
            for (auto *m : members) {
                m->flight = f;  // every member is in the launch until its pass is over
                m->may_leave = lane_member_may_leave(m->workgroups, m->pinned, m->huge_chunks);
            }
            f->waiting.store((int)members.size());
            flow.launched(f);
        }
        for (auto *m : members)
            if (m->huge_chunks) queued[main_idx].push_back('H');  // run_batch: behind the merged launch, on the member's stream
        return other;
    }
    // run_batch after the launch: a member that may leave does so through its word and is bound again; any other waits for
    // its event and keeps its stream; both are out of the flight then.  Returns the stream its fetch went to.
    int finish_pass(MockMember &m) {
        if (m.flight) {
            LaneFlightLeave out(m.flight.get());
            CHECK(out.leave() >= 0);
            CHECK(out.leave() == -1);  // once
            if (m.may_leave) m.stream = flow.round_stream(true);
        }
        queued[m.stream].push_back('f');
        return m.stream;
    }
};

static void stream_passes() {
    for (int first = 0; first < 2; first++) {
        MockLane lane;
        lane.flow.start_on(first);
        MockMember a, b, c;
        for (int pass = 0; pass < 5; pass++) {
            for (auto *m : {&a, &b, &c}) lane.begin_pass(*m);
            const int light = a.stream;
            CHECK(light == (pass % 2 == 0 ? first : 1 - first));  // the round stream alternates with the merged launches
            CHECK(lane.launch({&a, &b, &c}));                      // the general chain on the other stream
            CHECK(lane.queued[1 - light].back() == 'G' && lane.queued[light].back() == 'L');
            // the first to leave: the light chain is in flight on `light`; its fetch lands behind the general chain
            CHECK(lane.finish_pass(a) == 1 - light);
            CHECK(lane.queued[1 - light][lane.queued[1 - light].size() - 2] == 'G');
            CHECK(lane.finish_pass(b) == 1 - light);  // a lane-mate released later joins the same stream
            CHECK(lane.finish_pass(c) == 1 - light);  // the last one: nothing in flight any more, the rounds stay where they are
            CHECK(lane.flow.flights_in_view() == 0 && lane.flow.round_stream(true) == 1 - light);
            CHECK(lane.queued[light].back() == 'L');  // nothing was put behind the light chain
        }
        // a launch of one member flips nothing and gives no flight
        lane.begin_pass(a);
        const int before = a.stream;
        lane.launch({&a});
        CHECK(!a.flight && lane.finish_pass(a) == before && lane.flow.round_stream(true) == before);
    }
    printf("PASSES ok\n");
}

// who may leave: only a member for which the merged launch is everything the pass still has on the device
static void eligibility() {
    CHECK(lane_member_may_leave(6, true, 0));
    CHECK(!lane_member_may_leave(0, true, 0));   // nothing of its own in the merged kernels: nobody would report
    CHECK(!lane_member_may_leave(6, false, 0));  // no pinned page to report into
    CHECK(!lane_member_may_leave(6, true, 1));   // chunks of the global-memory class: their kernel is queued BEHIND the launch
    MockLane lane;
    MockMember a, h;
    h.huge_chunks = 2;
    lane.begin_pass(a);
    lane.begin_pass(h);
    lane.launch({&a, &h});
    CHECK(a.flight && a.may_leave && h.flight == a.flight && !h.may_leave && a.flight->waiting.load() == 2);
    const int light = h.stream;
    CHECK(lane.queued[light].back() == 'H');
    CHECK(lane.finish_pass(a) == 1 - light);  // a leaves and moves
    CHECK(lane.finish_pass(h) == light);       // h waits for the event behind its last kernel and keeps its stream:
    CHECK(lane.queued[light][lane.queued[light].size() - 2] == 'H');  // its fetch is behind that kernel
    CHECK(lane.flow.flights_in_view() == 0);
    // a launch in which nobody may leave: everybody keeps its stream
    MockMember h2;
    h2.huge_chunks = 1;
    lane.begin_pass(h);
    lane.begin_pass(h2);
    lane.launch({&h, &h2});
    CHECK(!h.may_leave && !h2.may_leave);
    CHECK(lane.finish_pass(h) == h.stream && lane.finish_pass(h2) == h2.stream && lane.flow.flights_in_view() == 0);
    // a member without a side stream: the general chain stays on the round stream
    MockMember n1, n2;
    n2.uses_side = false;
    lane.begin_pass(n1);
    lane.begin_pass(n2);
    CHECK(!lane.launch({&n1, &n2}));
    lane.finish_pass(n1);
    lane.finish_pass(n2);
    printf("ELIGIBLE ok\n");
}

// two members come round and merge while a third still waits in the launch before: the second launch does not fly, and the
// round stream does not move while a member is in its pass
static void two_flights() {
    MockLane lane;
    MockMember a, b, c;
    for (auto *m : {&a, &b, &c}) lane.begin_pass(*m);
    lane.launch({&a, &b, &c});  // L1: light chain on 0
    CHECK(lane.finish_pass(a) == 1 && lane.finish_pass(b) == 1);
    lane.begin_pass(a);
    lane.begin_pass(b);
    CHECK(a.stream == 1 && b.stream == 1);
    CHECK(!lane.launch({&a, &b}));  // L2: c has not left the light chain on 0, so the general chain goes behind the rounds on 1
    CHECK(!a.flight && !b.flight && lane.flow.flights_in_view() == 1);  // and L2 is no flight: a and b wait for their events
    CHECK(lane.finish_pass(a) == 1);
    lane.begin_pass(a);               // a is in its rounds, on 1 ...
    CHECK(a.stream == 1);
    CHECK(lane.finish_pass(c) == 1);  // ... when c leaves L1: the round stream stays, c's fetch and next pass join a on 1
    CHECK(lane.flow.flights_in_view() == 0);
    lane.begin_pass(c);               // (begin_pass checks that c and a are on one stream)
    CHECK(lane.finish_pass(b) == 1);
    lane.begin_pass(b);
    CHECK(lane.launch({&a, &c, &b}));  // all three again: a flight, light chain on 1, the general chain on 0
    CHECK(a.flight && lane.flow.round_stream(true) == 0);
    for (auto *m : {&a, &b, &c}) CHECK(lane.finish_pass(*m) == 0);
    // the guard takes a member out on a path that never reaches the wait
    auto f = std::make_shared<LaneFlight>();
    f->waiting.store(2);
    { LaneFlightLeave early(f.get()); }
    CHECK(f->waiting.load() == 1);
    printf("FLIGHTS ok\n");
}

// ---- the never-reset counter: a device that counts workgroups one by one
struct MockDevice {
    uint32_t counter;
    uint32_t word = 0;
    int reports = 0;
    void workgroup_ends(uint32_t target, uint32_t pass) {
        const uint32_t before = counter++;
        if (ChainDone::reports(before, target)) {
            word = pass;
            reports++;
        }
    }
};

static void targets(uint32_t start) {
    ChainDone host;
    host.target = start;
    MockDevice dev;
    dev.counter = start;
    // consecutive launches with different segment sets: {class 0} in both kernels, {class 0, class 1}, one kernel only, a
    // single workgroup, and a pass in which the session launches nothing (the target stays)
    const std::vector<std::vector<uint32_t>> launches = {{2 * 5}, {2 * 5, 2 * 3}, {7}, {1}, {}, {2 * 64, 2 * 1}};
    uint32_t last_pass = 0;
    for (const auto &kernels : launches) {
        uint32_t total = 0;
        for (uint32_t k : kernels) total += k;
        if (!total) {
            CHECK(dev.counter == host.target);
            continue;
        }
        host.advance(total);
        CHECK(host.pass != 0 && host.pass != last_pass);
        last_pass = host.pass;
        dev.word = 0;
        dev.reports = 0;
        for (uint32_t w = 0; w < total; w++) {
            CHECK(dev.word == 0);  // nobody reports before the last workgroup of either kernel has counted
            dev.workgroup_ends(host.target, host.pass);
        }
        CHECK(dev.reports == 1 && dev.word == host.pass && dev.counter == host.target);
    }
    printf("TARGETS ok from %u\n", start);
}

static void pass_ids() {
    ChainDone d;
    d.pass = 0xfffffffeu;
    d.advance(1);
    CHECK(d.pass == 0xffffffffu);
    d.advance(1);
    CHECK(d.pass == 1);  // 0 is what the word is cleared to
    printf("IDS ok\n");
}

// ---- word first, event second, error if neither
static void fallback() {
    int words = 0, events = 0, pauses = 0;
    auto reset = [&] { words = events = pauses = 0; };
    // the word shows at the first look: the event is not even asked
    CHECK(lane_leave_wait([&] { words++; return true; }, [&] { events++; return 0; }, [&] { pauses++; }) == JTK_LEAVE_WORD);
    CHECK(words == 1 && events == 0 && pauses == 0);
    reset();
    // pending for a while, then the word: every look at the event comes after a look at the word, with a pause between rounds
    CHECK(lane_leave_wait([&] { return ++words > 4; }, [&] { events++; return 0; }, [&] { pauses++; }) == JTK_LEAVE_WORD);
    CHECK(words == 5 && events == 4 && pauses == 4);
    reset();
    // the event completes and the word has not moved: the pass ends as the event ends it
    CHECK(lane_leave_wait([&] { words++; return false; }, [&] { return ++events > 2 ? 1 : 0; }, [&] { pauses++; }) == JTK_LEAVE_EVENT);
    CHECK(events == 3 && pauses == 2 && words == 4);  // (one more look at the word after the event)
    reset();
    // the word moves between the look at it and the look at the event: still the word
    CHECK(lane_leave_wait([&] { return ++words > 1; }, [&] { events++; return 1; }, [&] { pauses++; }) == JTK_LEAVE_WORD);
    CHECK(words == 2 && events == 1 && pauses == 0);
    reset();
    // neither: the event fails, the word does not move
    CHECK(lane_leave_wait([&] { words++; return false; }, [&] { events++; return -1; }, [&] { pauses++; }) == JTK_LEAVE_ERROR);
    CHECK(words == 2 && events == 1 && pauses == 0);
    printf("FALLBACK ok\n");
}

int main() {
    stream_choice();
    stream_passes();
    eligibility();
    two_flights();
    targets(0);
    targets(0xfffffff0u);  // the counter wraps with its target
    pass_ids();
    fallback();
    printf("FAILURES %d\n", failures);
    return failures ? 1 : 0;
}
